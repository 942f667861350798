"""Cross-channel affine colour transfer, rgb' = rgb @ A + t: the notebook's ``fit_ot_affine_rgb`` / ``apply_affine_rgb``
(Pairs_EMIT_S2_demo-2.ipynb, the cell after ``reproject_stack_to_grid``) and the all-valid-pixels fit ``fit_affine_rgb``, device
resident (csrc/hsr_color.hip): the 4 x 4 / 4 x 3 moments, the ``np.linalg.lstsq`` solve and the apply are HIP kernels; nothing
falls back to the host.  It is the counterpart of poly_regression.py's per-channel polynomial, which cannot mix channels.
"""
from __future__ import annotations

import numpy as np

from . import _engine as eng
from . import _native as nat

_MIN_COUNT_OT = 2          # the notebook's fallback: fewer than 2 usable rows on either side -> identity


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _device_image(torch, img, what):
    """(H, W, C >= 3) NumPy array or tensor -> float32 GPU tensor (a new one only when something has to change)."""
    if img.ndim != 3 or img.shape[-1] < 3:
        raise ValueError(f"{what} must be (H,W,C>=3). Got shape {tuple(img.shape)}")
    if _is_torch(img):
        if not img.is_cuda:
            raise ValueError(f"{what} must be a GPU tensor (or a NumPy array)")
        return img.to(torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).cuda()


def _device_mask(torch, mask, shape, device):
    if _is_torch(mask):
        m = mask.to(device=device)
    else:
        m = torch.from_numpy(np.ascontiguousarray(np.asarray(mask, dtype=np.bool_)).view(np.uint8)).to(device)
    if tuple(m.shape) != tuple(shape):
        raise IndexError(f"boolean index did not match indexed array: mask must be {tuple(shape)}, got {tuple(m.shape)}")
    return (m != 0).to(torch.uint8).contiguous().reshape(-1)


def _identity(torch, device):
    return torch.eye(3, dtype=torch.float64, device=device), torch.zeros(3, dtype=torch.float64, device=device)


def _fit_ot_device(torch, src, ref, mask, n_samples, reg, numItermax, stopThr, seed):
    """src, ref (H, W, C) float32 GPU tensors, mask (H, W) GPU tensor -> (A, t) GPU tensors, or None on too few rows."""
    from . import _ot
    s = _ot.sample_pairs_device(src, ref, mask, n_samples, seed, min_rows=_MIN_COUNT_OT)
    if s is None:
        return None
    X, Y = s
    # the draw above has synchronised already; polling the Sinkhorn state every 50 iterations enqueues nothing after convergence
    # (the same targets, ~1.5 ms less on a converging pair), as fit_ot_poly_rgb does
    Ybar = _ot.barycentric_targets_device(X, Y, reg, numItermax, stopThr, poll_every=50)
    ws = eng.AffineWorkspace(X.device)
    eng.affine_moments_f64(X, Ybar, ws)
    A, t = eng.affine_solve(ws, 0)
    return A, t


def fit_ot_affine_rgb(src_rgb, ref_rgb, mask, n_samples=5000, reg=0.05, numItermax=300, stopThr=1e-6, seed=0):
    """Fit f(x) = x A + t (A 3 x 3, t 3) by entropic OT + barycentric projection on the masked pixels, then least squares
    (the notebook's fit_ot_affine_rgb; same signature and defaults).  Sampling reproduces the reference's PCG64 stream
    (source draw first); Sinkhorn, the moments and the np.linalg.lstsq solve run on the GPU.  The identity comes back when either
    image has fewer than 2 finite rows inside the mask.  NumPy in -> float64 NumPy (3,3), (3,); GPU tensors in -> GPU tensors."""
    torch = nat.require_gpu()
    as_torch = _is_torch(src_rgb)
    src = _device_image(torch, src_rgb, "src_rgb")
    ref = _device_image(torch, ref_rgb, "ref_rgb")
    m = _device_mask(torch, mask, src.shape[:2], src.device).reshape(src.shape[:2])
    fit = _fit_ot_device(torch, src, ref, m, n_samples, reg, numItermax, stopThr, seed)
    A, t = fit if fit is not None else _identity(torch, src.device)
    if as_torch:
        return A.clone(), t.clone()
    return A.cpu().numpy(), t.cpu().numpy()


def _as_At(torch, A, t, device):
    A = A if _is_torch(A) else torch.from_numpy(np.ascontiguousarray(A, dtype=np.float64))
    t = t if _is_torch(t) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64))
    if tuple(A.shape) != (3, 3) or tuple(t.shape) != (3,):
        raise ValueError(f"A must be (3,3) and t (3,); got {tuple(A.shape)} and {tuple(t.shape)}")
    return torch.cat([A.to(device, torch.float64).reshape(9), t.to(device, torch.float64)]).contiguous()


def apply_affine_rgb(rgb, A, t, mask=None):
    """rgb' = clip(rgb A + t, 0, 1) inside ``mask`` (everywhere when None); pixels outside pass through unclipped (the notebook's
    apply_affine_rgb).  float32 out, the input is not modified; channels beyond the third pass through as float32.
    NumPy in -> NumPy out; GPU tensor in -> GPU tensor out."""
    torch = nat.require_gpu()
    as_torch = _is_torch(rgb)
    x = _device_image(torch, rgb, "rgb")
    H, W, Cc = (int(s) for s in x.shape)
    m = None if mask is None else _device_mask(torch, mask, (H, W), x.device)
    At = _as_At(torch, A, t, x.device)
    rows = x.reshape(-1, Cc)
    out = torch.empty_like(rows) if Cc == 3 else rows.clone()
    eng.affine_apply(rows, At, m, None, 1, nat.PIXMAJOR, out=out)
    if Cc >= 4:                                    # a row's fourth float is the kernel's pad: the channel goes back
        out[:, 3] = rows[:, 3]
    out = out.reshape(H, W, Cc)
    return out if as_torch else out.cpu().numpy()


def fit_affine_rgb(src, ref, mask, min_count=200, lohi_src=None, lohi_ref=None):
    """Least squares ref ~ src A + t over ALL pixels inside ``mask`` whose six values are finite - the affine counterpart of
    match_pair(use_ot=False) - wholly on the device, no host synchronisation for GPU-tensor input.  ``lohi_src`` / ``lohi_ref``
    ((3, 2) float64: lo, hi per channel) stretch the images first, float32(clip((v - lo) / (hi - lo + 1e-12), 0, 1)).  Fewer than
    ``min_count`` usable pixels give the identity.  NumPy in -> float64 NumPy (3,3), (3,); GPU tensors in -> GPU tensors."""
    torch = nat.require_gpu()
    as_torch = _is_torch(src)
    x = _device_image(torch, src, "src")
    y = _device_image(torch, ref, "ref")
    if x.shape[:2] != y.shape[:2]:
        raise ValueError(f"src and ref must cover the same grid; got {tuple(x.shape)} and {tuple(y.shape)}")
    m = _device_mask(torch, mask, x.shape[:2], x.device)

    def limits(lohi):
        if lohi is None:
            return None
        lohi = lohi if _is_torch(lohi) else torch.from_numpy(np.ascontiguousarray(lohi, dtype=np.float64))
        if tuple(lohi.shape) != (3, 2):
            raise ValueError(f"stretch limits must be (3, 2); got {tuple(lohi.shape)}")
        return lohi.to(x.device, torch.float64).contiguous()

    ws = eng.AffineWorkspace(x.device)
    eng.affine_moments(x.reshape(-1, x.shape[-1]), y.reshape(-1, y.shape[-1]), ws, m, limits(lohi_src), limits(lohi_ref),
                       nat.PIXMAJOR)
    A, t = eng.affine_solve(ws, int(min_count))
    if as_torch:
        return A.clone(), t.clone()
    return A.cpu().numpy(), t.cpu().numpy()
