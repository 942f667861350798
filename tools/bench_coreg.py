"""Benchmark of the co-registration stages (include/hsr_coreg.h, s2_emit/coreg.py) at the size of a real scene pair.

    python tools/bench_coreg.py                          # every row; one JSON line each
    python tools/bench_coreg.py --markdown FILE          # and the table of profiles/r18_coreg.md

Inputs (synthetic, built on the device from a seed): a 10 x 7452 x 7680 S2 scene, float32 and uint16, whose matching band is
smoothed noise; a 285 x 1242 x 1280 float32 EMIT scene whose matching band is the 6 x 6 block mean of the S2 band rolled by
(3, -2) pixels, so every tie point has a peak to find.  window = 32, step = 32, max_shift = 12, every grid point kept.
Rows: the four stages on preallocated outputs (the warp through both of its instances), and coregister_scene as a whole (out=
preallocated; the tie-point buffers are allocated by the call).  Per row: us, the median over SAMPLES samples of REPS back-to-back calls between two device events, after
warm-up, with the fastest and slowest sample.
Yardsticks from the same process: a device-to-device copy of the S2 scene (the warp reads and writes every byte once, so its
bytes / us is given as a fraction of the copy's), and the long double NumPy reference of tests/coreg_cases.py on NUMPY_POINTS tie
points on the host (wall clock; a baseline for the surface stage, not a competitor).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "hyperspectral_super-resolution_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

EMIT_BANDS, HE, WE, S2_BANDS, F = 285, 1242, 1280, 10, 6
WINDOW, STEP, MAX_SHIFT = 32, 32, 12
TRUE_SHIFT = (3, -2)
SAMPLES, REPS, WARMUP = 7, 5, 2
NUMPY_POINTS = 4


def timed(torch, fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for _ in range(SAMPLES):
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / REPS)
    us.sort()
    return us[len(us) // 2], us[0], us[-1]


def smooth_noise(torch, h, w, gen):
    """Noise with structure at a few and at a few tens of pixels, in [0, 1]."""
    import torch.nn.functional as fn
    x = torch.rand((1, 1, h, w), device="cuda", generator=gen)
    fine = fn.avg_pool2d(x, 5, 1, 2)
    coarse = fn.interpolate(fn.avg_pool2d(x, 24, 12, 6), size=(h, w), mode="bilinear", align_corners=False)
    y = (fine - fine.mean()) / fine.std() + (coarse - coarse.mean()) / coarse.std()
    return ((y - y.min()) / (y.max() - y.min()))[0, 0].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markdown", default=None, help="write the result table to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    import s2_emit
    from s2_emit import _engine as eng
    import coreg_cases as cc
    torch.cuda.set_device(0)
    hs, ws = HE * F, WE * F
    gen = torch.Generator(device="cuda").manual_seed(18)
    band = smooth_noise(torch, hs, ws, gen)
    emit = torch.rand((EMIT_BANDS, HE, WE), device="cuda", generator=gen)
    emit[40] = torch.roll(band, (-TRUE_SHIFT[0], -TRUE_SHIFT[1]), (0, 1)).reshape(HE, F, WE, F).mean(dim=(1, 3))
    grid = s2_emit.tie_point_grid(HE, WE, hs, ws, window=WINDOW, step=STEP, factor=F, max_shift=MAX_SHIFT, max_points=10 ** 6)
    origins = torch.from_numpy(grid).cuda()
    P, D = len(grid), 2 * MAX_SHIFT + 1
    min_valid = int(np.ceil(0.75 * WINDOW * WINDOW))
    rows = []
    for dtype in ("float32", "uint16"):
        s2 = torch.rand((S2_BANDS, hs, ws), device="cuda", generator=gen)
        s2[7] = band
        if dtype == "uint16":
            s2 = (s2 * 10000.0).round().to(torch.uint16)
        nbytes = s2.numel() * s2.element_size()
        out = torch.empty_like(s2)
        surface = torch.empty((P, D, D), dtype=torch.float64, device="cuda")
        table = torch.empty((P, 8), dtype=torch.float64, device="cuda")
        us, lo, hi = timed(torch, lambda: out.copy_(s2))
        copy_rate = 2 * nbytes / us / 1e6
        rows.append(dict(row=f"device-to-device copy of the S2 scene, {dtype} (yardstick)", us=us, lo=lo, hi=hi, bytes=2 * nbytes))
        us, lo, hi = timed(torch, lambda: eng.coreg_surface(emit[40], s2[7], origins, WINDOW, F, MAX_SHIFT, min_valid, out=surface))
        rows.append(dict(row=f"hsr_coreg_surface, {P} tie points, {dtype}", us=us, lo=lo, hi=hi, bytes=0, points=P))
        us, lo, hi = timed(torch, lambda: eng.coreg_peaks(surface, origins, WINDOW, F, MAX_SHIFT, (HE, WE), (hs, ws), 0.6, out=table))
        rows.append(dict(row=f"hsr_coreg_peaks, {P} tie points, {dtype}", us=us, lo=lo, hi=hi, bytes=0))
        keep = table.clone()

        def fit():
            table.copy_(keep)
            return eng.coreg_fit_model(table, 1, 1, 1.0, (hs, ws))
        us, lo, hi = timed(torch, fit)
        rows.append(dict(row=f"hsr_coreg_fit_model (affine; with the copy that restores the records), {dtype}", us=us, lo=lo, hi=hi, bytes=0))
        model = fit()
        m = model.cpu().numpy()
        status = np.bincount(table[:, 7].cpu().numpy().astype(int), minlength=6).tolist()
        us, lo, hi = timed(torch, lambda: eng.coreg_warp(s2, model, float("nan") if dtype == "float32" else 0.0, MAX_SHIFT + 1.0, 0.05,
                                                         None, out))
        rows.append(dict(row=f"hsr_coreg_warp, {dtype}", us=us, lo=lo, hi=hi, bytes=2 * nbytes, of_copy=2 * nbytes / us / 1e6 / copy_rate,
                         model=[round(float(v), 6) for v in m[:6]], status_counts=status))
        us, lo, hi = timed(torch, lambda: eng.coreg_warp(s2, model, float("nan") if dtype == "float32" else 0.0, MAX_SHIFT + 1.0, 2.0,
                                                         None, out))
        rows.append(dict(row=f"hsr_coreg_warp, {dtype}, direct-gather instance (slope bound 2.0)", us=us, lo=lo, hi=hi, bytes=2 * nbytes,
                         of_copy=2 * nbytes / us / 1e6 / copy_rate, model=[round(float(v), 6) for v in m[:6]], status_counts=status))
        kw = dict(emit_band=40, s2_band=7, factor=F, window=WINDOW, step=STEP, max_shift=MAX_SHIFT, max_points=10 ** 6, out=out)
        us, lo, hi = timed(torch, lambda: s2_emit.coregister_scene(emit, s2, **kw))
        rows.append(dict(row=f"coregister_scene, {dtype}", us=us, lo=lo, hi=hi, bytes=2 * nbytes))
        # the NumPy reference on a few tie points, and the kernel against it
        sub = grid[:: max(1, P // NUMPY_POINTS)][:NUMPY_POINTS]
        e_np, s_np = emit[40].cpu().numpy(), s2[7].cpu().numpy()
        t0 = time.perf_counter()
        ref, bar = cc.surface_ref(e_np, None, s_np, None, sub, WINDOW, F, MAX_SHIFT, min_valid)
        wall = (time.perf_counter() - t0) * 1e6
        got = surface.cpu().numpy()[:: max(1, P // NUMPY_POINTS)][:NUMPY_POINTS]
        worst = float(np.nanmax(np.abs(got - ref) / bar))
        rows.append(dict(row=f"NumPy long double reference, {len(sub)} tie points, {dtype} (host, wall clock)", us=wall, lo=wall, hi=wall,
                         bytes=0, per_point_us=wall / len(sub), kernel_error_over_bar=worst))
        del s2, out
    for r in rows:
        r["tbps"] = r["bytes"] / r["us"] / 1e6
        print(json.dumps(r))
    if a.markdown:
        lines = ["# r18: co-registration of an S2 scene to an EMIT scene (`hsr_coreg_*`)", "",
                 "MI355X, one GPU, one process. Command: `python tools/bench_coreg.py --markdown FILE`. Inputs and timing are described "
                 f"in the tool's docstring: EMIT {EMIT_BANDS} × {HE} × {WE}, S2 {S2_BANDS} × {hs} × {ws}, window {WINDOW}, step {STEP}, "
                 f"max_shift {MAX_SHIFT}, {P} tie points; the median of {SAMPLES} samples of {REPS} back-to-back calls between two "
                 f"device events after {WARMUP} warm-up calls. The warp's bytes are the scene read once and written once.", "",
                 "| row | µs (median) | min .. max | TB/s | note |", "|---|---|---|---|---|"]
        for r in rows:
            note = ""
            if "of_copy" in r:
                note = f"{100 * r['of_copy']:.0f} % of the copy's rate; status counts {r['status_counts']}; model {r['model']}"
            if "per_point_us" in r:
                note = f"{r['per_point_us'] / 1e3:.0f} ms per tie point; kernel within {r['kernel_error_over_bar']:.3g} of its bar on them"
            rate = f"{r['tbps']:.3f}" if r["bytes"] else ""
            lines.append(f"| {r['row']} | {r['us']:.1f} | {r['lo']:.1f} .. {r['hi']:.1f} | {rate} | {note} |")
        lines += ["", "For comparison, `profiles/r14_ortho.md` records 3.1 TB/s for the lookup-table gather of `hsr_ortho_glt`, the "
                  "comparable gather of this project."]
        with open(a.markdown, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
