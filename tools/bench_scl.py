"""Benchmark of the scene-classification family (include/hsr_scl.h, s2_emit.clouds) at the benchmark scene pair's sizes.

    python tools/bench_scl.py                          # every step; one JSON line each
    python tools/bench_scl.py --markdown FILE          # and the tables of profiles/r22_scl.md
    python tools/bench_scl.py --no-host --no-torch     # skip the NumPy and the torch comparators

Planes (synthetic, built on the device from a seed): the SCL of a 10 x 7452 x 7680 S2 scene, 3726 x 3840 at 20 m and 7452 x 7680
at 10 m - vegetation with cloud blobs (a smooth random field cut at the quantile that gives the cover) of class 9: clear, 10 %
and 60 % cloud.  Steps:
  counts_20m / counts_10m       hsr_scl_class_counts, one window the size of the plane (scl_metrics' launch);
  mask_<cover>_<shape>_r<r>     hsr_scl_mask on the 10 m plane, r = 0 (the lookup instance), 5, 15, 32, disc and square;
  coarse_<cover>                hsr_scl_coarse of the r = 5 disc mask, k = 6, with the count grid of 100 x 100 cell-windows;
  apply_<cover>                 hsr_scl_apply of that mask on a 32 x 7452 x 7680 float32 cube (7.3 GB), with the count;
  fuse_scene / fuse_scene_clear the two drivers end to end on EMIT 285 x 1242 x 1280 float32 and the S2 scene, 32 bands, batches of
                                64, SCL at 20 m with 10 % cloud, buffer 2 (wall clock around a synchronise: each holds its one
                                host synchronisation).
Per step: us, the median over SAMPLES samples of REPS back-to-back launches between two device events after WARMUP calls, with the
fastest and slowest sample; bytes, what the step has to move (counts and coarse: the plane read; mask: read + written; apply: the
mask read and four bytes per band under it written); copy_us, a device-to-device copy in the same process that moves the same
number of bytes (half read, half written); torch_us, the torch form of the mask on the same device - torch.isin, then max_pool2d
for the square and a conv2d with the disc for the disc (r = 5 and 15 only: the cost of both grows with r^2); numpy_ms, the NumPy
reference on this host, wall clock, once - np.unique; np.isin and one shifted OR per offset of the structuring element (r = 5
only); the block sum; the masked assignment (on 4 of the 32 bands).  Where a comparator runs its result is compared with the
kernel's.  The early exit is judged by mask_clear_* against mask_60_*.  Nothing is gated on a number.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "hyperspectral_super-resolution_amd"))

EMIT_SHAPE, S2_SHAPE, TILE, SCALE, NODATA = (285, 1242, 1280), (10, 7452, 7680), 100, 6, -9999.0
SAMPLES, REPS, WARMUP = 5, 3, 2
COVERS = (("clear", 0.0), ("10", 0.10), ("60", 0.60))
RADII = (0, 5, 15, 32)
GROW, FLAT = (1 << 8) | (1 << 9) | (1 << 10), 3


def timed(torch, fn, reps=REPS):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for _ in range(SAMPLES):
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / reps)
    us.sort()
    return us[len(us) // 2], us[0], us[-1]


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def numpy_dilate(scl, r, disc):
    g = np.isin(scl, [8, 9, 10])
    H, W = g.shape
    pad = np.zeros((H + 2 * r, W + 2 * r), dtype=bool)
    pad[r:r + H, r:r + W] = g
    out = np.isin(scl, [0, 1])
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if (dy * dy + dx * dx <= r * r) if disc else True:
                out |= pad[r + dy:r + dy + H, r + dx:r + dx + W]
    return out.astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markdown", default=None, help="write the result tables to this file")
    ap.add_argument("--no-host", action="store_true", help="skip the NumPy comparisons on the host")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch forms of the mask")
    ap.add_argument("--no-fuse", action="store_true", help="skip the two scene drivers")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import s2_emit
    from s2_emit import _native as nat
    from s2_emit._engine import _ptr, _stream
    assert torch.cuda.is_available(), "bench_scl needs a GPU"
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = _stream(torch)
    g = torch.Generator(device="cuda").manual_seed(22)
    rows = []
    _, H, W = S2_SHAPE

    def record(step, us3, nbytes, **extra):
        us, lo, hi = us3
        rec = dict(step=step, us=round(us, 1), us_min=round(lo, 1), us_max=round(hi, 1), bytes=int(nbytes), tbps=round(nbytes / us / 1e6, 3),
                   copy_us=round(copy_us(nbytes), 1), **extra)
        rows.append(rec)
        print(json.dumps(rec), flush=True)
        return rec

    copies = {}

    def copy_us(nbytes):
        n = max(int(nbytes) // 2, 1)
        if n not in copies:
            src, dst = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
            copies[n] = timed(torch, lambda: dst.copy_(src))[0]
            del src, dst
        return copies[n]

    def plane(h, w, cover):
        scl = torch.full((h, w), 4, dtype=torch.uint8, device=dev)
        if cover > 0:
            field = F.interpolate(torch.rand((1, 1, h // 96 + 2, w // 96 + 2), generator=g, device=dev), size=(h, w), mode="bicubic",
                                  align_corners=False)[0, 0]
            cut = torch.quantile(field[::7, ::7].flatten(), 1.0 - cover)
            scl[field > cut] = 9
        return scl

    planes10 = {name: plane(H, W, c) for name, c in COVERS}
    planes20 = {name: planes10[name][::2, ::2].contiguous() for name, _ in COVERS}

    # ---- class counts ---------------------------------------------------------------------------------------------------------------
    counts = torch.empty((1, 1, 16), dtype=torch.int32, device=dev)
    for tag, p in (("20m", planes20["10"]), ("10m", planes10["10"])):
        h, w = p.shape
        us3 = timed(torch, lambda: nat.check(lib.hsr_scl_class_counts(_ptr(p), h, w, w, h, w, _ptr(counts), st)))
        ms = None
        if not a.no_host:
            host = p.cpu().numpy()
            ms, (vals, cnt) = wall(lambda: np.unique(host, return_counts=True))
            got = counts.cpu().numpy()[0, 0]
            assert all(got[v] == c for v, c in zip(vals, cnt)) and got.sum() == cnt.sum(), "counts differ from np.unique"
        record(f"counts_{tag}", us3, h * w, numpy_ms=ms, cloud_frac=round(float((p == 9).float().mean().item()), 4))

    # ---- the mask -------------------------------------------------------------------------------------------------------------------
    mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
    classes = torch.tensor([8, 9, 10], dtype=torch.uint8, device=dev)
    flats = torch.tensor([0, 1], dtype=torch.uint8, device=dev)
    for cover, _ in COVERS:
        p = planes10[cover]
        host = p.cpu().numpy() if not a.no_host else None
        for shape, code in (("disc", 0), ("square", 1)):
            for r in RADII:
                if r == 0 and shape == "square":
                    continue
                us3 = timed(torch, lambda: nat.check(lib.hsr_scl_mask(_ptr(p), H, W, W, GROW, FLAT, r, code, _ptr(mask), W, st)))
                extra = dict(masked_frac=round(float((mask != 0).float().mean().item()), 4), torch_us=None, numpy_ms=None)
                if host is not None and r == 5 and cover == "10":
                    ms, want = wall(lambda: numpy_dilate(host, r, shape == "disc"))
                    assert np.array_equal(want, mask.cpu().numpy()), f"NumPy differs from the kernel ({shape}, r={r})"
                    extra["numpy_ms"] = round(ms, 1)
                record(f"mask_{cover}_{shape}_r{r}", us3, 2 * H * W, **extra)

    # ---- coarse and apply -------------------------------------------------------------------------------------------------------------
    k = SCALE
    hc, wc = H // k, W // k
    clear = torch.empty((hc, wc), dtype=torch.uint8, device=dev)
    win = torch.empty((hc // TILE, wc // TILE), dtype=torch.int32, device=dev)
    cube = torch.empty((32, H, W), dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    for cover, _ in COVERS:
        p = planes10[cover]
        nat.check(lib.hsr_scl_mask(_ptr(p), H, W, W, GROW, FLAT, 5, 0, _ptr(mask), W, st))
        us3 = timed(torch, lambda: nat.check(lib.hsr_scl_coarse(_ptr(mask), H, W, W, k, 0, _ptr(clear), None, TILE, TILE, _ptr(win), st)))
        ms = None
        host = mask.cpu().numpy() if not a.no_host else None
        if host is not None:
            ms, want = wall(lambda: ((host[:hc * k, :wc * k] != 0).reshape(hc, k, wc, k).sum(axis=(1, 3)) == 0).astype(np.uint8))
            assert np.array_equal(want, clear.cpu().numpy()), "coarse differs from NumPy"
            assert np.array_equal((1 - want[:hc // TILE * TILE, :wc // TILE * TILE].astype(np.int64)).reshape(hc // TILE, TILE, wc // TILE, TILE).sum(axis=(1, 3)),
                                  win.cpu().numpy()), "the window counts differ from NumPy"
        record(f"coarse_{cover}", us3, H * W, numpy_ms=ms, clear_frac=round(float(clear.float().mean().item()), 4))
        cube.normal_(generator=g)
        us3 = timed(torch, lambda: nat.check(lib.hsr_scl_apply(_ptr(cube), 32, H, W, H * W, W, _ptr(mask), H, W, W, 1, float("nan"), _ptr(count), st)))
        n = int(count.item())
        assert n == int((mask != 0).sum().item()) and int(torch.isnan(cube[31]).sum().item()) == n
        ms = None
        if host is not None:
            part = cube[:4].cpu().numpy()
            part[np.isnan(part)] = 0.5
            ms, _ = wall(lambda: part.__setitem__((slice(None), host != 0), np.float32(np.nan)))
            del part
        record(f"apply_{cover}", us3, H * W + 4 * 32 * n, numpy_ms=ms, numpy_bands=4, filled_frac=round(n / (H * W), 4))
    del cube

    # ---- the two drivers ------------------------------------------------------------------------------------------------------------------
    fuse = []
    if not a.no_fuse:
        emit = torch.rand(EMIT_SHAPE, generator=g, device=dev) * 0.6 + 0.02
        s2 = torch.randint(1, 4000, S2_SHAPE, generator=g, device=dev, dtype=torch.int16).view(torch.uint16)
        kw = dict(tile=TILE, factor=SCALE, batch=64, bands=32, emit_nodata=NODATA, s2_nodata=0.0)
        for step, fn in (("fuse_scene", lambda: s2_emit.fuse_scene(emit, s2, **kw)),
                         ("fuse_scene_clear", lambda: s2_emit.fuse_scene_clear(emit, s2, planes20["10"], buffer=2, **kw))):
            res = fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(3):
                del res
                t = time.perf_counter()
                res = fn()
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t) * 1e3)
            ms.sort()
            rec = dict(step=step, ms=round(ms[1], 2), ms_min=round(ms[0], 2), ms_max=round(ms[2], 2), tiles=len(res.tiles),
                       status_ok=int((res.status == 0).sum().item()), n_train_mean=round(float(res.n_train.float().mean().item()), 1),
                       nan_frac=round(float(torch.isnan(res.cube[0]).float().mean().item()), 4))
            fuse.append(rec)
            print(json.dumps(rec), flush=True)
            del res

    def us_of(step):
        return next(r["us"] for r in rows if r["step"] == step)

    verdict = dict(step="early_exit", **{f"{s}_r{r}": round(us_of(f"mask_60_{s}_r{r}") / us_of(f"mask_clear_{s}_r{r}"), 2)
                                         for s in ("disc", "square") for r in RADII[1:]})
    print(json.dumps(verdict), flush=True)

    def write_markdown():
        if not a.markdown:
            return
        with open(a.markdown, "w") as fh:
            fh.write("| step | us (median) | min .. max | bytes moved | TB/s | copy of the same bytes, us | x copy | torch, us | NumPy, ms | note |\n")
            fh.write("|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                note = ", ".join(f"{key} {r[key]}" for key in ("cloud_frac", "masked_frac", "clear_frac", "filled_frac") if key in r)
                if r.get("numpy_bands") and r.get("numpy_ms") is not None:
                    note += ", NumPy on 4 of the 32 bands"
                tch = "" if r.get("torch_us") is None else f"{r['torch_us']}"
                npy = "" if r.get("numpy_ms") is None else f"{r['numpy_ms']:.0f}"
                fh.write(f"| {r['step']} | {r['us']} | {r['us_min']} .. {r['us_max']} | {r['bytes'] / 1e6:.1f} MB | {r['tbps']} | {r['copy_us']} | "
                         f"{r['us'] / max(r['copy_us'], 1e-9):.1f} | {tch} | {npy} | {note} |\n")
            fh.write("\n" + "\n\n".join(f"{r['step']}: {json.dumps(r)}" for r in fuse) + f"\n\nearly exit, 60 % cloud over clear sky: {json.dumps(verdict)}\n")

    write_markdown()
    # ---- the torch forms of the mask, last: whatever they take, the tables above are written ---------------------------------------------
    if not a.no_torch:
        p = planes10["10"]
        for shape, code in (("disc", 0), ("square", 1)):
            for r in (5, 15):
                nat.check(lib.hsr_scl_mask(_ptr(p), H, W, W, GROW, FLAT, r, code, _ptr(mask), W, st))
                if shape == "square":
                    form = lambda: (F.max_pool2d(torch.isin(p, classes).half()[None, None], 2 * r + 1, 1, r)[0, 0] > 0) | torch.isin(p, flats)  # noqa: E731
                else:
                    yy, xx = torch.meshgrid(torch.arange(-r, r + 1, device=dev), torch.arange(-r, r + 1, device=dev), indexing="ij")
                    disc = ((yy * yy + xx * xx) <= r * r).float()[None, None]
                    form = lambda: (F.conv2d(torch.isin(p, classes).float()[None, None], disc, padding=r)[0, 0] > 0.5) | torch.isin(p, flats)  # noqa: E731
                assert torch.equal(form().to(torch.uint8), mask), f"the torch form differs from the kernel ({shape}, r={r})"
                row = next(x for x in rows if x["step"] == f"mask_10_{shape}_r{r}")
                row["torch_us"] = round(timed(torch, form, 1)[0], 1)
                print(json.dumps(dict(step=row["step"], torch_us=row["torch_us"])), flush=True)
                write_markdown()



if __name__ == "__main__":
    main()
