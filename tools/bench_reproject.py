"""Benchmark of the reprojection stages (include/hsr_reproject.h, s2_emit/reproject.py) at the size of a real EMIT scene.

    python tools/bench_reproject.py                          # every row; one JSON line each
    python tools/bench_reproject.py --markdown FILE          # and the table of profiles/r21_reproject.md

Inputs (synthetic, built on the device from a seed): a 285 x 1800 x 2200 float32 scene on a geographic grid of 0.000542 degree
cells whose top-left corner lies at 34.9 N, 118.0 W - first without an invalid sample, then with a masked (-9999) border strip
and 0.2 % scattered masked pixels (of which nearly every wave of 64 output pixels meets one); the target
is the grid `utm_target_grid` gives for a Sentinel-2 tile of UTM zone 11 N (10980 x 10980 pixels of 10 m) laid over it.
Rows: the coordinate launch; the remap under both sample rules through both instances (the staged one under the bound
reproject_scene derives, the direct one under a bound of 64) on a preallocated output; reproject_scene as a whole (out=
preallocated; the field is allocated by the call).  Per row: us, the median over SAMPLES samples of REPS back-to-back calls between
two device events, after warm-up, with the fastest and slowest sample.
Yardsticks from the same process: a device-to-device copy that moves as many bytes as the remap must (the touched box of the
source, read once, plus the output, written once: half of that is copied, so read + write equal it); and hsr_coreg_warp (the same
cubic with its per-band geometry) on a float32 scene of the output's shape, in ns per output sample.
The field of the kernel is compared with the NumPy float64 restatement (s2_emit.tm_inverse) on the whole grid.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "hyperspectral_super-resolution_amd"))

BANDS, HS, WS = 285, 1800, 2200
CELL = 0.000542
SRC_GT = (-118.0, CELL, 0.0, 34.9, 0.0, -CELL)
EPSG, S2_SHAPE = 32611, (10980, 10980)
SAMPLES, REPS, WARMUP = 5, 3, 2


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markdown", default=None, help="write the result table to this file")
    ap.add_argument("--bands", type=int, default=BANDS, help="bands of the scene (default: 285)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import s2_emit
    from s2_emit import _engine as eng
    from s2_emit import _native as nat
    torch.cuda.set_device(0)
    bands = a.bands
    E, N = s2_emit.tm_forward(SRC_GT[0], SRC_GT[3], s2_emit.utm_params(EPSG))
    s2gt = (60.0 * math.floor(float(E) / 60.0) - 1200.0, 10.0, 0.0, 60.0 * math.ceil(float(N) / 60.0) + 1200.0, 0.0, -10.0)
    grid = s2_emit.utm_target_grid(SRC_GT, (HS, WS), EPSG, s2gt, S2_SHAPE)
    rows_o, cols_o = grid[4:]
    gen = torch.Generator(device="cuda").manual_seed(21)
    src = torch.rand((bands, HS, WS), device="cuda", generator=gen)
    out = torch.empty((bands, rows_o, cols_o), dtype=torch.float32, device="cuda")
    coords = torch.empty((rows_o, cols_o, 2), dtype=torch.float64, device="cuda")
    counts, status = torch.empty(2, dtype=torch.int64, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    results = []

    def row(name, t, nbytes=0, **kw):
        results.append(dict(row=name, us=t[0], lo=t[1], hi=t[2], bytes=nbytes, **kw))

    # the coordinate launch, and its field against the NumPy restatement
    t = timed(torch, lambda: s2_emit.reproject_coords(grid, EPSG, SRC_GT, out=coords))
    left, _, _, top = grid[:4]
    EE, NN = np.meshgrid(left + (np.arange(cols_o) + 0.5) * 60.0, top - (np.arange(rows_o) + 0.5) * 60.0)
    lon, lat = s2_emit.tm_inverse(EE, NN, s2_emit.utm_params(EPSG))
    sx, sy = (lon - SRC_GT[0]) / CELL - 0.5, (lat - SRC_GT[3]) / -CELL - 0.5
    field = coords.cpu().numpy()
    err = float(max(np.abs(field[..., 0] - sy).max(), np.abs(field[..., 1] - sx).max()))
    row(f"hsr_reproject_coords, {rows_o} x {cols_o} cells", t, coords.numel() * 8, coord_err_px=err, bar_px=256 * float(np.spacing(180.0)) / CELL)
    # the bytes the remap must move: the touched box of the source and the output
    inside = (sy >= 0) & (sy <= HS - 1) & (sx >= 0) & (sx <= WS - 1)
    y0, y1 = max(int(sy[inside].min()) - 1, 0), min(int(sy[inside].max()) + 2, HS - 1)
    x0, x1 = max(int(sx[inside].min()) - 1, 0), min(int(sx[inside].max()) + 2, WS - 1)
    must = bands * ((y1 - y0 + 1) * (x1 - x0 + 1) + rows_o * cols_o) * 4
    half = torch.empty(must // 8, dtype=torch.float32, device="cuda")
    half2 = torch.empty_like(half)
    t_copy = timed(torch, lambda: half2.copy_(half))
    row("device-to-device copy moving the remap's bytes (yardstick)", t_copy, must)
    del half, half2
    # the footprint bound reproject_scene derives
    e2 = (2.0 - 1.0 / 298.257223563) / 298.257223563
    metres = math.pi * 6378137.0 / 180.0
    cos_lat = math.cos(math.radians(max(abs(SRC_GT[3]), abs(SRC_GT[3] - CELL * HS))))
    mf = 1.25 * 60.0 / min(CELL * metres * cos_lat, CELL * metres * (1.0 - e2))
    # a scene without one invalid sample: every pixel takes the remap's short path
    for inst, bound in (("LDS", mf), ("DIRECT", 64.0)):
        t = timed(torch, lambda: eng.reproject_warp(src, coords, -9999.0, nat.HSR_REPROJECT_RENORM, bound, -9999.0, out, counts, status))
        row(f"hsr_reproject_warp<{inst}, RENORM>, a scene without invalid samples", t, must, of_copy=t_copy[0] / t[0],
            counts=counts.cpu().numpy().tolist(), status=int(status.item()), ns_per_sample=t[0] * 1e3 / out.numel())
    # the masked scene: a border strip and 0.2 % scattered pixels, the same in every band
    src[:, :, :60] = -9999.0
    src[:, :40, :] = -9999.0
    src.masked_fill_(torch.rand((1, HS, WS), device="cuda", generator=gen) < 0.002, -9999.0)
    for inst, bound in (("LDS", mf), ("DIRECT", 64.0)):
        for rule, code in (("STRICT", nat.HSR_REPROJECT_STRICT), ("RENORM", nat.HSR_REPROJECT_RENORM)):
            t = timed(torch, lambda: eng.reproject_warp(src, coords, -9999.0, code, bound, -9999.0, out, counts, status))
            c = counts.cpu().numpy().tolist()
            row(f"hsr_reproject_warp<{inst}, {rule}>, max_footprint {bound:.3g}", t, must, of_copy=t_copy[0] / t[0], counts=c,
                status=int(status.item()), ns_per_sample=t[0] * 1e3 / out.numel())
    t = timed(torch, lambda: s2_emit.reproject_scene(src, SRC_GT, epsg=EPSG, s2_geotransform=s2gt, s2_shape=S2_SHAPE, out=out))
    row("reproject_scene (coords + remap, renorm)", t, must, of_copy=t_copy[0] / t[0], ns_per_sample=t[0] * 1e3 / out.numel())
    # hsr_coreg_warp on a scene of the output's shape: the same cubic, geometry recomputed per band
    del src
    scene = torch.rand((bands, rows_o, cols_o), device="cuda", generator=gen)
    model = torch.tensor([0.4, 0.002, -0.001, -0.7, 0.001, 0.002, 0.5 * (cols_o - 1), 0.5 * (rows_o - 1), 100.0, 1.0], dtype=torch.float64,
                         device="cuda")
    t = timed(torch, lambda: eng.coreg_warp(scene, model, float("nan"), 13.0, 0.05, None, out))
    row("hsr_coreg_warp, float32, a scene of the output's shape (yardstick)", t, 2 * scene.numel() * 4, ns_per_sample=t[0] * 1e3 / out.numel())
    for r in results:
        r["tbps"] = r["bytes"] / r["us"] / 1e6
        print(json.dumps(r))
    if a.markdown:
        lines = ["# r21: an EMIT scene onto the Sentinel-2 UTM grid (`hsr_reproject_*`)", "",
                 "MI355X, one GPU, one process. Command: `python tools/bench_reproject.py --markdown FILE`. Inputs and timing are described "
                 f"in the tool's docstring: source {bands} × {HS} × {WS} float32 on a {CELL}° grid, output {bands} × {rows_o} × {cols_o} "
                 f"on the 60 m lattice of UTM zone 11 N; the median of {SAMPLES} samples of {REPS} back-to-back calls between two device "
                 f"events after {WARMUP} warm-up calls. The remap's bytes are the touched box of the source ({y1 - y0 + 1} × {x1 - x0 + 1}) "
                 "read once plus the output written once.", "",
                 "| row | µs (median) | min .. max | TB/s | note |", "|---|---|---|---|---|"]
        for r in results:
            note = []
            if "of_copy" in r:
                note.append(f"{100 * r['of_copy']:.0f} % of the copy's rate")
            if "ns_per_sample" in r:
                note.append(f"{r['ns_per_sample']:.4f} ns per output sample")
            if "counts" in r:
                note.append(f"counts {r['counts']}, status {r['status']}")
            if "coord_err_px" in r:
                note.append(f"worst |Δ| against the NumPy float64 restatement {r['coord_err_px']:.3g} px (bar {r['bar_px']:.3g} px)")
            lines.append(f"| {r['row']} | {r['us']:.1f} | {r['lo']:.1f} .. {r['hi']:.1f} | {r['tbps']:.3f} | {'; '.join(note)} |")
        with open(a.markdown, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
