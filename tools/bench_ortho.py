"""Benchmark of s2_emit.ortho_scene (hsr_ortho_glt: EMIT swath -> orthorectified scene) at the size of a real granule.

    python tools/bench_ortho.py                          # every row; one JSON line each
    python tools/bench_ortho.py --markdown FILE          # and the table of profiles/r14_ortho.md

Inputs (synthetic, built on the device from a seed): a 1280 x 1242 x 285 float32 swath (1.8 GB); a lookup table of 1800 x 2200
cells for a footprint rotated by 20 degrees on a grid 1.22 x finer than the swath (so neighbouring cells repeat swath pixels, as a
real GLT does), no data outside the footprint; a quality mask with 10 % ones and a 36-byte packed band mask with 2 % of the bits
set.  Rows: both layouts, without and with both masks, and a window of 1800 x 1830 cells (the width of a Sentinel-2 tile at 60 m).
Per row: us, the median over SAMPLES samples of REPS back-to-back launches between two device events, after warm-up, with the
fastest and slowest sample (the output is preallocated: out=); bytes = the window's GLT entries + the distinct spectra it
references x 1140 + the output written (the masks' bytes are not counted); tbps = bytes / us.
Two yardsticks from the same process: hsr_probe_read mode 1 over the swath (a plain 16-byte-per-lane streaming read: what an
ordinary kernel reads on this device), and the torch form a user would write today - torch.full, an advanced-index assignment
through the valid cells, permute().contiguous() for bsq - timed by wall clock round a synchronise (boolean indexing synchronises
by itself), median of 5.  The torch result and the kernel's are compared in the same run (int32 views, torch.equal).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "hyperspectral_super-resolution_amd"))

ROWS, COLS, BANDS, GH, GW, BMASK_BYTES = 1280, 1242, 285, 1800, 2200, 36
ANGLE_DEG, FINER = 20.0, 1.22
WINDOW = (0, 185, 1800, 1830)
SAMPLES, REPS, WARMUP = 7, 10, 3
FILL = -9999.0


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


def wall_us(torch, fn, n=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def make_glt(torch):
    """The one-based (column, row) table of a swath footprint rotated about the grid's centre; 0 outside it."""
    th = math.radians(ANGLE_DEG)
    Y, X = torch.meshgrid(torch.arange(GH, device="cuda", dtype=torch.float32) - GH / 2,
                          torch.arange(GW, device="cuda", dtype=torch.float32) - GW / 2, indexing="ij")
    u = (math.cos(th) * X + math.sin(th) * Y) / FINER + COLS / 2
    v = (-math.sin(th) * X + math.cos(th) * Y) / FINER + ROWS / 2
    sx, sy = torch.floor(u).to(torch.int32), torch.floor(v).to(torch.int32)
    inside = (sx >= 0) & (sx < COLS) & (sy >= 0) & (sy < ROWS)
    glt = torch.stack([torch.where(inside, sx + 1, 0), torch.where(inside, sy + 1, 0)], dim=-1).to(torch.int32).contiguous()
    return glt, inside


def torch_form(torch, swath, glt, layout):
    out = torch.full((glt.shape[0], glt.shape[1], swath.shape[2]), FILL, dtype=torch.float32, device=swath.device)
    valid = (glt != 0).all(dim=-1)
    g = glt[valid].to(torch.int64) - 1
    out[valid] = swath[g[:, 1], g[:, 0]]
    return out.permute(2, 0, 1).contiguous() if layout == "bsq" else out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markdown", default=None, help="write the result table to this file")
    a = ap.parse_args()
    import torch
    import s2_emit
    from s2_emit import _native as nat
    from s2_emit._engine import _stream
    torch.cuda.set_device(0)
    lib = nat.load()
    gen = torch.Generator(device="cuda").manual_seed(14)
    swath = torch.rand((ROWS, COLS, BANDS), device="cuda", generator=gen) * 0.55 + 0.05
    glt, inside = make_glt(torch)
    qmask = (torch.rand((ROWS, COLS), device="cuda", generator=gen) < 0.10).to(torch.uint8)
    bits = torch.rand((ROWS, COLS, BMASK_BYTES, 8), device="cuda", generator=gen) < 0.02
    weights = torch.tensor([128, 64, 32, 16, 8, 4, 2, 1], device="cuda", dtype=torch.int32)
    bmask = (bits.to(torch.int32) * weights).sum(dim=-1).to(torch.uint8).contiguous()
    del bits
    valid_frac = float(inside.float().mean())

    def distinct(win):
        r0, c0, h, w = win
        g = glt[r0:r0 + h, c0:c0 + w].reshape(-1, 2).to(torch.int64)
        g = g[(g != 0).all(dim=-1)]
        return int(torch.unique(g[:, 1] * (COLS + 1) + g[:, 0]).numel()), int(g.shape[0])

    rows, lines = [], []
    full = (0, 0, GH, GW)
    probe_sink = torch.zeros(64, dtype=torch.float32, device="cuda")
    nbytes = swath.numel() * 4 // 16 * 16
    st = _stream(torch)
    us, lo, hi = timed(torch, lambda: nat.check(lib.hsr_probe_read(C.c_void_p(swath.data_ptr()), nbytes, 1, C.c_void_p(probe_sink.data_ptr()), st)))
    rows.append(dict(row="hsr_probe_read mode 1 over the swath (yardstick)", us=us, lo=lo, hi=hi, bytes=nbytes))
    for layout in ("bip", "bsq"):
        for masks in (False, True):
            for win in ((full, "whole grid"), (WINDOW, "window 1800 x 1830")) if not masks else ((full, "whole grid"),):
                (r0, c0, h, w), label = win
                shape = (h, w, BANDS) if layout == "bip" else (BANDS, h, w)
                out = torch.empty(shape, dtype=torch.float32, device="cuda")
                kw = dict(qmask=qmask, band_mask=bmask) if masks else {}
                fn = lambda: s2_emit.ortho_scene(swath, glt, window=win[0], layout=layout, out=out, **kw)   # noqa: E731
                us, lo, hi = timed(torch, fn)
                nd, nvalid = distinct(win[0])
                moved = h * w * 8 + nd * BANDS * 4 + h * w * BANDS * 4
                rows.append(dict(row=f"ortho_scene {layout}, {'both masks' if masks else 'no mask'}, {label}", us=us, lo=lo, hi=hi,
                                 bytes=moved, valid=nvalid, distinct=nd, dropped=int(fn().dropped)))
                del out
        ref = torch_form(torch, swath, glt, layout)
        got = s2_emit.ortho_scene(swath, glt, layout=layout).scene
        same = bool(torch.equal(ref.view(torch.int32), got.view(torch.int32)))
        del ref, got
        us, lo, hi = wall_us(torch, lambda: torch_form(torch, swath, glt, layout))
        nd, nvalid = distinct(full)
        rows.append(dict(row=f"torch form {layout} (full, index assign{', permute().contiguous()' if layout == 'bsq' else ''}), whole grid",
                         us=us, lo=lo, hi=hi, bytes=GH * GW * 8 + nd * BANDS * 4 + GH * GW * BANDS * 4, same_bits_as_kernel=same))
    for r in rows:
        r["tbps"] = r["bytes"] / r["us"] / 1e6
        print(json.dumps(r))
    if a.markdown:
        lines += ["# r14: EMIT swath -> orthorectified scene (`hsr_ortho_glt`)", "",
                  "MI355X, one GPU, one process. Command: `python tools/bench_ortho.py --markdown FILE`. Inputs, timing and the byte "
                  "count are described in the tool's docstring: a 1280 × 1242 × 285 float32 swath, a synthetic lookup table of a rotated "
                  f"footprint, the median of {SAMPLES} samples of {REPS} back-to-back launches between two device events after {WARMUP} "
                  "warm-up launches (torch form: wall clock round a synchronise, median of 5); bytes = GLT entries + distinct spectra "
                  "referenced + output written.", ""]
        lines.append("| row | µs (median) | min .. max | bytes moved | TB/s |")
        lines.append("|---|---|---|---|---|")
        for r in rows:
            lines.append(f"| {r['row']} | {r['us']:.1f} | {r['lo']:.1f} .. {r['hi']:.1f} | {r['bytes'] / 1e6:.1f} MB | {r['tbps']:.3f} |")
        kern = {r["row"]: r for r in rows}
        note = [f"GLT: {GH} x {GW} cells, {100 * valid_frac:.1f} % valid; whole grid: {rows[1]['valid']} valid cells on "
                f"{rows[1]['distinct']} distinct swath pixels of {ROWS * COLS}.",
                "torch form and kernel give the same bits: " +
                ", ".join(f"{k.split()[2]} {v['same_bits_as_kernel']}" for k, v in kern.items() if "same_bits_as_kernel" in v) + "."]
        with open(a.markdown, "w") as f:
            f.write("\n".join(lines) + "\n\n" + "\n".join(note) + "\n")


if __name__ == "__main__":
    main()
