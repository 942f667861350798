"""Benchmark of the affine colour kernels (csrc/hsr_color.hip) and of match_pair(model="affine"), to be run by hand on an MI355X.

    python tools/bench_affine.py                          # every row; one JSON line each
    python tools/bench_affine.py --markdown FILE          # and the table of profiles/r16_affine.md

Kernel rows, at 1024 x 1024 and 6144 x 6144 pixels (the 60 m and the 10 m image of one full tile), padded rows (npix, 4) and planar
(3, npix), inputs built on the device from a seed, mask 85 % set, both stretches on:
    affine_moments   hsr_affine_moments (+ nothing else: the reduce + solve is a row of its own)
    affine_apply     hsr_affine_apply, clip_mode 2, stretch, mask, output preallocated
    yardsticks       the parent's own kernels on the SAME buffers: hsr_poly_moments (deg 4, 3 bands, mask, both stretches) and
                     hsr_poly_apply (deg 4, stretch, mask, clip) - the polynomial form of the same step
Per row: us = the median over SAMPLES samples of REPS back-to-back launches between two device events after WARMUP launches, with
the fastest and slowest sample; bytes = what the algorithm has to move (moments: 2 images x 12 or 16 B per pixel + 1 mask byte;
apply: image in + image out + mask), tbps = bytes / us.  A padded row's pad float is counted: the 16-byte load fetches it.
Driver rows: match_pair on a 1024 x 1024 x 285 cube and a 6144 x 6144 x 3 uint8 image (HW=170 gives the 1020 x 1020 image of the
small size), model "affine" against "poly" (deg 4), for both fits, wall clock round a synchronise, median of 5 after one warm-up,
the two models alternating in the same process.
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

SAMPLES, REPS, WARMUP = 7, 10, 3
SIZES = (1024, 6144)


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


def kernel_rows(torch, side):
    from s2_emit import _engine as eng, _native as nat
    npix = side * side
    gen = torch.Generator(device="cuda").manual_seed(16)
    rows = []
    mask = (torch.rand(npix, device="cuda", generator=gen) < 0.85).to(torch.uint8)
    lohi_x = torch.tensor([[0.05, 0.9], [0.1, 1.05], [-0.05, 0.8]], dtype=torch.float64, device="cuda")
    lohi_y = torch.tensor([[0.0, 0.95], [0.08, 0.9], [0.02, 1.1]], dtype=torch.float64, device="cuda")
    At = torch.tensor([0.8, 0.1, -0.05, 0.15, 0.7, 0.1, -0.1, 0.2, 0.9, 0.03, -0.02, 0.05], dtype=torch.float64, device="cuda")
    coeffs = torch.tensor([[0.1, -0.2, 0.3, 0.8, 0.01]] * 3, dtype=torch.float64, device="cuda")
    aws, pws = eng.AffineWorkspace("cuda"), eng.MomentWorkspace("cuda", 3, 4)
    for layout, shape, per_px in ((nat.PIXMAJOR, (npix, 4), 16), (nat.PLANAR, (3, npix), 12)):
        x = torch.rand(shape, device="cuda", generator=gen) * 1.3 - 0.15
        y = torch.rand(shape, device="cuda", generator=gen)
        out = torch.empty_like(x)
        tag = f"{side} x {side}, {'padded rows' if layout == nat.PIXMAJOR else 'planar'}"
        mom_bytes, app_bytes = npix * (2 * per_px + 1), npix * (2 * per_px + 1)
        for name, fn, nbytes in (
                ("affine_moments", lambda: eng.affine_moments(x, y, aws, mask, lohi_x, lohi_y, layout), mom_bytes),
                ("poly_moments deg 4 (yardstick)", lambda: eng.poly_moments(x, y, 4, pws, mask, lohi_x=lohi_x, lohi_y=lohi_y, layout=layout, nb=3), mom_bytes),
                ("affine_apply", lambda: eng.affine_apply(x, At, mask, lohi_x, 2, layout, out=out), app_bytes),
                ("poly_apply deg 4 (yardstick)", lambda: eng.poly_apply(x, coeffs, mask, lohi_x, True, layout, out=out, nb=3), app_bytes)):
            us, lo, hi = timed(torch, fn)
            rows.append(dict(row=f"{name}, {tag}", us=us, lo=lo, hi=hi, bytes=nbytes, tbps=nbytes / us / 1e6))
        del x, y, out
    us, lo, hi = timed(torch, lambda: eng.affine_solve(aws, 200))
    rows.append(dict(row=f"affine_solve (reduce {aws.slots} slots + solve), after {side} x {side}", us=us, lo=lo, hi=hi, bytes=aws.slots * 176,
                     tbps=aws.slots * 176 / us / 1e6))
    return rows


def driver_rows(torch, hw):
    import s2_emit
    from s2_emit.synthetic import device_problem
    prob = device_problem(hw, hw, 285, deg=3, seed=0, device=torch.device("cuda", 0))
    rgb = prob.real.reshape(hw, hw, -1)[..., [2, 1, 0]].clamp(0, 1)
    s2 = (rgb.repeat_interleave(6, 0).repeat_interleave(6, 1) ** 0.8 * 255 + 4 * torch.randn(hw * 6, hw * 6, 3, device="cuda")).clamp(0, 255).to(torch.uint8)
    rows = []
    for use_ot in (False, True):
        ms = {"affine": [], "poly": []}
        for rep in range(6):
            for model in ("affine", "poly"):                                      # alternating, same process
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s2_emit.match_pair(prob.cube, prob.emit_w, prob.srf, prob.good_mask, s2, 6, deg=4, use_ot=use_ot, as_numpy=False, model=model)
                torch.cuda.synchronize()
                if rep:
                    ms[model].append((time.perf_counter() - t0) * 1e3)
        for model in ("affine", "poly"):
            v = sorted(ms[model])
            rows.append(dict(row=f"match_pair model={model}, use_ot={use_ot}, {hw} x {hw} EMIT / {hw * 6} x {hw * 6} S2", ms=v[len(v) // 2], lo=v[0], hi=v[-1]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markdown", default=None, help="write the result table to this file")
    ap.add_argument("--skip-driver", action="store_true", help="kernel rows only")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_affine.py measures on a GPU; there is no other path"
    torch.cuda.set_device(0)
    krows = [r for side in SIZES for r in kernel_rows(torch, side)]
    for r in krows:
        print(json.dumps(r), flush=True)
    drows = []
    if not a.skip_driver:
        for hw in (170, 1024):
            drows += driver_rows(torch, hw)
            torch.cuda.empty_cache()
        for r in drows:
            print(json.dumps(r), flush=True)
    if a.markdown:
        lines = ["# r16: cross-channel affine colour transfer (`csrc/hsr_color.hip`)", "",
                 "MI355X, one GPU, one process. Command: `python tools/bench_affine.py --markdown FILE`. Inputs, timing and the byte counts are "
                 f"described in the tool's docstring: the median of {SAMPLES} samples of {REPS} back-to-back launches between two device events "
                 f"after {WARMUP} warm-up launches; bytes = the images and the mask the step has to move. The yardstick rows are the polynomial "
                 "kernels of the same step on the same buffers.", "",
                 "| row | µs (median) | min .. max | bytes moved | TB/s |", "|---|---|---|---|---|"]
        for r in krows:
            lines.append(f"| {r['row']} | {r['us']:.1f} | {r['lo']:.1f} .. {r['hi']:.1f} | {r['bytes'] / 1e6:.1f} MB | {r['tbps']:.3f} |")
        if drows:
            lines += ["", "Driver, wall clock round a synchronise, median of 5 after one warm-up, the two models alternating:", "",
                      "| row | ms (median) | min .. max |", "|---|---|---|"]
            for r in drows:
                lines.append(f"| {r['row']} | {r['ms']:.2f} | {r['lo']:.2f} .. {r['hi']:.2f} |")
        with open(a.markdown, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
