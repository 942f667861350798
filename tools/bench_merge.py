"""Benchmark of the scene-merging family (include/hsr_merge.h, s2_emit.merge) at the size of EMIT scenes.

    python tools/bench_merge.py                      # every step; one JSON line each
    python tools/bench_merge.py --markdown FILE      # and the table of profiles/r26_merge.md
    python tools/bench_merge.py --small              # swaths of 128 x 124 x 285: a rehearsal of the tool, not a measurement

Two and three consecutive swaths of 1280 x 1242 x 285 float32, synthetic, built on the device from a seed.  Each has a lookup table
of 1408 x 1366 cells - the swath one to one in its middle, a border of no-data cells round it - and the tables overlap by 10 % of
their height on the union grid (merge_grid).  Both layouts, without masks and with a quality mask (5 % of the pixels) and a band
mask (36 bytes a pixel, 2 % of the bits) on every swath.  Per configuration, timed in the same process one after the other:
  ortho_merge      the N swaths straight onto the merged grid, ONE launch;
  chain            N x ortho_scene (into preallocated scenes) + merge_scenes: what ortho_merge replaces;
  merge_scenes     the last step of the chain alone;
  copy             a device-to-device copy of the merged scene's bytes.
us is the median over SAMPLES samples of REPS back-to-back calls between two device events after WARMUP calls, with the fastest and
slowest sample.  bytes is what a step has to move, from the shapes: ortho_merge reads the swath pixels it keeps and the tables and
writes the result once; the chain also writes the N scenes and reads them again.

The tool exits non-zero when ortho_merge's scene, dropped counts or source plane differ from the chain's by a bit.  Nothing is gated
on a time.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "hyperspectral_super-resolution_amd"))

SAMPLES, REPS, WARMUP = 5, 3, 2
BANDS, BMASK_BYTES = 285, 36


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markdown", default=None, help="write the result table to this file")
    ap.add_argument("--small", action="store_true", help="swaths of 128 x 124: a rehearsal, not a measurement")
    a = ap.parse_args()
    import torch
    import s2_emit
    assert torch.cuda.is_available(), "bench_merge needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device="cuda").manual_seed(26)
    rows_, cols_ = (128, 124) if a.small else (1280, 1242)
    my, mx = rows_ // 20, cols_ // 20                                     # the no-data border of a table
    gh, gw = rows_ + 2 * my, cols_ + 2 * mx
    step_y = gh - gh // 10                                                 # 10 % overlap
    gt = lambda k: (500000.0 + 60.0 * 3 * k, 60.0, 0.0, 4100000.0 - 60.0 * step_y * k, 0.0, -60.0)  # noqa: E731
    rows, mismatches = [], []

    def swath(k):
        s = torch.rand((rows_, cols_, BANDS), generator=g, device=dev, dtype=torch.float32)
        s[:: 97, :: 89, :: 7] = -9999.0                                    # the producer's own no-data elements
        return s

    def table():
        t = torch.zeros((gh, gw, 2), dtype=torch.int32, device=dev)
        t[my: my + rows_, mx: mx + cols_, 0] = torch.arange(1, cols_ + 1, dtype=torch.int32, device=dev)[None, :]
        t[my: my + rows_, mx: mx + cols_, 1] = torch.arange(1, rows_ + 1, dtype=torch.int32, device=dev)[:, None]
        t[my + 3, mx: mx + 50, 0] = cols_ + 5                              # entries that leave the swath: dropped
        return t

    swaths = [swath(k) for k in range(3)]
    tables = [table() for _ in range(3)]
    qmasks = [(torch.rand((rows_, cols_), generator=g, device=dev) < 0.05).to(torch.uint8) for _ in range(3)]
    bmasks = []
    for _ in range(3):
        hit = torch.rand((rows_, cols_, BMASK_BYTES), generator=g, device=dev) < 0.16          # one bit in 16 % of the bytes: 2 % of the bits
        shift = torch.randint(0, 8, hit.shape, generator=g, device=dev, dtype=torch.int32)
        bmasks.append((hit.to(torch.int32) << shift).to(torch.uint8).contiguous())
        del hit, shift

    def record(cfg, step, us3, nbytes, **extra):
        us, lo, hi = us3
        rec = dict(config=cfg, step=step, us=round(us, 1), us_min=round(lo, 1), us_max=round(hi, 1), bytes=int(nbytes),
                   tbps=round(nbytes / us / 1e6, 3), **extra)
        rows.append(rec)
        print(json.dumps(rec), flush=True)
        return rec

    for n in (2, 3):
        grid = s2_emit.merge_grid([gt(k) for k in range(n)], [(gh, gw)] * n)
        H, W = grid.shape
        for layout in ("bsq", "bip"):
            for masks in (False, True):
                cfg = f"n{n}-{layout}-{'masks' if masks else 'plain'}"
                kw = dict(qmasks=qmasks[:n], band_masks=bmasks[:n]) if masks else {}
                shape = (BANDS, H, W) if layout == "bsq" else (H, W, BANDS)
                one = (BANDS, gh, gw) if layout == "bsq" else (gh, gw, BANDS)
                fused_out = torch.empty(shape, dtype=torch.float32, device=dev)
                chain_out = torch.empty(shape, dtype=torch.float32, device=dev)
                scenes = [torch.empty(one, dtype=torch.float32, device=dev) for _ in range(n)]
                res = {}

                def fused():
                    res["fused"] = s2_emit.ortho_merge(swaths[:n], tables[:n], grid=grid, layout=layout, source=True, out=fused_out, **kw)

                def chain():
                    res["one"] = [s2_emit.ortho_scene(swaths[k], tables[k], qmask=qmasks[k] if masks else None,
                                                      band_mask=bmasks[k] if masks else None, layout=layout, out=scenes[k]) for k in range(n)]
                    res["chain"] = s2_emit.merge_scenes(scenes, grid=grid, layout=layout, source=True, out=chain_out)

                def merge_only():
                    s2_emit.merge_scenes(scenes, grid=grid, layout=layout, source=True, out=chain_out)

                scene_bytes = H * W * BANDS * 4
                kept = n * rows_ * cols_ * BANDS * 4                       # every swath pixel is looked up once by its table
                tables_bytes = n * gh * gw * 8
                t_fused = record(cfg, "ortho_merge", timed(torch, fused), kept + tables_bytes + scene_bytes)
                t_chain = record(cfg, "chain", timed(torch, chain), kept + tables_bytes + 2 * n * gh * gw * BANDS * 4 + scene_bytes)
                record(cfg, "merge_scenes", timed(torch, merge_only), n * gh * gw * BANDS * 4 + scene_bytes)
                record(cfg, "copy", timed(torch, lambda: chain_out.copy_(fused_out)), 2 * scene_bytes)
                fused(), chain()
                torch.cuda.synchronize()
                same = (torch.equal(fused_out.view(torch.int32), chain_out.view(torch.int32))
                        and torch.equal(res["fused"].source, res["chain"].source)
                        and res["fused"].dropped.tolist() == [int(o.dropped) for o in res["one"]])
                filled = float((res["fused"].source != 255).float().mean().item())
                print(json.dumps(dict(config=cfg, fused_vs_chain="equal" if same else "DIFFERS", grid=[H, W], covered=round(filled, 4),
                                      dropped=res["fused"].dropped.tolist(), chain_over_fused=round(t_chain["us"] / t_fused["us"], 3))), flush=True)
                for r in rows[-4:]:
                    r["equal"] = "equal" if same else "DIFFERS"
                if not same:
                    mismatches.append(cfg)
                del fused_out, chain_out, scenes, res
                torch.cuda.empty_cache()

    if a.markdown:
        with open(a.markdown, "w") as fh:
            fh.write("| configuration | step | us (median) | min .. max | bytes moved | TB/s | ortho_merge vs chain |\n|---|---|---|---|---|---|---|\n")
            for r in rows:
                fh.write(f"| {r['config']} | {r['step']} | {r['us']} | {r['us_min']} .. {r['us_max']} | {r['bytes'] / 1e6:.1f} MB | {r['tbps']} | "
                         f"{r['equal']} |\n")
    if mismatches:
        print(json.dumps(dict(error="ortho_merge differs from the chain", configs=mismatches)), flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
