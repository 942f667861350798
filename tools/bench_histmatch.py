"""Benchmark of the histogram-matching family (include/hsr_hist.h, s2_emit.color.histogram_match_rgb on GPU tensors).

    python tools/bench_histmatch.py                      # every configuration; one JSON line per row
    python tools/bench_histmatch.py --markdown FILE      # and the table of profiles/r24_histmatch.md
    python tools/bench_histmatch.py --sizes 1024         # a subset of the sizes
    python tools/bench_histmatch.py --no-torch           # skip the torch form

Images (synthetic, built on the device from a seed): (H, W, 3) float32 at 1024 x 1024 and 6144 x 6144, pixel-major as match_pair
holds them.  `continuous`: both images uniform random; `ref8`: the reference is an 8-bit product over 255 (the S2 visual product), so
every reference value is a run of n / 256 samples and the lookup searches hi and lo.  Masks of 100 % and 60 %.
Rows per configuration:
  keys, pass0 .. pass3, lookup   the stages as the entries of the C ABI (hsr_hist_keys, hsr_hist_sort_pass, hsr_hist_lookup);
  match                          hsr_hist_match, the whole chain in one workspace;
  python                         s2_emit.histogram_match_rgb on the tensors (the workspace from torch's allocator);
  torch                          the same definition written with torch on the same device: boolean indexing (masked_select: a
                                 host synchronisation for the size), torch.sort, torch.searchsorted, float64 arithmetic, per channel.
                                 Its result is compared with the library's (equal by value, or the row says how many differ and the run exits non-zero);
  numpy                          at 1024 x 1024 only: the host function on NumPy arrays, by the host clock.
Per row: us, the median over SAMPLES samples of REPS back-to-back calls between two device events after WARMUP calls, with the
fastest and slowest sample; bytes, what the stage has to stream (keys: both images and the mask in, 6 planes out; a pass: 6 planes in
twice - count and scatter - and out once; lookup: both images and the mask in, the image out; the searches are not counted); copy_us, a
device-to-device copy in the same process that moves the same number of bytes (half read, half written).  Nothing is gated on a number.
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

SAMPLES, REPS, WARMUP = 5, 3, 2
C3 = 3


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


def torch_form(torch, src, ref, mask):
    """The definition of include/hsr_hist.h with torch operators, per channel; every masked sample finite."""
    out = src.clamp(0.0, 1.0)
    for c in range(C3):
        sv, rv = src[..., c][mask], ref[..., c][mask]                   # the size of the result: a host synchronisation
        n = sv.numel()
        if n == 0:
            continue
        S, R = torch.sort(sv + 0.0)[0], torch.sort(rv + 0.0)[0]
        cs = torch.searchsorted(S, sv, right=True)
        a = R[cs - 1]
        hi, lo = torch.searchsorted(R, a, right=True), torch.searchsorted(R, a, right=False)
        b = R[(lo - 1).clamp(min=0)].double()
        nn = torch.tensor(float(n), dtype=torch.float64, device=src.device)   # a device tensor: by a Python scalar torch multiplies by 1 / n
        ad = a.double()
        res = ((ad - b) / (hi.double() / nn - lo.double() / nn)) * (cs.double() / nn - lo.double() / nn) + b
        res = torch.where((hi == cs) | (lo == 0), ad, res)
        out[..., c][mask] = res.float().clamp(0.0, 1.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markdown", default=None, help="write the result table to this file")
    ap.add_argument("--sizes", default="1024,6144", help="comma-separated image edges")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch form")
    a = ap.parse_args()
    import numpy as np
    import torch
    import s2_emit
    from s2_emit import _native as nat
    from s2_emit._engine import _ptr, _stream
    assert torch.cuda.is_available(), "bench_histmatch needs a GPU"
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = _stream(torch)
    rows, copies = [], {}

    def copy_us(nbytes):
        n = max(int(nbytes) // 2, 1)
        if n not in copies:
            s, d = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
            copies[n] = timed(torch, lambda: d.copy_(s))[0]
            del s, d
        return copies[n]

    def record(config, step, us3, nbytes=None, **extra):
        us, lo, hi = us3
        rec = dict(config=config, step=step, us=round(us, 1), us_min=round(lo, 1), us_max=round(hi, 1))
        if nbytes:
            cu = copy_us(nbytes)
            rec.update(bytes=int(nbytes), tbps=round(nbytes / us / 1e6, 3), copy_us=round(cu, 1), x_copy=round(us / cu, 2))
        rec.update(extra)
        rows.append(rec)
        print(json.dumps(rec), flush=True)
        return rec

    def write_markdown():
        if not a.markdown:
            return
        with open(a.markdown, "w") as fh:
            fh.write("| configuration | step | us (median) | min .. max | bytes streamed | TB/s | copy of the same bytes, us | x copy | note |\n")
            fh.write("|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                b = f"{r['bytes'] / 1e6:.1f} MB | {r['tbps']} | {r['copy_us']} | {r['x_copy']}" if "bytes" in r else " | | | "
                fh.write(f"| {r['config']} | {r['step']} | {r['us']} | {r['us_min']} .. {r['us_max']} | {b} | {r.get('note', '')} |\n")

    for edge in (int(v) for v in a.sizes.split(",")):
        npix = edge * edge
        g = torch.Generator(device="cuda").manual_seed(24 + edge)
        src = torch.rand((edge, edge, C3), generator=g, device=dev)
        refs = {"continuous": torch.rand((edge, edge, C3), generator=g, device=dev) ** 2,
                "ref8": torch.randint(0, 256, (edge, edge, C3), generator=g, device=dev).float() / 255.0}
        masks = {"mask100": torch.ones((edge, edge), dtype=torch.bool, device=dev),
                 "mask60": torch.rand((edge, edge), generator=g, device=dev) < 0.6}
        stride = lib.hsr_hist_plane_stride(npix)
        need = lib.hsr_hist_scratch_bytes(npix, C3)
        cbytes, pbytes = lib.hsr_hist_sort_bytes(npix, 2 * C3), lib.hsr_hist_pivot_bytes(npix, C3)
        work = torch.empty(need + 256, dtype=torch.uint8, device=dev)
        base = (work.data_ptr() + 255) & ~255
        planes = -(-2 * C3 * stride * 4 // 256) * 256
        keys, tmp, counters, pivots = base, base + planes, base + 2 * planes, base + 2 * planes + -(-cbytes // 256) * 256
        out, n_valid = torch.empty_like(src), torch.empty(C3, dtype=torch.int64, device=dev)
        img, plane_b = npix * C3 * 4, 2 * C3 * npix * 4
        for rname, ref in refs.items():
            for mname, mask in masks.items():
                cfg = f"{edge}x{edge}x3 {rname} {mname}"
                m8 = mask.view(torch.uint8).reshape(-1)
                images = (_ptr(src), 1, C3, _ptr(ref), 1, C3, _ptr(m8), npix, C3)
                f_keys = lambda: nat.check(lib.hsr_hist_keys(*images, keys, stride, _ptr(n_valid), st))  # noqa: E731
                f_match = lambda: nat.check(lib.hsr_hist_match(*images, _ptr(out), 1, C3, _ptr(n_valid), base, need, st))  # noqa: E731
                f_look = lambda: nat.check(lib.hsr_hist_lookup(keys, stride, _ptr(n_valid), pivots, pbytes, *images, _ptr(out), 1, C3, st))  # noqa: E731
                record(cfg, "keys", timed(torch, f_keys), 2 * img + npix + plane_b)
                # a pass is timed on what the passes before it left: keys -> tmp -> keys -> tmp -> keys, each pass repeated in place
                for p, (src_k, dst_k) in enumerate(((keys, tmp), (tmp, keys), (keys, tmp), (tmp, keys))):
                    f_pass = lambda: nat.check(lib.hsr_hist_sort_pass(src_k, dst_k, stride, npix, 2 * C3, p, counters, cbytes, st))  # noqa: E731
                    record(cfg, f"pass{p}", timed(torch, f_pass), 3 * plane_b)
                record(cfg, "lookup", timed(torch, f_look), 2 * img + npix + img)
                whole = record(cfg, "match", timed(torch, f_match), 2 * img + npix + plane_b + 4 * 3 * plane_b + 2 * img + npix + img,
                               note=f"n_valid {n_valid.tolist()}")
                got = out.clone()
                f_py = lambda: s2_emit.histogram_match_rgb(src, ref, mask)  # noqa: E731
                record(cfg, "python", timed(torch, f_py), note="histogram_match_rgb on the tensors, allocation included")
                assert torch.equal(f_py(), got), "the Python function differs from the C entry"
                write_markdown()
                if not a.no_torch:
                    f_torch = lambda: torch_form(torch, src, ref, mask)  # noqa: E731
                    us3 = timed(torch, f_torch, 1)
                    note = f"masked_select syncs with the host per channel; library / torch = {whole['us'] / us3[0]:.2f}"
                    t = f_torch()
                    diff = int(((t != got) & ~(t.isnan() & got.isnan())).sum().item())
                    note += "; equal to the library by value" if diff == 0 else f"; {diff} elements differ from the library"
                    record(cfg, "torch", us3, note=note)
                    if diff:                                # written into the table first, then the run fails
                        write_markdown()
                        raise SystemExit(f"{cfg}: {diff} elements of the torch form differ from the library")
                if edge <= 1024:
                    hs, hr, hm = src.cpu().numpy(), ref.cpu().numpy(), mask.cpu().numpy()
                    t0 = time.perf_counter()
                    hout = s2_emit.histogram_match_rgb(hs, hr, hm)
                    dt = (time.perf_counter() - t0) * 1e6
                    same = bool(np.array_equal(hout, got.cpu().numpy()))
                    record(cfg, "numpy", (dt, dt, dt), note=f"host function, one run by the host clock; equal to the library by value: {same}")
                write_markdown()
        del src, refs, masks, work, out


if __name__ == "__main__":
    main()
