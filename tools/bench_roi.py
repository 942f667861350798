"""Benchmark of the polygon family (include/hsr_roi.h, s2_emit.roi) at the sizes of a Sentinel-2 granule.

    python tools/bench_roi.py                          # every step; one JSON line each
    python tools/bench_roi.py --markdown FILE          # and the tables of profiles/r27_roi.md
    python tools/bench_roi.py --sizes 5490             # one plane size only

Polygons: "footprint", a 5-vertex rotated footprint whose bounding box is about half empty, and "circle", 1500 vertices.  Planes:
10980 x 10980 (10 m) and 5490 x 5490 (20 m).  Steps, each under the centre and the touched rule:
  rasterize_<poly>_<rule>_<n>   hsr_roi_rasterize of the whole plane (vertices already on the device);
                                copy_us: a device-to-device copy of the n x n bytes it writes.
  counts_<poly>_<rule>_<n>      hsr_roi_class_counts over the polygon's bounding window of a random SCL plane;
                                scl_us: hsr_scl_class_counts on that window - the rectangle, which reads the same bytes and answers
                                another question; torch_us: the torch form - a host-rasterised mask (the host twin's, not timed)
                                copied to the device, then torch.bincount(plane[mask]) - copy and count timed together.
  subset_<poly>                 hsr_roi_glt_clip + hsr_roi_glt_reindex on an 1800 x 2200 GLT (the chain of spatial_subset, device
                                events), and subset_call_us: s2_emit.spatial_subset itself, wall clock around a synchronise,
                                upload of the polygon included.
Per step: us, the median over SAMPLES samples of REPS back-to-back launches between two device events after WARMUP calls, with the
fastest and slowest sample.  Every device result is compared with the host twin (the counts with NumPy under the host twin's
mask): the bench exits non-zero on a difference.  Nothing is gated on a number.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "hyperspectral_super-resolution_amd"))

SAMPLES, REPS, WARMUP = 7, 3, 2
GLT_SHAPE, SWATH = (1800, 2200), (1280, 1242)
RULES = (("center", 0), ("touched", 1))


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
    return dict(us=us[len(us) // 2], us_min=us[0], us_max=us[-1])


def polygon(kind, H, W):
    """Pixel coordinates on an H x W grid with the identity geotransform."""
    if kind == "footprint":
        return np.array([[0.31 * W, 0.04 * H], [0.93 * W, 0.27 * H], [0.71 * W, 0.95 * H], [0.08 * W, 0.72 * H], [0.12 * W, 0.41 * H]]) + 0.137
    t = 2 * np.pi * np.arange(1500) / 1500
    return np.stack([W * (0.5 + 0.43 * np.cos(t)) + 0.137, H * (0.5 + 0.43 * np.sin(t)) + 0.137], axis=1)


def bbox(verts, H, W):
    c0, c1 = max(math.floor(verts[:, 0].min()), 0), min(math.floor(verts[:, 0].max()), W - 1)
    r0, r1 = max(math.floor(verts[:, 1].min()), 0), min(math.floor(verts[:, 1].max()), H - 1)
    return r0, c0, r1 - r0 + 1, c1 - c0 + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markdown")
    ap.add_argument("--sizes", type=int, nargs="*", default=[10980, 5490])
    args = ap.parse_args()
    import torch
    import s2_emit
    from s2_emit import _native as nat
    from s2_emit._engine import _stream
    lib = nat.load()
    dev = torch.device("cuda", 0)
    gt = (C.c_double * 6)(0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    gt_t = (0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    st = _stream(torch)
    rows, bad = [], 0

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for n in args.sizes:
        H = W = n
        rng = np.random.default_rng(n)
        plane_h = rng.integers(0, 12, (H, W), dtype=np.uint8)
        plane = torch.from_numpy(plane_h).to(dev)
        out = torch.empty((H, W), dtype=torch.uint8, device=dev)
        src = torch.empty((H, W), dtype=torch.uint8, device=dev)
        copy = timed(torch, lambda: out.copy_(src))
        for kind in ("footprint", "circle"):
            verts = np.ascontiguousarray(polygon(kind, H, W))
            offs = np.array([0, len(verts)], np.int32)
            V, O = torch.from_numpy(verts).to(dev), torch.from_numpy(offs).to(dev)
            win = bbox(verts, H, W)
            r0, c0, h, w = win
            for rule_name, rule in RULES:
                def raster():
                    nat.check(lib.hsr_roi_rasterize(V.data_ptr(), O.data_ptr(), 1, len(verts), gt, H, W, rule, 0, 0, H, W, 1, 0, out.data_ptr(), W, st))
                t = timed(torch, raster)
                host = np.empty((H, W), np.uint8)
                nat.check(lib.hsr_roi_rasterize_host(verts.ctypes.data, offs.ctypes.data, 1, len(verts), gt, H, W, rule, 0, 0, H, W, 1, 0,
                                                     host.ctypes.data, W))
                same = bool(np.array_equal(out.cpu().numpy(), host))
                bad += not same
                emit(dict(step=f"rasterize_{kind}_{rule_name}_{n}", **t, bytes=H * W, copy_us=copy["us"], copy_min=copy["us_min"],
                          copy_max=copy["us_max"], inside_frac=float(host.mean()), equals_host=same))
                res = torch.empty((17,), dtype=torch.int32, device=dev)

                def counts():
                    nat.check(lib.hsr_roi_class_counts(V.data_ptr(), O.data_ptr(), 1, len(verts), gt, H, W, rule, r0, c0, h, w, plane.data_ptr(), W,
                                                       res.data_ptr(), res.data_ptr() + 64, st))
                t = timed(torch, counts)
                mask_h = host[r0:r0 + h, c0:c0 + w].astype(bool)
                want = np.bincount(plane_h[r0:r0 + h, c0:c0 + w][mask_h], minlength=16)
                got = res.cpu().numpy()
                same = got[:16].tolist() == want.tolist() and int(got[16]) == int(mask_h.sum())
                bad += not same
                rect = torch.empty((16,), dtype=torch.int32, device=dev)
                sub = plane.data_ptr() + r0 * W + c0
                scl = timed(torch, lambda: nat.check(lib.hsr_scl_class_counts(sub, h, w, W, h, w, rect.data_ptr(), st)))
                pinned = torch.from_numpy(np.ascontiguousarray(mask_h))
                view = plane[r0:r0 + h, c0:c0 + w]

                def torch_form():
                    return torch.bincount(view[pinned.to(dev)].to(torch.int64), minlength=16)
                tt = timed(torch, torch_form, reps=1)
                same_t = torch_form().cpu().numpy().tolist() == want.tolist()
                emit(dict(step=f"counts_{kind}_{rule_name}_{n}", **t, window=list(win), bytes=h * w, inside=int(got[16]), scl_us=scl["us"],
                          scl_min=scl["us_min"], scl_max=scl["us_max"], torch_us=tt["us"], torch_min=tt["us_min"], torch_max=tt["us_max"],
                          equals_numpy=same, torch_equals_numpy=same_t))
    # spatial_subset
    GH, GW = GLT_SHAPE
    yy, xx = np.meshgrid(np.arange(GH), np.arange(GW), indexing="ij")
    glt_h = np.stack([1 + (xx * SWATH[1]) // GW, 1 + (yy * SWATH[0]) // GH], axis=-1).astype(np.int32)
    glt_h[np.random.default_rng(1).random((GH, GW)) < 0.2] = 0
    G = torch.from_numpy(glt_h).to(dev)
    for kind in ("footprint", "circle"):
        verts = np.ascontiguousarray(polygon(kind, GH, GW))
        offs = np.array([0, len(verts)], np.int32)
        V, O = torch.from_numpy(verts).to(dev), torch.from_numpy(offs).to(dev)
        r0, c0, h, w = bbox(verts, GH, GW)
        og = torch.empty((h, w, 2), dtype=torch.int32, device=dev)
        rec = torch.empty((8,), dtype=torch.int32, device=dev)

        def chain():
            nat.check(lib.hsr_roi_glt_clip(V.data_ptr(), O.data_ptr(), 1, len(verts), gt, GH, GW, G.data_ptr(), r0, c0, h, w, og.data_ptr(),
                                           rec.data_ptr(), st))
            nat.check(lib.hsr_roi_glt_reindex(og.data_ptr(), h, w, rec.data_ptr(), st))
        t = timed(torch, chain)
        hg, hrec = np.empty((h, w, 2), np.int32), np.empty(8, np.int32)
        nat.check(lib.hsr_roi_glt_clip_host(verts.ctypes.data, offs.ctypes.data, 1, len(verts), gt, GH, GW, glt_h.ctypes.data, r0, c0, h, w,
                                            hg.ctypes.data, hrec.ctypes.data))
        nat.check(lib.hsr_roi_glt_reindex_host(hg.ctypes.data, h, w, hrec.ctypes.data))
        same = bool(np.array_equal(og.cpu().numpy(), hg)) and rec.cpu().numpy().tolist() == hrec.tolist()
        bad += not same
        wall = []
        for _ in range(SAMPLES + WARMUP):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s2_emit.spatial_subset(G, gt_t, [verts])
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e6)
        wall = sorted(wall[WARMUP:])
        emit(dict(step=f"subset_{kind}", **t, window=[r0, c0, h, w], bytes=16 * h * w, record=hrec[:5].tolist(), subset_call_us=wall[len(wall) // 2],
                  subset_call_min=wall[0], subset_call_max=wall[-1], equals_host=same))
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write("| step | us (min - max) | bytes | comparators, us (min - max) | equal |\n|---|---|---|---|---|\n")
            for r in rows:
                span = lambda k, lo, hi: "%.1f (%.1f - %.1f)" % (r[k], r[lo], r[hi])  # noqa: E731
                if r["step"].startswith("rasterize"):
                    comp, eq = "copy " + span("copy_us", "copy_min", "copy_max"), r["equals_host"]
                elif r["step"].startswith("counts"):
                    comp = "scl rectangle " + span("scl_us", "scl_min", "scl_max") + "; torch " + span("torch_us", "torch_min", "torch_max")
                    eq = r["equals_numpy"] and r["torch_equals_numpy"]
                else:
                    comp, eq = "spatial_subset call " + span("subset_call_us", "subset_call_min", "subset_call_max"), r["equals_host"]
                f.write("| %s | %s | %d | %s | %s |\n" % (r["step"], span("us", "us_min", "us_max"), r["bytes"], comp, "yes" if eq else "NO"))
    if bad:
        print(f"{bad} device results differ from the host twin", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
