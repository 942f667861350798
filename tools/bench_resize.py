"""Benchmark of the area-resampling family (include/hsr_resize.h, s2_emit.resize) at the sizes of a Sentinel-2 scene.

    python tools/bench_resize.py                      # every step; one JSON line each
    python tools/bench_resize.py --markdown FILE      # and the table of profiles/r25_resize.md
    python tools/bench_resize.py --no-torch           # skip the torch comparator

Images are synthetic, built on the device from a seed.  Steps (hsr_area_resample, one launch each, with the invalid counts):
  rgb_u8_f6            (7452, 7680, 3) uint8 pixel-major -> (1242, 1280), factor 6, aligned; also with a float32 output, beside
                       hsr_block_mean on the same buffers and beside torch.nn.functional.interpolate(mode="area");
  rgb_u8_7455          (7455, 7683, 3) uint8 pixel-major -> (1242, 1280): scale 6.0024 x 6.0023;
  planes_u16_60m       10 x 7452 x 7680 uint16 planar -> 60 m with an origin of (0.25, -0.4): 10 x 1242 x 1280;
  granule_u16_1024     10980 x 10980 uint16 -> 1024 x 1024 (scale 10.72: the gather kernel);
  f32_nan_<rule>       3 x 7452 x 7680 float32 planar with 10 % NaN -> 1242 x 1280 under STRICT and under RENORM.
Per step: us, the median over SAMPLES samples of REPS back-to-back launches between two device events after WARMUP calls, with the
fastest and slowest sample; bytes, what the step has to move (every source byte under the destination once, every output byte
once); copy_us, a device-to-device copy in the same process that moves the same number of bytes (half read, half written).  The
torch form is a timing baseline only: its windows are integer-bounded (adaptive pooling), so its values differ from the
definition's at every ratio that is no integer, and it needs a float32 NCHW copy of the image, which is timed with it.

Every step's device result is compared with hsr_area_resample_host on the top left 512 x 512 source pixels of the same inputs, same
origin and scale: the tool exits non-zero when a bit differs (also when the aligned factor-6 float32 result differs from hsr_block_mean's).  Nothing is gated on a time.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "hyperspectral_super-resolution_amd"))

SAMPLES, REPS, WARMUP = 5, 3, 2
CROP = 512
CODES = {"float32": 0, "uint8": 1, "uint16": 2}
NP = {"float32": np.float32, "uint8": np.uint8, "uint16": np.uint16}


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
    ap.add_argument("--no-torch", action="store_true", help="skip the torch form")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from s2_emit import _native as nat
    from s2_emit._engine import _ptr, _stream
    assert torch.cuda.is_available(), "bench_resize needs a GPU"
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = _stream(torch)
    g = torch.Generator(device="cuda").manual_seed(25)
    rows, mismatches = [], []
    copies = {}

    def copy_us(nbytes):
        n = max(int(nbytes) // 2, 1)
        if n not in copies:
            src, dst = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
            copies[n] = timed(torch, lambda: dst.copy_(src))[0]
            del src, dst
        return copies[n]

    def record(step, us3, nbytes, **extra):
        us, lo, hi = us3
        cu = copy_us(nbytes)
        rec = dict(step=step, us=round(us, 1), us_min=round(lo, 1), us_max=round(hi, 1), bytes=int(nbytes), tbps=round(nbytes / us / 1e6, 3),
                   copy_us=round(cu, 1), x_copy=round(us / cu, 2), **extra)
        rows.append(rec)
        print(json.dumps(rec), flush=True)
        return rec

    def image(dtype, shape):
        if dtype == "uint8":
            return torch.randint(0, 256, shape, generator=g, device=dev, dtype=torch.uint8)
        if dtype == "uint16":
            return torch.randint(-32768, 32768, shape, generator=g, device=dev, dtype=torch.int16)       # every bit pattern of a uint16
        return torch.rand(shape, generator=g, device=dev, dtype=torch.float32)

    def last_launch():
        buf = C.create_string_buffer(4096)
        lib.hsr_resize_last_launch(buf, 4096)
        return buf.value.decode()

    def step(name, src, dtype, Cn, h, w, sst, H, W, origin, scale, out_dtype, rule=1, mvf=0.0, **extra):
        """Times hsr_area_resample on src (strides sst = (cs, rs, ps) in elements), checks a crop against the host twin."""
        pix = sst[0] == 1 and Cn > 1
        dst_st = (1, W * Cn, Cn) if pix else (H * W, W, 1)
        tdt = {"float32": torch.float32, "uint8": torch.uint8, "uint16": torch.int16}[out_dtype]
        out = torch.empty(Cn * H * W, dtype=tdt, device=dev)
        invalid = torch.empty(Cn, dtype=torch.int64, device=dev)

        def call(src_p, hh, ww, ss, o, dst_p, HH, WW, ds, inv_p, fn, *tail):
            return fn(src_p, CODES[dtype], Cn, hh, ww, ss[0], ss[1], ss[2], o[0], o[1], scale[0], scale[1], 0, 0.0, rule, mvf, dst_p,
                      CODES[out_dtype], HH, WW, ds[0], ds[1], ds[2], C.c_float(1.0), C.c_float(float("nan")), 0, inv_p, *tail)

        fn = lambda: nat.check(call(_ptr(src), h, w, sst, origin, _ptr(out), H, W, dst_st, _ptr(invalid), lib.hsr_area_resample, st))  # noqa: E731
        lib.hsr_resize_last_launch(None, 0)
        us3 = timed(torch, fn)
        kernel = last_launch().split("; ")[-1]
        esize, osize = np.dtype(NP[dtype]).itemsize, np.dtype(NP[out_dtype]).itemsize
        covered_h = min(h, int(np.ceil(origin[0] + H * scale[0]))) - max(0, int(np.floor(origin[0])))
        covered_w = min(w, int(np.ceil(origin[1] + W * scale[1]))) - max(0, int(np.floor(origin[1])))
        nbytes = Cn * covered_h * covered_w * esize + Cn * H * W * osize
        frac = float(invalid.sum().item()) / (Cn * H * W)
        rec = record(name, us3, nbytes, kernel=kernel, invalid_frac=round(frac, 4), **extra)
        # the same launch against the host twin on the top left CROP x CROP source pixels: the same origin and scale, so the cells'
        # edges are the same expressions, and as many cells as end inside the crop, so that no edge is clipped differently
        r0, c0, r1, c1 = 0, 0, min(h, CROP), min(w, CROP)
        n, m = min(H, int((r1 - origin[0]) / scale[0])), min(W, int((c1 - origin[1]) / scale[1]))
        while origin[0] + n * scale[0] > r1:
            n -= 1
        while origin[1] + m * scale[1] > c1:
            m -= 1
        Y0, X0 = 0, 0
        if pix:
            crop = src.view(h, w, Cn)[r0:r1, c0:c1, :].contiguous().cpu().numpy().view(NP[dtype])
            css = (1, (c1 - c0) * Cn, Cn)
        else:
            crop = src.view(Cn, h, w)[:, r0:r1, c0:c1].contiguous().cpu().numpy().view(NP[dtype])
            css = ((r1 - r0) * (c1 - c0), c1 - c0, 1)
        hout = np.zeros(Cn * n * m, NP[out_dtype])
        hinv = np.zeros(Cn, np.int64)
        hds = (1, m * Cn, Cn) if pix else (n * m, m, 1)
        rcode = call(C.c_void_p(crop.ctypes.data), r1 - r0, c1 - c0, css, origin, C.c_void_p(hout.ctypes.data), n, m, hds,
                     C.c_void_p(hinv.ctypes.data), lib.hsr_area_resample_host)
        assert rcode == 0, lib.hsr_last_error()
        full = out.view(H, W, Cn)[Y0:Y0 + n, X0:X0 + m, :] if pix else out.view(Cn, H, W)[:, Y0:Y0 + n, X0:X0 + m]
        dev_bits = full.contiguous().cpu().numpy().view(np.uint8).reshape(-1)
        same = np.array_equal(dev_bits, hout.view(np.uint8).reshape(-1))
        rec["host_crop"] = "equal" if same else "DIFFERS"
        if not same:
            mismatches.append(name)
        print(json.dumps(dict(step=name, host_crop=rec["host_crop"], crop_cells=[n, m])), flush=True)
        return out

    # ---- the steps ----------------------------------------------------------------------------------------------------------------------
    H, W = 1242, 1280
    rgb = image("uint8", (7452 * 7680 * 3,))
    pixst = lambda w_: (1, w_ * 3, 3)  # noqa: E731
    step("rgb_u8_f6", rgb, "uint8", 3, 7452, 7680, pixst(7680), H, W, (0.0, 0.0), (6.0, 6.0), "uint8")
    area32 = step("rgb_u8_f6_to_f32", rgb, "uint8", 3, 7452, 7680, pixst(7680), H, W, (0.0, 0.0), (6.0, 6.0), "float32")
    bm = torch.empty(H * W * 3, dtype=torch.float32, device=dev)
    bm_fn = lambda: nat.check(lib.hsr_block_mean(_ptr(rgb), 1, 1, 3, 3, H, W, 6, 1.0, _ptr(bm), 1, 3, st))  # noqa: E731
    record("block_mean_rgb_u8_f6_to_f32", timed(torch, bm_fn), 7452 * 7680 * 3 + H * W * 12, kernel="hsr_block_mean")
    if not torch.equal(bm.view(torch.int32), area32.view(torch.int32)):
        mismatches.append("rgb_u8_f6_to_f32 vs hsr_block_mean")
    del bm, area32
    if not a.no_torch:
        x = rgb.view(7452, 7680, 3)
        tfn = lambda: F.interpolate(x.permute(2, 0, 1)[None].float(), size=(H, W), mode="area")  # noqa: E731
        record("torch_area_rgb_u8_f6", timed(torch, tfn, 1), 7452 * 7680 * 3 + H * W * 12, kernel="torch interpolate(area) on a float32 copy")
    del rgb
    rgb = image("uint8", (7455 * 7683 * 3,))
    step("rgb_u8_7455", rgb, "uint8", 3, 7455, 7683, pixst(7683), H, W, (0.0, 0.0), (7455 / H, 7683 / W), "uint8")
    del rgb
    planes = image("uint16", (10 * 7452 * 7680,))
    step("planes_u16_60m", planes, "uint16", 10, 7452, 7680, (7452 * 7680, 7680, 1), H, W, (0.25, -0.4), (6.0, 6.0), "uint16")
    del planes
    gran = image("uint16", (10980 * 10980,))
    step("granule_u16_1024", gran, "uint16", 1, 10980, 10980, (10980 * 10980, 10980, 1), 1024, 1024, (0.0, 0.0), (10980 / 1024, 10980 / 1024),
         "uint16")
    del gran
    f32 = image("float32", (3 * 7452 * 7680,))
    f32[torch.rand(f32.shape, generator=g, device=dev) < 0.1] = float("nan")
    for rname, rcode in (("strict", 0), ("renorm", 1)):
        step(f"f32_nan_{rname}", f32, "float32", 3, 7452, 7680, (7452 * 7680, 7680, 1), H, W, (0.0, 0.0), (6.0, 6.0), "float32", rule=rcode)
    del f32

    if a.markdown:
        with open(a.markdown, "w") as fh:
            fh.write("| step | kernel | us (median) | min .. max | bytes moved | TB/s | copy of the same bytes, us | x copy | invalid | host twin on a crop |\n")
            fh.write("|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                fh.write(f"| {r['step']} | `{r['kernel']}` | {r['us']} | {r['us_min']} .. {r['us_max']} | {r['bytes'] / 1e6:.1f} MB | {r['tbps']} | "
                         f"{r['copy_us']} | {r['x_copy']} | {r.get('invalid_frac', '')} | {r.get('host_crop', '')} |\n")
    if mismatches:
        print(json.dumps(dict(error="device result differs", steps=mismatches)), flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
