"""Benchmark of the S2 stack family (include/hsr_s2stack.h, s2_emit.s2stack) at the size of a Sentinel-2 granule.

    python tools/bench_s2stack.py                      # every step; one JSON line each
    python tools/bench_s2stack.py --markdown FILE      # and the table of profiles/r23_s2stack.md
    python tools/bench_s2stack.py --no-torch           # skip the torch comparator

Planes (synthetic, built on the device from a seed): the ten bands of S2_STACK_BANDS, four at 10980 x 10980 and six at 5490 x 5490,
uint16 DN in 1 .. 9999; the window is the benchmark scene's 7452 x 7680 at an odd origin.  `clean`: no nodata inside the window -
every thread of a bilinear band takes the separable path; `border`: the planes are nodata within 194 10 m pixels of the window's
edge, 10 % of the window - the rows and columns along it go through the per-pixel path.  Steps:
  stack_<dtype>_<rule>_<content>   hsr_s2_stack, ten bands in one launch, with the invalid counts;
  expand_scl                       hsr_s2_expand_u8 of a 20 m SCL plane under the same window.
Per step: us, the median over SAMPLES samples of REPS back-to-back launches between two device events after WARMUP calls, with the
fastest and slowest sample; bytes, what the step has to move (the source pixels under the window once, every output byte once);
copy_us, a device-to-device copy in the same process that moves the same number of bytes (half read, half written); torch_us, the
torch form on the same device - interpolate(scale_factor=2, mode="bilinear", align_corners=False) per 20 m band, then cat, slice
and cast - a timing baseline only: its edges differ (it has no nodata rule and its window is cut after the resampling) and it is
compared with nothing.  The clean uint16 result is compared with assemble_s2_stack's own on a sub-window.  Nothing is gated on a
number.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "hyperspectral_super-resolution_amd"))

H10 = W10 = 10980
ROW0, COL0, H, W = 1765, 1651, 7452, 7680
BORDER = 194
SAMPLES, REPS, WARMUP = 5, 3, 2


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
    import s2_emit
    from s2_emit import _native as nat
    from s2_emit._engine import _ptr, _stream
    from s2_emit.scenes import Window
    assert torch.cuda.is_available(), "bench_s2stack needs a GPU"
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = _stream(torch)
    g = torch.Generator(device="cuda").manual_seed(23)
    rows = []

    def plane(up):
        h, w = -(-H10 // up), -(-W10 // up)
        return torch.randint(1, 10000, (h, w), generator=g, device=dev, dtype=torch.int16)

    def with_border(p, up):
        q = p.clone()
        r0, c0, r1, c1 = ROW0 // up, COL0 // up, (ROW0 + H) // up, (COL0 + W) // up
        d = BORDER // up
        q[r0:r0 + d, c0:c1] = 0
        q[r1 - d:r1, c0:c1] = 0
        q[r0:r1, c0:c0 + d] = 0
        q[r0:r1, c1 - d:c1] = 0
        return q

    ups = [1 if m == "nearest" else 2 for _, _, m in s2_emit.S2_STACK_BANDS]
    contents = {"clean": [plane(up) for up in ups]}
    contents["border"] = [with_border(p, up) for p, up in zip(contents["clean"], ups)]
    nb = len(ups)

    def table_of(planes):
        t = (nat.S2Band * nb)()
        for e, p, up, (_, _, m) in zip(t, planes, ups, s2_emit.S2_STACK_BANDS):
            e.plane_dev, e.rs, e.H, e.W, e.up, e.method = p.data_ptr(), p.stride(0), p.shape[0], p.shape[1], up, 0 if m == "nearest" else 1
        return t

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

    read_bytes = sum(2 * (H // up) * (W // up) for up in ups)
    invalid = torch.empty(nb, dtype=torch.int64, device=dev)
    for dname, dcode, esize in (("uint16", 0, 2), ("float32", 1, 4)):
        out = torch.empty((nb, H, W), dtype=torch.int16 if dcode == 0 else torch.float32, device=dev)
        for rname, rcode in (("strict", 0), ("renorm", 1)):
            for cname, planes in contents.items():
                t = table_of(planes)
                fn = lambda: nat.check(lib.hsr_s2_stack(t, nb, H10, W10, ROW0, COL0, H, W, 1, 0, rcode, dcode, _ptr(out), H * W, W, 0,  # noqa: E731
                                                        C.c_float(float("nan")), C.c_double(10000.0), _ptr(invalid), st))
                us3 = timed(torch, fn)
                frac = float(invalid.sum().item()) / (nb * H * W)
                record(f"stack_{dname}_{rname}_{cname}", us3, read_bytes + nb * H * W * esize, invalid_frac=round(frac, 4), torch_us=None)
        if dcode == 0:                                      # the launch above against the driver, on a sub-window
            t = table_of(contents["clean"])
            nat.check(lib.hsr_s2_stack(t, nb, H10, W10, ROW0, COL0, H, W, 1, 0, 0, 0, _ptr(out), H * W, W, 0, C.c_float(float("nan")),
                                       C.c_double(10000.0), None, st))
            keys = [k for _, k, _ in s2_emit.S2_STACK_BANDS]
            bands = {k: p.view(torch.uint16) for k, p in zip(keys, contents["clean"])}
            sub = s2_emit.assemble_s2_stack(bands, window=Window(COL0 + 3, ROW0 + 5, 1001, 777))
            assert torch.equal(sub.stack.view(torch.int16), out[:, 5:5 + 777, 3:3 + 1001]), "the driver differs from the launch"
        del out

    scl = torch.randint(0, 12, (H10 // 2, W10 // 2), generator=g, device=dev, dtype=torch.uint8)
    scl10 = torch.empty((H, W), dtype=torch.uint8, device=dev)
    us3 = timed(torch, lambda: nat.check(lib.hsr_s2_expand_u8(_ptr(scl), H10 // 2, W10 // 2, W10 // 2, 2, H10, W10, ROW0, COL0, H, W,
                                                              _ptr(scl10), W, st)))
    record("expand_scl", us3, (H // 2) * (W // 2) + H * W, torch_us=None)

    def write_markdown():
        if not a.markdown:
            return
        with open(a.markdown, "w") as fh:
            fh.write("| step | us (median) | min .. max | bytes moved | TB/s | copy of the same bytes, us | x copy | torch form, us | note |\n")
            fh.write("|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                note = f"invalid_frac {r['invalid_frac']}" if "invalid_frac" in r else ""
                tch = "" if r.get("torch_us") is None else f"{r['torch_us']}"
                fh.write(f"| {r['step']} | {r['us']} | {r['us_min']} .. {r['us_max']} | {r['bytes'] / 1e6:.1f} MB | {r['tbps']} | {r['copy_us']} | "
                         f"{r['x_copy']} | {tch} | {note} |\n")

    write_markdown()
    # ---- the torch form, last: whatever it takes, the table above is written -----------------------------------------------------------------
    if not a.no_torch:
        planes = contents["clean"]
        for dname, cast in (("uint16", lambda x: x.round().to(torch.int32).to(torch.int16)), ("float32", lambda x: x / 10000.0)):
            def form():
                full = [p.float() if up == 1 else F.interpolate(p.float()[None, None], scale_factor=2, mode="bilinear", align_corners=False)[0, 0]
                        for p, up in zip(planes, ups)]
                return cast(torch.cat([f[None] for f in full])[:, ROW0:ROW0 + H, COL0:COL0 + W])
            us = round(timed(torch, form, 1)[0], 1)
            for r in rows:
                if r["step"].startswith(f"stack_{dname}_") and r["step"].endswith("_clean"):
                    r["torch_us"] = us
            print(json.dumps(dict(step=f"torch_{dname}", torch_us=us)), flush=True)
            write_markdown()


if __name__ == "__main__":
    main()
