"""Benchmark of s2_emit.scenes (black-window scan, tile gather, mosaic, fuse_scene) at the reference's scene sizes.

    python tools/bench_scene.py                          # every step; one JSON line each
    python tools/bench_scene.py --markdown FILE          # and the table of profiles/r12_scene_tiles.md
    python tools/bench_scene.py --no-numpy               # skip the host comparisons

Scenes (synthetic, built on the device from a seed): EMIT 285 x 1242 x 1280 float32 (12 x 12 windows of 100 x 100, nodata
-9999) and S2 10 x 7452 x 7680 uint16 (windows of 600 x 600).  Steps:
  scan_emit_0 / _35 / _100   hsr_scene_black_counts on the EMIT scene with no black pixel, with a black border that covers
                             about 35 % of the window area, and all black;
  scan_s2                    the same on the S2 scene (a zero border);
  gather_emit / _encode      hsr_scene_gather_tiles of all 144 EMIT windows, as float32 and quantised to uint16;
  gather_s2                  the 144 S2 windows;
  mosaic_T32 / mosaic_T8     hsr_scene_mosaic of 144 cubes of T x 600 x 600 into T x 7452 x 7680;
  blend_T32_half_stride      hsr_scene_mosaic_blend of the half-stride window set - 23 x 24 cubes of 32 x 600 x 600 (25.4 GB), four
                             over every inner pixel - into 32 x 7452 x 7680; bytes: the output once plus every contributor read;
                             blend_vs_mosaic is its rate over mosaic_T32's in the same process;
  fuse_scene                 find -> gather -> fuse_tile_pairs -> mosaic end to end (wall clock around a synchronise: it holds the
                             one host synchronisation), 32 bands, batches of 64;
  fuse_scene_stride50        the same with stride=50: windows at half stride, their cubes kept in one stack and blended at the end.
Per step: us, the median over SAMPLES samples of REPS back-to-back launches between two device events, after warm-up, with the
fastest and slowest sample; bytes, what the step has to move (scan: one band of every covered pixel that is not black and
every band of every black one; gather and mosaic: read + written); tbps = bytes / us; floor_us = bytes at 8 TB/s; numpy_ms, the
same step in NumPy on this host (wall clock, once): the scan as the reference runs it, window by window, with the
restatement of np.isclose's arithmetic below; gather as np.stack of slices (+ the quantisation statements); mosaic (T = 8 only)
as slice assignments into a NaN-filled array.
The early exit is judged by scan_emit_0 against scan_emit_100: the first reads about 1 / 285 of the second's bytes.
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
BORDER = 233                           # rows and columns: 1 - (967 / 1200)^2 = 35 % of the window area
SAMPLES, REPS, WARMUP = 7, 10, 3
PEAK_TBPS = 8.0


def black_rule(arr, nodata=None, masked_val=-0.01, nodata_atol=1e-3, zero_atol=1e-6):
    """is_black_mask's arithmetic as NumPy 2 evaluates it: float32 arrays in float32, integer arrays in float64."""
    ft = np.float32 if arr.dtype == np.float32 else np.float64
    x = arr.astype(ft, copy=False)

    def close(v):
        with np.errstate(invalid="ignore"):
            return np.abs(x - ft(v)) <= ft(nodata_atol + 1e-5 * abs(v))

    out = close(masked_val).all(0) | (np.abs(x) < ft(zero_atol)).all(0)
    return out | close(nodata).all(0) if nodata is not None else out


def numpy_counts(scene, t, nodata):
    """The reference's walk: is_black_mask per window."""
    ny, nx = scene.shape[1] // t, scene.shape[2] // t
    out = np.zeros((ny, nx), np.int32)
    for i in range(ny):
        for j in range(nx):
            out[i, j] = black_rule(scene[:, i * t:(i + 1) * t, j * t:(j + 1) * t], nodata).sum()
    return out


def numpy_encode(emit, scale=10000.0, nodata=NODATA, nd16=65535):
    valid = np.isfinite(emit) & (emit != nodata)
    with np.errstate(invalid="ignore"):
        q = np.clip(np.rint(emit * np.float32(scale)).astype(np.int32), 0, nd16 - 1)
    out = np.full(emit.shape, nd16, dtype=np.uint16)
    out[valid] = q[valid].astype(np.uint16)
    return out


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


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markdown", default=None, help="write the result table to this file")
    ap.add_argument("--no-numpy", action="store_true", help="skip the NumPy comparisons on the host")
    a = ap.parse_args()
    import torch
    import s2_emit
    from s2_emit import _native as nat, scenes
    from s2_emit._engine import _stream
    assert torch.cuda.is_available(), "bench_scene needs a GPU"
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = _stream(torch)
    g = torch.Generator(device="cuda").manual_seed(12)
    rows = []

    def record(step, us3, nbytes, numpy_ms=None, **extra):
        us, lo, hi = us3
        rec = dict(step=step, us=round(us, 1), us_min=round(lo, 1), us_max=round(hi, 1), bytes=int(nbytes),
                   tbps=round(nbytes / us / 1e6, 3), floor_us=round(nbytes / PEAK_TBPS / 1e6, 1),
                   numpy_ms=None if numpy_ms is None else round(numpy_ms, 1), **extra)
        rows.append(rec)
        print(json.dumps(rec), flush=True)

    # ---- the scans ----------------------------------------------------------------------------------------------------------
    B, H, W = EMIT_SHAPE
    ts = TILE * SCALE
    ny, nx = H // TILE, W // TILE
    covered = ny * TILE * nx * TILE
    emit = torch.rand(EMIT_SHAPE, generator=g, device=dev) * 0.6 + 0.02
    counts = torch.empty((ny, nx), dtype=torch.int32, device=dev)
    nd = (1, NODATA)

    def scan_emit():
        scenes._scan(lib, st, emit, "float32", EMIT_SHAPE, TILE, TILE, nd, -0.01, 1e-3, 1e-6, counts)

    def scan_case(step, with_numpy):
        us3 = timed(torch, scan_emit)
        black = int(counts.sum().item())
        ms = None
        if with_numpy:
            host = emit.cpu().numpy()
            ms, want = wall(lambda: numpy_counts(host, TILE, NODATA))
            assert (want == counts.cpu().numpy()).all(), f"{step}: the device counts differ from NumPy's"
        record(step, us3, 4 * ((covered - black) + black * B), ms, black_frac=round(black / covered, 4))
        return us3[0]

    t0 = scan_case("scan_emit_0", False)
    emit[:, :BORDER, :] = NODATA
    emit[:, :, :BORDER] = NODATA
    scan_case("scan_emit_35", not a.no_numpy)
    border = emit.clone()
    emit.fill_(NODATA)
    t100 = scan_case("scan_emit_100", False)
    emit.copy_(border)
    del border

    Bs, Hs, Ws = S2_SHAPE
    nys, nxs = Hs // ts, Ws // ts
    s2 = torch.randint(1, 4000, S2_SHAPE, generator=g, device=dev, dtype=torch.int16)
    s2[:, :BORDER * SCALE, :] = 0
    s2[:, :, :BORDER * SCALE] = 0
    counts_s = torch.empty((nys, nxs), dtype=torch.int32, device=dev)
    us3 = timed(torch, lambda: scenes._scan(lib, st, s2, "uint16", S2_SHAPE, ts, ts, (0, 0.0), -0.01, 1e-3, 1e-6, counts_s))
    black = int(counts_s.sum().item())
    ms = None
    if not a.no_numpy:
        host = s2.cpu().numpy().view(np.uint16)
        ms, want = wall(lambda: numpy_counts(host, ts, None))
        assert (want == counts_s.cpu().numpy()).all(), "scan_s2: the device counts differ from NumPy's"
    cov_s = nys * nxs * ts * ts
    record("scan_s2", us3, 2 * ((cov_s - black) + black * Bs), ms, black_frac=round(black / cov_s, 4))

    # ---- the gathers: all 144 windows -----------------------------------------------------------------------------------------
    eo = np.array([(i * TILE, j * TILE) for i in range(ny) for j in range(nx)], dtype=np.int32)
    so = eo * SCALE
    P = len(eo)
    eo_d, so_d = torch.from_numpy(eo).to(dev), torch.from_numpy(so).to(dev)
    enc = (10000.0, 1, NODATA, 65535)
    n_e, n_s = P * B * TILE * TILE, P * Bs * ts * ts
    ms = ms_enc = ms_s2 = None
    if not a.no_numpy:
        host = emit.cpu().numpy()
        ms, tiles = wall(lambda: np.stack([host[:, r:r + TILE, c:c + TILE] for r, c in eo]))
        ms_q, q = wall(lambda: numpy_encode(tiles))
        ms_enc = ms + ms_q
        got = scenes._gather(lib, torch, st, emit, "float32", EMIT_SHAPE, eo, TILE, TILE, enc)
        assert (got.view(torch.int16).cpu().numpy().view(np.uint16) == q).all(), "gather_emit_encode differs from NumPy's"
        del host, tiles, q, got
        host = s2.cpu().numpy()
        ms_s2, _ = wall(lambda: np.stack([host[:, r:r + ts, c:c + ts] for r, c in so]))
        del host
    record("gather_emit", timed(torch, lambda: scenes._gather(lib, torch, st, emit, "float32", EMIT_SHAPE, eo_d, TILE, TILE)),
           8 * n_e, ms, tiles=P)
    record("gather_emit_encode", timed(torch, lambda: scenes._gather(lib, torch, st, emit, "float32", EMIT_SHAPE, eo_d, TILE, TILE, enc)),
           6 * n_e, ms_enc, tiles=P)
    record("gather_s2", timed(torch, lambda: scenes._gather(lib, torch, st, s2, "uint16", S2_SHAPE, so_d, ts, ts)), 4 * n_s, ms_s2,
           tiles=P)

    # ---- the mosaic -----------------------------------------------------------------------------------------------------------
    slot = torch.arange(nys * nxs, dtype=torch.int32, device=dev).reshape(nys, nxs)
    for T in (32, 8):
        cubes = torch.rand((nys * nxs, T, ts, ts), generator=g, device=dev)
        out = torch.empty((T, Hs, Ws), dtype=torch.float32, device=dev)
        us3 = timed(torch, lambda: scenes._mosaic_into(lib, torch, st, cubes, out, slot, ts, ts, float("nan"), True))
        ms = None
        if T == 8 and not a.no_numpy:
            host = cubes.cpu().numpy()

            def assemble():
                o = np.full((T, Hs, Ws), np.nan, dtype=np.float32)
                for k in range(nys * nxs):
                    i, j = divmod(k, nxs)
                    o[:, i * ts:(i + 1) * ts, j * ts:(j + 1) * ts] = host[k]
                return o
            ms, want = wall(assemble)
            assert np.array_equal(want, out.cpu().numpy(), equal_nan=True), "mosaic differs from NumPy's"
            del host, want
        record(f"mosaic_T{T}", us3, 4 * (cubes.numel() + out.numel()), ms, tiles=nys * nxs)
        del cubes, out

    # ---- the feathered mosaic: the half-stride window set, 23 x 24 windows of 600 x 600 (four over an inner pixel) -----------------
    half = ts // 2
    nyb, nxb = (Hs - ts) // half + 1, (Ws - ts) // half + 1
    start = torch.arange(nyb * nxb, dtype=torch.int32, device=dev).reshape(nyb, nxb)
    cubes = torch.rand((nyb * nxb, 32, ts, ts), generator=g, device=dev)
    out = torch.empty((32, Hs, Ws), dtype=torch.float32, device=dev)
    us3 = timed(torch, lambda: scenes._blend_into(lib, torch, st, cubes, out, start, half, half, ts, ts, float("nan")))
    record("blend_T32_half_stride", us3, 4 * (cubes.numel() + out.numel()), None, tiles=nyb * nxb)
    mosaic = next(r for r in rows if r["step"] == "mosaic_T32")
    blend_verdict = dict(step="blend_vs_mosaic", blend_tbps=rows[-1]["tbps"], mosaic_tbps=mosaic["tbps"],
                         ratio=round(rows[-1]["tbps"] / mosaic["tbps"], 3))
    print(json.dumps(blend_verdict), flush=True)
    del cubes, out

    # ---- end to end -----------------------------------------------------------------------------------------------------------
    s2u = s2.view(torch.uint16)
    kw = dict(tile=TILE, factor=SCALE, batch=64, bands=32, emit_nodata=NODATA, s2_nodata=0.0)
    res = s2_emit.fuse_scene(emit, s2u, **kw)
    torch.cuda.synchronize()
    ms = []
    for _ in range(3):
        del res
        t = time.perf_counter()
        res = s2_emit.fuse_scene(emit, s2u, **kw)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    ms.sort()
    nt = len(res.tiles)
    moved = 4 * covered + 2 * cov_s + nt * (8 * B * TILE * TILE + 4 * Bs * ts * ts) + 4 * 32 * (2 * nt * ts * ts + Hs * Ws)
    rec = dict(step="fuse_scene", ms=round(ms[1], 2), ms_min=round(ms[0], 2), ms_max=round(ms[2], 2), tiles=nt,
               ms_per_tile=round(ms[1] / max(nt, 1), 3), scene_step_bytes=int(moved), floor_us=round(moved / PEAK_TBPS / 1e6, 1),
               status_ok=int((res.status == 0).sum().item()))
    print(json.dumps(rec), flush=True)
    # the same with windows at half stride, cross-faded: every kept window's cube stays in one stack until the one blend launch
    kw["stride"] = TILE // 2
    res = s2_emit.fuse_scene(emit, s2u, **kw)
    torch.cuda.synchronize()
    ms = []
    for _ in range(3):
        del res
        t = time.perf_counter()
        res = s2_emit.fuse_scene(emit, s2u, **kw)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    ms.sort()
    nb = len(res.tiles)
    rec_b = dict(step="fuse_scene_stride50", ms=round(ms[1], 2), ms_min=round(ms[0], 2), ms_max=round(ms[2], 2), tiles=nb,
                 ms_per_tile=round(ms[1] / max(nb, 1), 3), stack_bytes=scenes._blend_stack_bytes(nb, 32, ts, ts),
                 status_ok=int((res.status == 0).sum().item()))
    print(json.dumps(rec_b), flush=True)
    del res
    verdict = dict(step="early_exit", scan_emit_0_us=round(t0, 1), scan_emit_100_us=round(t100, 1), ratio=round(t100 / t0, 1),
                   works=bool(t0 * 4 < t100))
    print(json.dumps(verdict), flush=True)
    if a.markdown:
        with open(a.markdown, "w") as fh:
            fh.write("| step | us (median) | min .. max | bytes moved | TB/s | floor at 8 TB/s, us | x floor | NumPy, ms | NumPy / GPU |\n")
            fh.write("|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                npy = "not measured" if r["numpy_ms"] is None else f"{r['numpy_ms']:.0f}"
                ratio = "" if r["numpy_ms"] is None else f"{r['numpy_ms'] * 1e3 / r['us']:.0f} x"
                fh.write(f"| {r['step']} | {r['us']} | {r['us_min']} .. {r['us_max']} | {r['bytes'] / 1e6:.1f} MB | {r['tbps']} | "
                         f"{r['floor_us']} | {r['us'] / max(r['floor_us'], 1e-9):.1f} | {npy} | {ratio} |\n")
            fh.write(f"\nfuse_scene: {json.dumps(rec)}\n\nfuse_scene, stride 50: {json.dumps(rec_b)}\n\n"
                     f"blend against mosaic: {json.dumps(blend_verdict)}\n\nearly exit: {json.dumps(verdict)}\n")


if __name__ == "__main__":
    main()
