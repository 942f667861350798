"""Benchmark of s2_emit.fuse_tile_pairs (tile pairs -> fused 10 m cubes) at the notebook's shape.

    python tools/bench_tile_pairs.py                       # every configuration, each in a fresh process
    python tools/bench_tile_pairs.py --profile DIR         # the same under rocprofv3 --kernel-trace --stats (kernel times)
    python tools/bench_tile_pairs.py --report              # report=False vs report=True at P = 64, T = 32 and T = 285
    python tools/bench_tile_pairs.py --report --profile DIR   # the report=True batch under rocprofv3 (the report kernels)
    python tools/bench_tile_pairs.py --validate            # validate=False vs validate=True at P = 64, T = 32 and T = 285
    python tools/bench_tile_pairs.py --validate --profile DIR # the validate=True batch under rocprofv3 (the score kernels)
    python tools/bench_tile_pairs.py --pool                # pool=None vs pool="all" vs groups of 8 at P = 64, T = 32 and T = 285
    python tools/bench_tile_pairs.py --pool --profile DIR  # the two pooled batches under rocprofv3 (the pooling kernels)

Configurations: P = 1, 8, 64 pairs at T = 32 targets, and P = 64 at T = 285 (EMIT 285 x 100 x 100 uint16, S2 10 x 600 x 600
uint16, factor 6).  One JSON line per configuration:
  ms_per_pair         the batch (fuse_tile_pairs) over device events after warm-up, divided by P;
  loop_ms_per_pair    fuse_tile_pair called once per pair in a loop, same process, same events;
  host_ms_per_pair    today's host-driven chain for one pair: D2H, NumPy block mean / flatten_pixels / logit, PolyRidge.fit,
                      predict_cube (wall clock, synchronised; up to 4 pairs);
  ratio               ms_per_pair / loop_ms_per_pair;
and with --profile, from the kernel trace: launches_per_batch, the Gram's float64 and the predict's float32 FLOP rates over
their kernel time, and the per-kernel share of a batch.
With --report: plain_ms_per_pair / report_ms_per_pair, the batch without and with ``report=True`` timed alternately in one
process, and added_ms_per_pair, their difference; with --profile as well, report_us_per_batch (the two report kernels) and
q_read_tbps, the bytes of Q the report reads (P x 10 000 rows x na float64) over the report's partial kernel time.
With --validate: the same pair of timings for ``validate=True`` (validate_ms_per_pair, added_ms_per_pair), and the score call of
one view alone against a yardstick that is not the code under test, timed alternately over device events in the same process:
score_us_per_view (hsr_pair_score_f64 on (P, T, 10 000) float32 pred and y, every valid pixel in the fit group),
score_held_out_us_per_view (the same with a checkerboard of 10 x 10 blocks held out, so both groups in every chunk) and clone_us (torch ``clone()`` of one such tensor,
which moves the same 2 P T npix 4 bytes), their rates and score_over_clone.  With --profile as well, from the kernel trace:
score_us_per_batch (both views), score_read_tbps (4 P T npix 4 bytes over the partial kernels' time), and the block mean's and
the coarse predict's time per batch.
With --pool: none_ms_per_batch, all_ms_per_batch and groups_ms_per_batch - the batch without pooling, with ``pool="all"`` and with
P / 8 groups of 8 pairs (``pool=arange(P) // 8``), timed in turn in one process over device events (median) - and each pooled
time over the unpooled one; with --profile as well, one record per pooled mode with pool_us_per_batch (the three pooling kernels)
and the per-kernel times.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(1, 32), (8, 32), (64, 32), (64, 285)]
REPORT_CONFIGS = [(64, 32), (64, 285)]


def _pairs(torch, P, seed=0):
    """P synthetic pairs on the device: S2 DN from three sources, EMIT reflectance correlated with them (uint16 x 1e4)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    ab = torch.rand((P, 3, 100, 100), generator=g, device="cuda")
    spec = 0.05 + 0.4 * torch.rand((3, 285), generator=g, device="cuda")
    resp = 600 + 2200 * torch.rand((3, 10), generator=g, device="cuda")
    emit = (1e4 * torch.einsum("pkij,kb->pbij", ab, spec)).round().clamp(1, 9000).to(torch.int32)
    coarse = torch.einsum("pkij,kc->pcij", ab, resp)
    fine = coarse.repeat_interleave(6, dim=2).repeat_interleave(6, dim=3)
    s2 = (fine + 20 * torch.rand(fine.shape, generator=g, device="cuda")).round().clamp(1, 10000).to(torch.int32)
    return emit.to(torch.int16).view(torch.uint16), s2.to(torch.int16).view(torch.uint16)


def _host_chain(torch, s2_emit, E, S, bands):
    """The chain a caller runs today for one pair (wall clock, synchronised)."""
    import numpy as np
    t0 = time.perf_counter()
    e = (E.view(torch.int16).to(torch.int32) & 0xFFFF).cpu().numpy()
    s = (S.view(torch.int16).to(torch.int32) & 0xFFFF).cpu().numpy()
    X = s.astype(np.float64).reshape(10, 100, 6, 100, 6).sum(axis=(2, 4)) / 36.0
    X = np.where((s == 0).reshape(10, 100, 6, 100, 6).any(axis=(2, 4)), np.nan, X).astype(np.float32)
    Y = np.where(e[bands] == 65535, np.float32(np.nan), e[bands].astype(np.float32) * np.float32(1e-4))
    Xtr, Ytr = s2_emit.flatten_pixels(X, Y, x_nodata=0.0)
    Yl = s2_emit.ridge.logit(Ytr.astype(np.float64))
    m = s2_emit.PolyRidge(3, 1.0).fit(torch.from_numpy(Xtr).cuda(), torch.from_numpy(Yl).cuda())
    cube = m.predict_cube(torch.from_numpy(s.astype(np.float32)).cuda(), nodata=0.0)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, cube


def child(P, T, iters, warmup, host_pairs):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "hyperspectral_super-resolution_amd"))
    import torch
    import s2_emit
    bands = 32 if T == 32 else "all"
    E, S = _pairs(torch, P)
    kw = dict(bands=bands, s2_nodata=0.0)
    for _ in range(warmup):
        s2_emit.fuse_tile_pairs(E, S, **kw)
        for i in range(P):
            s2_emit.fuse_tile_pair(E[i], S[i], **kw)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    batch_ms, loop_ms = [], []
    for _ in range(iters):
        ev[0].record()
        out = s2_emit.fuse_tile_pairs(E, S, **kw)
        ev[1].record()
        for i in range(P):
            s2_emit.fuse_tile_pair(E[i], S[i], **kw)
        ev[2].record()
        torch.cuda.synchronize()
        batch_ms.append(ev[0].elapsed_time(ev[1]))
        loop_ms.append(ev[1].elapsed_time(ev[2]))
        del out
    host = []
    if host_pairs:
        idx = s2_emit.subsample_bands_evenly(285, 32) if T == 32 else list(range(285))
        _host_chain(torch, s2_emit, E[0], S[0], idx)                      # warm-up
        for i in range(min(host_pairs, P)):
            host.append(_host_chain(torch, s2_emit, E[i], S[i], idx)[0])
    bm, lm = sorted(batch_ms)[len(batch_ms) // 2], sorted(loop_ms)[len(loop_ms) // 2]
    rec = dict(P=P, T=T, iters=iters, ms_per_batch=round(bm, 4), ms_per_pair=round(bm / P, 4),
               loop_ms_per_pair=round(lm / P, 4), ratio=round(bm / lm, 3))
    if host:
        rec["host_ms_per_pair"] = round(sorted(host)[len(host) // 2], 3)
    print(json.dumps(rec), flush=True)


def child_report(P, T, iters, warmup, flag="report"):
    """The plain batch and the batch with report=True (or validate=True), alternately, over device events (median of each)."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "hyperspectral_super-resolution_amd"))
    import torch
    import s2_emit
    E, S = _pairs(torch, P)
    kw = dict(bands=32 if T == 32 else "all", s2_nodata=0.0)
    on = {flag: True}
    for _ in range(warmup):
        s2_emit.fuse_tile_pairs(E, S, **kw)
        s2_emit.fuse_tile_pairs(E, S, **on, **kw)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    plain, report = [], []
    for _ in range(iters):
        ev[0].record()
        a = s2_emit.fuse_tile_pairs(E, S, **kw)
        ev[1].record()
        b = s2_emit.fuse_tile_pairs(E, S, **on, **kw)
        ev[2].record()
        torch.cuda.synchronize()
        plain.append(ev[0].elapsed_time(ev[1]))
        report.append(ev[1].elapsed_time(ev[2]))
        del a, b
    pm, rm = sorted(plain)[len(plain) // 2], sorted(report)[len(report) // 2]
    rec = dict(P=P, T=T, iters=iters, plain_ms_per_pair=round(pm / P, 4))
    rec[f"{flag}_ms_per_pair"] = round(rm / P, 4)
    rec["added_ms_per_pair"] = round((rm - pm) / P, 4)
    if flag == "validate":
        rec.update(_score_vs_clone(torch, s2_emit, E, S, kw, max(iters, 20)))
    print(json.dumps(rec), flush=True)


def _score_vs_clone(torch, s2_emit, E, S, kw, iters):
    """hsr_pair_score_f64 on one view of a validate=True batch against torch's clone() of one (P, T, npix) float32 tensor:
    the same bytes moved (pred and y read once / one tensor read and written), alternately, median over device events."""
    from s2_emit import _native as nat
    from s2_emit._engine import _ptr, _stream
    lib = nat.load()
    out = s2_emit.fuse_tile_pairs(E, S, validate=True, **kw)
    val = out.validation
    pred, y = val.pred_coarse, val.cube_coarse                       # two (P, T, h, w) float32 arrays of the real thing
    P, T, h, w = pred.shape
    npix = h * w
    group = out.mask.to(torch.uint8).contiguous()
    sw = lib.hsr_pair_score_work_bytes(npix, T) // 8
    work = torch.empty((P, sw), dtype=torch.float64, device=pred.device)
    o = val
    n, rmse, r2, mean_ref = [torch.empty_like(t[:, 0].contiguous()) for t in (o.n, o.rmse, o.r2, o.mean_ref)]
    sam, n_sam, ergas = [torch.empty_like(t[:, 0].contiguous()) for t in (o.sam, o.n_sam, o.ergas)]
    sam_map = torch.empty((P, npix), dtype=torch.float32, device=pred.device)
    st = _stream(torch)

    def score():                                                      # reads `group` as bound at the call
        nat.check(lib.hsr_pair_score_f64(_ptr(pred), T * npix, _ptr(y), T * npix, _ptr(group), npix, npix, T, 100.0 / 6, _ptr(work),
                                         sw, _ptr(n), _ptr(rmse), _ptr(r2), _ptr(mean_ref), 2 * T, _ptr(sam), _ptr(n_sam),
                                         _ptr(ergas), 2, _ptr(sam_map), npix, P, st), "hsr_pair_score_f64")
    fit_only = group
    ii, jj = torch.meshgrid(torch.arange(h, device=pred.device), torch.arange(w, device=pred.device), indexing="ij")
    board = (((ii // 10 + jj // 10) % 2) + 1).to(torch.uint8).expand(P, h, w)
    held_out = (out.mask.to(torch.uint8) * board).contiguous()       # a checkerboard of 10 x 10 blocks held out (code 2)
    for _ in range(3):
        score()
        c = pred.clone()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ts, th, tc = [], [], []
    for _ in range(iters):
        group = fit_only
        ev[0].record()
        score()
        ev[1].record()
        c = pred.clone()
        ev[2].record()
        group = held_out
        score()
        ev[3].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]))
        tc.append(ev[1].elapsed_time(ev[2]))
        th.append(ev[2].elapsed_time(ev[3]))
        del c
    sm, cm, hm = (sorted(t)[len(t) // 2] for t in (ts, tc, th))
    nbytes = 2.0 * P * T * npix * 4
    return dict(score_us_per_view=round(sm * 1e3, 1), score_held_out_us_per_view=round(hm * 1e3, 1), clone_us=round(cm * 1e3, 1),
                score_tbps=round(nbytes / sm / 1e9, 2), clone_tbps=round(nbytes / cm / 1e9, 2),
                score_over_clone=round(sm / cm, 2), score_held_out_over_clone=round(hm / cm, 2))


def _pool_arg(mode, P):
    """--pool-mode -> the ``pool`` argument: none, all, or groups of 8 pairs."""
    import numpy as np
    return {"none": None, "all": "all", "groups": np.arange(P) // 8}[mode]


def child_pool(P, T, iters, warmup):
    """pool=None, pool="all" and groups of 8, in turn, over device events (median of each)."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "hyperspectral_super-resolution_amd"))
    import torch
    import s2_emit
    E, S = _pairs(torch, P)
    kw = dict(bands=32 if T == 32 else "all", s2_nodata=0.0)
    modes = ("none", "all", "groups")
    for _ in range(warmup):
        for m in modes:
            s2_emit.fuse_tile_pairs(E, S, pool=_pool_arg(m, P), **kw)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(modes) + 1)]
    ms = {m: [] for m in modes}
    for _ in range(iters):
        for i, m in enumerate(modes):
            ev[i].record()
            out = s2_emit.fuse_tile_pairs(E, S, pool=_pool_arg(m, P), **kw)
            del out
        ev[len(modes)].record()
        torch.cuda.synchronize()
        for i, m in enumerate(modes):
            ms[m].append(ev[i].elapsed_time(ev[i + 1]))
    med = {m: sorted(v)[len(v) // 2] for m, v in ms.items()}
    rec = dict(P=P, T=T, iters=iters, groups=(P + 7) // 8)
    for m in modes:
        rec[f"{m}_ms_per_batch"] = round(med[m], 4)
        rec[f"{m}_min_max_ms"] = [round(min(ms[m]), 4), round(max(ms[m]), 4)]
    rec["all_over_none"] = round(med["all"] / med["none"], 3)
    rec["groups_over_none"] = round(med["groups"] / med["none"], 3)
    print(json.dumps(rec), flush=True)


def _kernel_stats(out_dir):
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as fh:
            rows += list(csv.DictReader(fh))
    return rows


def profile_one(P, T, iters, out_dir, report=False, validate=False, pool="none"):
    """One configuration under rocprofv3, twice (1 and 1 + iters batches after the input generation): the difference of the two
    traces is `iters` batches alone - launches per batch, kernel time per batch, and the Gram / predict FLOP rates over it."""
    def run(n):
        d = os.path.join(out_dir, f"P{P}_T{T}_n{n}" + ("_report" if report else "") + ("_validate" if validate else "") +
                         (f"_pool_{pool}" if pool != "none" else ""))
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
               os.path.abspath(__file__), "--child", f"{P},{T}", "--iters", str(n), "--batch-only"] + \
              (["--report"] if report else []) + (["--validate"] if validate else []) + ["--pool-mode", pool]
        subprocess.run(cmd, check=True, cwd=ROOT)
        per = {}
        for r in _kernel_stats(d):
            c, t = per.get(r["Name"], (0, 0.0))
            per[r["Name"]] = (c + int(r["Calls"]), t + float(r["TotalDurationNs"]))
        for path in glob.glob(os.path.join(d, "**", "*"), recursive=True):     # keep the stats, drop the full trace
            if os.path.isfile(path) and not path.endswith("kernel_stats.csv"):
                os.remove(path)
        return per
    a, b = run(1), run(1 + iters)
    diff = {k: (b[k][0] - a.get(k, (0, 0.0))[0], b[k][1] - a.get(k, (0, 0.0))[1]) for k in b}
    diff = {k: v for k, v in diff.items() if v[0] > 0}
    calls = sum(v[0] for v in diff.values())
    sys.path.insert(0, os.path.join(ROOT, "hyperspectral_super-resolution_amd"))
    from s2_emit.ridge import ridge_dims
    dims = ridge_dims(10, 3, T)
    nf, na, ldq = dims.nf, dims.na, dims.ldq
    npix, npix10 = 100 * 100, 600 * 600

    def ns(pred):
        return sum(v[1] for k, v in diff.items() if pred(k)) / iters
    gram_ns = ns(lambda n: "gram_f64_lds_kernel" in n)
    pred_ns = ns(lambda n: "predict" in n)
    total_ns = ns(lambda n: True)
    rec = dict(P=P, T=T, launches_per_batch=calls / iters, kernel_ms_per_batch=round(total_ns / 1e6, 4),
               kernel_ms_per_pair=round(total_ns / 1e6 / P, 4),
               gram_tflops_f64=round(2.0 * npix * na * ldq * P / gram_ns / 1e3, 2) if gram_ns else None,
               predict_tflops_f32=round(2.0 * npix10 * nf * T * P / pred_ns / 1e3, 2) if pred_ns else None,
               **(report_fields(ns, P, npix, na, iters) if report else {}),
               **(validate_fields(ns, P, npix, T) if validate else {}),
               **(dict(pool=pool, pool_us_per_batch=round(ns(lambda n: "pool_" in n) / 1e3, 1)) if pool != "none" else {}),
               kernel_us_per_batch={k.split("(")[0][-60:]: round(v[1] / iters / 1e3, 1) for k, v in sorted(diff.items(), key=lambda kv: -kv[1][1])})
    print(json.dumps(rec), flush=True)


def report_fields(ns, P, npix, na, iters):
    part_ns = ns(lambda n: "pair_report_partial" in n)
    all_ns = ns(lambda n: "pair_report" in n)
    return dict(report_us_per_batch=round(all_ns / 1e3, 1), report_us_per_pair=round(all_ns / 1e3 / P, 2),
                q_read_tbps=round(P * npix * na * 8 / part_ns / 1e3, 2) if part_ns else None)


def validate_fields(ns, P, npix, T):
    part_ns = ns(lambda n: "pair_score_partial" in n)
    all_ns = ns(lambda n: "pair_score" in n)
    return dict(score_us_per_batch=round(all_ns / 1e3, 1), score_us_per_pair=round(all_ns / 1e3 / P, 2),
                score_read_tbps=round(4.0 * P * T * npix * 4 / part_ns / 1e3, 2) if part_ns else None,
                block_mean_us_per_batch=round(ns(lambda n: "block_mean" in n) / 1e3, 1),
                holdout_us_per_batch=round(ns(lambda n: "pair_holdout" in n) / 1e3, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help="P,T: run one configuration in this process")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-pairs", type=int, default=4)
    ap.add_argument("--batch-only", action="store_true", help="(profiling) time the batch only, no per-pair loop")
    ap.add_argument("--profile", default=None, help="directory for rocprofv3 output: profile every configuration")
    ap.add_argument("--configs", default=None, help="P,T;P,T... (default: all; with --report 64,32;64,285)")
    ap.add_argument("--report", action="store_true", help="time report=False against report=True")
    ap.add_argument("--validate", action="store_true", help="time validate=False against validate=True, and the score call "
                    "against a clone of the same bytes")
    ap.add_argument("--pool", action="store_true", help="time pool=None against pool='all' and groups of 8 pairs")
    ap.add_argument("--pool-mode", default="none", choices=("none", "all", "groups"), help="(profiling) the pooling of --batch-only")
    a = ap.parse_args()
    if a.child:
        P, T = map(int, a.child.split(","))
        if a.batch_only:
            sys.path.insert(0, ROOT)
            sys.path.insert(0, os.path.join(ROOT, "hyperspectral_super-resolution_amd"))
            import torch
            import s2_emit
            E, S = _pairs(torch, P)
            for _ in range(a.iters):
                kw = dict(pool=_pool_arg(a.pool_mode, P)) if a.pool_mode != "none" else {}
                s2_emit.fuse_tile_pairs(E, S, bands=32 if T == 32 else "all", s2_nodata=0.0, report=a.report, validate=a.validate, **kw)
            torch.cuda.synchronize()
            return
        if a.pool:
            child_pool(P, T, a.iters, a.warmup)
        elif a.validate:
            child_report(P, T, a.iters, a.warmup, "validate")
        elif a.report:
            child_report(P, T, a.iters, a.warmup)
        else:
            child(P, T, a.iters, a.warmup, a.host_pairs)
        return
    configs = [tuple(map(int, c.split(","))) for c in a.configs.split(";")] if a.configs else (REPORT_CONFIGS if a.report or a.validate or a.pool else CONFIGS)
    for P, T in configs:
        if a.profile and a.pool:
            for mode in ("all", "groups"):
                profile_one(P, T, a.iters, a.profile, pool=mode)
        elif a.profile:
            profile_one(P, T, a.iters, a.profile, a.report, a.validate)
        elif a.pool:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{P},{T}", "--iters", str(max(a.iters, 9)),
                            "--warmup", str(a.warmup), "--pool"], check=True)
        elif a.report or a.validate:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{P},{T}", "--iters", str(max(a.iters, 9)),
                            "--warmup", str(a.warmup), "--validate" if a.validate else "--report"], check=True)
        else:
            iters = a.iters if P * T < 64 * 285 else max(2, a.iters // 2)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{P},{T}", "--iters", str(iters),
                            "--warmup", str(a.warmup), "--host-pairs", str(a.host_pairs)], check=True)


if __name__ == "__main__":
    main()
