"""CPU-side tests of the product: host logic, the C-ABI surface, loud failure without a GPU."""
import ctypes
import os
import re
import zipfile

import numpy as np
import pytest

from conftest import ROOT, load_golden, unpack_srf
from oracle import oracle_np as onp

import s2_emit
from s2_emit import _engine as eng
from s2_emit import _native as nat


# ---------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------
def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "hsr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(hsr_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    lib = nat.load()
    names = _declared_symbols()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/hsr.h but not exported"
        assert n in nat.SIGNATURES, f"{n} has no ctypes signature in _native.py"
    assert set(nat.SIGNATURES) == set(names)
    assert lib.hsr_abi_version() == 5


def test_sizing_helpers_and_error_strings():
    lib = nat.load()
    assert [lib.hsr_moment_count(d) for d in (1, 2, 3, 4)] == [5, 8, 11, 14]
    assert lib.hsr_moment_count(0) == -1 and lib.hsr_moment_count(5) == -1
    assert lib.hsr_partial_slots(1, None) == 1 and lib.hsr_partial_slots(64, None) == 1 and lib.hsr_partial_slots(65, None) == 2
    assert lib.hsr_partial_slots(1 << 20, None) == 512 and lib.hsr_partial_slots(1 << 30, None) == 512
    # the slot layout is a function of (npix, options) only: no process-wide tuning state exists any more
    o = nat.SrfOptions(64, 0, 0, 0)
    assert lib.hsr_partial_slots(65, ctypes.byref(o)) == 2 and lib.hsr_partial_slots(1 << 20, ctypes.byref(o)) == 512
    assert lib.hsr_partial_slots(65, ctypes.byref(nat.SrfOptions(32, 0, 0, 0))) == -1        # 32-pixel geometry removed
    o = nat.SrfOptions(0, 8, 0, 0)
    assert lib.hsr_partial_slots(1 << 20, ctypes.byref(o)) == 496 and lib.hsr_partial_slots(1 << 20, None) == 512
    assert lib.hsr_partial_slots(100, ctypes.byref(nat.SrfOptions(48, 0, 0, 0))) == -1 and b"tile_pixels" in lib.hsr_last_error()
    assert lib.hsr_partial_slots(100, ctypes.byref(nat.SrfOptions(0, 200, 0, 0))) == -1
    assert not hasattr(lib, "hsr_set_srf_tile") and not hasattr(lib, "hsr_set_srf_reserved_cus")
    assert lib.hsr_partials_bytes(12, 3) == 12 * 11 * 4096 * 8
    assert lib.hsr_percentile_work_bytes(3) > 3 * (2048 + 4 * 2048 + 4 * 1024) * 4
    # argument validation happens before any device work -> testable without a GPU
    k = (ctypes.c_int32 * 1)(0)
    rc = lib.hsr_srf_integrate(None, 10, 285, None, k, k, 1, None, 10, 1, None, None)
    assert rc == 1 and b"NULL" in lib.hsr_last_error()
    rc = lib.hsr_srf_integrate(ctypes.c_void_p(16), 10, 9999, ctypes.c_void_p(16), k, k, 1, ctypes.c_void_p(16), 10, 1, None, None)
    assert rc == 2 and b"B=9999" in lib.hsr_last_error()
    rc = lib.hsr_poly_solve(None, 3, 2, 50, None, None)
    assert rc == 1
    # strides must describe band-major planes or pixel-major rows
    rc = lib.hsr_srf_integrate(ctypes.c_void_p(16), 10, 285, ctypes.c_void_p(16), k, k, 1, ctypes.c_void_p(16), 3, 7, None, None)
    assert rc == 1 and b"neither band-major nor pixel-major" in lib.hsr_last_error()
    bad = nat.SrfOptions(0, 0, 0, 7)
    rc = lib.hsr_srf_integrate(ctypes.c_void_p(16), 10, 285, ctypes.c_void_p(16), k, k, 1, ctypes.c_void_p(16), 10, 1, ctypes.byref(bad), None)
    assert rc == 1 and b"unknown bits" in lib.hsr_last_error()
    # the rows added later in the round validate the same way
    P = ctypes.c_void_p(256)
    assert lib.hsr_tile_decode_u16(P, 10, 1e-4, 70000, P, None) == 1 and b"not a uint16 value" in lib.hsr_last_error()
    assert lib.hsr_tile_decode_u16(None, 0, 1e-4, 65535, None, None) == 0            # empty input: nothing to do
    assert lib.hsr_tile_encode_u16(P, 10, 1e4, 0, 0.0, 0, P, None) == 1 and b"nodata_u16" in lib.hsr_last_error()
    assert lib.hsr_srf_integrate_u16(P, 10, 285, 1e-4, 1 << 20, P, k, k, 1, P, 10, 1, None, None) == 1
    assert lib.hsr_percentile_hist(4, P, 10, 1, None, 10, 1, P, None) == 1
    off, cnt = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.hsr_percentile_hist_region(1, 3, ctypes.byref(off), ctypes.byref(cnt)) == 0 and cnt.value == 3 * (2048 + 4)
    assert lib.hsr_percentile_hist_region(3, 3, ctypes.byref(off), ctypes.byref(cnt)) == 0 and cnt.value == 3 * 4 * 1024
    assert off.value + cnt.value * 4 <= lib.hsr_percentile_work_bytes(3)
    assert lib.hsr_ot_work_bytes(5000, 5000) > 5000 * 5000 * 8 and lib.hsr_ot_work_bytes(0, 5) == 0
    assert lib.hsr_ot_sinkhorn_barycentric(P, 10, P, 10, -1.0, 5, 1e-6, P, P, None, None) == 1 and b"reg must be > 0" in lib.hsr_last_error()
    assert lib.hsr_ot_iterate(10, 10, 0, 5, 1e-6, ctypes.c_void_p(8), None, None) == 1 and b"256-byte aligned" in lib.hsr_last_error()
    assert lib.hsr_gram_f64(P, 30, 32, P, 48, 48, 10, P, P, 48, None) == 1
    # one 2 KB tile of partial sums per (chunk, output tile): 29 chunks of <= 1024 rows for the register-operand kernel
    # (the LDS-panel kernel uses fewer, longer chunks: one workgroup per CU)
    assert lib.hsr_gram_work_bytes(288, 576, 29127) >= 29 * 18 * 36 * 256 * 8
    assert lib.hsr_gram_work_bytes(288, 320, 29127) >= 29 * 18 * 20 * 256 * 8 and lib.hsr_gram_work_bytes(8, 16, 100) == 0
    assert lib.hsr_probe_read(P, 1 << 20, 4, P, None) == 1 and b"mode" in lib.hsr_last_error()
    # entry points added in round 2 validate the same way (no launch without a GPU: every call below fails its checks first)
    assert lib.hsr_srf_integrate_fit(P, 10, 285, P, k, k, 1, P, 1, 16, P, 1, 16, None, 0.0, 0.0, 3, P, None, None, None, None) == 1
    assert b"NULL hsr_fused_fit" in lib.hsr_last_error()
    bad_fit = nat.FusedFit(0, 0, 0, 0, 50)
    assert lib.hsr_srf_integrate_fit(P, 10, 285, P, k, k, 1, P, 1, 16, P, 1, 16, None, 0.0, 0.0, 3, P, None, ctypes.byref(bad_fit), None, None) == 1
    assert b"NULL pointer in hsr_fused_fit" in lib.hsr_last_error()
    assert lib.hsr_ridge_stats_work_bytes(10) == 64 * 10 * 2 * 8 and lib.hsr_ridge_stats_work_bytes(17) == 0
    assert lib.hsr_ridge_stats(P, 10, 1, 0, 10, P, P, P, P, None) == 1 and b"hsr_ridge_stats" in lib.hsr_last_error()
    assert lib.hsr_ridge_assemble(P, 300, 288, 285, 32, 1.0, P, 256, P, 32, P, None) == 1 and b"bad shape" in lib.hsr_last_error()   # npad < nf
    assert lib.hsr_ridge_finish(P, 288, 285, 32, P, 16, P, P, 10, 286, P, P, P, P, P, None) == 1                                  # ldw < T
    assert lib.hsr_polyfeat_predict_cube(None, 1, 1, P, P, 10, 10, 3, P, 32, P, 32, 1, 1, -9999.0, 1, P, 10, None) == 1 and b"NULL" in lib.hsr_last_error()
    assert lib.hsr_interleave_to_bip(P, 0, 3, 4, 4, 4, P, 0, None) == 1


def test_ot_entry_points_refuse_bad_arguments():
    """Every refusal of the five Sinkhorn entry points comes before the first launch: none of these calls touches a device."""
    lib = nat.load()
    P, nan, big = ctypes.c_void_p(256), float("nan"), (1 << 20) + 1

    def refused(fn, ok, at, bad, code=1):
        args = list(ok)
        args[at] = bad
        rc = fn(*args)
        assert rc == code and lib.hsr_last_error(), (fn.__name__, at, bad, rc)

    begin = [P, 10, P, 10, 0.05, P, None]
    for at, bad in ((0, None), (2, None), (5, None), (4, 0.0), (4, nan), (4, -0.05), (5, ctypes.c_void_p(264))):
        refused(lib.hsr_ot_begin, begin, at, bad)
    iterate = [10, 10, 0, 5, 1e-6, P, None, None]
    for at, bad in ((5, None), (2, -1), (3, -1)):
        refused(lib.hsr_ot_iterate, iterate, at, bad)
    finish = [P, 10, 10, 5, P, P, None, None]
    for at, bad in ((0, None), (5, None), (4, None), (3, -1)):
        refused(lib.hsr_ot_finish, finish, at, bad)
    whole = [P, 10, P, 10, 0.05, 5, 1e-6, P, P, None, None]
    for at, bad in ((0, None), (2, None), (8, None), (7, None), (4, 0.0), (4, nan), (5, -1)):
        refused(lib.hsr_ot_sinkhorn_barycentric, whole, at, bad)
    refused(lib.hsr_ot_sinkhorn_barycentric, whole, 8, None)
    assert b"NULL ybar" in lib.hsr_last_error()                                  # refused by the call itself, not after begin's launch
    for fn, ok, n_at, m_at in ((lib.hsr_ot_begin, begin, 1, 3), (lib.hsr_ot_iterate, iterate, 0, 1), (lib.hsr_ot_finish, finish, 1, 2),
                               (lib.hsr_ot_sinkhorn_barycentric, whole, 1, 3)):
        for at in (n_at, m_at):
            for bad in (0, -1, big):
                refused(fn, ok, at, bad, code=2)
            assert b"outside [1, 2^20]" in lib.hsr_last_error()


def test_ot_work_regions():
    """hsr_ot_work_region: eight disjoint 256-byte aligned regions in the order state, K, partial, errpart, u0, u1, v0, v1 that end
    at hsr_ot_work_bytes; counts in 8-byte elements."""
    lib = nat.load()
    off, cnt = ctypes.c_int64(-1), ctypes.c_int64(-1)
    for n, m in ((1, 1), (1, 2), (64, 64), (65, 2), (257, 129), (3, 4162), (5000, 5000), (1 << 20, 1), (1, 1 << 20)):
        at = 0
        nchunks = (n + 63) // 64
        for which, want in enumerate((3, n * m, nchunks * m, (m + 63) // 64, n, n, m, m)):
            assert lib.hsr_ot_work_region(n, m, which, ctypes.byref(off), ctypes.byref(cnt)) == 0
            assert off.value == at and off.value % 256 == 0 and cnt.value == want, (n, m, which, off.value, cnt.value)
            at = off.value + (cnt.value * 8 + 255) // 256 * 256
        assert at == lib.hsr_ot_work_bytes(n, m)
    for which in (-1, 8, 1 << 30):
        assert lib.hsr_ot_work_region(10, 10, which, ctypes.byref(off), ctypes.byref(cnt)) == 1 and b"which" in lib.hsr_last_error()
    assert lib.hsr_ot_work_region(10, 10, 1, None, ctypes.byref(cnt)) == 1 and b"NULL" in lib.hsr_last_error()
    assert lib.hsr_ot_work_region(10, 10, 1, ctypes.byref(off), None) == 1
    for n, m in ((0, 10), (10, 0), ((1 << 20) + 1, 10), (10, (1 << 20) + 1)):
        assert lib.hsr_ot_work_region(n, m, 1, ctypes.byref(off), ctypes.byref(cnt)) == 2


def test_batch_plan_host_side():
    """hsr_batch_plan is pure host code: per-tile slot ranges == hsr_partial_slots of each tile, one unit per
    (tile, slot), longest units first, part_dev pointers inside the workspace."""
    lib = nat.load()
    npix = [10000, 64, 65, 1 << 20, 10000, 1]
    T = len(npix)
    tiles = (nat.BatchTile * T)()
    for i, n in enumerate(npix):
        tiles[i].cube_dev = 0x10000000 + i * 0x1000000
        tiles[i].real_dev = 0x20000000 + i * 0x1000000
        tiles[i].pseudo_dev = 0x30000000 + i * 0x1000000
        tiles[i].matched_dev = 0x40000000 + i * 0x1000000
        tiles[i].npix = n
    info = nat.BatchInfo()
    nb, deg, M = 12, 3, 11
    assert lib.hsr_batch_plan(tiles, T, nb, deg, None, None, None, 0, ctypes.byref(info)) == 0
    slots = [lib.hsr_partial_slots(n, None) for n in npix]
    assert [tiles[i].slots for i in range(T)] == slots == [64, 1, 2, 512, 64, 1]     # 157 groups -> 64 slots (hsr.h)
    assert [tiles[i].ngroups for i in range(T)] == [157, 1, 2, 16384, 157, 1]
    assert [tiles[i].slot0 for i in range(T)] == list(np.cumsum([0] + slots[:-1]))
    assert info.nunits == sum(slots) and info.total_pixels == sum(npix) and info.max_npix == 1 << 20
    assert info.ntiles == T and info.aligned16 == 1
    assert lib.hsr_batch_partials_bytes(info.nunits, nb, deg) == info.nunits * nb * M * 8
    n = int(info.nunits)
    buf = (ctypes.c_uint8 * (64 * n))()
    base = 0x50000000
    assert lib.hsr_batch_plan(tiles, T, nb, deg, ctypes.c_void_p(base), None, buf, n - 1, ctypes.byref(info)) == 1   # too small
    assert lib.hsr_batch_plan(tiles, T, nb, deg, ctypes.c_void_p(base), None, buf, n, ctypes.byref(info)) == 0
    rec = np.frombuffer(buf, dtype=np.dtype([("cube", "<u8"), ("real", "<u8"), ("mask", "<u8"), ("pseudo", "<u8"), ("part", "<u8"),
                                              ("npix", "<i8"), ("slots", "<i4"), ("slot", "<i4"), ("ngroups", "<i4"), ("pad", "<i4")]))
    assert len(rec) == n
    seen = set()
    lens = []
    for r in rec:
        t = [i for i in range(T) if tiles[i].cube_dev == int(r["cube"])][0]
        assert (int(r["npix"]), int(r["slots"]), int(r["ngroups"])) == (npix[t], slots[t], tiles[t].ngroups)
        assert 0 <= r["slot"] < slots[t] and (t, int(r["slot"])) not in seen
        seen.add((t, int(r["slot"])))
        assert int(r["part"]) == base + 8 * (int(tiles[t].slot0) + int(r["slot"])) * nb * M      # slot-major partials
        lens.append((tiles[t].ngroups - int(r["slot"]) + slots[t] - 1) // slots[t])
    assert len(seen) == n and lens == sorted(lens, reverse=True) and lens[0] == 32 and lens[-1] == 1
    # options: reserved CUs shrink the slot cap of the big tile only
    o = nat.SrfOptions(0, 8, 0, 0)
    assert lib.hsr_batch_plan(tiles, T, nb, deg, None, ctypes.byref(o), None, 0, ctypes.byref(info)) == 0
    assert tiles[3].slots == 496 and tiles[0].slots == 64
    # validation
    tiles[1].npix = 0
    assert lib.hsr_batch_plan(tiles, T, nb, deg, None, None, None, 0, ctypes.byref(info)) == 1 and b"npix" in lib.hsr_last_error()
    tiles[1].npix = 64
    tiles[2].pseudo_dev = 0x30000004
    assert lib.hsr_batch_plan(tiles, T, nb, deg, None, None, None, 0, ctypes.byref(info)) == 1 and b"16-byte" in lib.hsr_last_error()


def test_fused_launch_predicate_and_exchange_validation_host_side():
    """hsr_srf_fused_launch_supported is pure host code: the one predicate behind hsr_pipeline_create_fused / _exchange (ADVICE r3:
    Python's looser test let a launch fail with tiles in flight).  And the argument checks of the ABI 5 entry points that need no GPU."""
    lib = nat.load()
    from oracle import oracle_np as onp
    from s2_emit import _engine as eng
    w, good = onp.synthetic_wavelengths()
    t12 = eng.build_srf_table(w, onp.synthetic_srf(), good)
    k0 = (ctypes.c_int32 * t12.nb)(*[int(v) for v in t12.k0])
    kl = (ctypes.c_int32 * t12.nb)(*[int(v) for v in t12.klen])
    ok = lambda *a: lib.hsr_srf_fused_launch_supported(*a)
    assert ok(0, 285, t12.nb, k0, kl, 12, 3, None) == 0 and ok(2, 285, t12.nb, k0, kl, 12, 3, None) == 0
    assert ok(0, 285, t12.nb, k0, kl, 12, 0, None) == 2 and ok(0, 285, t12.nb, k0, kl, 10, 3, None) == 2      # degree 0; rows of 10 floats
    assert ok(2, 285, t12.nb, k0, kl, 12, 3, ctypes.byref(nat.SrfOptions(0, 0, 1, 0))) == 2                    # single-buffer uint16 kernel
    assert ok(1, 285, t12.nb, k0, kl, 12, 3, None) == 1
    # uint16 tiles with a wide spectrum, 13 bands in rows of 16 and long supports: the two ring buffers no longer fit next to them
    B = 300
    k0w = (ctypes.c_int32 * 13)(*[int(i * 10) for i in range(13)])
    klw = (ctypes.c_int32 * 13)(*([70] * 13))                   # 13 x 80 padded taps = 1040 > the 1024 floats reserved -> no LDS weights
    assert ok(2, B, 13, k0w, klw, 16, 3, None) == 2 and b"weight taps" in lib.hsr_last_error()
    klm = (ctypes.c_int32 * 13)(*([40] * 13))                   # 13 x 48 = 624 taps: fit, but 2 x 38 400 B + rows of 16 + taps > 80 KB
    assert ok(2, B, 13, k0w, klm, 16, 3, None) == 2 and b"80 KB" in lib.hsr_last_error()
    assert ok(0, B, 13, k0w, klm, 16, 3, None) == 0             # the float32 kernel has no such limit at B = 300
    assert ok(2, 40, 3, k0w, (ctypes.c_int32 * 3)(8, 8, 8), 4, 2, None) == 2                                   # B < 48: group buffers too small for the ring
    # exchange pipeline / communicator: argument errors come back as codes, nothing is dereferenced
    import torch  # noqa: F401  (first: hsr_comm_* binds the librccl.so.1 that is already mapped - PyTorch's own copy; loading ROCm's
    #                            copy and then PyTorch's puts two rocm_smi instances into the process, a double free at exit)
    assert lib.hsr_comm_available() in (0, 1)
    h = ctypes.c_void_p()
    assert lib.hsr_comm_init(3, 2, (ctypes.c_ubyte * 128)(), ctypes.byref(h)) == 1 and lib.hsr_comm_init(0, 1, None, ctypes.byref(h)) == 1
    assert lib.hsr_comm_unique_id(None) == 1 and lib.hsr_comm_destroy(None) == 0
    assert lib.hsr_comm_ranks(None) == -1 and lib.hsr_comm_rank(None) == -1
    assert lib.hsr_allreduce_f64(None, None, 0, None) == 1 and lib.hsr_bcast(None, None, 0, 0, None) == 1
    x = nat.Exchange()
    assert lib.hsr_pipeline_create_exchange(None, None, ctypes.byref(x), ctypes.byref(h)) == 1
    four = (ctypes.c_void_p * 4)()
    assert lib.hsr_pipeline_create_exchange(four, ctypes.c_void_p(1), ctypes.byref(x), ctypes.byref(h)) == 1 and b"exactly one" in lib.hsr_last_error()
    code = ctypes.c_uint32(7)
    assert lib.hsr_pipeline_status(None, None, ctypes.byref(code)) == 1


def test_k1_instance_table_and_launch_record_host_side():
    """The K1 diagnostics need no device: the table query reports the 106 instances (5 degrees x 22 variants, minus the four
    degree-0 apply slots) and refuses entries outside the table; the launch record starts empty, a call refused before its
    launch leaves it empty, and a read clears it."""
    lib = nat.load()
    present = {(d, v) for d in range(nat.HSR_MAX_DEG + 1) for v in range(22) if lib.hsr_srf_kernel_instance(d, v) == 1}
    empty = {(d, v) for d in range(nat.HSR_MAX_DEG + 1) for v in range(22) if lib.hsr_srf_kernel_instance(d, v) == 0}
    assert len(present) == 106 and empty == {(0, 5), (0, 6), (0, 18), (0, 19)}
    for d, v in ((-1, 0), (5, 0), (0, -1), (0, 22), (4, 1 << 20)):
        assert lib.hsr_srf_kernel_instance(d, v) == -1 and b"hsr_srf_kernel_instance" in lib.hsr_last_error()
    deg, var, lds = ctypes.c_int32(7), ctypes.c_int32(7), ctypes.c_int64(7)
    lib.hsr_srf_last_launch(None, None, None)                    # whatever an earlier test left
    assert lib.hsr_srf_last_launch(ctypes.byref(deg), ctypes.byref(var), ctypes.byref(lds)) == 0
    assert (deg.value, var.value, lds.value) == (-1, -1, -1)
    k = (ctypes.c_int32 * 1)(0)
    rc = lib.hsr_srf_integrate(ctypes.c_void_p(16), 10, 9999, ctypes.c_void_p(16), k, k, 1, ctypes.c_void_p(16), 10, 1, None, None)
    assert rc == 2 and lib.hsr_srf_last_launch(ctypes.byref(deg), ctypes.byref(var), ctypes.byref(lds)) == 0


def test_step_plan_and_pipeline_creation_checks_host_side():
    """hsr_step_plan_create makes no HIP call, and the pipeline create functions check every argument before their first one:
    plans over fake device pointers (none is dereferenced) and the pipelines over them are refused with their messages."""
    lib = nat.load()
    w, good = onp.synthetic_wavelengths()
    t12 = eng.build_srf_table(w, onp.synthetic_srf(), good)
    nb = t12.nb
    k0 = (ctypes.c_int32 * nb)(*[int(v) for v in t12.k0])
    kl = (ctypes.c_int32 * nb)(*[int(v) for v in t12.klen])
    fake = iter(range(0x7f0000000000, 0x7f0100000000, 1 << 20))          # distinct, 16-byte aligned, never dereferenced

    def desc(reserved_cus=0, **kw):
        d = nat.StepDesc()
        d.cube_dtype, d.B, d.npix, d.nb, d.deg, d.min_count = 0, 285, 64 * 64, nb, 3, 5
        d.k0, d.klen = ctypes.cast(k0, ctypes.POINTER(ctypes.c_int32)), ctypes.cast(kl, ctypes.POINTER(ctypes.c_int32))
        d.out_bs, d.out_ps, d.matched_bs, d.matched_ps, d.real_bs, d.real_ps = 1, 12, 1, 12, 1, 12
        d.opts = nat.SrfOptions(0, reserved_cus, 0, 0)
        for f in ("wn_dev", "pseudo_dev", "partials_dev", "moments_dev", "coeffs_dev", "matched_dev"):
            setattr(d, f, next(fake))
        for f, v in kw.items():
            setattr(d, f, v)
        return d

    made = []

    def plan(d):
        h = ctypes.c_void_p()
        assert lib.hsr_step_plan_create(ctypes.byref(d), ctypes.byref(h)) == 0, lib.hsr_last_error()
        made.append(h)
        return h

    def refused(rc, code, msg):
        assert rc == code and msg in lib.hsr_last_error(), (rc, lib.hsr_last_error())

    h = ctypes.c_void_p()
    refused(lib.hsr_step_plan_create(None, ctypes.byref(h)), 1, b"NULL argument")
    refused(lib.hsr_step_plan_create(ctypes.byref(desc(nb=0)), ctypes.byref(h)), 1, b"nb=0 outside")
    refused(lib.hsr_step_plan_create(ctypes.byref(desc(k0=None)), ctypes.byref(h)), 1, b"NULL band tables")
    refused(lib.hsr_step_plan_create(ctypes.byref(desc(deg=5)), ctypes.byref(h)), 1, b"deg=5 outside")
    refused(lib.hsr_step_plan_create(ctypes.byref(desc(cube_dtype=1)), ctypes.byref(h)), 1, b"cube_dtype 1")
    refused(lib.hsr_step_plan_create(ctypes.byref(desc(coeffs_dev=None)), ctypes.byref(h)), 1, b"NULL device pointer")
    refused(lib.hsr_step_plan_create(ctypes.byref(desc(npix=0)), ctypes.byref(h)), 1, b"npix < 1")
    try:
        ds = [desc() for _ in range(4)]
        p = [plan(d) for d in ds]
        assert lib.hsr_step_plan_slots(p[0]) == 0 and lib.hsr_step_plan_slots(None) == -1
        side = ctypes.c_void_p(0x1000)                 # a stream handle is only compared with NULL before the first HIP call
        for field in ("partials_dev", "moments_dev", "coeffs_dev", "pseudo_dev", "matched_dev"):
            shared = plan(desc(**{field: getattr(ds[1], field)}))
            refused(lib.hsr_pipeline_create_fused(p[0], p[1], shared, side, 0, ctypes.byref(h)), 1, b"plans 1 and 2 share a work buffer")
            four = (ctypes.c_void_p * 4)(p[0], p[1], p[2], shared)
            refused(lib.hsr_pipeline_create_group(four, 4, 2, side, side, side, side, ctypes.byref(h)), 1, b"plans 1 and 3 share a work buffer")
        refused(lib.hsr_pipeline_create_fused(p[0], p[1], p[1], side, 0, ctypes.byref(h)), 1, b"distinct plans needed")
        refused(lib.hsr_pipeline_create_fused(p[0], None, p[2], side, 0, ctypes.byref(h)), 1, b"NULL plan")
        refused(lib.hsr_pipeline_create_fused(p[0], p[1], p[2], side, 1, ctypes.byref(h)), 2, b"no exchange in the three-slot form")
        refused(lib.hsr_pipeline_create_fused(p[0], p[1], p[2], None, 0, ctypes.byref(h)), 1, b"side stream must be a real stream")
        refused(lib.hsr_pipeline_create_fused(p[0], p[1], p[2], side, 0, None), 1, b"NULL argument")
        # geometry: every plan like the first, 16-byte aligned pixel-major rows of 4 / 8 / 12 / 16 floats
        for kw in (dict(npix=64 * 63), dict(B=284), dict(deg=2), dict(out_ps=16, matched_ps=16), dict(pseudo_dev=next(fake) + 4),
                   dict(matched_ps=16), dict(out_bs=2), dict(cube_dtype=2), dict(reserved_cus=8)):
            odd = plan(desc(**kw))
            refused(lib.hsr_pipeline_create_fused(p[0], p[1], odd, side, 0, ctypes.byref(h)), 2, b"the same geometry")
            four = (ctypes.c_void_p * 4)(p[0], p[1], p[2], odd)
            refused(lib.hsr_pipeline_create_group(four, 4, 2, side, side, side, side, ctypes.byref(h)), 2, b"the same geometry")
        # group sizes: group_tiles + 2 plans, 2 .. 64 tiles
        four = (ctypes.c_void_p * 4)(*p)
        for nslots, tiles in ((4, 1), (3, 1), (2, 0), (4, 3), (5, 2), (67, 65)):
            refused(lib.hsr_pipeline_create_group(four, nslots, tiles, side, side, side, side, ctypes.byref(h)), 1, b"groups of 2 .. 64 tiles")
        refused(lib.hsr_pipeline_create_group(four, 4, 2, side, None, side, side, ctypes.byref(h)), 1, b"NULL argument")
        refused(lib.hsr_pipeline_create_group(four, 4, 2, side, side, side, None, ctypes.byref(h)), 1, b"side stream must be a real stream")
        # exchange: CUs kept free for the side stream, then the same plan checks as the other fused forms
        x = nat.Exchange()
        x.mode, x.host_sum = nat.HSR_SYNC_ALLREDUCE, nat.HOST_SUM_FN(lambda user, values, count: 0)
        refused(lib.hsr_pipeline_create_exchange(four, side, ctypes.byref(x), ctypes.byref(h)), 1, b"at least 8 CUs free")
        ds8 = [desc(reserved_cus=8) for _ in range(3)]
        p8 = [plan(d) for d in ds8] + [plan(desc(reserved_cus=8, coeffs_dev=ds8[0].coeffs_dev))]
        refused(lib.hsr_pipeline_create_exchange((ctypes.c_void_p * 4)(*p8), side, ctypes.byref(x), ctypes.byref(h)), 1,
                b"plans 0 and 3 share a work buffer")
        refused(lib.hsr_pipeline_create_exchange((ctypes.c_void_p * 4)(*p8[:3], p8[0]), side, ctypes.byref(x), ctypes.byref(h)), 1,
                b"distinct plans needed")
        assert not h.value                             # nothing was created
    finally:
        for m in made:
            lib.hsr_step_plan_destroy(m)


def test_polyfeat_table_matches_sklearn_order():
    lib = nat.load()
    assert lib.hsr_polyfeat_count(10, 3) == 285 and lib.hsr_polyfeat_count(10, 2) == 65
    assert lib.hsr_polyfeat_count(17, 3) == -1 and lib.hsr_polyfeat_count(10, 4) == -1
    buf = (ctypes.c_uint8 * (285 * 3))()
    assert lib.hsr_polyfeat_table(10, 3, buf) == 0
    idx = np.frombuffer(buf, dtype=np.uint8).reshape(285, 3)
    expo = np.zeros((285, 10), int)
    for f in range(285):
        for k in idx[f]:
            if k < 10:
                expo[f, k] += 1
    np.testing.assert_array_equal(expo, load_golden("g7_ridge")["powers"])     # sklearn's powers_


def test_polyfeat_predict_kernel_selection_host_side():
    """hsr_polyfeat_predict_kernel, the rule launch_predict takes, at every slot boundary: (10, 3) with the orbit rows on the
    device takes x16 (0) up to 16 targets, then slice<per> (1 .. 3) for the 32-target tiles per slice up to 512; every other
    shape - and (10, 3) without the rows - the generic predict_kernel<1 / 2 / 4> (4 .. 6) by the tiles a wave pair covers."""
    lib = nat.load()
    q = lib.hsr_polyfeat_predict_kernel
    orb = {1: 0, 16: 0, 17: 1, 32: 1, 33: 2, 64: 2, 65: 3, 96: 3, 97: 2, 128: 2, 129: 3, 192: 3, 193: 3, 256: 3, 257: 3,
           285: 3, 512: 3, 513: 6}
    generic = {1: 4, 16: 4, 17: 4, 32: 4, 33: 4, 64: 4, 65: 5, 96: 5, 97: 5, 128: 5, 129: 6, 256: 6, 257: 6, 285: 6, 513: 6}
    for T, slot in orb.items():
        assert q(10, 3, T, 1) == slot, T
    for T, slot in generic.items():
        assert q(10, 3, T, 0) == slot, T
        for n_in, deg in ((9, 3), (10, 2), (1, 1), (4, 3), (16, 2), (12, 3), (13, 3)):
            assert q(n_in, deg, T, 1) == slot and q(n_in, deg, T, 0) == slot and q(n_in, deg, T, -1) == slot, (n_in, deg, T)
    # as the library stands: the rows are either on the device (after a (10, 3) prepare on a GPU) or not, for every T alike
    now = [q(10, 3, T, -1) for T in orb]
    assert now == list(orb.values()) or now == [q(10, 3, T, 0) for T in orb], now
    # shapes no kernel takes: no monomial table, no target, or a feature tile beyond the generic kernel's LDS
    for n_in, deg, T in ((17, 3, 32), (10, 4, 32), (0, 1, 32), (10, 3, 0), (14, 3, 32), (16, 3, 1)):
        assert q(n_in, deg, T, 1) == -1 and b"hsr_polyfeat_predict_kernel" in lib.hsr_last_error(), (n_in, deg, T)


def test_polyridge_rejects_systems_beyond_the_cholesky_bound(monkeypatch):
    """More than 512 polynomial features (13 inputs at degree 3: 559) is a ValueError naming nf and the bound, raised by fit and
    local_gram before anything is launched (the GPU is never asked for); 12 inputs (454) pass the check."""
    from s2_emit import ridge

    def no_gpu():
        raise AssertionError("the GPU was asked for")

    monkeypatch.setattr(nat, "require_gpu", no_gpu)
    assert ridge.check_fit_features(12, 3) == 454 == nat.load().hsr_polyfeat_count(12, 3)
    assert ridge.check_fit_features(16, 2) == 152 and ridge.check_fit_features(10, 3) == 285
    for n_in, deg, nf in ((13, 3, 559), (16, 3, 968)):
        X, Y = np.zeros((20, n_in), np.float32), np.zeros((20, 2))
        with pytest.raises(ValueError, match=f"nf={nf} .* at most 512"):
            s2_emit.PolyRidge(deg, 1.0).fit(X, Y)
        with pytest.raises(ValueError, match=f"nf={nf} .* at most 512"):
            s2_emit.PolyRidge(deg, 1.0).local_gram(X, Y, None, None)
    with pytest.raises(AssertionError, match="GPU was asked"):
        s2_emit.PolyRidge(3, 1.0).fit(np.zeros((20, 12), np.float32), np.zeros((20, 2)))


def test_compute_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    srf = onp.synthetic_srf()
    w, good = onp.synthetic_wavelengths()
    with pytest.raises(nat.HsrUnavailable):
        s2_emit.pseudo_s2_srf_integral(np.zeros((2, 2, 285), np.float32), w, srf, good)
    with pytest.raises(nat.HsrUnavailable):
        s2_emit.apply_poly_rgb(np.zeros((2, 2, 3), np.float32), np.zeros((3, 3)))
    with pytest.raises(nat.HsrUnavailable):
        s2_emit.apply_shared_percentile_stretch(np.zeros((2, 2, 3), np.float32), np.ones((2, 2), bool))


def test_missing_library_message(monkeypatch):
    monkeypatch.setattr(nat, "_lib", None)
    monkeypatch.setenv("HSR_LIBRARY", "/nonexistent/libhsr.so")
    with pytest.raises(nat.HsrUnavailable) as ei:
        nat.load()
    assert "no CPU fallback" in str(ei.value)
    monkeypatch.delenv("HSR_LIBRARY")
    nat.load()


# ---------------------------------------------------------------------------------------------
# host solve: np.polyfit from moments
# ---------------------------------------------------------------------------------------------
def _moments(x, y, deg):
    x = x.astype(np.float64)
    S = [np.sum(x ** k) for k in range(2 * deg + 1)]
    T = [np.sum(x ** j * y) for j in range(deg + 1)]
    return np.array(S + T)


@pytest.mark.parametrize("deg", [1, 2, 3, 4])
def test_solve_host_matches_polyfit_golden(deg):
    g = load_golden("g3_polyfit")
    for N in (200, 5000):
        x, y = g[f"x_{N}"], g[f"y_{N}"]
        c = eng.poly_solve_host(_moments(x, y, deg)[None], deg, 0)[0]
        np.testing.assert_allclose(c, g[f"coef_{N}_{deg}"], rtol=2e-8, atol=1e-10)
    xf, yf = g["xf32"].astype(np.float64), g["yf32"].astype(np.float64)
    c = eng.poly_solve_host(_moments(xf, yf, deg)[None], deg, 50)[0]
    np.testing.assert_allclose(c, g[f"coef_f32_{deg}"], rtol=2e-8, atol=1e-10)


def test_solve_host_fallbacks_and_rank_loss():
    m = _moments(np.linspace(0, 1, 40), np.linspace(0, 1, 40), 2)
    np.testing.assert_array_equal(eng.poly_solve_host(m[None], 2, 50)[0], [0.0, 1.0, 0.0])
    np.testing.assert_array_equal(eng.poly_solve_host(np.zeros((1, 14)), 4, 0)[0], [0, 0, 0, 1, 0])
    # constant x: rank-1 Vandermonde -> minimum-norm solution like np.polyfit (no NaN, same values)
    x = np.full(300, 0.5)
    y = np.full(300, 0.25)
    c = eng.poly_solve_host(_moments(x, y, 2)[None], 2, 50)[0]
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = np.polyfit(x, y, 2)
    np.testing.assert_allclose(c, ref, rtol=1e-9, atol=1e-12)
    # x = 0.3: its powers round in float64, so the Gram is singular only up to rounding; the coefficients (the unique
    # minimum-norm solution) must still be np.polyfit's, not noise inflated into the null space
    x = np.full(10000, np.float32(0.3))
    y = np.random.default_rng(0).uniform(0, 1, 10000).astype(np.float32)
    for deg in (1, 2, 3, 4):
        c = eng.poly_solve_host(_moments(x, y, deg)[None], deg, 50)[0]
        ref = _polyfit_quiet(x, y, deg)
        assert np.max(np.abs(c - ref)) <= 1e-9 * np.max(np.abs(ref)), (deg, c, ref)


def _polyfit_quiet(x, y, deg):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.polyfit(x.astype(np.float64), y.astype(np.float64), deg)


RANK_VALUES = {1: [0.3], 2: [0.2, 0.7], 3: [0.2, 0.5, 0.9], 4: [0.1, 0.4, 0.7, 0.95]}


@pytest.mark.parametrize("nd", [1, 2, 3, 4])
def test_solve_host_rank_deficient_matches_polyfit_coefficients(nd):
    """Exactly rank-deficient bands (nd distinct float32 values, deg >= nd) have one minimum-norm solution: the host twin
    must return np.polyfit's coefficients, and the polynomial must agree beyond the data.  Worst measured: 2e-11."""
    rng = np.random.default_rng(nd)
    for n in (50, 333, 1000, 10000, 100000):
        for scale in (1e-3, 1.0, 1e3):
            for deg in range(nd, 5):
                x = np.repeat(np.float32(np.array(RANK_VALUES[nd]) * scale), (n + nd - 1) // nd)[:n]
                y = rng.uniform(0, 1, n).astype(np.float32)
                c = eng.poly_solve_host(_moments(x, y, deg)[None], deg, 0)[0]
                ref = _polyfit_quiet(x, y, deg)
                what = (nd, n, scale, deg, c, ref)
                assert np.max(np.abs(c - ref)) <= 1e-9 * np.max(np.abs(ref)), what
                grid = np.linspace(0, 1.5 * scale, 64)
                pr = np.polyval(ref, grid)
                assert np.max(np.abs(np.polyval(c, grid) - pr)) <= 1e-9 * np.max(np.abs(pr)), what


def test_solve_host_conditioning_envelope():
    """Raw power sums lose the centred information of a narrow x range (solve).  Whenever cond(V/s) <= 1e5 the
    predictions on the training x must match np.polyfit's to 1e-9; the sweep reaches cond ~1e16 and must stay finite."""
    rng = np.random.default_rng(0)
    checked = 0
    for lo, hi in ((0.0, 1.0), (0.1, 0.12), (0.28, 0.32), (0.30, 0.31), (0.79, 0.81), (0.5, 0.505), (0.9, 0.9001)):
        for deg in (1, 2, 3, 4):
            x = rng.uniform(lo, hi, 10000).astype(np.float32)
            y = (np.sin(3 * x) + 0.5 * x * x + 0.01 * rng.standard_normal(10000)).astype(np.float32)
            X = x.astype(np.float64)
            V = np.vander(X, deg + 1)
            cond = np.linalg.cond(V / np.sqrt((V * V).sum(0)))
            c = eng.poly_solve_host(_moments(x, y, deg)[None], deg, 0)[0]
            err = np.max(np.abs(np.polyval(c, X) - np.polyval(_polyfit_quiet(x, y, deg), X)))
            assert np.isfinite(c).all() and err < 1e-2, (lo, hi, deg, cond, err)
            if cond <= 1e5:
                assert err <= 1e-9, (lo, hi, deg, cond, err)
                checked += 1
    assert checked >= 12


def test_poly_launch_record_host_side():
    """hsr_poly_last_launch: empty at the start, no record after calls refused before their launch, cleared on read."""
    lib = nat.load()
    buf = ctypes.create_string_buffer(64)
    lib.hsr_poly_last_launch(None, 0)                            # whatever an earlier test left
    buf.value = b"junk"
    assert lib.hsr_poly_last_launch(buf, 64) == 0 and buf.value == b""
    f = ctypes.c_void_p(16)
    assert lib.hsr_poly_apply(None, 1, 4, None, None, 1, 1, 10, None, 0, None, 1, 4, None) == 1
    assert lib.hsr_poly_apply(f, 1, 4, None, None, 17, 1, 10, None, 0, f, 1, 4, None) == 2
    assert lib.hsr_poly_moments(f, 1, 4, f, 1, 4, None, 10, 1, 9, 0.0, 0.0, None, None, f, None, None) == 2
    assert lib.hsr_moments_reduce(f, 0, 1, 1, f, None) == 1 and lib.hsr_moments_reduce_solve(f, 5000, 1, 1, 0, f, f, None) == 1
    assert lib.hsr_poly_solve(None, 1, 1, 0, f, None) == 1 and lib.hsr_valid_mask(None, 1, 1, 1, 0, None, 0, 0, 0, None, 1, f, None) == 1
    assert lib.hsr_moments_reduce_solve_batched(f, 0, f, 1, 1, 0, f, f, None) == 2
    assert lib.hsr_poly_apply_batched(f, 1, 10, f, 4, 1, 2, 0, 0, None) == 2
    assert lib.hsr_poly_apply(f, 1, 4, None, None, 1, 1, 0, None, 0, f, 1, 4, None) == 0      # npix 0: nothing launched
    assert lib.hsr_poly_last_launch(buf, 64) == 0 and buf.value == b""
    assert lib.hsr_poly_last_launch(None, 0) == 0


def test_aux_launch_record_host_side():
    """hsr_aux_last_launch: empty at the start, no record after calls refused (or with nothing to do) before their launch,
    capacity handling, cleared on read."""
    lib = nat.load()
    lib.hsr_aux_last_launch(None, 0)                             # whatever an earlier test left
    buf = ctypes.create_string_buffer(64)
    buf.value = b"junk"
    assert lib.hsr_aux_last_launch(buf, 64) == 0 and buf.value == b""
    buf.value = b"junk"
    assert lib.hsr_aux_last_launch(buf, 0) == 0 and buf.value == b"junk"      # capacity < 1: the buffer is not touched
    assert lib.hsr_aux_last_launch(buf, -5) == 0 and buf.value == b"junk"
    assert lib.hsr_aux_last_launch(buf, 1) == 0 and buf.raw[0] == 0            # room for the terminator alone
    f = ctypes.c_void_p(16)
    assert lib.hsr_percentile_limits(None, 10, 1, None, 10, 1, 2.0, 98.0, f, f, None) == 1
    assert lib.hsr_percentile_limits(f, 10, 1, None, 10, 1, 2.0, 101.0, f, f, None) == 1
    assert lib.hsr_percentile_limits(f, 10, 1, None, 10, 17, 2.0, 98.0, f, f, None) == 2
    assert lib.hsr_percentile_hist(4, f, 10, 1, None, 10, 1, f, None) == 1
    assert lib.hsr_percentile_hist(1, f, 5, 1, None, 10, 1, f, None) == 1         # neither band-major nor pixel-major
    assert lib.hsr_percentile_hist(1, f, 10, 1, None, 0, 1, f, None) == 0         # npix 0: nothing launched
    assert lib.hsr_percentile_scan(0, 1, 2.0, 98.0, f, f, None) == 1
    assert lib.hsr_block_mean(None, 0, 1, 1, 1, 1, 1, 1, 1.0, f, 1, 1, None) == 1
    assert lib.hsr_block_mean(f, 0, 1, 1, 1, 1, 1, 65, 1.0, f, 1, 1, None) == 1
    assert lib.hsr_bilinear_upsample(f, 1, 1, 1, 0, 1, 1, f, 1, 1, None) == 1
    assert lib.hsr_bilinear_upsample_mask_hist(f, 1, 4, 5, 1, 1, 1, f, f, f, None) == 2
    assert lib.hsr_tile_encode_u16(f, -1, 1e4, 0, 0.0, 65535, f, None) == 1
    assert lib.hsr_tile_encode_u16(None, 0, 1e4, 0, 0.0, 65535, None, None) == 0  # n 0: nothing launched
    assert lib.hsr_tile_decode_u16(None, 0, 1e-4, 65535, None, None) == 0
    assert lib.hsr_tile_decode_u16(f, 4, 1e-4, 70000, f, None) == 1
    assert lib.hsr_interleave_to_bip(f, 0, 3, 1, 1, 1, f, 0, None) == 1
    assert lib.hsr_interleave_to_bip(f, 0, 1, 0, 1, 1, f, 0, None) == 1
    assert lib.hsr_aux_last_launch(buf, 64) == 0 and buf.value == b""
    assert lib.hsr_aux_last_launch(None, 0) == 0


def test_k4_launch_record_host_side():
    """hsr_k4_last_launch: empty without a launch, nothing added by calls refused by their argument checks (NULL pointer,
    n % 32 != 0, ldw < T, ...), capacity handling, cleared on read; hsr_k4_instance_name: unique, stable, the spellings of the
    sources with every host-computed path as a suffix."""
    lib = nat.load()
    lib.hsr_k4_last_launch(None, 0)                              # whatever an earlier test left
    buf = ctypes.create_string_buffer(64)
    buf.value = b"junk"
    assert lib.hsr_k4_last_launch(buf, 64) == 0 and buf.value == b""
    buf.value = b"junk"
    assert lib.hsr_k4_last_launch(buf, 0) == 0 and buf.value == b"junk"       # capacity < 1: the buffer is not touched
    assert lib.hsr_k4_last_launch(buf, -5) == 0 and buf.value == b"junk"
    assert lib.hsr_k4_last_launch(buf, 1) == 0 and buf.raw[0] == 0             # room for the terminator alone
    f = ctypes.c_void_p(16)
    assert lib.hsr_ridge_stats(None, 1, 1, 10, 1, f, f, f, f, None) == 1 and b"NULL" in lib.hsr_last_error()
    assert lib.hsr_ridge_stats(f, 1, 1, 0, 1, f, f, f, f, None) == 1
    assert lib.hsr_ridge_stats(f, 1, 1, 10, 17, f, f, f, f, None) == 1
    assert lib.hsr_polyfeat_expand_f64(None, 1, 1, f, f, 10, 1, 1, f, 2, 2, None) == 1
    assert lib.hsr_pair_expand_f64(f, 0, f, f, 0, f, 0, None, 0, 10, 1, 1, 1, 1e-4, f, 32, 0, 16, 1, None) == 1
    assert lib.hsr_gram_f64(f, 16, 16, None, 16, 16, 10, f, f, 16, None) == 1
    assert lib.hsr_gram_f64(f, 16, 24, f, 16, 16, 10, f, f, 16, None) == 1           # na % 16 != 0
    assert lib.hsr_gram_f64_batched(f, 16, 32, 16, 10, 0, f, 0, f, 16, 0, 1, None) == 1   # nb < na
    assert lib.hsr_chol_solve_f64(f, 48, 48, f, 1, 1, f, f, None) == 2 and b"multiple of 32" in lib.hsr_last_error()
    assert lib.hsr_chol_solve_f64(f, 32, 32, f, 1, 1, f, None, None) == 1
    assert lib.hsr_chol_solve_f64(f, 31, 32, f, 1, 1, f, f, None) == 1                # lda < n
    assert lib.hsr_chol_solve_f64_batched(f, 544, 544, 0, f, 1, 1, 0, f, f, 1, None) == 2
    assert lib.hsr_ridge_assemble(f, 20, 16, 4, 8, 1.0, f, 32, f, 7, f, None) == 1    # ldb < T
    assert lib.hsr_ridge_assemble_batched(f, 24, 0, 16, 4, 8, 1.0, f, 32, 0, f, 8, 0, f, 0, None) == 1
    assert lib.hsr_ridge_finish(f, 16, 4, 8, f, 7, f, f, 4, 4, f, f, f, f, f, None) == 1   # ldw < T
    assert lib.hsr_ridge_finish_batched(f, 0, 16, 4, 8, f, 8, 0, f, f, 0, 4, 4, f, f, 0, f, 0, f, f, 0, f, None, 1, None) == 1
    assert lib.hsr_polyfeat_predict(f, 4, 1, f, f, 10, 4, 1, f, 7, f, 8, 0, f, 10, None) == 1       # ldw < T
    assert lib.hsr_polyfeat_predict_cube(f, 4, 1, f, f, 10, 4, 1, f, 8, f, 8, 0, 0, 0.0, 0, f, 9, None) == 1   # out_stride < npix
    assert lib.hsr_polyfeat_predict_cube_batched(f, 4, 1, 0, f, f, 0, 10, 4, 1, f, 8, 0, f, 0, 8, 0, 0, 0.0, 0, f, 10, 0, 0,
                                                 None) == 1
    assert lib.hsr_k4_last_launch(buf, 64) == 0 and buf.value == b""
    assert lib.hsr_k4_last_launch(None, 0) == 0
    n = lib.hsr_k4_instance_count()
    assert n == 31 and lib.hsr_k4_instance_count() == n
    names = [lib.hsr_k4_instance_name(i) for i in range(n)]
    assert all(isinstance(s, bytes) and s for s in names) and len(set(names)) == n
    assert names == [lib.hsr_k4_instance_name(i) for i in range(n)]
    for bad in (-1, n, 1 << 20):
        assert lib.hsr_k4_instance_name(bad) is None and b"hsr_k4_instance_name" in lib.hsr_last_error()
    want = ({"expand_f64_kernel", "pair_expand_f64_kernel", "ridge_stats_partial_kernel", "ridge_stats_finish_kernel",
             "ridge_assemble_kernel", "ridge_finish_kernel", "predict_kernel<1>", "predict_kernel<2>", "predict_kernel<4>"}
            | {f"{k} {arm}" for k in ("predict103_x16_kernel", "predict103_slice_kernel<1>", "predict103_slice_kernel<2>",
                                      "predict103_slice_kernel<3>") for arm in ("x2", "scalar")}
            | {f"gram_f64_lds_kernel {k}" for k in ("wide", "diag", "narrow", "wide+diag", "wide+narrow", "diag+narrow",
                                                    "wide+diag+narrow")}
            | {"gram_f64_kernel sym", "gram_f64_kernel full", "gram_reduce_kernel", "chol_factor_res_kernel", "chol_factor_kernel",
               "chol_solve_kernel lds", "chol_solve_kernel global"})
    assert {s.decode() for s in names} == want
    assert max(len(a) + 2 + len(b) for a in names for b in names) < 96     # any two names joined fit a 96-byte buffer


def test_pairs_launch_record_host_side():
    """hsr_pairs_last_launch: empty without a launch (reads as 0), nothing added by calls their argument checks refuse, capacity
    handling; hsr_pairs_instance_name: the 12 names in the table's order, NULL and the error text outside [0, 12)."""
    lib = nat.load()
    lib.hsr_pairs_last_launch(None, 0)                           # whatever an earlier test left
    buf = ctypes.create_string_buffer(64)
    buf.value = b"junk"
    assert lib.hsr_pairs_last_launch(buf, 64) == 0 and buf.value == b""
    buf.value = b"junk"
    assert lib.hsr_pairs_last_launch(buf, 0) == 0 and buf.value == b"junk"    # capacity < 1: the buffer is not touched
    assert lib.hsr_pairs_last_launch(buf, -5) == 0 and buf.value == b"junk"
    assert lib.hsr_pairs_last_launch(buf, 1) == 0 and buf.raw[0] == 0          # room for the terminator alone
    f = ctypes.c_void_p(16)
    assert lib.hsr_pair_prep(f, 2, 0, 4, f, 5, f, 2, 0, 1, 2, 2, 2, 0.0, 0, 0.0, 0, f, f, f, 1, None) == 1     # T > emit_bands
    assert lib.hsr_pair_prep(f, 2, 0, 4, f, 1, f, 2, 0, 17, 2, 2, 2, 0.0, 0, 0.0, 0, f, f, f, 1, None) == 1    # nb = 17
    assert lib.hsr_pair_prep(f, 2, 0, 4, f, 1, f, 2, 0, 1, 2, 2, 0, 0.0, 0, 0.0, 0, f, f, f, 1, None) == 2     # a uint16 coarse image
    assert lib.hsr_pair_stats(f, f, 0, 1, f, f, f, f, 1, None) == 1
    assert lib.hsr_pair_report_f64(f, 16, 0, 24, 10, f, 0, f, 1, 0, 3, f, 0, f, 0, 1, f, f, 4, f, f, 0, 1, None) == 1   # na % 16 != 0
    assert lib.hsr_pair_holdout(f, None, 10, 10, f, f, 1, None) == 1
    assert lib.hsr_pair_score_f64(f, 0, f, 0, f, 0, 10, 1, 1.0, f, 1, f, f, f, f, 0, f, f, f, 0, f, 0, 1, None) == 1    # pair_work
    assert lib.hsr_pool_stats(f, 1, 2, f, f, 3, f, f, f, f, f, f, None) == 1                                            # M > P
    assert lib.hsr_pool_gram(f, 4, 8, f, 1, 2, f, f, 1, f, 8, None) == 1                                                # pair_g < n_elems
    assert lib.hsr_pool_models(f, 0, f, f, 0, f, f, f, f, f, f, 4, 3, 4, 1, 1, f, f, f, f, f, f, f, f, 1, 1, None) == 1  # npad < nf
    assert lib.hsr_pairs_last_launch(buf, 64) == 0 and buf.value == b""
    assert lib.hsr_pairs_last_launch(None, 0) == 0
    n = lib.hsr_pairs_instance_count()
    assert n == 12 and lib.hsr_pairs_instance_count() == n and lib.hsr_k4_instance_count() == 31
    names = [lib.hsr_pairs_instance_name(i) for i in range(n)]
    assert names == [lib.hsr_pairs_instance_name(i) for i in range(n)]
    assert [s.decode() for s in names] == [
        "pair_prep_kernel", "pair_stats_kernel", "pair_report_partial_kernel", "pair_report_finish_kernel", "pair_holdout_kernel",
        "pair_score_partial_kernel<false>", "pair_score_partial_kernel<true>", "pair_score_finish_kernel", "pool_stats_kernel",
        "pool_gram_kernel<false>", "pool_gram_kernel<true>", "pool_models_kernel"]
    for bad in (-1, n, 1 << 20):
        assert lib.hsr_pairs_instance_name(bad) is None and b"hsr_pairs_instance_name" in lib.hsr_last_error()
    assert sum(len(s) + 2 for s in names) < 2048                 # the whole table joined fits the tests' 2048-byte buffer


def test_aux_instance_enumeration():
    """hsr_aux_instance_name: every name the record can return - unique, stable, the template spellings of the sources."""
    lib = nat.load()
    n = lib.hsr_aux_instance_count()
    assert n == 32 and lib.hsr_aux_instance_count() == n
    names = [lib.hsr_aux_instance_name(i) for i in range(n)]
    assert all(isinstance(s, bytes) and s for s in names) and len(set(names)) == n
    assert names == [lib.hsr_aux_instance_name(i) for i in range(n)]
    for bad in (-1, n, 1 << 20):
        assert lib.hsr_aux_instance_name(bad) is None and b"hsr_aux_instance_name" in lib.hsr_last_error()
    want = ({f"select_hist_kernel<{p}, {m}>" for p in (1, 2, 3) for m in (0, 1)}
            | {f"select_hist_rows4_kernel<{p}>" for p in (1, 2, 3)} | {f"select_scan_kernel<{p}>" for p in (1, 2, 3)}
            | {"select_tiny_kernel"}
            | {f"{k}<{t}>" for k in ("block_mean_tile_kernel", "block_mean_kernel") for t in ("float", "uint8_t", "uint16_t")}
            | {"bilinear_up_kernel<false, false>", "bilinear_up_kernel<true, false>", "bilinear_up_kernel<true, true>",
               "bilinear_up_hist_kernel<true>", "bilinear_up_hist_kernel<false>"}
            | {f"tile_{c}_kernel {v}" for c in ("encode", "decode") for v in ("vec", "scalar")}
            | {f"transpose_rc_kernel<{a}, {b}>" for a, b in (("float", "float"), ("uint16_t", "uint16_t"), ("uint16_t", "float"),
                                                             ("int16_t", "float"))})
    assert {s.decode() for s in names} == want
    # every template instance the three sources name in a launch is in the table (kernel names with explicit arguments)
    csrc = os.path.join(ROOT, "hyperspectral_super-resolution_amd", "csrc")
    text = "".join(open(os.path.join(csrc, f)).read() for f in ("hsr_select.hip", "hsr_resample.hip", "hsr_tile.hip"))
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?((?:select|block_mean|bilinear|transpose)\w*<[\w, ]+>)", text))
    assert len(launched) >= 17 and {s for s in launched if not re.search(r"<(PASS|T|TI, TO)>", s)} <= want
    assert max(len(s) for s in names) < 64


# ---------------------------------------------------------------------------------------------
# SRF weight table
# ---------------------------------------------------------------------------------------------
def test_srf_table_matches_oracle_weights():
    g = load_golden("g1_srf")
    srf = unpack_srf(g)
    t = eng.build_srf_table(g["emit_w"], srf, g["good_mask"])
    Wn, names = onp.srf_weight_matrix(g["emit_w"], srf, g["good_mask"])
    assert t.names == list(srf) and t.supported == names and "B10" not in t.supported
    np.testing.assert_array_equal(t.weights, Wn)
    for b in range(t.nb):
        nz = np.nonzero(t.weights[b])[0]
        assert t.k0[b] == nz[0] and t.k0[b] + t.klen[b] == nz[-1] + 1
    assert t.klen.sum() < 400            # the sparse structure the kernel exploits
    # weight-matrix product reproduces the reference planes (float64)
    got = g["R"].astype(np.float64) @ t.weights.T
    for i, k in enumerate(t.supported):
        np.testing.assert_allclose(got[..., i], g[f"masked_{k}"], rtol=1e-12, atol=1e-15)
    t2 = eng.build_srf_table(g["emit_w"], srf, None)
    assert "B10" in t2.supported and t2.nb == 13


def test_shape_errors_match_reference_text():
    g = load_golden("g2_srf_edge")
    srf = unpack_srf(g)
    R, w = g["R"], g["emit_w"]
    for (bR, bw), msg in zip(((R[0], w), (R, w[:-1]), (R, w.reshape(1, -1))), g["error_messages"]):
        with pytest.raises(ValueError) as ei:
            s2_emit.pseudo_s2_srf_integral(bR, bw, srf)
        assert str(ei.value) == str(msg)
    with pytest.raises(ValueError) as ei:
        s2_emit.pseudo_s2_rgb({"B4": np.zeros((2, 2)), "B3": np.zeros((2, 2)), "B2": None})
    assert str(ei.value) == "Band B2 is None/missing in pseudo_s2."
    rgb = s2_emit.pseudo_s2_rgb({"B4": np.ones((2, 2)), "B3": np.zeros((2, 2)), "B2": np.zeros((2, 2))})
    assert rgb.shape == (2, 2, 3) and rgb[0, 0, 0] == 1
    # every band unsupported -> dict of None, no GPU needed
    out = s2_emit.pseudo_s2_srf_integral(R, w, srf, np.zeros(285, bool))
    assert list(out) == list(srf) and all(v is None for v in out.values())


# ---------------------------------------------------------------------------------------------
# SRF table loader (xlsx / csv / npz), API surface
# ---------------------------------------------------------------------------------------------
def _write_xlsx(path, sheets):
    """Minimal xlsx writer for the test: sheets = {name: (header list, rows list)}."""
    def col(i):
        s = ""
        i += 1
        while i:
            i, r = divmod(i - 1, 26)
            s = chr(65 + r) + s
        return s
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("[Content_Types].xml", "<Types xmlns='http://schemas.openxmlformats.org/package/2006/content-types'/>")
        wb = ["<workbook xmlns='http://schemas.openxmlformats.org/spreadsheetml/2006/main' "
              "xmlns:r='http://schemas.openxmlformats.org/officeDocument/2006/relationships'><sheets>"]
        rels = ["<Relationships xmlns='http://schemas.openxmlformats.org/package/2006/relationships'>"]
        for i, (name, (header, rows)) in enumerate(sheets.items(), 1):
            wb.append(f"<sheet name='{name}' sheetId='{i}' r:id='rId{i}'/>")
            rels.append(f"<Relationship Id='rId{i}' Type='x' Target='worksheets/sheet{i}.xml'/>")
            xml = ["<worksheet xmlns='http://schemas.openxmlformats.org/spreadsheetml/2006/main'><sheetData>"]
            xml.append("<row r='1'>" + "".join(
                f"<c r='{col(j)}1' t='inlineStr'><is><t>{h}</t></is></c>" for j, h in enumerate(header)) + "</row>")
            for r, row in enumerate(rows, 2):
                cells = []
                for j, v in enumerate(row):
                    if v is None:
                        continue
                    if isinstance(v, str):
                        cells.append(f"<c r='{col(j)}{r}' t='inlineStr'><is><t>{v}</t></is></c>")
                    else:
                        cells.append(f"<c r='{col(j)}{r}'><v>{v!r}</v></c>")
                xml.append(f"<row r='{r}'>" + "".join(cells) + "</row>")
            xml.append("</sheetData></worksheet>")
            z.writestr(f"xl/worksheets/sheet{i}.xml", "".join(xml))
        wb.append("</sheets></workbook>")
        rels.append("</Relationships>")
        z.writestr("xl/workbook.xml", "".join(wb))
        z.writestr("xl/_rels/workbook.xml.rels", "".join(rels))


def test_load_s2_srf_from_xlsx_local_file(tmp_path):
    lam = np.arange(400.0, 460.0)
    header = ["SR_WL"] + [f"S2A_SR_AV_{b}" for b in s2_emit.S2_BANDS_13]
    rows = []
    for i, l in enumerate(lam):
        row = [float(l)]
        for j in range(13):
            v = float(np.exp(-0.5 * ((l - 410 - 3 * j) / 6.0) ** 2))
            row.append(v if v > 1e-3 else 0.0)
        rows.append(row)
    rows[5][1] = None            # blank cell -> NaN -> dropped
    rows[6][2] = "n/a"           # text -> coerced to NaN -> dropped
    p = tmp_path / "srf.xlsx"
    _write_xlsx(p, {"Readme": (["x"], [[1.0]]), "Spectral Responses (S2A)": (header, rows),
                    "Spectral Responses (S2B)": (header, rows)})
    srf = s2_emit.load_s2_srf_from_xlsx(str(p))
    assert list(srf) == s2_emit.S2_BANDS_13
    lam1, r1 = srf["B1"]
    assert lam1.dtype == np.float64 and (r1 > 0).all() and 405.0 not in lam1
    assert 406.0 not in srf["B2"][0]
    assert len(srf["B12"][0]) < len(lam)           # zero responses filtered (resp > 0)
    sub = s2_emit.load_s2_srf_from_xlsx(str(p), bands=["B2", "B3"])
    assert list(sub) == ["B2", "B3"]
    with pytest.raises(ValueError) as ei:
        s2_emit.load_s2_srf_from_xlsx(str(p), platform="S2C")
    assert "No sheet containing 'Spectral Responses' and 'S2C' found." in str(ei.value)
    with pytest.raises(KeyError) as ei:
        s2_emit.load_s2_srf_from_xlsx(str(p), bands=["B99"])
    assert "Column 'S2A_SR_AV_B99' not found in sheet 'Spectral Responses (S2A)'." in str(ei.value)
    # csv / npz / dict sources give the same table
    import csv
    with open(tmp_path / "srf.csv", "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(header)
        for row in rows:
            wr.writerow(["" if v is None else v for v in row])
    c = s2_emit.load_s2_srf_from_xlsx(str(tmp_path / "srf.csv"))
    for b in srf:
        np.testing.assert_array_equal(c[b][0], srf[b][0])
        np.testing.assert_allclose(c[b][1], srf[b][1], rtol=1e-15)


def test_api_surface_matches_reference_all():
    ref_all = ["load_s2_srf_from_xlsx", "load_emit_envi_rfl", "load_emit_wavelengths_from_nc",
               "pseudo_s2_srf_integral", "pseudo_s2_rgb", "show_side_by_side", "resize_s2_rgb_to",
               "robust_norm", "robust_norm_rgb", "apply_shared_percentile_stretch",
               "histogram_match_rgb", "ot_match_rgb_sinkhorn_pot", "load_s2_rgb_u8"]
    assert s2_emit.__all__[:13] == ref_all
    for n in s2_emit.__all__:
        assert callable(getattr(s2_emit, n))
    import inspect
    sig = inspect.signature(s2_emit.fit_ot_poly_rgb)
    assert [(k, v.default) for k, v in sig.parameters.items()][3:] == [
        ("deg", 2), ("n_samples", 5000), ("reg", 0.05), ("numItermax", 300), ("stopThr", 1e-6), ("seed", 0)]
    assert list(inspect.signature(s2_emit.apply_poly_rgb).parameters) == ["rgb", "coeffs", "mask"]
    assert list(inspect.signature(s2_emit.pseudo_s2_srf_integral).parameters)[:4] == ["R", "emit_w", "srf_dict", "good_mask"]
    assert list(inspect.signature(s2_emit.apply_shared_percentile_stretch).parameters) == ["img", "mask", "pmin", "pmax"]


def test_host_numpy_api_functions_against_golden():
    g5 = load_golden("g5_stretch")
    np.testing.assert_array_equal(s2_emit.robust_norm_rgb(g5["img"], g5["mask"]), g5["robust_norm_rgb"])
    np.testing.assert_array_equal(s2_emit.robust_norm(g5["img"][..., 0]), g5["robust_norm"])
    g8 = load_golden("g8_histmatch")
    np.testing.assert_array_equal(s2_emit.histogram_match_rgb(g8["src"], g8["ref"], g8["mask"]), g8["out"])
    g9 = load_golden("g9_fit_fallback")     # identity fallback needs no GPU
    np.testing.assert_array_equal(s2_emit.fit_ot_poly_rgb(g9["src"], g9["ref"], g9["mask"], deg=2), g9["coeffs_deg2"])
    np.testing.assert_array_equal(s2_emit.fit_ot_poly_rgb(g9["src_nan"], g9["ref"], g9["mask_b"], deg=3), g9["coeffs_nan_deg3"])


def test_envi_loader_layouts(tmp_path):
    rng = np.random.default_rng(0)
    cube = rng.random((5, 7, 9)).astype(np.float32)          # (H, W, B)
    for inter, arr in (("bip", cube), ("bil", cube.transpose(0, 2, 1)), ("bsq", cube.transpose(2, 0, 1))):
        np.ascontiguousarray(arr).tofile(tmp_path / f"c_{inter}.bin")
        (tmp_path / f"c_{inter}.hdr").write_text(
            f"ENVI\ndescription = {{\n test }}\nsamples = 7\nlines = 5\nbands = 9\nheader offset = 0\n"
            f"data type = 4\ninterleave = {inter}\nbyte order = 0\n")
        R = s2_emit.load_emit_envi_rfl(str(tmp_path / f"c_{inter}.hdr"), str(tmp_path / f"c_{inter}.bin"))
        assert R.dtype == np.float32 and R.flags.c_contiguous
        np.testing.assert_array_equal(R, cube)
