"""Every K1 kernel instance (csrc/hsr_srf.hip, kSrfKernels: 5 degrees x 22 variants less the four degree-0 apply slots)
against float64 references.

One case table.  A row names a geometry (cube dtype, B, cube alignment, output layout, nb, degree, options), an entry point
(hsr_srf_integrate[_u16], _moments[_u16], _fit[_u16], _moments[_u16]_apply, hsr_srf_integrate_moments_batched) and the
(degree, variant) of kSrfKernels that srf_select must launch for it - or None where the entry must refuse the geometry
without launching.  For every row:
  * the library's own launch record (hsr_srf_last_launch) names the expected instance, for both launches of the row;
  * planes against oracle_np.pseudo_s2_srf_integral in float64 (uint16 cubes: of oracle_np.tile_decode_u16 of the same
    tile): rel 2e-6, 3e-6 where the weights are read from global memory (as test_k1_spectral_size_sweep); NaN / +-Inf
    placement exact; uint16 nodata pixels NaN in every band; pad columns of 16-byte aligned pixel-major rows zero, every
    element outside what the call owns untouched;
  * moments (deg >= 1) against float64 sums over the kernel's own planes and targets with the per_band_valid rule, the
    mask and min_x / min_y: count exact, the other sums rtol 1e-12;
  * a fit in the launch (the fused fit, the tail fit of an apply launch): moments and coefficients bit-identical to
    hsr_moments_reduce_solve over the same partials, coefficients within 1e-7 (1e-6 at degree 4) of
    oracle_np.fit_per_band_poly relative to the band's largest coefficient; band 1 has no valid pixel (identity fallback);
  * an apply job: the older tile's matched rows bit-exact to oracle_np.apply_poly_planes (clip / no clip, mask / no mask),
    pad columns passed through, rows past apply_npix untouched;
  * a batch: each tile's rows and moments equal the references of that tile alone;
  * a second launch gives identical bits; between the launches the ticket counter goes back to the row's ticket base and the
    ready words to their initial values.
The last two tests check that the rows reach every instance the table query (hsr_srf_kernel_instance) reports, and that every
job-carrying instance (variants 5, 6, 18, 19 at degrees 1..4) has run each job form below.

Job forms of an apply launch (csrc/hsr_fused_dev.h: lazy_fit, apply_prephase).  'plain' is what the fused pipeline sends: an
ungated K3 pre-phase, a tail that reduces and solves one tile.  The exchange and group pipelines (csrc/hsr_exec.hip: job_fit,
job_apply) send three more, and every form keeps the checks above (launch record, planes, moments, apply, second launch):
  * every tail, whatever its form: the tile's moments carry the bits of hsr_moments_reduce over the previous launch's partials and
    pass the float64 comparison above; the ticket counter ends at base + workgroups (mod 2^32); sync_error_dev stays 0;
  * exchange (fit_ready_dev): *fit_ready_dev grows by exactly nb from a non-zero start (one row: from 0xFFFFFFFF - 3, across the
    wrap); fit_coeffs_dev keeps its sentinel in every element (no solve);
  * gated pre-phase (coeffs_ready_dev), with the exchange tail and without any tail: the matched rows carry the bits of
    oracle_np.apply_poly_planes as in the plain form; the word is unchanged.  Pairs (word, value): equal, word three past the value,
    and value 0xFFFFFFFF with word 1 (a word that has wrapped past its target).  Every row's wait is satisfied BEFORE the launch is
    enqueued (asserted on the host): a word behind its value would spin for HSR_SYNC_TIMEOUT_S.  The time-out branch of
    wait_word_at_least is deliberately not exercised;
  * group_mid (fit_group_index < T - 1): fit_moments_dev is entry `index` of [T][nb][M]; the other T - 1 entries,
    fit_group_total_dev and fit_coeffs_dev keep their sentinels;
  * group_last (index T - 1), T in {2, 3, 31, 32, 33, 63, 64} - both halves of the group sum (l < T, l + 32 < T) and their edges.  The
    other T - 1 entries are float64 moment sets of small random pixel sets; the last tile's own entry is poisoned in memory before
    every launch (the kernel takes it from LDS, then overwrites it); two rows point fit_moments_dev away from the array - the host
    does not check it - so the array's last entry stays poisoned and a sum that read it back from memory would show.  fit_group_total_dev and fit_coeffs_dev carry the bits of
    hsr_moments_reduce_solve over the T entries as T slots.  The total against math.fsum of the entries:
    |got - exact| <= 16 * 2^-53 * fsum(|entries|) per element, counts exact - every entry passes through at most seven correctly
    rounded adds (one pair add, the butterfly levels), which bounds the error by 8 * 2^-53 * sum|e|; derived, not measured.  The
    coefficients against oracle_np.fit_per_band_poly over the UNION of the group's pixels at the bar of the plain tail (1e-7, 1e-6 at
    degree 4, relative to the band's largest coefficient).  Band 1 has no valid pixel in any entry (identity fallback); one row
    gives it pixels in the other entries only (fitted, not the identity); one row puts min_count between the last tile's count
    and the group's;
  * ticket base: a plain, an exchange and a group_last row run with base and counter 0xFFFFFFF8 on more than 8 workgroups - the
    counter wraps inside the launch - and carry the bits of the same launch at base 0;
  * refusals (HSR_ERR_INVALID with the message of hsr_srf.hip, nothing launched): fit_group_tiles 65, fit_group_index T, NULL
    fit_group_total_dev, a group together with fit_ready_dev.

Support layouts: 'std' = bands of 17..32 taps (32 LDS taps each after rounding to 16-tap chunks), the first starting at
sample 0 and the last ending at sample B - 1, with a zero response and a bad (good_mask False) sample inside; 'w64' / 'w65' =
16 bands of 64 / 65 taps (1024 LDS taps fit kWeightCap, 16 x 80 do not); B < 16: the 16-tap chunks do not fit the row.
"""
import ctypes as C
import math
import zlib
from dataclasses import dataclass

import numpy as np
import pytest

from gpu_harness import torch_gpu  # noqa: F401
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu

# variant numbers of kSrfKernels (enum SrfVariant, csrc/hsr_srf.hip) and the instance each one names
TEMPLATES = {
    0: "srf_kernel<{d}, false, false, 64, false, false>",
    1: "srf_kernel<{d}, false, true, 64, false, false>",
    2: "srf_kernel<{d}, false, true, 64, true, false>",
    3: "srf_kernel<{d}, true, true, 64, false, false>",
    4: "srf_kernel<{d}, true, true, 64, true, false>",
    5: "srf_kernel<{d}, false, true, 64, true, false, true>",
    6: "srf_kernel<{d}, true, true, 64, true, false, true>",
    7: "srf_kernel<{d}, false, true, 64, true, true>",
    8: "srf_kernel<{d}, true, true, 64, true, true>",
    9: "srf_u16_kernel<{d}, false, false, false>",
    10: "srf_u16_kernel<{d}, false, true, false>",
    11: "srf_u16_kernel<{d}, true, false, false>",
    12: "srf_u16_kernel<{d}, true, true, false>",
    13: "srf_u16_kernel<{d}, false, true, true>",
    14: "srf_u16_kernel<{d}, true, true, true>",
    15: "srf_u16_ring_kernel<{d}, false, false, false>",
    16: "srf_u16_ring_kernel<{d}, true, false, false>",
    17: "srf_u16_ring_kernel<{d}, true, false, true>",
    18: "srf_u16_ring_kernel<{d}, true, false, false, true>",
    19: "srf_u16_ring_kernel<{d}, true, false, true, true>",
    20: "srf_u16_ring_kernel<{d}, true, true, false>",
    21: "srf_u16_ring_kernel<{d}, true, true, true>",
}
NODATA = 65535
MIN_COUNT = 20
SENTINEL = -7.75          # what the buffers hold where the call must not write


class ApplyJob(C.Structure):
    """hsr_apply_job (include/hsr.h)."""
    _fields_ = [("x_dev", C.c_void_p), ("out_dev", C.c_void_p), ("coeffs_dev", C.c_void_p), ("mask_dev", C.c_void_p),
                ("npix", C.c_int64), ("clip", C.c_int32), ("fit_slots", C.c_int32), ("fit_partials_dev", C.c_void_p),
                ("fit_moments_dev", C.c_void_p), ("fit_coeffs_dev", C.c_void_p), ("fit_min_count", C.c_int64),
                ("fit_counter_dev", C.c_void_p), ("fit_ticket_base", C.c_uint32), ("reserved", C.c_int32),
                ("fit_ready_dev", C.c_void_p), ("coeffs_ready_dev", C.c_void_p), ("coeffs_ready_value", C.c_uint32),
                ("reserved2", C.c_uint32), ("sync_error_dev", C.c_void_p), ("fit_group_tiles", C.c_int32),
                ("fit_group_index", C.c_int32), ("fit_group_moments_dev", C.c_void_p), ("fit_group_total_dev", C.c_void_p)]


@dataclass(frozen=True)
class Case:
    expect: object          # variant of kSrfKernels[deg] the call must launch; None: refused, nothing launched
    entry: str              # integrate | moments | fit | apply | batch
    dtype: str              # f32 | u16
    B: int
    nb: int
    deg: int
    npix: tuple             # the tile (one entry), or the tiles of a batch
    aligned: tuple = (True,)   # per tile: cube 16-byte aligned (False: 4-byte / 2-byte aligned)
    out: str = "pix"        # pix: 16-byte aligned rows of padded_row(nb); pix_off: the same rows 4 bytes off; narrow: rows of nb; planar
    taps: str = "std"       # std | w64 | w65
    rc: int = 0             # options.reserved_cus
    single: bool = False    # options.u16_single_buffer
    fastu: bool = False     # options.flags = HSR_SRF_U16_FAST
    clip: bool = True       # apply job
    mask: bool = True       # fit mask (single tile) / apply mask
    tail: bool = False      # apply launch carries the previous tile's fit
    job_x: bool = True      # apply launch carries a K3 job
    apply_npix: int = 61
    minv: float = 0.0
    # the job forms of the exchange and group pipelines (apply rows; every form but "plain" carries a tail)
    form: str = "plain"     # plain | exchange | group_mid | group_last
    group_T: int = 0        # fit_group_tiles
    group_index: int = -1   # group_mid: fit_group_index (group_last: group_T - 1)
    tbase: int = 0          # fit_ticket_base and the counter's value before the launch
    ready: tuple = None     # gated pre-phase: (*coeffs_ready_dev, coeffs_ready_value); the word must have reached the value
    ready0: int = 7         # exchange: *fit_ready_dev before the launch
    band1: str = "none"     # group_last: band 1 has no valid pixel in any entry (none) / only in the last tile's (others)
    min_count: int = MIN_COUNT
    detached: bool = False  # group_last: fit_moments_dev points away from the group's array (the host does not check it)
    bad: str = ""           # refusals: T65 | index | total | ready
    err: int = 2            # what a refusal returns (HSR_ERR_UNSUPPORTED; the job checks: HSR_ERR_INVALID = 1)

    @property
    def id(self):
        s = f"d{self.deg}v{self.expect}-{self.entry}-{self.dtype}-B{self.B}-nb{self.nb}-n{'_'.join(map(str, self.npix))}"
        if not all(self.aligned):
            s += "-unal"
        s += "" if self.entry == "batch" or self.out == "pix" else f"-{self.out}"
        for flag, tag in ((self.taps != "std", self.taps), (self.rc, f"rc{self.rc}"), (self.single, "single"),
                          (self.fastu, "fastu"), (self.tail, "tail"), (self.entry == "apply" and not self.job_x, "nojob"),
                          (self.form != "plain", self.form), (self.group_T, f"T{self.group_T}"),
                          (self.group_index >= 0, f"i{self.group_index}"), (self.tbase, f"tb{self.tbase:x}"),
                          (self.ready is not None, "gate{:x}_{:x}".format(*(self.ready or (0, 0)))), (self.ready0 != 7, f"r{self.ready0:x}"),
                          (self.band1 != "none", f"b1{self.band1}"), (self.min_count != MIN_COUNT, f"mc{self.min_count}"),
                          (self.detached, "detached"), (self.bad, f"bad{self.bad}")):
            if flag:
                s += f"-{tag}"
        return s


def _cases():
    cs = []
    add = lambda *a, **k: cs.append(Case(*a, **k))
    # -- the largest LDS of any K1 launch first: (4, kF32Apply) starts at B = 560; (1, kF32Apply) gets B = 560 after the
    #    base rows below have run it with less LDS (raise_lds_limit's per-kernel cache)
    add(5, "apply", "f32", 560, 16, 4, (1029,), tail=True, clip=False)
    # -- every instance: a ragged tile (npix not a multiple of 64) and one below 64 pixels
    for d in range(5):
        rag = 64 * (5 + d) + 27
        small = (1, 37, 63, 50, 5)[d]
        nbs = (1, 16, 13, 1, 16)[d]
        e1, e2 = ("integrate", "integrate") if d == 0 else (("moments", "fit") if d % 2 else ("fit", "moments"))
        minv = 0.0625 if d % 2 == 0 else 0.0
        k = dict(minv=minv)
        # float32 single-tile kernels
        add(0, e1, "f32", 285, 16, d, (rag,), taps="w65", **k)
        add(0, e2, "f32", (7, 15, 3, 11, 9)[d], (3, 1, 3, 1, 3)[d], d, (small,), **k)
        add(1, e1, "f32", 284, 13, d, (rag,), out="planar", **k)
        add(1, e2, "f32", 285, nbs, d, (small,), aligned=(False,), out="pix_off", **k)
        add(2, e1, "f32", 285, 13, d, (rag,), aligned=(False,), **k)
        add(2, e2, "f32", 284, nbs, d, (small,), **k)
        add(3, e1, "f32", 285, 13, d, (rag,), out="planar", **k)
        add(3, e2, "f32", 285, 13, d, (small,), out="narrow", **k)
        add(4, e1, "f32", 285, 13, d, (rag,), **k)
        add(4, e2, "f32", 101, nbs, d, (small,), **k)
        # uint16 single-buffer kernels
        add(9, e1, "u16", 285, 13, d, (rag,), aligned=(False,), out="planar", **k)
        add(9, e2, "u16", 284, nbs, d, (small,), aligned=(False,), out="pix_off", **k)
        add(10, e1, "u16", 285, 13, d, (rag,), aligned=(False,), fastu=True, **k)
        add(10, e2, "u16", 284, nbs, d, (small,), aligned=(False,), **k)
        add(11, e1, "u16", 285, 13, d, (rag,), out="planar", single=True, **k)
        add(11, e2, "u16", 285, 13, d, (small,), out="narrow", single=True, **k)
        add(12, e1, "u16", 299, 13, d, (rag,), **k)
        add(12, e2, "u16", 285, nbs, d, (small,), single=True, fastu=True, **k)
        # uint16 ring kernels
        add(15, e1, "u16", 285, 13, d, (rag,), out="planar", fastu=True, **k)
        add(15, e2, "u16", 284, nbs, d, (small,), out="pix_off", **k)
        add(16, e1, "u16", 285, 13, d, (rag,), **k)
        add(16, e2, "u16", 284, nbs, d, (small,), **k)
        add(17, e1, "u16", 285, 13, d, (rag,), fastu=True, **k)
        add(17, e2, "u16", 284, nbs, d, (small,), fastu=True, **k)
        # batches (degree 0: no targets)
        add(7, "batch", "f32", 285, 13, d, (rag, 37, 130), aligned=(True, False, True), **k)
        add(7, "batch", "f32", 284, nbs, d, (small,), **k)
        add(8, "batch", "f32", 285, 13, d, (rag, 37, 130), **k)
        add(8, "batch", "f32", 101, nbs, d, (small, 1), **k)
        add(13, "batch", "u16", 285, 13, d, (rag, 37, 130), aligned=(True, True, False), fastu=True, **k)
        add(13, "batch", "u16", 284, nbs, d, (small,), aligned=(False,), **k)
        add(14, "batch", "u16", 285, 13, d, (rag, 37, 130), single=True, **k)
        add(14, "batch", "u16", 299, 13, d, (small, 1), **k)
        add(20, "batch", "u16", 285, 13, d, (rag, 37, 130), **k)
        add(20, "batch", "u16", 284, nbs, d, (small,), **k)
        add(21, "batch", "u16", 285, 13, d, (rag, 37, 130), fastu=True, **k)
        add(21, "batch", "u16", 284, nbs, d, (small, 1), fastu=True, **k)
        if d == 0:
            continue
        # apply launches: the ragged tile carries the previous tile's fit (>= nb workgroups), the small one a K3 job only
        tr = 64 * 14 + 27                         # 15 groups >= 13 bands
        c1, m1 = d % 2 == 1, d <= 2
        add(5, "apply", "f32", 284, 13, d, (tr,), tail=True, clip=c1, mask=m1, apply_npix=700, **k)
        add(5, "apply", "f32", 285, nbs, d, (small,), aligned=(False,), clip=not c1, mask=not m1, **k)
        add(6, "apply", "f32", 285, 13, d, (tr,), tail=True, clip=not c1, mask=m1, apply_npix=700, **k)
        add(6, "apply", "f32", 101, nbs, d, (small,), clip=c1, mask=not m1, **k)
        add(18, "apply", "u16", 285, 13, d, (tr,), tail=True, clip=c1, mask=not m1, apply_npix=700, **k)
        add(18, "apply", "u16", 284, nbs, d, (small,), clip=not c1, mask=m1, **k)
        add(19, "apply", "u16", 285, 13, d, (tr,), tail=True, fastu=True, clip=not c1, mask=not m1, apply_npix=700, **k)
        add(19, "apply", "u16", 284, nbs, d, (small,), fastu=True, clip=c1, mask=m1, **k)
    # -- selection boundaries
    # ring double buffer (80 KB with the 32-tap supports) <-> single buffer: nb 13 / 16 in rows of 16, nb 1 in rows of 4
    add(16, "moments", "u16", 298, 13, 2, (347,))
    add(12, "moments", "u16", 299, 13, 2, (347,))
    add(17, "integrate", "u16", 294, 16, 0, (347,), fastu=True)
    add(12, "integrate", "u16", 295, 16, 0, (347,), fastu=True)
    add(16, "fit", "u16", 316, 1, 3, (347,))
    add(12, "fit", "u16", 317, 1, 3, (347,))
    add(18, "apply", "u16", 298, 13, 1, (923,), tail=True, clip=False, mask=True, apply_npix=64)
    add(None, "apply", "u16", 299, 13, 1, (923,), tail=True)
    add(20, "batch", "u16", 298, 13, 4, (347, 37))
    add(14, "batch", "u16", 299, 13, 4, (347, 37))
    # (a batch's ring also holds the next units' records [2][16]: nb 16 fits up to B = 293, nb 13 up to 298)
    add(21, "batch", "u16", 293, 16, 3, (347, 37), fastu=True)
    add(14, "batch", "u16", 294, 16, 3, (347, 37), fastu=True)
    # the ring's group buffers must hold the apply job: 48 <= B
    add(19, "apply", "u16", 48, 1, 3, (37,), fastu=True, tail=True, job_x=False)
    add(19, "apply", "u16", 48, 1, 2, (347,), fastu=True, clip=False, mask=False, apply_npix=129)
    add(None, "apply", "u16", 47, 1, 3, (347,))
    add(16, "integrate", "u16", 47, 1, 0, (347,))
    # weights in LDS (16 x 64 taps = kWeightCap) <-> from global memory (16 x 80)
    add(4, "moments", "f32", 285, 16, 1, (347,), taps="w64")
    add(0, "moments", "f32", 285, 16, 1, (347,), taps="w65")
    add(6, "apply", "f32", 285, 16, 2, (1109,), taps="w64", tail=True, clip=True, mask=False, apply_npix=200)
    add(None, "apply", "f32", 285, 16, 2, (1109,), taps="w65", tail=True)
    add(8, "batch", "f32", 285, 16, 3, (347, 37), taps="w64")
    add(None, "batch", "f32", 285, 16, 3, (347, 37), taps="w65")
    add(17, "integrate", "u16", 285, 16, 0, (347,), taps="w64", fastu=True)
    add(16, "integrate", "u16", 285, 16, 0, (347,), taps="w65", fastu=True)      # FASTU needs the weights in LDS
    add(21, "batch", "u16", 285, 16, 4, (347,), taps="w64", fastu=True)
    add(None, "batch", "u16", 285, 16, 4, (347,), taps="w65")
    add(19, "apply", "u16", 285, 16, 1, (1109,), taps="w64", fastu=True, tail=True, clip=False, mask=True, apply_npix=200)
    # float32 apply up to HSR_MAX_SPECTRAL: the largest LDS of any K1 launch
    add(5, "apply", "f32", 560, 16, 1, (389,), clip=True, mask=False)
    add(6, "apply", "f32", 559, 13, 2, (1000,), tail=True, clip=False, mask=True)
    add(2, "integrate", "f32", 560, 16, 0, (389,))
    # tiny B: global weights at every degree through moments and the fused fit; the uint16 ring with global weights
    add(0, "moments", "f32", 15, 1, 2, (347,))
    add(0, "fit", "f32", 3, 3, 4, (347,))
    add(0, "fit", "f32", 15, 1, 1, (63,), aligned=(False,))
    add(16, "moments", "u16", 7, 3, 1, (347,), fastu=True)
    # FAST loader: odd B and an aligned cube
    add(1, "integrate", "f32", 285, 13, 0, (347,), aligned=(False,), out="planar")
    add(3, "integrate", "f32", 285, 13, 0, (411,), out="planar")
    add(1, "moments", "f32", 286, 13, 3, (347,), out="planar")
    add(2, "fit", "f32", 286, 13, 3, (347,))
    add(8, "batch", "f32", 285, 13, 2, (347, 37), aligned=(True, True))
    add(7, "batch", "f32", 286, 13, 2, (347, 37), aligned=(True, True))
    # partial slots: 64 / 65 groups, 512 / 513 groups, above the resident-workgroup cap with 0, 8 and 128 reserved CUs
    slot_pts = [((4096,), 0), ((4097,), 0), ((32768,), 0), ((32769,), 0), ((38417,), 0), ((38417,), 8), ((38417,), 128)]
    for i, (n, rc) in enumerate(slot_pts):
        d = 1 + i % 4
        e = "moments" if i % 2 else "fit"
        add(3, e, "f32", 63, 13, d, n, out="planar", rc=rc)
        add(4, "fit" if i % 2 else "moments", "f32", 63, 13, 1 + (i + 1) % 4, n, rc=rc)
        add(16, e, "u16", 63, 13, 1 + (i + 2) % 4, n, rc=rc)
        add(6, "apply", "f32", 63, 13, d, n, rc=rc, tail=True, clip=i % 2 == 0, mask=i % 3 == 0, apply_npix=1000 + i)
        add(18, "apply", "u16", 63, 13, 1 + (i + 3) % 4, n, rc=rc, tail=True, clip=i % 2 == 1, mask=i % 3 == 1, apply_npix=999)
        add(8, "batch", "f32", 63, 13, i % 5, n + (37,), rc=rc)
        add(20, "batch", "u16", 63, 13, (i + 2) % 5, (100,) + n, rc=rc)
    # -- the job forms of the exchange and group pipelines: every job-carrying instance at every degree, ragged tiles of
    #    >= nb and > 8 workgroups; nb 1 / 13 / 16 (rows of 4 and 16 floats), clip and the apply mask on and off
    inst = ((5, "f32", False, False), (6, "f32", True, False), (18, "u16", True, False), (19, "u16", True, True))
    shape = {1: 64 * 9 + 27, 13: 64 * 14 + 27, 16: 64 * 16 + 27}
    mids = ((2, 0), (64, 62), (33, 0), (3, 1), (32, 30), (63, 31), (31, 15))
    i = nx = nm = nl = 0
    for d in range(1, 5):
        for vi, (v, dt, al, fu) in enumerate(inst):
            for form in ("exchange", "group_mid", "group_last"):
                nb = (13, 16, 1)[(i + d) % 3]
                k = dict(aligned=(al,), fastu=fu, tail=True, clip=i % 2 == 0, mask=(i // 2) % 2 == 0, apply_npix=(61, 333, 700)[i % 3],
                         minv=0.0625 if d % 2 == 0 else 0.0, form=form)
                if form == "exchange":              # every other row with a gated pre-phase, the three pairs in turn
                    gated = (d + vi) % 2 == 0
                    add(v, "apply", dt, 285, nb, d, (shape[nb],), ready=GATES[nx % 3] if gated else None, **k)
                    nx += gated
                elif form == "group_mid":
                    add(v, "apply", dt, 285, nb, d, (shape[nb],), group_T=mids[nm % 7][0], group_index=mids[nm % 7][1], **k)
                    nm += 1
                else:
                    add(v, "apply", dt, 285, nb, d, (shape[nb],), group_T=GROUP_T[nl % 7], **k)
                    nl += 1
                i += 1
    # the gated pre-phase without any tail (fit_partials_dev NULL): small tiles, every pair on every instance
    for i, (v, dt, al, fu) in enumerate(inst):
        for g, gate in enumerate(GATES):
            add(v, "apply", dt, 285, (1, 13, 16)[(i + g) % 3], 1 + (i + g) % 4, ((37, 63, 50, 5)[i],), aligned=(al,), fastu=fu,
                clip=g % 2 == 0, mask=i % 2 == 0, ready=gate)
    # a ready word that wraps inside the launch; ticket bases eight below the wrap (15 workgroups draw tickets)
    add(6, "apply", "f32", 285, 13, 2, (923,), tail=True, form="exchange", ready0=0xFFFFFFFF - 3, ready=GATES[2])
    add(5, "apply", "f32", 284, 13, 1, (923,), tail=True, clip=False, apply_npix=700, tbase=0xFFFFFFF8)
    add(19, "apply", "u16", 285, 13, 3, (923,), fastu=True, tail=True, form="group_last", group_T=32, tbase=0xFFFFFFF8)
    add(18, "apply", "u16", 285, 13, 4, (923,), tail=True, form="exchange", tbase=0xFFFFFFF8)
    # band 1 valid in the other entries only: fitted, not the identity; min_count between the last tile's count and the group's
    add(6, "apply", "f32", 285, 13, 2, (923,), tail=True, form="group_last", group_T=33, band1="others")
    add(18, "apply", "u16", 285, 13, 3, (923,), tail=True, form="group_last", group_T=64, min_count=923 + 50)
    # the last entry of the sum is what the launch has just reduced, not what memory holds: fit_moments_dev elsewhere, entry T - 1 stays poisoned
    add(5, "apply", "f32", 285, 13, 3, (923,), aligned=(False,), tail=True, form="group_last", group_T=33, detached=True)
    add(19, "apply", "u16", 285, 16, 2, (1051,), fastu=True, tail=True, form="group_last", group_T=32, detached=True, minv=0.0625)
    # group jobs the entry refuses (HSR_ERR_INVALID)
    k = dict(tail=True, err=1)
    add(None, "apply", "f32", 285, 13, 1, (923,), form="group_last", group_T=65, bad="T65", **k)
    add(None, "apply", "f32", 285, 13, 2, (923,), form="group_mid", group_T=4, group_index=4, bad="index", **k)
    add(None, "apply", "u16", 285, 13, 3, (923,), form="group_last", group_T=4, bad="total", **k)
    add(None, "apply", "u16", 285, 13, 4, (923,), form="group_mid", group_T=4, group_index=1, bad="ready", **k)
    return cs


GROUP_T = (2, 3, 31, 32, 33, 63, 64)                      # either side of the two halves of the group sum (l < T, l + 32 < T)
GATES = ((5, 5), (9, 6), (1, 0xFFFFFFFF))                 # (word, value): equal, three past, wrapped past its target
APPLY_VARIANTS = (5, 6, 18, 19)                           # the instances that carry a job
POISON = 1.0e30                                           # the last tile's own entry in memory before a group_last launch
CASES = _cases()
SEEN = set()
FORMS_SEEN = set()                                        # (degree, variant, form) of every tail row that passed


def _record():
    from s2_emit import _native as nat
    d, v, lds = C.c_int32(), C.c_int32(), C.c_int64()
    got = nat.load().hsr_srf_last_launch(C.byref(d), C.byref(v), C.byref(lds))
    return (d.value, v.value, lds.value) if got == 1 else None


# ---- inputs --------------------------------------------------------------------------------------------------------------
def _supports(B, nb, taps, rng):
    if taps in ("w64", "w65"):
        kl = np.full(nb, 64 if taps == "w64" else 65)
    elif B < 16:
        kl = rng.integers(1, B + 1, nb)
    else:
        kl = np.minimum(rng.integers(17, 33, nb), B)
    k0 = np.array([rng.integers(0, B - kl[b] + 1) for b in range(nb)])
    k0[0] = 0                                              # the first support starts at sample 0 ...
    k0[-1] = B - kl[-1]                                    # ... the last one ends at sample B - 1
    return k0.astype(np.int32), kl.astype(np.int32)


def _srf(B, nb, taps, rng):
    """Wavelengths, an SRF dict and a good-band mask whose resampled supports are exactly the chosen ones."""
    w = np.linspace(400.0, 2400.0, B).astype(np.float32)
    wd = w.astype(np.float64)
    dx = (wd[-1] - wd[0]) / max(B - 1, 1)
    k0, kl = _supports(B, nb, taps, rng)
    ends = set(k0.tolist()) | set((k0 + kl - 1).tolist())
    inner = [k for k in range(1, B - 1) if k not in ends]
    good = np.ones(B, bool)
    if len(inner) > 4:
        good[rng.choice(inner, 2, replace=False)] = False    # zero-weight samples inside the supports
    srf = {}
    for b in range(nb):
        a, e = int(k0[b]), int(k0[b] + kl[b] - 1)
        rsp = rng.uniform(0.2, 1.0, e - a + 1)
        if e - a >= 2:
            rsp[rng.integers(1, e - a)] = 0.0                 # a zero of the response inside the support
        srf[f"S{b}"] = (np.concatenate([[wd[a] - 0.5 * dx], wd[a:e + 1], [wd[e] + 0.5 * dx]]), np.concatenate([[0.0], rsp, [0.0]]))
    return w, srf, good, k0, kl


def _cube(case, npix, rng):
    """(host float32 reflectance the oracle sees, host array the kernel reads, bad pixels (nodata))."""
    B = case.B
    if case.dtype == "f32":
        R = (rng.random((npix, 1)) * (0.5 + 0.5 * rng.random((npix, B))) * 0.9 - 0.03).astype(np.float32)   # planes spread over [0, 0.9)
        if npix >= 8:
            R[npix // 3, rng.integers(0, B)] = np.nan
            R[npix // 2, rng.integers(0, B)] = np.inf
            R[npix - 2, rng.integers(0, B)] = -np.inf
            R[npix // 4, 0] = np.inf
            R[npix // 4 + 1, B - 1] = -np.inf
        return R, R, np.zeros(npix, bool)
    u = (rng.random((npix, 1)) * (0.5 + 0.5 * rng.random((npix, B))) * 9000).astype(np.uint16)
    u[0, 0] = NODATA
    u[npix - 1, B - 1] = NODATA
    nbad = max(1, npix // 60)
    u[rng.integers(0, npix, nbad), rng.integers(0, B, nbad)] = NODATA
    return onp.tile_decode_u16(u, None, NODATA), u, (u == NODATA).any(axis=1)


def _device_cube(torch, host, aligned):
    """The cube on the device: 16-byte aligned, or 4 (float32) / 2 (uint16) bytes past a 16-byte boundary."""
    off = 0 if aligned else 1
    flat = np.zeros(host.size + 16, host.dtype)
    flat[off:off + host.size] = host.reshape(-1)
    d = torch.from_numpy(flat).cuda()[off:off + host.size].view(host.shape)
    assert (d.data_ptr() % 16 == 0) == aligned
    return d


def _oracle_planes(R, w, srf, good):
    ref = onp.pseudo_s2_srf_integral(R[None], w, srf, good)
    return np.stack([ref[k][0] for k in srf]).astype(np.float64)          # (nb, npix)


def _targets(ref, nb, row, rng):
    """Real-S2 rows correlated with the pseudo bands (a well-posed fit), some non-finite; band 1 never valid."""
    with np.errstate(invalid="ignore"):
        base = 0.9 * np.abs(np.nan_to_num(ref.T, nan=0.3, posinf=0.3, neginf=0.3)) ** 0.9 + 0.02
    y = np.zeros((ref.shape[1], row), np.float32)
    y[:, :nb] = base + 0.01 * rng.standard_normal(base.shape)
    n = y.shape[0]
    if n >= 8:
        y[n // 5, 0] = np.nan
        y[n // 6, nb - 1] = np.inf
    if nb >= 2:
        y[:, 1] = -1.0
    return y


# ---- references ----------------------------------------------------------------------------------------------------------
def _check_planes(got, ref, tol, what):
    """got, ref: (nb, npix).  NaN / +-Inf placement exact, finite values rel tol (scale floor 1e-3 of the band's largest)."""
    got = np.asarray(got, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN placement differs"
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.array_equal(np.isneginf(got), np.isneginf(ref)), f"{what}: Inf placement differs"
    for b in range(ref.shape[0]):
        fin = np.isfinite(ref[b])
        if not fin.any():
            continue
        scale = np.maximum(np.abs(ref[b, fin]), 1e-3 * np.abs(ref[b, fin]).max() + 1e-30)
        err = float(np.max(np.abs(got[b, fin] - ref[b, fin]) / scale))
        assert err <= tol, f"{what}: band {b} rel err {err:.3g} > {tol}"


def _valid(x, y, mask, minv):
    """per_band_valid of every band: x, y (nb, npix) -> (nb, npix) bool."""
    with np.errstate(invalid="ignore"):
        return np.stack([onp.per_band_valid(x[b], y[b], mask, minv) for b in range(x.shape[0])])


def _moments_ref(x, y, ok, deg):
    xs, ys = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
    S = [np.where(ok, xs ** k, 0.0).sum(axis=1) for k in range(2 * deg + 1)]
    T = [(np.where(ok, xs ** j, 0.0) * ys).sum(axis=1) for j in range(deg + 1)]
    return np.stack(S + T, axis=1)                                        # (nb, 3 deg + 2)


def _check_moments(got, x, y, mask, minv, deg, what):
    ok = _valid(x, y, mask, minv)
    want = _moments_ref(x.astype(np.float64), y.astype(np.float64), ok, deg)
    assert np.array_equal(got[:, 0], ok.sum(axis=1).astype(np.float64)), f"{what}: counts {got[:, 0]} != {ok.sum(axis=1)}"
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=what)


def _check_coeffs(got, x, y, mask, minv, deg, what, min_count=MIN_COUNT, band1_empty=True):
    want, counts = onp.fit_per_band_poly(x, y, mask, deg, minv, min_count)
    tol = 1e-6 if deg == 4 else 1e-7
    for b in range(want.shape[0]):
        err = float(np.max(np.abs(got[b] - want[b])))
        assert err <= tol * max(1.0, float(np.max(np.abs(want[b])))), f"{what}: band {b} ({counts[b]} pixels) coefficients off by {err:.3g}"
    if x.shape[0] >= 2 and band1_empty:
        assert counts[1] == 0 and np.array_equal(got[1], want[1])        # under-populated band: identity fallback
    return counts


def _u32(torch, v):
    """A device word holding the unsigned value v."""
    return torch.from_numpy(np.array([v], np.uint32).view(np.int32)).cuda()


def _set_u32(t, v):
    t.fill_(v - (1 << 32) if v >= (1 << 31) else v)


def _get_u32(t):
    return int(t.cpu().numpy().view(np.uint32)[0])


def _synthetic_entries(case, n, rng):
    """The other n tiles of a group as float64 moment sets of small random pixel sets with the targets' relation to x (the sums of
    _moments_ref, so that the union with the real tile determines one polynomial): (x (nb, N), y (nb, N), entries (n, nb, M))."""
    nb, deg = case.nb, case.deg
    xs, ys, ent = [], [], np.zeros((n, nb, 3 * deg + 2))
    for j in range(n):
        k = int(rng.integers(12, 24))
        x = rng.uniform(0.1, 0.9, (nb, k)).astype(np.float32)
        y = (0.9 * x.astype(np.float64) ** 0.9 + 0.02 + 0.01 * rng.standard_normal((nb, k))).astype(np.float32)
        if nb >= 2 and case.band1 == "none":
            y[1] = -1.0
        ok = _valid(x, y, np.ones(k, bool), case.minv)
        ent[j] = _moments_ref(x.astype(np.float64), y.astype(np.float64), ok, deg)
        xs.append(x)
        ys.append(y)
    return np.concatenate(xs, axis=1), np.concatenate(ys, axis=1), ent


def _check_group_sum(got, entries, what):
    """got (nb, M) against the exact sum of the T entries (T, nb, M).  Every entry reaches the result through at most seven adds
    (one pair add of entries l and l + 32, then the butterfly levels), each correctly rounded, so the result is within
    ((1 + u)^7 - 1) sum|e| < 8 u sum|e| of the exact sum, u = 2^-53; the bound asserted is 16 u sum|e|.  It follows from the tree,
    it is not measured.  Counts are integers far below 2^53: exact."""
    T, nb, M = entries.shape
    worst = 0.0
    for b in range(nb):
        for m in range(M):
            col = [float(v) for v in entries[:, b, m]]
            exact, mag = math.fsum(col), math.fsum(abs(v) for v in col)
            bound = 16.0 * 2.0 ** -53 * mag
            worst = max(worst, abs(got[b, m] - exact) / bound) if bound > 0 else worst
            assert abs(got[b, m] - exact) <= bound, f"{what}: band {b} moment {m}: {got[b, m]!r} vs {exact!r} (sum|e| {mag!r})"
    print(f"{what}: T = {T}, largest |got - exact| / bound = {worst:.3g}")
    assert np.array_equal(got[:, 0], entries[:, :, 0].sum(axis=0)), f"{what}: counts"


def _same_bits(a, b, what):
    import torch
    a, b = a.contiguous(), b.contiguous()
    iv = torch.int64 if a.dtype == torch.float64 else torch.int32
    assert torch.equal(a.view(iv), b.view(iv)), f"{what}: bits differ"


# ---- one case ------------------------------------------------------------------------------------------------------------
def _launch_checked(case, call):
    """Run one K1 call; return the launch record after asserting it names the expected instance."""
    from s2_emit import _native as nat
    _record()                                                   # clear what an earlier call left
    rc = call()
    rec = _record()
    if case.expect is None:
        assert rc == case.err and rec is None, (rc, rec, nat.load().hsr_last_error())
        if case.bad:                                            # the message of hsr_srf.hip, with the job's own numbers
            T, idx = case.group_T, case.group_T - 1 if case.form == "group_last" else case.group_index
            text = f"group fit of {T} tiles (at most 64), index {idx}, or NULL group buffers, or combined with fit_ready_dev"
            assert text.encode() in nat.load().hsr_last_error(), nat.load().hsr_last_error()
        return None
    assert rc == 0, nat.load().hsr_last_error()
    assert rec is not None, "the call launched no K1 kernel"
    assert rec[:2] == (case.deg, case.expect), f"launched {TEMPLATES[rec[1]].format(d=rec[0])}, expected {TEMPLATES[case.expect].format(d=case.deg)}"
    assert 0 < rec[2] <= 160 * 1024
    SEEN.add(rec[:2])
    return rec


def _opts(case):
    from s2_emit import _native as nat
    return nat.SrfOptions(0, case.rc, 1 if case.single else 0, nat.HSR_SRF_U16_FAST if case.fastu else 0)


def _run_single(torch, case, rng):
    from s2_emit import _engine as eng, _native as nat
    lib = nat.load()
    npix, nb, B, deg = case.npix[0], case.nb, case.B, case.deg
    w, srf, good, k0, kl = _srf(B, nb, case.taps, rng)
    table = eng.build_srf_table(w, srf, good)
    assert table.nb == nb and np.array_equal(table.k0, k0) and np.array_equal(table.klen, kl)
    R, host, bad = _cube(case, npix, rng)
    ref = _oracle_planes(R, w, srf, good)
    cube = _device_cube(torch, host, case.aligned[0])
    row = eng.padded_row(nb)
    # output with guard elements around what the call owns
    if case.out == "planar":
        ostore = torch.full((nb, npix + 3), SENTINEL, device="cuda")
        oview, obs, ops = ostore[:, :npix], npix + 3, 1
    elif case.out == "narrow":
        ostore = torch.full((npix + 1, nb), SENTINEL, device="cuda")
        oview, obs, ops = ostore[:npix], 1, nb
    else:
        off = 1 if case.out == "pix_off" else 0
        flat = torch.full(((npix + 2) * row,), SENTINEL, device="cuda")
        ostore = flat[off:off + (npix + 1) * row].view(npix + 1, row)
        oview, obs, ops = ostore[:npix], 1, row
    owned = case.out == "pix" and row <= 16                  # 16-byte aligned rows of 4..16 floats: pad columns written (zeros)
    real = torch.from_numpy(_targets(ref, nb, row, rng)).cuda() if deg > 0 else None
    mask_np = (rng.random(npix) > 0.25) if case.mask else np.ones(npix, bool)
    mask = torch.from_numpy(mask_np.astype(np.uint8)).cuda() if case.mask else None
    wn = table.device_weights("cuda")
    k0p, klp = k0.ctypes.data_as(C.POINTER(C.c_int32)), kl.ctypes.data_as(C.POINTER(C.c_int32))
    o = _opts(case)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    u16 = case.dtype == "u16"
    sc = float(np.float32(1e-4))
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    ws = eng.MomentWorkspace("cuda", nb, deg) if deg > 0 else None
    slots = C.c_int32(0)
    ws_fit = eng.MomentWorkspace("cuda", nb, deg) if case.entry == "fit" else None
    fit = ws_fit.fused_fit(MIN_COUNT) if ws_fit is not None else None

    # apply job: the older tile (its rows, coefficients, mask) and the previous tile's partials for the tail fit
    job = ready_w = gate_w = sync_w = garr = gtotal = None
    if case.entry == "apply":
        an = case.apply_npix
        xa = (rng.random((an, row)) * 1.7 - 0.3).astype(np.float32)
        xa[an // 2, 0] = np.nan
        xd = torch.from_numpy(xa).cuda()
        aout = torch.full((an + 2, row), SENTINEL, device="cuda")
        co = np.zeros((nb, deg + 1))
        co[:, -2] = rng.uniform(0.8, 1.2, nb)
        co[:, -1] = rng.uniform(-0.05, 0.05, nb)
        if deg >= 2:
            co[:, :-2] = rng.uniform(-0.3, 0.3, (nb, deg - 1))
        cod = torch.from_numpy(co).cuda()
        amask = rng.random(an) > 0.4
        amd = torch.from_numpy(amask.astype(np.uint8)).cuda()
        job = ApplyJob()
        if case.job_x:
            job.x_dev, job.out_dev, job.coeffs_dev = xd.data_ptr(), aout.data_ptr(), cod.data_ptr()
            job.mask_dev = amd.data_ptr() if case.mask else None
            job.npix, job.clip = an, int(case.clip)
        if case.tail:
            prev = eng.MomentWorkspace("cuda", nb, deg)
            pimg = torch.empty((npix, row), device="cuda")
            rc = (lib.hsr_srf_integrate_moments_u16 if u16 else lib.hsr_srf_integrate_moments)(
                *((P(cube), npix, B, sc, NODATA) if u16 else (P(cube), npix, B)), P(wn), k0p, klp, nb, P(pimg), 1, row,
                P(real), 1, row, P(mask), case.minv, case.minv, deg, P(prev.partials), C.byref(slots), C.byref(o), st)
            if case.expect is not None:
                assert rc == 0, lib.hsr_last_error()
            prev.slots = slots.value
            # what the tail must not write holds the sentinel (the plain rows keep their zeros: the tail writes all of both)
            M, T = 3 * deg + 2, case.group_T
            f64 = dict(dtype=torch.float64, device="cuda")
            fill = 0.0 if case.form == "plain" else SENTINEL
            if T:                                               # fit_moments_dev is entry gidx of [T][nb][M], as job_fit (hsr_exec.hip) sets it
                gidx = T - 1 if case.form == "group_last" else case.group_index
                garr = torch.full((max(T, gidx + 1), nb, M), SENTINEL, **f64)
                gtotal = torch.full((nb, M), SENTINEL, **f64)
                tail_mom = torch.full((nb, M), SENTINEL, **f64) if case.detached else garr[gidx]
                if case.form == "group_last":
                    syn_x, syn_y, syn_ent = _synthetic_entries(case, T - 1, rng)
                    garr[:T - 1] = torch.from_numpy(syn_ent).cuda()
            else:
                tail_mom = torch.full((nb, M), fill, **f64)
            tail_co = torch.full((nb, deg + 1), fill, **f64)
            counter = _u32(torch, case.tbase)
            job.fit_slots, job.fit_partials_dev = prev.slots, prev.partials.data_ptr()
            job.fit_moments_dev, job.fit_coeffs_dev = tail_mom.data_ptr(), tail_co.data_ptr()
            job.fit_min_count, job.fit_counter_dev, job.fit_ticket_base = case.min_count, counter.data_ptr(), case.tbase
            if case.form == "exchange" or case.bad == "ready":
                ready_w = _u32(torch, case.ready0)
                job.fit_ready_dev = ready_w.data_ptr()
            if T:
                job.fit_group_tiles, job.fit_group_index = T, gidx
                job.fit_group_moments_dev = garr.data_ptr()
                job.fit_group_total_dev = None if case.bad == "total" else gtotal.data_ptr()
        if case.form != "plain" or case.ready is not None:
            sync_w = _u32(torch, 0)
            job.sync_error_dev = sync_w.data_ptr()
        if case.ready is not None:
            # the wait must be satisfied before the launch is enqueued: a word behind its value would spin for the time limit
            assert case.job_x and ((case.ready[0] - case.ready[1]) & 0xFFFFFFFF) < 0x80000000, case.ready
            gate_w = _u32(torch, case.ready[0])
            job.coeffs_ready_dev, job.coeffs_ready_value = gate_w.data_ptr(), case.ready[1]

    def restore(tbase):
        """The words and entries a launch changes, back to what they held before the first launch."""
        if case.tail:
            _set_u32(counter, tbase)
            job.fit_ticket_base = tbase
        if ready_w is not None:
            _set_u32(ready_w, case.ready0)
        if gate_w is not None:
            _set_u32(gate_w, case.ready[0])
        if case.form == "group_last":
            garr[case.group_T - 1] = POISON                     # the kernel takes this entry from what it has just reduced

    def tail_state():
        return (tail_mom.clone(), tail_co.clone()) + ((garr.clone(), gtotal.clone()) if case.group_T else ())

    def call():
        head = (P(cube), npix, B, sc, NODATA) if u16 else (P(cube), npix, B)
        bands = (P(wn), k0p, klp, nb, P(oview), obs, ops)
        if deg == 0:
            return (lib.hsr_srf_integrate_u16 if u16 else lib.hsr_srf_integrate)(*head, *bands, C.byref(o), st)
        fit_args = (P(real), 1, row, P(mask), case.minv, case.minv, deg, P(ws.partials), C.byref(slots))
        if case.entry == "moments":
            return (lib.hsr_srf_integrate_moments_u16 if u16 else lib.hsr_srf_integrate_moments)(*head, *bands, *fit_args, C.byref(o), st)
        if case.entry == "fit":
            return (lib.hsr_srf_integrate_fit_u16 if u16 else lib.hsr_srf_integrate_fit)(*head, *bands, *fit_args, C.byref(fit), C.byref(o), st)
        return (lib.hsr_srf_integrate_moments_u16_apply if u16 else lib.hsr_srf_integrate_moments_apply)(
            *head, *bands, *fit_args, C.byref(o), C.byref(job), st)

    runs = []
    for rep in range(2):
        restore(case.tbase)
        if _launch_checked(case, call) is None:
            return
        torch.cuda.synchronize()
        if case.tail:                                           # one ticket per workgroup: what the pipeline advances its base by
            assert slots.value > 8 or not case.tbase, "the counter must wrap inside the launch"
            assert _get_u32(counter) == (case.tbase + slots.value) & 0xFFFFFFFF, "ticket counter"
        if ready_w is not None:
            assert _get_u32(ready_w) == (case.ready0 + nb) & 0xFFFFFFFF, "*fit_ready_dev must grow by nb"
        if gate_w is not None:
            assert _get_u32(gate_w) == case.ready[0], "*coeffs_ready_dev written"
        if sync_w is not None:
            assert _get_u32(sync_w) == 0, "sync_error_dev"
        snap = {"out": ostore.clone()}
        if deg > 0:
            ws.slots = slots.value
            assert ws.slots == lib.hsr_partial_slots(npix, C.byref(o))
            snap["mom"] = eng.moments_reduce(ws).clone()
        if ws_fit is not None:
            snap["fit"] = (ws_fit.moments.clone(), ws_fit.coeffs.clone())
            assert int(ws_fit.tickets.abs().sum()) == 0
        if job is not None and case.job_x:
            snap["apply"] = aout.clone()
        if case.tail:
            snap["tail"] = tail_state()
        runs.append(snap)
    if case.tbase:                                              # the same launch at base 0: the same bits
        restore(0)
        assert call() == 0, lib.hsr_last_error()
        torch.cuda.synchronize()
        for a, b in zip(runs[0]["tail"], tail_state()):
            _same_bits(a, b, f"ticket base {case.tbase:#x} against base 0")
    for key in runs[0]:
        for a, b in zip(*(r[key] if isinstance(r[key], tuple) else (r[key],) for r in runs)):
            _same_bits(a, b, key)
    r = runs[0]
    out = r["out"].cpu().numpy()
    tol = 3e-6 if table_taps_global(k0, kl, B) else 2e-6
    if case.out == "planar":
        got = out[:, :npix]
        assert np.all(out[:, npix:] == SENTINEL), "planar: elements past npix written"
    else:
        got = out[:npix, :nb].T
        assert np.all(out[npix:] == SENTINEL), "rows past npix written"
        if out.shape[1] > nb:
            assert np.all(out[:npix, nb:] == 0.0) if owned else np.all(out[:npix, nb:] == SENTINEL), "pad columns"
    _check_planes(got, ref, tol, "planes")
    if bad.any():
        assert np.isnan(got[:, bad]).all(), "nodata pixels must be NaN in every band"
    if deg == 0:
        return
    x = got.astype(np.float32)
    y = real.cpu().numpy()[:, :nb].T
    _check_moments(r["mom"].cpu().numpy(), x, y, mask_np, case.minv, deg, "moments")
    if ws_fit is not None:
        want = eng.reduce_solve_slots(ws.partials, ws.slots, ws, MIN_COUNT, torch.empty_like(ws_fit.moments), torch.empty_like(ws_fit.coeffs))
        _same_bits(r["fit"][0], want[0], "fused fit moments vs hsr_moments_reduce_solve")
        _same_bits(r["fit"][1], want[1], "fused fit coefficients vs hsr_moments_reduce_solve")
        _check_coeffs(r["fit"][1].cpu().numpy(), x, y, mask_np, case.minv, deg, "fused fit")
    if case.tail:
        tm, tc = r["tail"][0], r["tail"][1]
        tc_np = tc.cpu().numpy()
        # every form writes the tile's own moments: the bits of hsr_moments_reduce, and the float64 sums
        _same_bits(tm, eng.reduce_slots(prev.partials, prev.slots, nb, deg), f"{case.form}: tile moments vs hsr_moments_reduce")
        _check_moments(tm.cpu().numpy(), x, y, mask_np, case.minv, deg, f"{case.form}: tile moments")
        if case.form == "plain":
            want = eng.reduce_solve_slots(prev.partials, prev.slots, prev, MIN_COUNT, torch.empty_like(tail_mom), torch.empty_like(tail_co))
            _same_bits(tm, want[0], "tail fit moments vs hsr_moments_reduce_solve")
            _same_bits(tc, want[1], "tail fit coefficients vs hsr_moments_reduce_solve")
            _check_coeffs(tc_np, x, y, mask_np, case.minv, deg, "tail fit")
        else:
            ga, gt = (r["tail"][2].cpu().numpy(), r["tail"][3].cpu().numpy()) if case.group_T else (None, None)
            if case.form != "group_last":                        # no solve in this launch
                assert np.all(tc_np == SENTINEL), f"{case.form}: fit_coeffs_dev written"
            if case.form == "group_mid":
                others = np.arange(case.group_T) != case.group_index
                assert np.all(ga[others] == SENTINEL) and np.all(gt == SENTINEL), "group_mid: another entry or the group's total written"
            if case.form == "group_last":
                T = case.group_T
                assert np.array_equal(ga[:T - 1].view(np.int64), syn_ent.view(np.int64)), "group_last: another tile's entry written"
                if case.detached:
                    assert np.all(ga[T - 1] == POISON), "group_last: the array's last entry written though fit_moments_dev points elsewhere"
                ent = torch.cat([torch.from_numpy(syn_ent).cuda(), tm[None]])        # the T entries, the true last one in place
                want = eng.reduce_solve_slots(ent, T, prev, case.min_count, torch.empty_like(gtotal), torch.empty_like(tail_co))
                _same_bits(r["tail"][3], want[0], "group total vs hsr_moments_reduce_solve over the T entries")
                _same_bits(tc, want[1], "group coefficients vs hsr_moments_reduce_solve over the T entries")
                _check_group_sum(gt, ent.cpu().numpy(), "group total")
                # the polynomial of the union of the group's pixels: the tile's valid ones and the synthetic sets
                ux, uy = np.concatenate([x, syn_x], axis=1), np.concatenate([y, syn_y], axis=1)
                um = np.concatenate([mask_np, np.ones(syn_x.shape[1], bool)])
                counts = _check_coeffs(tc_np, ux, uy, um, case.minv, deg, "group fit", case.min_count, case.band1 == "none")
                own = _valid(x, y, mask_np, case.minv).sum(axis=1)
                fitted = [b for b in range(nb) if b != 1]
                if case.band1 == "others":                       # no pixel of its own, fitted from the other entries
                    ident = np.zeros(deg + 1)
                    ident[-2] = 1.0
                    assert own[1] == 0 and counts[1] >= case.min_count and not np.array_equal(tc_np[1], ident), (own[1], counts[1], tc_np[1])
                if case.min_count != MIN_COUNT:                  # the group's count decides, not the last tile's
                    assert all(own[b] < case.min_count <= counts[b] for b in fitted), (own, counts)
                    ident = np.zeros(deg + 1)
                    ident[-2] = 1.0
                    assert all(not np.array_equal(tc_np[b], ident) for b in fitted)
        FORMS_SEEN.add((deg, case.expect, case.form))
    if "apply" in r:
        ao = r["apply"].cpu().numpy()
        want = onp.apply_poly_planes(xa[:, :nb].T, co, amask if case.mask else None, clip=case.clip)
        np.testing.assert_array_equal(ao[:an, :nb].T, want, err_msg="matched rows")
        fin = np.isfinite(want)
        assert np.array_equal(ao[:an, :nb].T[fin].view(np.int32), want[fin].view(np.int32)), "matched rows: bits"
        assert np.array_equal(ao[:an, nb:].view(np.int32), xa[:, nb:].view(np.int32)), "pad columns pass through"
        assert np.all(ao[an:] == SENTINEL), "rows past apply_npix written"


def table_taps_global(k0, kl, B):
    """Do the weights stay in global memory (srf_prepare_bands: 16-tap chunks inside [0, B), 1024 taps at most)?"""
    nc = (kl + 15) // 16
    return bool(np.any(16 * nc > B) or int((16 * nc).sum()) > 1024)


def _run_batch(torch, case, rng):
    from s2_emit import _engine as eng, _native as nat
    lib = nat.load()
    nb, B, deg = case.nb, case.B, case.deg
    w, srf, good, k0, kl = _srf(B, nb, case.taps, rng)
    table = eng.build_srf_table(w, srf, good)
    assert table.nb == nb and np.array_equal(table.k0, k0) and np.array_equal(table.klen, kl)
    row = eng.padded_row(nb)
    aligned = case.aligned if len(case.aligned) == len(case.npix) else case.aligned * len(case.npix)
    tiles = []
    for n, al in zip(case.npix, aligned):
        R, host, bad = _cube(case, n, rng)
        ref = _oracle_planes(R, w, srf, good)
        y = _targets(ref, nb, row, rng) if deg > 0 else None
        m = (rng.random(n) > 0.25) if case.mask and len(tiles) % 2 == 0 else None
        tiles.append(dict(n=n, ref=ref, bad=bad, cube=_device_cube(torch, host, al), y=y, m=m))
    reals = [torch.from_numpy(t["y"]).cuda() for t in tiles] if deg > 0 else None
    masks = [torch.from_numpy(t["m"].astype(np.uint8)).cuda() if t["m"] is not None else None for t in tiles]
    tb = eng.TileBatch([t["cube"] for t in tiles], reals, masks, table, deg, _opts(case))
    assert tb.info.aligned16 == int(all(aligned))
    tb.pseudo.fill_(SENTINEL)
    runs = []
    for rep in range(2):
        if _launch_checked(case, lambda: _batch_call(lib, tb, case)) is None:
            return
        snap = [tb.pseudo.clone()]
        if deg > 0:
            eng.batch_reduce_solve(tb, MIN_COUNT)
            snap.append(tb.moments.clone())
        runs.append(snap)
    for a, b in zip(*runs):
        _same_bits(a, b, "batch")
    pseudo = runs[0][0].cpu().numpy()
    tol = 3e-6 if table_taps_global(k0, kl, B) else 2e-6
    for i, t in enumerate(tiles):
        rows = pseudo[tb.offsets[i]:tb.offsets[i + 1]]
        got = rows[:, :nb].T
        assert np.all(rows[:, nb:] == 0.0), f"tile {i}: pad columns"
        _check_planes(got, t["ref"], tol, f"tile {i} planes")
        if t["bad"].any():
            assert np.isnan(got[:, t["bad"]]).all(), f"tile {i}: nodata pixels must be NaN in every band"
        if deg > 0:
            mk = t["m"] if t["m"] is not None else np.ones(t["n"], bool)
            _check_moments(runs[0][1][i].cpu().numpy(), got.astype(np.float32), t["y"][:, :nb].T, mk, case.minv, deg, f"tile {i} moments")


def _batch_call(lib, tb, case):
    import torch
    from s2_emit import _engine as eng
    wn = tb.table.device_weights(tb.device)
    k0 = np.ascontiguousarray(tb.table.k0, np.int32)
    kl = np.ascontiguousarray(tb.table.klen, np.int32)
    o = _opts(case)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lib.hsr_srf_integrate_moments_batched(C.c_void_p(tb.units_dev.data_ptr()), C.byref(tb.info), 2 if tb.u16 else 0,
                                                 float(np.float32(1e-4)), NODATA, tb.table.B, C.c_void_p(wn.data_ptr()),
                                                 k0.ctypes.data_as(C.POINTER(C.c_int32)), kl.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 tb.nb, tb.row, tb.real_row, case.minv, case.minv, tb.deg, C.byref(o), st)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_k1_instance_vs_float64_reference(torch_gpu, case):
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    if case.entry == "batch":
        _run_batch(torch_gpu, case, rng)
    else:
        _run_single(torch_gpu, case, rng)


def test_k1_case_table_reaches_every_instance(torch_gpu):
    """The rows above launched every instance the library's table holds - no more, no fewer.  A new instance without a
    row, or a selection change that leaves an instance unreachable from these geometries, fails here."""
    from s2_emit import _native as nat
    lib = nat.load()
    table = {(d, v) for d in range(nat.HSR_MAX_DEG + 1) for v in range(len(TEMPLATES)) if lib.hsr_srf_kernel_instance(d, v) == 1}
    assert lib.hsr_srf_kernel_instance(0, len(TEMPLATES)) == -1          # TEMPLATES covers the whole table
    assert len(table) == 106
    missing = sorted(table - SEEN)
    assert not missing, "instances no row launched: " + "; ".join(TEMPLATES[v].format(d=d) for d, v in missing)
    assert SEEN <= table


def test_k1_case_table_runs_every_job_form_on_every_apply_instance(torch_gpu):
    """Every job-carrying instance the table query reports has been launched - and has passed its row - in each of the forms
    the exchange and group pipelines use, besides the plain one."""
    from s2_emit import _native as nat
    lib = nat.load()
    carriers = {(d, v) for d in range(nat.HSR_MAX_DEG + 1) for v in APPLY_VARIANTS if lib.hsr_srf_kernel_instance(d, v) == 1}
    assert len(carriers) == 16
    missing = sorted((d, v, f) for d, v in carriers for f in ("plain", "exchange", "group_mid", "group_last") if (d, v, f) not in FORMS_SEEN)
    assert not missing, "job forms no row launched: " + "; ".join(f"{TEMPLATES[v].format(d=d)} {f}" for d, v, f in missing)
    for v in APPLY_VARIANTS:                                   # the gated pre-phase with the exchange tail and without any tail
        for tail in (True, False):
            assert any(c.expect == v and c.ready is not None and c.tail == tail for c in CASES), (v, tail)
