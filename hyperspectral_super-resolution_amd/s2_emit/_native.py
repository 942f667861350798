"""ctypes binding of libhsr_mi355x.so (C ABI: include/hsr.h, include/hsr_color.h, include/hsr_coreg.h, include/hsr_reproject.h, include/hsr_scl.h, include/hsr_s2stack.h, include/hsr_hist.h, include/hsr_resize.h, include/hsr_merge.h and include/hsr_roi.h).

The HIP library is the product path.  There is deliberately NO CPU fallback: if the shared
library is missing, or no MI355X-class device is visible, every compute entry point raises
``HsrUnavailable`` loudly instead of silently computing something else.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
_DEFAULT_SO = os.path.join(os.path.dirname(_HERE), "lib", "libhsr_mi355x.so")

HSR_OK = 0
HSR_MAX_BANDS = 16
HSR_MAX_DEG = 4
HSR_MAX_APPLY_DEG = 8
HSR_MAX_SPECTRAL = 560
HSR_TILE_PIXELS = 64
HSR_SRF_U16_FAST = 1
HSR_MAX_PARTIALS = 4096
HSR_FIT_GROUPS = 64
HSR_FIT_TICKETS = 65
PLANAR = "planar"        # band-major planes: tensor (nb, npix), unit pixel stride
PIXMAJOR = "pixmajor"    # pixel-major / band-last: tensor (npix, row) with row >= nb, unit band stride


class HsrUnavailable(RuntimeError):
    """The HIP extension (or a GPU to run it on) is not available."""


class HsrError(RuntimeError):
    """A library call returned an error code."""


_i32, _i64, _f32, _f64, _vp = C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_void_p
_pi32 = C.POINTER(C.c_int32)


class SrfOptions(C.Structure):
    """hsr_srf_options (include/hsr.h): per-call tuning of the K1 launches; the library keeps no tuning state."""
    _fields_ = [("tile_pixels", _i32), ("reserved_cus", _i32), ("u16_single_buffer", _i32), ("flags", _i32)]


class BatchTile(C.Structure):
    """hsr_batch_tile: one tile of a batch (64 bytes)."""
    _fields_ = [("cube_dev", _vp), ("real_dev", _vp), ("mask_dev", _vp), ("pseudo_dev", _vp), ("matched_dev", _vp),
                ("npix", _i64), ("slot0", _i64), ("slots", _i32), ("ngroups", _i32)]


class BatchInfo(C.Structure):
    """hsr_batch_info: what hsr_batch_plan found."""
    _fields_ = [("nunits", _i64), ("total_pixels", _i64), ("max_npix", _i64), ("ntiles", _i32), ("aligned16", _i32)]


class FusedFit(C.Structure):
    """hsr_fused_fit: workspaces and outputs of the reduce + solve folded into K1 (hsr_srf_integrate_fit)."""
    _fields_ = [("group_partials_dev", _vp), ("tickets_dev", _vp), ("moments_dev", _vp), ("coeffs_dev", _vp),
                ("min_count", _i64)]


class StepDesc(C.Structure):
    """hsr_step_desc: every argument of one tile's step for fixed output / workspace buffers (include/hsr.h, ABI 4)."""
    _fields_ = [("cube_dtype", _i32), ("B", _i32), ("npix", _i64), ("scale", _f32), ("nodata", _i32),
                ("wn_dev", _vp), ("k0", _pi32), ("klen", _pi32), ("nb", _i32), ("deg", _i32),
                ("pseudo_dev", _vp), ("out_bs", _i64), ("out_ps", _i64), ("real_bs", _i64), ("real_ps", _i64),
                ("min_x", _f32), ("min_y", _f32), ("partials_dev", _vp), ("moments_dev", _vp), ("coeffs_dev", _vp),
                ("min_count", _i64), ("matched_dev", _vp), ("matched_bs", _i64), ("matched_ps", _i64),
                ("apply_mask", _i32), ("clip", _i32), ("opts", SrfOptions)]


HSR_ABI_VERSION = 5
HSR_COMM_ID_BYTES = 128
HSR_SYNC_ALLREDUCE, HSR_SYNC_BROADCAST = 1, 2
# hsr_host_sum_fn: int (*)(void* user, double* values, int32_t count) - the host transport of an exchange pipeline
HOST_SUM_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int32)


class Exchange(C.Structure):
    """hsr_exchange: how the fit crosses the ranks in hsr_pipeline_create_exchange (an RCCL communicator or a host callback)."""
    _fields_ = [("comm", _vp), ("mode", _i32), ("root", _i32), ("host_sum", HOST_SUM_FN), ("host_user", _vp),
                ("rehearsal_us", _i32), ("rehearsal_blocks", _i32)]


BATCH_RECORD_BYTES = 64          # sizeof(hsr_batch_tile) == sizeof(hsr_batch_unit)
assert C.sizeof(BatchTile) == BATCH_RECORD_BYTES
_popt = C.POINTER(SrfOptions)

# name -> (restype, argtypes); must list every symbol include/hsr.h declares
SIGNATURES = {
    "hsr_abi_version": (C.c_int, []),
    "hsr_last_error": (C.c_char_p, []),
    "hsr_moment_count": (C.c_int, [_i32]),
    "hsr_partial_slots": (C.c_int, [_i64, _popt]),
    "hsr_partials_bytes": (C.c_size_t, [_i32, _i32]),
    "hsr_srf_integrate": (C.c_int, [_vp, _i64, _i32, _vp, _pi32, _pi32, _i32, _vp, _i64, _i64, _popt, _vp]),
    "hsr_srf_integrate_moments": (C.c_int, [_vp, _i64, _i32, _vp, _pi32, _pi32, _i32, _vp, _i64, _i64,
                                            _vp, _i64, _i64, _vp, _f32, _f32, _i32, _vp, _pi32, _popt, _vp]),
    "hsr_poly_moments": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i32, _i32, _f32, _f32, _vp, _vp,
                                   _vp, _pi32, _vp]),
    "hsr_poly_moments_f64": (C.c_int, [_vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _pi32, _vp]),
    "hsr_moments_reduce": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "hsr_poly_solve": (C.c_int, [_vp, _i32, _i32, _i64, _vp, _vp]),
    "hsr_moments_reduce_solve": (C.c_int, [_vp, _i32, _i32, _i32, _i64, _vp, _vp, _vp]),
    "hsr_poly_solve_host": (C.c_int, [C.POINTER(_f64), _i32, _i32, _i64, C.POINTER(_f64)]),
    "hsr_poly_apply": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i32, _i32, _i64, _vp, _i32, _vp, _i64, _i64, _vp]),
    "hsr_percentile_work_bytes": (C.c_size_t, [_i32]),
    "hsr_percentile_limits": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i32, _f64, _f64, _vp, _vp, _vp]),
    "hsr_percentile_begin": (C.c_int, [_vp, _i32, _vp]),
    "hsr_percentile_hist_region": (C.c_int, [_i32, _i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "hsr_percentile_hist": (C.c_int, [_i32, _vp, _i64, _i64, _vp, _i64, _i32, _vp, _vp]),
    "hsr_percentile_scan": (C.c_int, [_i32, _i32, _f64, _f64, _vp, _vp, _vp]),
    "hsr_tile_encode_u16": (C.c_int, [_vp, _i64, _f32, _i32, _f32, _i32, _vp, _vp]),
    "hsr_tile_decode_u16": (C.c_int, [_vp, _i64, _f32, _i32, _vp, _vp]),
    "hsr_srf_integrate_u16": (C.c_int, [_vp, _i64, _i32, _f32, _i32, _vp, C.POINTER(_i32), C.POINTER(_i32), _i32,
                                        _vp, _i64, _i64, _popt, _vp]),
    "hsr_srf_integrate_moments_u16": (C.c_int, [_vp, _i64, _i32, _f32, _i32, _vp, C.POINTER(_i32), C.POINTER(_i32),
                                                _i32, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _f32, _f32, _i32, _vp,
                                                C.POINTER(_i32), _popt, _vp]),
    "hsr_srf_integrate_moments_apply": (C.c_int, [_vp, _i64, _i32, _vp, _pi32, _pi32, _i32, _vp, _i64, _i64,
                                                  _vp, _i64, _i64, _vp, _f32, _f32, _i32, _vp, _pi32, _popt, _vp, _vp]),
    "hsr_srf_integrate_moments_u16_apply": (C.c_int, [_vp, _i64, _i32, _f32, _i32, _vp, _pi32, _pi32, _i32, _vp, _i64, _i64,
                                                      _vp, _i64, _i64, _vp, _f32, _f32, _i32, _vp, _pi32, _popt, _vp, _vp]),
    "hsr_srf_integrate_fit": (C.c_int, [_vp, _i64, _i32, _vp, _pi32, _pi32, _i32, _vp, _i64, _i64, _vp, _i64, _i64, _vp,
                                        _f32, _f32, _i32, _vp, _pi32, C.POINTER(FusedFit), _popt, _vp]),
    "hsr_srf_integrate_fit_u16": (C.c_int, [_vp, _i64, _i32, _f32, _i32, _vp, _pi32, _pi32, _i32, _vp, _i64, _i64, _vp,
                                            _i64, _i64, _vp, _f32, _f32, _i32, _vp, _pi32, C.POINTER(FusedFit), _popt, _vp]),
    "hsr_batch_partials_bytes": (C.c_size_t, [_i64, _i32, _i32]),
    "hsr_batch_plan": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _popt, _vp, _i64, C.POINTER(BatchInfo)]),
    "hsr_srf_integrate_moments_batched": (C.c_int, [_vp, C.POINTER(BatchInfo), _i32, _f32, _i32, _i32, _vp, _pi32, _pi32,
                                                    _i32, _i32, _i32, _f32, _f32, _i32, _popt, _vp]),
    "hsr_moments_reduce_solve_batched": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i64, _vp, _vp, _vp]),
    "hsr_poly_apply_batched": (C.c_int, [_vp, _i32, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "hsr_interleave_to_bip": (C.c_int, [_vp, _i32, _i32, _i64, _i64, _i64, _vp, _i32, _vp]),
    "hsr_ot_work_bytes": (_i64, [_i64, _i64]),
    "hsr_ot_work_region": (C.c_int, [_i64, _i64, _i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "hsr_ot_begin": (C.c_int, [_vp, _i64, _vp, _i64, _f64, _vp, _vp]),
    "hsr_ot_iterate": (C.c_int, [_i64, _i64, _i32, _i32, _f64, _vp, _vp, _vp]),
    "hsr_ot_finish": (C.c_int, [_vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp]),
    "hsr_ot_sinkhorn_barycentric": (C.c_int, [_vp, _i64, _vp, _i64, _f64, _i32, _f64, _vp, _vp, _vp, _vp]),
    "hsr_chol_work_bytes": (C.c_size_t, [_i32]),
    "hsr_chol_solve_f64": (C.c_int, [_vp, _i64, _i32, _vp, _i64, _i32, _vp, _vp, _vp]),
    "hsr_valid_mask": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _vp]),
    "hsr_polyfeat_count": (C.c_int, [_i32, _i32]),
    "hsr_polyfeat_table": (C.c_int, [_i32, _i32, _vp]),
    "hsr_polyfeat_prepare": (C.c_int, [_i32, _i32]),
    "hsr_polyfeat_expand_f64": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _i32, _vp]),
    "hsr_gram_work_bytes": (C.c_size_t, [_i32, _i32, _i64]),
    "hsr_gram_f64": (C.c_int, [_vp, _i64, _i32, _vp, _i64, _i32, _i64, _vp, _vp, _i64, _vp]),
    "hsr_polyfeat_predict": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _vp, _i32, _i32,
                                       _vp, _i64, _vp]),
    "hsr_ridge_stats_work_bytes": (C.c_size_t, [_i32]),
    "hsr_ridge_stats": (C.c_int, [_vp, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp]),
    "hsr_ridge_assemble": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _f64, _vp, _i32, _vp, _i64, _vp, _vp]),
    "hsr_ridge_finish": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hsr_polyfeat_predict_cube": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _vp, _i32, _i32,
                                            _i32, _f32, _i32, _vp, _i64, _vp]),
    "hsr_pair_prep": (C.c_int, [_vp, _i32, _i64, _i32, _vp, _i32, _vp, _i32, _i64, _i32, _i32, _i32, _i32, _f32, _i32, _f32,
                                _i32, _vp, _vp, _vp, _i32, _vp]),
    "hsr_pair_stats": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "hsr_pair_expand_f64": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _f64, _vp, _i64,
                                      _i64, _i32, _i32, _vp]),
    "hsr_gram_f64_batched": (C.c_int, [_vp, _i64, _i32, _i32, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _vp]),
    "hsr_ridge_assemble_batched": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _f64, _vp, _i32, _i64, _vp, _i64, _i64, _vp, _i32,
                                             _vp]),
    "hsr_chol_solve_f64_batched": (C.c_int, [_vp, _i64, _i32, _i64, _vp, _i64, _i32, _i64, _vp, _vp, _i32, _vp]),
    "hsr_ridge_finish_batched": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _i64, _i64, _vp, _vp, _i64, _i32, _i32, _vp, _vp,
                                           _i64, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i32, _vp]),
    "hsr_polyfeat_predict_cube_batched": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i32, _i32, _vp, _i64, _i64, _vp,
                                                    _i64, _i32, _i32, _i32, _f32, _i32, _vp, _i64, _i64, _i32, _vp]),
    "hsr_pair_report_work_bytes": (C.c_size_t, [_i64, _i32]),
    "hsr_pair_report_f64": (C.c_int, [_vp, _i64, _i64, _i32, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _i32, _vp,
                                      _vp, _i64, _vp, _vp, _i64, _i32, _vp]),
    "hsr_pair_holdout": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp, _i32, _vp]),
    "hsr_pair_score_work_bytes": (C.c_size_t, [_i64, _i32]),
    "hsr_pair_score_f64": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _f64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp,
                                     _vp, _i64, _vp, _i64, _i32, _vp]),
    "hsr_pool_stats": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hsr_pool_gram": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i32, _vp, _vp, _i32, _vp, _i64, _vp]),
    "hsr_pool_models": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp,
                                  _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "hsr_scene_black_counts": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f64, _f64, _f64, _f64, _vp, _vp]),
    "hsr_scene_gather_tiles": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _f32, _i32, _f32, _i32, _vp, _vp]),
    "hsr_scene_mosaic": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _i32, _i32, _f32, _i32, _vp]),
    "hsr_scene_mosaic_blend": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _i32, _i32, _f32, _vp]),
    "hsr_ortho_glt": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _f32, _f32, _i32,
                                _vp, _vp, _vp]),
    "hsr_block_mean": (C.c_int, [_vp, _i32, _i64, _i64, _i32, _i32, _i32, _i32, _f32, _vp, _i64, _i64, _vp]),
    "hsr_bilinear_upsample": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _i64, _i64, _vp]),
    "hsr_bilinear_upsample_mask_hist": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "hsr_probe_read": (C.c_int, [_vp, _i64, _i32, _vp, _vp]),
    "hsr_srf_last_launch": (C.c_int, [_pi32, _pi32, C.POINTER(_i64)]),
    "hsr_srf_kernel_instance": (C.c_int, [_i32, _i32]),
    "hsr_poly_last_launch": (C.c_int, [C.c_char_p, _i32]),
    "hsr_aux_last_launch": (C.c_int, [C.c_char_p, _i32]),
    "hsr_aux_instance_count": (C.c_int, []),
    "hsr_aux_instance_name": (C.c_char_p, [_i32]),
    "hsr_scene_last_launch": (C.c_int, [C.c_char_p, _i32]),
    "hsr_scene_instance_count": (C.c_int, []),
    "hsr_scene_instance_name": (C.c_char_p, [_i32]),
    "hsr_polyfeat_predict_kernel": (C.c_int, [_i32, _i32, _i32, _i32]),
    "hsr_k4_last_launch": (C.c_int, [C.c_char_p, _i32]),
    "hsr_k4_instance_count": (C.c_int, []),
    "hsr_k4_instance_name": (C.c_char_p, [_i32]),
    "hsr_pairs_last_launch": (C.c_int, [C.c_char_p, _i32]),
    "hsr_pairs_instance_count": (C.c_int, []),
    "hsr_pairs_instance_name": (C.c_char_p, [_i32]),
    "hsr_ortho_last_launch": (C.c_int, [C.c_char_p, _i32]),
    "hsr_ortho_instance_count": (C.c_int, []),
    "hsr_ortho_instance_name": (C.c_char_p, [_i32]),
    "hsr_step_plan_create": (C.c_int, [C.POINTER(StepDesc), C.POINTER(_vp)]),
    "hsr_step_plan_destroy": (None, [_vp]),
    "hsr_step_plan_slots": (C.c_int, [_vp]),
    "hsr_step_run": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "hsr_step_run_k1": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "hsr_step_run_reduce": (C.c_int, [_vp, _vp]),
    "hsr_step_run_solve": (C.c_int, [_vp, _vp]),
    "hsr_step_run_apply": (C.c_int, [_vp, _vp, _vp]),
    "hsr_pipeline_create": (C.c_int, [_vp, _vp, _vp, _i32, C.POINTER(_vp)]),
    "hsr_pipeline_create_fused": (C.c_int, [_vp, _vp, _vp, _vp, _i32, C.POINTER(_vp)]),
    "hsr_pipeline_destroy": (None, [_vp]),
    "hsr_pipeline_submit": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _pi32, _vp, _vp]),
    "hsr_pipeline_fit_done": (C.c_int, [_vp]),
    "hsr_pipeline_flush": (C.c_int, [_vp, _vp, _vp, _pi32]),
    "hsr_pipeline_count": (_i64, [_vp]),
    "hsr_pipeline_create_exchange": (C.c_int, [C.POINTER(_vp), _vp, C.POINTER(Exchange), C.POINTER(_vp)]),
    "hsr_pipeline_status": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint32)]),
    "hsr_pipeline_create_group": (C.c_int, [C.POINTER(_vp), _i32, _i32, _vp, _vp, _vp, _vp, C.POINTER(_vp)]),
    "hsr_srf_fused_launch_supported": (C.c_int, [_i32, _i32, _i32, _pi32, _pi32, _i64, _i32, _popt]),
    "hsr_comm_available": (C.c_int, []),
    "hsr_comm_version": (C.c_int, []),
    "hsr_comm_unique_id": (C.c_int, [_vp]),
    "hsr_comm_init": (C.c_int, [_i32, _i32, _vp, C.POINTER(_vp)]),
    "hsr_comm_destroy": (C.c_int, [_vp]),
    "hsr_comm_rank": (C.c_int, [_vp]),
    "hsr_comm_ranks": (C.c_int, [_vp]),
    "hsr_allreduce_f64": (C.c_int, [_vp, _vp, _i64, _vp]),
    "hsr_reduce_f64": (C.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "hsr_allreduce_u32": (C.c_int, [_vp, _vp, _i64, _vp]),
    "hsr_bcast": (C.c_int, [_vp, _vp, _i64, _i32, _vp]),
}

# The affine colour family, include/hsr_color.h: a table of its own (SIGNATURES is hsr.h's, name for name); load() types both.
_pf64 = C.POINTER(_f64)
HSR_AFFINE_MOMENTS = 22
HSR_AFFINE_MAX_SLOTS = 512
HSR_AFFINE_SLOT_PIXELS = 2048
COLOR_SIGNATURES = {
    "hsr_affine_partial_slots": (C.c_int, [_i64]),
    "hsr_affine_partials_bytes": (C.c_size_t, []),
    "hsr_affine_moments": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _pi32, _vp]),
    "hsr_affine_moments_f64": (C.c_int, [_vp, _i64, _vp, _i64, _i64, _vp, _pi32, _vp]),
    "hsr_affine_reduce_solve": (C.c_int, [_vp, _i32, _i64, _vp, _vp, _vp]),
    "hsr_affine_solve_host": (C.c_int, [_pf64, _i64, _pf64]),
    "hsr_affine_apply": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _vp, _i32, _vp, _i64, _i64, _vp]),
    "hsr_color_last_launch": (C.c_int, [C.c_char_p, _i32]),
    "hsr_color_instance_count": (C.c_int, []),
    "hsr_color_instance_name": (C.c_char_p, [_i32]),
}

# The co-registration family, include/hsr_coreg.h: again a table of its own; load() types all three.
HSR_COREG_RECORD = 8
HSR_COREG_MODEL = 10
COREG_SIGNATURES = {
    "hsr_coreg_surface": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _i64, _vp, _i32, _i64, _i32, _i32, _i32, _f64, _vp, _i32, _i32,
                                    _i32, _i32, _i32, _vp, _vp]),
    "hsr_coreg_peaks": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f64, _vp, _vp]),
    "hsr_coreg_fit_model": (C.c_int, [_vp, _i32, _i32, _i32, _f64, _i32, _i32, _vp, _vp]),
    "hsr_coreg_fit_model_host": (C.c_int, [_pf64, _i32, _i32, _i32, _f64, _i32, _i32, _pf64]),
    "hsr_coreg_warp": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i64, _i64, _vp, _i32, _f64, _f64, _f64, _f64, _vp, _i64, _i64, _vp,
                                 _vp]),
    "hsr_coreg_last_launch": (C.c_int, [C.c_char_p, _i32]),
    "hsr_coreg_instance_count": (C.c_int, []),
    "hsr_coreg_instance_name": (C.c_char_p, [_i32]),
}

# The reprojection family, include/hsr_reproject.h: a table of its own like the two above; load() types all four.
HSR_REPROJECT_STRICT, HSR_REPROJECT_RENORM = 0, 1
HSR_REPROJECT_TILE_W, HSR_REPROJECT_TILE_H = 64, 8
_REPROJECT_GEOMETRY = [_f64, _f64, _f64, _f64, _i32, _i32, _f64, _f64, _f64, _f64, _f64, _f64, _f64, _f64, _f64, _f64]
REPROJECT_SIGNATURES = {
    "hsr_reproject_coords": (C.c_int, _REPROJECT_GEOMETRY + [_vp, _vp]),
    "hsr_reproject_coords_host": (C.c_int, _REPROJECT_GEOMETRY + [_pf64]),
    "hsr_reproject_warp": (C.c_int, [_vp, _i32, _i32, _i32, _i64, _i64, _vp, _i32, _i32, _i32, _f64, _f64, _i32, _f64, _vp, _i64, _i64,
                                     _vp, _vp, _vp]),
    "hsr_reproject_last_launch": (C.c_int, [C.c_char_p, _i32]),
    "hsr_reproject_instance_count": (C.c_int, []),
    "hsr_reproject_instance_name": (C.c_char_p, [_i32]),
}

# The scene-classification family, include/hsr_scl.h: a table of its own like the three above; load() types all five.
HSR_SCL_BINS = 16
HSR_SCL_MAX_RADIUS = 32
HSR_SCL_DISC, HSR_SCL_SQUARE = 0, 1
HSR_SCL_MAX_K = 16
_u32 = C.c_uint32
_SCL_MASK = [_vp, _i32, _i32, _i64, _u32, _u32, _i32, _i32, _vp, _i64]
SCL_SIGNATURES = {
    "hsr_scl_class_counts": (C.c_int, [_vp, _i32, _i32, _i64, _i32, _i32, _vp, _vp]),
    "hsr_scl_mask": (C.c_int, _SCL_MASK + [_vp]),
    "hsr_scl_mask_host": (C.c_int, _SCL_MASK),
    "hsr_scl_coarse": (C.c_int, [_vp, _i32, _i32, _i64, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp]),
    "hsr_scl_gather_tiles": (C.c_int, [_vp, _i32, _i32, _i64, _vp, _i32, _i32, _i32, _vp, _vp]),
    "hsr_scl_apply": (C.c_int, [_vp, _i32, _i32, _i32, _i64, _i64, _vp, _i32, _i32, _i64, _i32, C.c_float, _vp, _vp]),
    "hsr_scl_last_launch": (C.c_int, [C.c_char_p, _i32]),
    "hsr_scl_instance_count": (C.c_int, []),
    "hsr_scl_instance_name": (C.c_char_p, [_i32]),
}

# The S2 stack family, include/hsr_s2stack.h: a table of its own like the four above; load() types all six.
HSR_S2_MAX_BANDS = 16
HSR_S2_NEAREST, HSR_S2_BILINEAR = 0, 1
HSR_S2_STRICT, HSR_S2_RENORM = 0, 1
HSR_S2_U16, HSR_S2_F32 = 0, 1
HSR_S2_TILE_H, HSR_S2_TILE_W = 16, 512


class S2Band(C.Structure):
    """hsr_s2_band: one band of the table of hsr_s2_stack (40 bytes)."""
    _fields_ = [("plane_dev", _vp), ("rs", _i64), ("H", _i32), ("W", _i32), ("up", _i32), ("method", _i32), ("add_offset", _i32),
                ("reserved", _i32)]


_S2_STACK = [C.POINTER(S2Band), _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _i64, _i32, _f32, _f64, _vp]
S2STACK_SIGNATURES = {
    "hsr_s2_stack": (C.c_int, _S2_STACK + [_vp]),
    "hsr_s2_stack_host": (C.c_int, _S2_STACK),
    "hsr_s2_expand_u8": (C.c_int, [_vp, _i32, _i32, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp]),
    "hsr_s2stack_last_launch": (C.c_int, [C.c_char_p, _i32]),
    "hsr_s2stack_instance_count": (C.c_int, []),
    "hsr_s2stack_instance_name": (C.c_char_p, [_i32]),
}

# The histogram-matching family, include/hsr_hist.h: a table of its own like the five above; load() types all seven.
HSR_HIST_MAX_CHANNELS = 16
HSR_HIST_SORT_TILE = 8192
HSR_HIST_SORT_BITS = 8
HSR_HIST_SCAN_STEP = 4096
HSR_HIST_PIVOT = 256
HSR_HIST_MAX_NPIX = 2147483647
HSR_HIST_SENTINEL = 0xFFFFFFFF
_HIST_IMAGES = [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i32]          # src, cs, ps, ref, cs, ps, mask, npix, C
HIST_SIGNATURES = {
    "hsr_hist_plane_stride": (_i64, [_i64]),
    "hsr_hist_sort_bytes": (C.c_size_t, [_i64, _i32]),
    "hsr_hist_pivot_bytes": (C.c_size_t, [_i64, _i32]),
    "hsr_hist_scratch_bytes": (C.c_size_t, [_i64, _i32]),
    "hsr_hist_keys": (C.c_int, _HIST_IMAGES + [_vp, _i64, _vp, _vp]),
    "hsr_hist_sort": (C.c_int, [_vp, _vp, _i64, _i64, _i32, _vp, C.c_size_t, _vp]),
    "hsr_hist_sort_pass": (C.c_int, [_vp, _vp, _i64, _i64, _i32, _i32, _vp, C.c_size_t, _vp]),
    "hsr_hist_lookup": (C.c_int, [_vp, _i64, _vp, _vp, C.c_size_t] + _HIST_IMAGES + [_vp, _i64, _i64, _vp]),
    "hsr_hist_match": (C.c_int, _HIST_IMAGES + [_vp, _i64, _i64, _vp, _vp, C.c_size_t, _vp]),
    "hsr_hist_match_host": (C.c_int, _HIST_IMAGES + [_vp, _i64, _i64, _vp]),
    "hsr_hist_key_host": (C.c_uint32, [_f32]),
    "hsr_hist_last_launch": (C.c_int, [C.c_char_p, _i32]),
    "hsr_hist_instance_count": (C.c_int, []),
    "hsr_hist_instance_name": (C.c_char_p, [_i32]),
}

# The area-resampling family, include/hsr_resize.h: a table of its own like the six above; load() types all eight.
HSR_AREA_MAX_SCALE = 64
HSR_AREA_MAX_CHANNELS = 16
HSR_AREA_F32, HSR_AREA_U8, HSR_AREA_U16 = 0, 1, 2
HSR_AREA_STRICT, HSR_AREA_RENORM = 0, 1
HSR_AREA_TILE_H, HSR_AREA_TILE_W = 8, 32
HSR_AREA_LDS_BYTES = 81920
# src, in_dtype, C, h, w, cs, rs, ps, y0, x0, sy, sx, has_nodata, nodata, rule, min_valid_frac, dst, out_dtype, H, W, cs, rs, ps,
# post_scale, fill, nodata_out, invalid
_AREA = [_vp, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _f64, _f64, _f64, _f64, _i32, _f64, _i32, _f64, _vp, _i32, _i32, _i32, _i64, _i64,
         _i64, _f32, _f32, _i32, _vp]
RESIZE_SIGNATURES = {
    "hsr_area_resample": (C.c_int, _AREA + [_vp]),
    "hsr_area_resample_host": (C.c_int, _AREA),
    "hsr_area_resample_instance": (C.c_int, [_i32, _i32, _i32, _i64, _i64, _f64, _f64]),
    "hsr_area_grid_from_geotransforms": (C.c_int, [_pf64, _pf64, _pf64]),
    "hsr_resize_last_launch": (C.c_int, [C.c_char_p, _i32]),
    "hsr_resize_instance_count": (C.c_int, []),
    "hsr_resize_instance_name": (C.c_char_p, [_i32]),
}

# The scene-merging family, include/hsr_merge.h: a table of its own like the seven above; load() types all nine.
HSR_MERGE_MAX_SOURCES = 8
HSR_MERGE_MAX_BANDS = 512
HSR_MERGE_RUN = 1024
HSR_MERGE_NO_SOURCE = 255


class MergeScene(C.Structure):
    """hsr_merge_scene: one orthorectified scene of hsr_merge_scenes (32 bytes)."""
    _fields_ = [("scene_dev", _vp), ("h", _i32), ("w", _i32), ("off_y", _i32), ("off_x", _i32), ("bands", _i32), ("reserved", _i32)]


class MergeSwath(C.Structure):
    """hsr_merge_swath: one swath of hsr_ortho_merge (64 bytes)."""
    _fields_ = [("swath_dev", _vp), ("glt_dev", _vp), ("qmask_dev", _vp), ("bmask_dev", _vp), ("rows", _i32), ("cols", _i32),
                ("glt_h", _i32), ("glt_w", _i32), ("off_y", _i32), ("off_x", _i32), ("bmask_bytes", _i32), ("bands", _i32)]


assert C.sizeof(MergeScene) == 32 and C.sizeof(MergeSwath) == 64
_MERGE_SCENES = [C.POINTER(MergeScene), _i32, _i32, _i32, _i32, _f32, _i32, _vp, _vp]
MERGE_SIGNATURES = {
    "hsr_merge_grid": (C.c_int, [_pf64, _pi32, _i32, _pf64, _pf64, _pi32, _pi32, _pf64]),
    "hsr_merge_scenes": (C.c_int, _MERGE_SCENES + [_vp]),
    "hsr_merge_scenes_host": (C.c_int, _MERGE_SCENES),
    "hsr_ortho_merge": (C.c_int, [C.POINTER(MergeSwath), _i32, _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp]),
    "hsr_merge_last_launch": (C.c_int, [C.c_char_p, _i32]),
    "hsr_merge_instance_count": (C.c_int, []),
    "hsr_merge_instance_name": (C.c_char_p, [_i32]),
}

# The polygon family, include/hsr_roi.h: a table of its own like the eight above; load() types all ten.
HSR_ROI_MAX_EDGES = 8192
HSR_ROI_CENTER, HSR_ROI_TOUCHED = 0, 1
HSR_ROI_TILE_H, HSR_ROI_TILE_W = 64, 256
HSR_ROI_RUN = 16
HSR_ROI_RECORD = 8
_u8 = C.c_uint8
_ROI_GRID = [_vp, _vp, _i32, _i32, _pf64, _i32, _i32]                        # verts, ring_offsets, nrings, nverts, gt, H, W
_ROI_RASTER = _ROI_GRID + [_i32, _i32, _i32, _i32, _i32, _u8, _u8, _vp, _i64]  # rule, window, inside, outside, out, out_rs
_ROI_CLIP = _ROI_GRID + [_vp, _i32, _i32, _i32, _i32, _vp, _vp]               # glt, window, out_glt, record
ROI_SIGNATURES = {
    "hsr_roi_check_host": (C.c_int, [_vp, _vp, _i32, _i32]),
    "hsr_roi_rasterize": (C.c_int, _ROI_RASTER + [_vp]),
    "hsr_roi_rasterize_host": (C.c_int, _ROI_RASTER),
    "hsr_roi_class_counts": (C.c_int, _ROI_GRID + [_i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp]),
    "hsr_roi_glt_clip": (C.c_int, _ROI_CLIP + [_vp]),
    "hsr_roi_glt_clip_host": (C.c_int, _ROI_CLIP),
    "hsr_roi_glt_reindex": (C.c_int, [_vp, _i32, _i32, _vp, _vp]),
    "hsr_roi_glt_reindex_host": (C.c_int, [_vp, _i32, _i32, _vp]),
    "hsr_roi_last_launch": (C.c_int, [C.c_char_p, _i32]),
    "hsr_roi_instance_count": (C.c_int, []),
    "hsr_roi_instance_name": (C.c_char_p, [_i32]),
}

_lib: Optional[C.CDLL] = None
_lib_path: Optional[str] = None


def library_path() -> str:
    return os.environ.get("HSR_LIBRARY", _DEFAULT_SO)


def load() -> C.CDLL:
    """Load the shared library (once) and type every entry point."""
    global _lib, _lib_path
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.isfile(path):
        raise HsrUnavailable(
            f"HIP extension not built: {path} is missing. Build it with "
            f"`make -C hyperspectral_super-resolution_amd/csrc` (or __graft_entry__.build()). "
            f"There is no CPU fallback for the s2_emit hot path.")
    try:
        lib = C.CDLL(path)
    except OSError as e:  # e.g. libamdhip64 not resolvable
        raise HsrUnavailable(f"cannot load {path}: {e}") from e
    for name, (res, args) in list(SIGNATURES.items()) + list(COLOR_SIGNATURES.items()) + list(COREG_SIGNATURES.items()) \
            + list(REPROJECT_SIGNATURES.items()) + list(SCL_SIGNATURES.items()) + list(S2STACK_SIGNATURES.items()) + list(HIST_SIGNATURES.items()) \
            + list(RESIZE_SIGNATURES.items()) + list(MERGE_SIGNATURES.items()) + list(ROI_SIGNATURES.items()):
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib, _lib_path = lib, path
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != HSR_OK:
        msg = load().hsr_last_error().decode("utf-8", "replace")
        raise HsrError(f"{what or 'libhsr'} failed (code {rc}): {msg}")


def require_gpu():
    """torch is the device-memory / stream plumbing; a real GPU is mandatory for compute."""
    import torch
    if not torch.cuda.is_available():
        raise HsrUnavailable("no ROCm device visible (torch.cuda.is_available() is False); "
                             "the s2_emit hot path runs only on the GPU - there is no CPU fallback.")
    load()
    return torch
