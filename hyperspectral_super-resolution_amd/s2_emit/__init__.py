"""s2_emit on MI355X: drop-in for the reference package ``s2_emit`` (same names, same signatures).

The hot path - SRF band integration, percentile stretch, per-band polynomial fit and apply - runs as
hand-written HIP kernels for gfx950 behind a C ABI (include/hsr.h, csrc/*.hip -> lib/libhsr_mi355x.so).
Importing the package needs neither the GPU nor the extension; calling a compute function without
them raises ``HsrUnavailable`` (no CPU fallback).
"""
from .srf import load_s2_srf_from_xlsx, S2_BANDS_13, DEFAULT_SRF_XLSX_URL
from .emit_io import load_emit_envi_rfl, load_emit_wavelengths_from_nc
from .synth import pseudo_s2_srf_integral, pseudo_s2_rgb
from .viz import show_side_by_side, load_s2_rgb_u8
from .resize import AreaResampleOutput, resample_area, resample_to_grid, resize_s2_rgb_to
from .color import (
    robust_norm, robust_norm_rgb, apply_shared_percentile_stretch,
    histogram_match_rgb, ot_match_rgb_sinkhorn_pot, histogram_match_planes
)
from .poly_regression import fit_ot_poly_rgb, apply_poly_rgb
from .affine import fit_ot_affine_rgb, apply_affine_rgb, fit_affine_rgb
from .fusion import SpectralFusion, fuse_pair, match_pair, calibrate_pseudo_to_real_linear
from .ridge import PolyRidge, predict_cube_logit, flatten_pixels, subsample_bands_evenly
from .pairs import TilePairOutput, TilePairValidation, fuse_tile_pair, fuse_tile_pairs
from .scenes import (Window, SceneOutput, scene_windows, select_tiles, find_valid_paired_tiles, extract_tile_pairs,
                     mosaic_tiles, fuse_scene)
from .clouds import (SCL_NAMES, CLOUD_CLASSES, ClearSceneOutput, scl_metrics, count_cloud_pixels, cloud_mask, coarse_clear_mask,
                     mask_cube, fuse_scene_clear)
from .s2stack import S2_STACK_BANDS, S2StackOutput, s2_crop_window, assemble_s2_stack
from .ortho import OrthoOutput, apply_glt, ortho_scene, glt_from_xy, quality_mask
from .merge import MergeGrid, MergeOutput, OrthoMergeOutput, merge_grid, merge_scenes, ortho_merge, is_adjacent, merge_emit
from .roi import SubsetOutput, rasterize_roi, scl_metrics_roi, count_cloud_pixels_roi, spatial_subset, clip_cube
from .coreg import (TiePoints, ShiftModel, CoregOutput, closest_band, tie_point_grid, match_windows, fit_shift_model, warp_scene,
                    coregister_scene)
from .reproject import (ReprojectOutput, utm_params, tm_forward, tm_inverse, utm_target_grid, reproject_coords, remap_scene,
                        reproject_scene)
from ._native import HsrUnavailable, HsrError

# SCL_NAMES, CLOUD_CLASSES and S2_STACK_BANDS, the reference's tables, are attributes of the package and stay out of __all__: every
# name in it is callable (tests/test_host_logic.py).
# The public surface: first the 13 names of the reference's __all__ (s2_emit/__init__.py:10-24, same order -
# tests/test_host_logic.py checks it), then what callers of the reference copy out of poly_regression.py and
# the notebooks, then this build's fused / pipelined entry points.
_REFERENCE_SURFACE = (
    "load_s2_srf_from_xlsx load_emit_envi_rfl load_emit_wavelengths_from_nc pseudo_s2_srf_integral "
    "pseudo_s2_rgb show_side_by_side resize_s2_rgb_to robust_norm robust_norm_rgb "
    "apply_shared_percentile_stretch histogram_match_rgb ot_match_rgb_sinkhorn_pot load_s2_rgb_u8"
).split()
_COPIED_BY_CALLERS = ["fit_ot_poly_rgb", "apply_poly_rgb", "fit_ot_affine_rgb", "apply_affine_rgb", "fit_affine_rgb"]
_FUSED = ["SpectralFusion", "fuse_pair", "match_pair", "calibrate_pseudo_to_real_linear",
          "PolyRidge", "predict_cube_logit", "flatten_pixels", "subsample_bands_evenly",
          "fuse_tile_pair", "fuse_tile_pairs", "TilePairOutput", "TilePairValidation",
          "histogram_match_planes",
          "merge_grid", "merge_scenes", "ortho_merge", "is_adjacent", "merge_emit", "MergeGrid", "MergeOutput", "OrthoMergeOutput",
          "rasterize_roi", "scl_metrics_roi", "count_cloud_pixels_roi", "spatial_subset", "clip_cube", "SubsetOutput",
          "resample_area", "resample_to_grid", "AreaResampleOutput",
          "assemble_s2_stack", "s2_crop_window", "S2StackOutput",
          "find_valid_paired_tiles", "extract_tile_pairs", "mosaic_tiles", "fuse_scene", "scene_windows", "select_tiles",
          "Window", "SceneOutput",
          "fuse_scene_clear", "cloud_mask", "coarse_clear_mask", "mask_cube", "scl_metrics", "count_cloud_pixels", "ClearSceneOutput",
          "coregister_scene", "match_windows", "fit_shift_model", "warp_scene", "tie_point_grid", "closest_band",
          "TiePoints", "ShiftModel", "CoregOutput",
          "reproject_scene", "remap_scene", "reproject_coords", "utm_target_grid", "utm_params", "tm_forward", "tm_inverse",
          "ReprojectOutput",
          "apply_glt", "ortho_scene", "glt_from_xy", "quality_mask", "OrthoOutput"]
__all__ = _REFERENCE_SURFACE + _COPIED_BY_CALLERS + _FUSED
