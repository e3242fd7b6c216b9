"""ctypes binding of the C-ABI in include/linuxfg_hip.h (liblinuxfg_hip.so).

This is the only way Python code (tests/, bench.py, __graft_entry__) reaches the HIP path.
There is no fallback: if the library is missing, does not export a declared symbol, or no GPU
is present, the failure is raised, never papered over.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# LFG_LIB: a diagnostic build of the same library (tools/build_variant.sh); never a different implementation.
LIB_PATH = os.environ.get("LFG_LIB") or os.path.join(_HERE, "liblinuxfg_hip.so")

FORMAT_RGBA8 = 0
FORMAT_MV_S8X2 = 1
FORMAT_MV_S16X2_Q2 = 2
STAGE_SCALE, STAGE_MOTION, STAGE_INTERPOLATE = 0, 1, 2
MOTION_PREFILTERED, MOTION_EXACT_ONLY = 0, 1
SEMANTICS_REFERENCE, SEMANTICS_INTENDED = 0, 1
ESTIMATOR_FULL_SEARCH, ESTIMATOR_PYRAMID = 0, 1
INTERPOLATOR_SHADER, INTERPOLATOR_COMPENSATED = 0, 1
GENERATION_INTERPOLATE, GENERATION_EXTRAPOLATE = 0, 1
SAMPLING_BILINEAR, SAMPLING_BICUBIC = 0, 1
DEFAULT_MATCH_SAD = 48
HOLE_REACH_MAX = 255
YUV_BT601, YUV_BT709 = 0, 1
YUV_LIMITED, YUV_FULL = 0, 1
CHROMA_REPLICATE, CHROMA_LEFT = 0, 1
_BPP = {FORMAT_RGBA8: 4, FORMAT_MV_S8X2: 2, FORMAT_MV_S16X2_Q2: 4}
COMM_ID_BYTES = 128
MAX_LANES = 4
MAX_SHARPEN = 64
FILTER_NEAREST, FILTER_BILINEAR, FILTER_CATMULL_ROM, FILTER_MITCHELL, FILTER_LANCZOS2, FILTER_LANCZOS3 = range(6)
LIGHT_GAMMA, LIGHT_LINEAR, LIGHT_SIGMOID = range(3)
RESAMPLE_MAX_TAPS = 64
ERR_INVALID, ERR_UNSUPPORTED = -1, -4


class LfgError(RuntimeError):
    pass


class Frame(ctypes.Structure):
    """struct lfg_frame."""
    _fields_ = [("data", ctypes.c_void_p), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("pitch", ctypes.c_uint32), ("format", ctypes.c_uint32), ("owned", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class Nv12(ctypes.Structure):
    """struct lfg_nv12."""
    _fields_ = [("y", ctypes.c_void_p), ("uv", ctypes.c_void_p), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("y_pitch", ctypes.c_uint32), ("uv_pitch", ctypes.c_uint32)]


class Mask(ctypes.Structure):
    """struct lfg_mask."""
    _fields_ = [("data", ctypes.c_void_p), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("pitch", ctypes.c_uint32)]


class PairStats(ctypes.Structure):
    """struct lfg_pair_stats."""
    _fields_ = [("pixels", ctypes.c_uint64), ("matched", ctypes.c_uint64), ("sad_sum", ctypes.c_uint64)]

    def as_tuple(self):
        return int(self.pixels), int(self.matched), int(self.sad_sum)


class FrameDiffStats(ctypes.Structure):
    """struct lfg_frame_diff_stats."""
    _fields_ = [("pixels", ctypes.c_uint64), ("sse", ctypes.c_uint64 * 4), ("hist", ctypes.c_uint64 * 256)]

    def as_tuple(self):
        return int(self.pixels), tuple(int(v) for v in self.sse), tuple(int(v) for v in self.hist)


class FrameDiffSummary(ctypes.Structure):
    """struct lfg_frame_diff_summary."""
    _fields_ = [("pixels", ctypes.c_uint64), ("differing", ctypes.c_uint64), ("over_1", ctypes.c_uint64),
                ("max_abs", ctypes.c_uint32), ("p50", ctypes.c_uint32), ("p99", ctypes.c_uint32),
                ("mse", ctypes.c_double), ("psnr_db", ctypes.c_double)]

    def as_dict(self):
        return {name: (float if name in ("mse", "psnr_db") else int)(getattr(self, name)) for name, _ in self._fields_}


class FrameHistogramStats(ctypes.Structure):
    """struct lfg_frame_histogram_stats."""
    _fields_ = [("pixels", ctypes.c_uint64), ("hist", (ctypes.c_uint64 * 256) * 4)]


class LevelsMap(ctypes.Structure):
    """struct lfg_levels_map."""
    _fields_ = [("pixels", ctypes.c_uint64), ("shift_sum", ctypes.c_uint64), ("active", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("forward", (ctypes.c_uint8 * 256) * 3), ("inverse", (ctypes.c_uint8 * 256) * 3)]


LEVELS_FORWARD, LEVELS_AT = 0, 1
LEVELS_MAX_SHIFT16 = 4080


class FrameSsimStats(ctypes.Structure):
    """struct lfg_frame_ssim_stats."""
    _fields_ = [("windows", ctypes.c_uint64), ("sum", ctypes.c_int64 * 4), ("hist", ctypes.c_uint64 * 65), ("worst", ctypes.c_uint64)]

    def as_tuple(self):
        return int(self.windows), tuple(int(v) for v in self.sum), tuple(int(v) for v in self.hist), int(self.worst)


class FrameSsimSummary(ctypes.Structure):
    """struct lfg_frame_ssim_summary."""
    _fields_ = [("windows", ctypes.c_uint64), ("identical", ctypes.c_uint64), ("below_half", ctypes.c_uint64),
                ("ssim", ctypes.c_double * 4), ("all", ctypes.c_double), ("db", ctypes.c_double), ("worst_value", ctypes.c_double),
                ("worst_x", ctypes.c_uint32), ("worst_y", ctypes.c_uint32)]

    def as_dict(self):
        return {"windows": int(self.windows), "identical": int(self.identical), "below_half": int(self.below_half),
                "ssim": tuple(float(v) for v in self.ssim), "all": float(self.all), "db": float(self.db),
                "worst_value": float(self.worst_value), "worst_x": int(self.worst_x), "worst_y": int(self.worst_y)}


# How frame_ssim.hip tiles a frame (its kSsimStripWindows, kSsimSegmentRows, kSsimWaves and kSsimGroupsPerCu, held equal by
# tests/test_ssim_model.py): a wave owns 63 windows of a block row, an item of its walk is 8 window rows of them, a workgroup is 4
# waves and the grid at most 4 workgroups per CU.  No result depends on them; the GPU tests name their seam sizes from them.
SSIM_STRIP_WINDOWS, SSIM_SEGMENT_ROWS, SSIM_GROUP_WAVES, SSIM_GROUPS_PER_CU = 63, 8, 4, 4

_vp, _i, _u32, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_size_t
_FP = ctypes.POINTER(Frame)

# name -> (restype, argtypes): every entry point include/linuxfg_hip.h declares.
SIGNATURES = {
    "lfg_abi_version": (_i, []),
    "lfg_device_count": (_i, []),
    "lfg_context_create": (_i, [_i, ctypes.POINTER(_vp)]),
    "lfg_context_destroy": (None, [_vp]),
    "lfg_context_set_stream": (_i, [_vp, _vp]),
    "lfg_context_get_stream": (_vp, [_vp]),
    "lfg_context_device": (_i, [_vp]),
    "lfg_sync": (_i, [_vp]),
    "lfg_lanes": (_i, [_vp, _i]),
    "lfg_lane_count": (_i, [_vp]),
    "lfg_lane_current": (_i, [_vp]),
    "lfg_lane_select": (_i, [_vp, _i]),
    "lfg_lane_mark": (_i, [_vp]),
    "lfg_lane_wait": (_i, [_vp, _i]),
    "lfg_lane_sync": (_i, [_vp]),
    "lfg_last_error": (ctypes.c_char_p, [_vp]),
    "lfg_frame_create": (_i, [_vp, _u32, _u32, _u32, _FP]),
    "lfg_frame_destroy": (None, [_vp, _FP]),
    "lfg_frame_wrap": (_i, [_vp, _u32, _u32, _u32, _u32, _FP]),
    "lfg_frame_copy": (_i, [_vp, _FP, _FP]),
    "lfg_staging_create": (_i, [_vp, _sz, ctypes.POINTER(_vp)]),
    "lfg_staging_destroy": (None, [_vp, _vp]),
    "lfg_frame_upload": (_i, [_vp, _FP, _vp, _sz]),
    "lfg_frame_download": (_i, [_vp, _FP, _vp, _sz]),
    "lfg_ring_create": (_i, [_vp, _u32, _sz, ctypes.POINTER(_vp)]),
    "lfg_ring_destroy": (None, [_vp]),
    "lfg_ring_acquire": (_i, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_u32)]),
    "lfg_ring_upload": (_i, [_vp, _u32, _FP]),
    "lfg_ring_download": (_i, [_vp, _u32, _FP]),
    "lfg_ring_wait": (_i, [_vp, _u32]),
    "lfg_ring_fence_slot": (_i, [_vp, _u32]),
    "lfg_scale": (_i, [_vp, _FP, _FP]),
    "lfg_motion": (_i, [_vp, _FP, _FP, _FP, _i, ctypes.c_float]),
    "lfg_set_motion_mode": (_i, [_vp, _i]),
    "lfg_motion_last_stats": (_i, [_vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(ctypes.c_double)]),
    "lfg_motion_open_segments": (_i, [_vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32)]),
    "lfg_motion_hand_over_stats": (_i, [_vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32)]),
    "lfg_motion_lean_stats": (_i, [_vp, ctypes.POINTER(_i), ctypes.POINTER(_u32), ctypes.POINTER(_u32)]),
    "lfg_motion_strip_stats": (_i, [_vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32)]),
    "lfg_motion_prediction_stats": (_i, [_vp] + [ctypes.POINTER(ctypes.c_uint64)] * 4),
    "lfg_motion_workspace_size": (_i, [_vp, _u32, _u32, ctypes.POINTER(ctypes.c_uint64)]),
    "lfg_motion_plan": (_i, [_vp, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "lfg_motion_pyramid": (_i, [_vp, _FP, _FP, _FP, _i, _i, _i]),
    "lfg_set_motion_estimator": (_i, [_vp, _i]),
    "lfg_set_semantics": (_i, [_vp, _i]),
    "lfg_interpolate": (_i, [_vp, _FP, _FP, _FP, _FP, ctypes.c_float]),
    "lfg_interpolate_frames": (_i, [_vp, _FP, _FP, _FP, ctypes.c_float]),
    "lfg_interpolate_multi": (_i, [_vp, _FP, _FP, _FP, ctypes.POINTER(_FP), ctypes.POINTER(ctypes.c_float), _u32]),
    "lfg_interpolate_frames_multi": (_i, [_vp, _FP, _FP, ctypes.POINTER(_FP), ctypes.POINTER(ctypes.c_float), _u32]),
    "lfg_interpolate_scale": (_i, [_vp, _FP, _FP, _FP, _FP, ctypes.c_float]),
    "lfg_interpolate_compensated": (_i, [_vp, _FP, _FP, _FP, _FP, ctypes.c_float, _i]),
    "lfg_interpolate_compensated_multi": (_i, [_vp, _FP, _FP, _FP, ctypes.POINTER(_FP), ctypes.POINTER(ctypes.c_float), _u32, _i]),
    "lfg_set_interpolator": (_i, [_vp, _i, _i]),
    "lfg_static_mask": (_i, [_vp, _FP, _FP, _i, ctypes.POINTER(Mask)]),
    "lfg_interpolate_compensated_masked": (_i, [_vp, _FP, _FP, _FP, ctypes.POINTER(Mask), _FP, ctypes.c_float, _i]),
    "lfg_interpolate_compensated_masked_multi": (_i, [_vp, _FP, _FP, _FP, ctypes.POINTER(Mask), ctypes.POINTER(_FP),
                                                      ctypes.POINTER(ctypes.c_float), _u32, _i]),
    "lfg_set_static_protection": (_i, [_vp, _i]),
    "lfg_extrapolate_compensated": (_i, [_vp, _FP, _FP, _FP, _FP, ctypes.c_float, _i]),
    "lfg_extrapolate_compensated_multi": (_i, [_vp, _FP, _FP, _FP, ctypes.POINTER(_FP), ctypes.POINTER(ctypes.c_float), _u32, _i]),
    "lfg_set_generation": (_i, [_vp, _i]),
    "lfg_motion_consistency": (_i, [_vp, _FP, _FP, _i, ctypes.POINTER(Mask)]),
    "lfg_interpolate_compensated_bidirectional": (_i, [_vp, _FP, _FP, _FP, _FP, _FP, ctypes.c_float, _i, _i]),
    "lfg_interpolate_compensated_bidirectional_multi": (_i, [_vp, _FP, _FP, _FP, _FP, ctypes.POINTER(_FP),
                                                             ctypes.POINTER(ctypes.c_float), _u32, _i, _i]),
    "lfg_set_bidirectional": (_i, [_vp, _i]),
    "lfg_hole_fill_plane": (_i, [_vp, _FP, _i, _i, _FP]),
    "lfg_set_hole_reach": (_i, [_vp, _i]),
    "lfg_motion_refine": (_i, [_vp, _FP, _FP, _FP, _FP, _i]),
    "lfg_set_vector_refinement": (_i, [_vp, _i]),
    "lfg_frame_halve": (_i, [_vp, _FP, _FP]),
    "lfg_motion_expand": (_i, [_vp, _FP, _FP, _FP, _FP, _i]),
    "lfg_set_half_resolution_motion": (_i, [_vp, _i]),
    "lfg_motion_subpel": (_i, [_vp, _FP, _FP, _FP, _FP, _i]),
    "lfg_interpolate_compensated_subpel": (_i, [_vp, _FP, _FP, _FP, _FP, ctypes.c_float, _i]),
    "lfg_interpolate_compensated_subpel_multi": (_i, [_vp, _FP, _FP, _FP, ctypes.POINTER(_FP), ctypes.POINTER(ctypes.c_float), _u32, _i]),
    "lfg_set_subpixel_vectors": (_i, [_vp, _i]),
    "lfg_sampling_weights": (_i, [ctypes.POINTER(ctypes.c_int16)]),
    "lfg_interpolate_compensated_sampled": (_i, [_vp, _FP, _FP, _FP, _FP, ctypes.c_float, _i, _i]),
    "lfg_interpolate_compensated_sampled_multi": (_i, [_vp, _FP, _FP, _FP, ctypes.POINTER(_FP), ctypes.POINTER(ctypes.c_float), _u32, _i, _i]),
    "lfg_set_sampling": (_i, [_vp, _i]),
    "lfg_sampling_effective": (_i, [_vp]),
    "lfg_pair_match": (_i, [_vp, _FP, _FP, _FP, _i, _vp]),
    "lfg_cut_fallback": (_i, [_vp, _FP, _FP, _vp, _i, ctypes.POINTER(_FP), ctypes.POINTER(ctypes.c_float), _u32]),
    "lfg_set_cut_detection": (_i, [_vp, _i]),
    "lfg_last_pair_stats": (_i, [_vp, ctypes.POINTER(PairStats), ctypes.POINTER(_i)]),
    "lfg_frame_diff": (_i, [_vp, _FP, _FP, _u32, _i, _vp]),
    "lfg_frame_diff_summarize": (_i, [ctypes.POINTER(FrameDiffStats), _u32, ctypes.POINTER(FrameDiffSummary)]),
    "lfg_frame_histogram": (_i, [_vp, _FP, _i, _vp]),
    "lfg_levels_match": (_i, [_vp, _vp, _vp, _i, _vp]),
    "lfg_levels_apply": (_i, [_vp, _FP, _FP, _vp, _i, ctypes.c_float]),
    "lfg_set_level_matching": (_i, [_vp, _i]),
    "lfg_last_level_match": (_i, [_vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(_i)]),
    "lfg_frame_ssim": (_i, [_vp, _FP, _FP, _u32, _i, _vp]),
    "lfg_frame_ssim_summarize": (_i, [ctypes.POINTER(FrameSsimStats), _u32, ctypes.POINTER(FrameSsimSummary)]),
    "lfg_nv12_to_rgba": (_i, [_vp, ctypes.POINTER(Nv12), _FP, _i, _i, _i]),
    "lfg_rgba_to_nv12": (_i, [_vp, _FP, ctypes.POINTER(Nv12), _i, _i, _i]),
    "lfg_sharpen": (_i, [_vp, _FP, _FP, _i]),
    "lfg_deband": (_i, [_vp, _FP, _FP, _i, _i, _i, _i, _u32]),
    "lfg_deband_draw": (_i, [_u32, _u32, _u32, _i, _i, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "lfg_denoise_temporal": (_i, [_vp, _FP, ctypes.POINTER(_FP), ctypes.POINTER(_FP), _i, _FP, _i, _i, _i, _i]),
    "lfg_resample": (_i, [_vp, _FP, _FP, _i]),
    "lfg_resample_taps": (_i, [_i, _u32, _u32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int16)]),
    "lfg_resample_antiring": (_i, [_vp, _FP, _FP, _i, _i]),
    "lfg_resample_brackets": (_i, [_u32, _u32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "lfg_resample_light": (_i, [_vp, _FP, _FP, _i, _i]),
    "lfg_light_tables": (_i, [_i, ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint16)]),
    "lfg_upscale_edge": (_i, [_vp, _FP, _FP]),
    "lfg_upscale_edge_positions": (_i, [_u32, _u32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8)]),
    "lfg_upscale_edge_shapes": (_i, [ctypes.POINTER(ctypes.c_int16)]),
    "lfg_yuv_coefficients": (_i, [_i, _i, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "lfg_set_fused_interpolate_scale": (_i, [_vp, _i]),
    "lfg_set_fused_motion_interpolate": (_i, [_vp, _i]),
    "lfg_mv_export_rgba32f": (_i, [_vp, _FP, _vp]),
    "lfg_selftest_sqrt": (_i, [_vp, _u32, _u32, ctypes.POINTER(ctypes.c_uint64)]),
    "lfg_comm_unique_id": (_i, [_vp]),
    "lfg_comm_init": (_i, [_vp, _i, _i, _vp]),
    "lfg_comm_rank": (_i, [_vp]),
    "lfg_comm_ranks": (_i, [_vp]),
    "lfg_broadcast_frame": (_i, [_vp, _FP, _i]),
    "lfg_comm_wait": (_i, [_vp]),
    "lfg_comm_destroy": (_i, [_vp]),
    "lfg_comm_sync": (_i, [_vp]),
    "lfg_comm_reserved_cus": (_i, [_vp]),
    "lfg_comm_cu_mask": (_i, [_vp, ctypes.POINTER(_u32), _i]),
    "lfg_comm_probe": (_i, [_vp, _i, _i, _i]),
    "lfg_broadcast_frame_lane": (_i, [_vp, _FP, _i]),
    "lfg_comm_probe_ms": (_i, [_vp, ctypes.POINTER(ctypes.c_float)]),
    "lfg_motion_last_variant": (_i, [_vp]),
    "lfg_scale_last_kernel": (_i, [_vp]),
    "lfg_diag_scale_2x_strip": (_i, [_u32, _u32, _u32, ctypes.POINTER(_u32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "lfg_profile_enable": (_i, [_vp, _i]),
    "lfg_profile_reset": (_i, [_vp]),
    "lfg_profile_get": (_i, [_vp, _i, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]),
}

_lib = None


def summarize(record, channel_mask: int = 0xF) -> dict:
    """A record (pixels, sse, hist) -- read_diff_record's tuple -- as lfg_frame_diff_summarize's figures: a dict of pixels,
    differing, over_1, max_abs, p50, p99, mse and psnr_db (inf on identical frames).  Needs no context and no GPU."""
    pixels, sse, hist = record
    s, out = FrameDiffStats(int(pixels), (ctypes.c_uint64 * 4)(*sse), (ctypes.c_uint64 * 256)(*hist)), FrameDiffSummary()
    rc = load().lfg_frame_diff_summarize(ctypes.byref(s), int(channel_mask), ctypes.byref(out))
    if rc != 0:
        raise LfgError(f"lfg_frame_diff_summarize failed ({rc}): bad mask, no pixels, or a histogram that does not sum to them")
    return out.as_dict()


def summarize_ssim(record, channel_mask: int = 0xF) -> dict:
    """A record (windows, sum, hist, worst) -- read_ssim_record's tuple -- as lfg_frame_ssim_summarize's figures: a dict of
    windows, identical, below_half, ssim (4), all, db (inf on identical frames), worst_value, worst_x and worst_y.  Needs no
    context and no GPU."""
    windows, total, hist, worst = record
    s, out = FrameSsimStats(int(windows), (ctypes.c_int64 * 4)(*total), (ctypes.c_uint64 * 65)(*hist), int(worst)), FrameSsimSummary()
    rc = load().lfg_frame_ssim_summarize(ctypes.byref(s), int(channel_mask), ctypes.byref(out))
    if rc != 0:
        raise LfgError(f"lfg_frame_ssim_summarize failed ({rc}): bad mask, no windows, or a histogram that does not sum to them")
    return out.as_dict()


def yuv_coefficients(matrix: int, yuv_range: int):
    """(to_rgb, to_yuv) of lfg_yuv_coefficients: the 5 + 9 integers, scaled by 2^14, that the conversion kernels use.  Needs no
    context and no GPU."""
    to_rgb, to_yuv = (ctypes.c_int32 * 5)(), (ctypes.c_int32 * 9)()
    rc = load().lfg_yuv_coefficients(int(matrix), int(yuv_range), to_rgb, to_yuv)
    if rc != 0:
        raise LfgError(f"lfg_yuv_coefficients failed ({rc}): unknown matrix or range")
    return tuple(int(v) for v in to_rgb), tuple(int(v) for v in to_yuv)


def resample_taps(filt: int, n_in: int, n_out: int):
    """(first[n_out] int32, count[n_out] uint32, weights[n_out, RESAMPLE_MAX_TAPS] int16) of lfg_resample_taps: the table of one
    axis that lfg_resample uploads.  Needs no context and no GPU.  Raises LfgError, with the code as `.code`, where the call refuses."""
    n_in, n_out = int(n_in), int(n_out)
    rows = n_out if 0 < n_out < 2 ** 32 else 0
    first, count = np.zeros(rows, np.int32), np.zeros(rows, np.uint32)
    weights = np.zeros((rows, RESAMPLE_MAX_TAPS), np.int16)
    rc = load().lfg_resample_taps(int(filt), n_in if 0 < n_in < 2 ** 32 else 0, rows,
                                  first.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), count.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                  weights.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)))
    if rc != 0:
        err = LfgError(f"lfg_resample_taps failed ({rc}): " + ("more than RESAMPLE_MAX_TAPS taps per sample" if rc == ERR_UNSUPPORTED
                                                                 else "a size of 0 or an unknown filter"))
        err.code = rc
        raise err
    return first, count, weights


def resample_brackets(n_in: int, n_out: int):
    """(lo[n_out] int32, hi[n_out] int32) of lfg_resample_brackets: the two source samples that bracket each output sample of
    one axis, which lfg_resample_antiring uploads.  Needs no context and no GPU.  Raises LfgError, with the code as `.code`."""
    n_in, n_out = int(n_in), int(n_out)
    rows = n_out if 0 < n_out < 2 ** 32 else 0
    lo, hi = np.zeros(rows, np.int32), np.zeros(rows, np.int32)
    rc = load().lfg_resample_brackets(n_in if 0 < n_in < 2 ** 32 else 0, rows, lo.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                      hi.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    if rc != 0:
        err = LfgError(f"lfg_resample_brackets failed ({rc}): a size of 0, or an input of 2^31 samples or more")
        err.code = rc
        raise err
    return lo, hi


def light_tables(light: int):
    """(forward[256] uint16, threshold[255] uint16) of lfg_light_tables: a colour byte's 14 bits of light under LIGHT_LINEAR or
    LIGHT_SIGMOID, and the midpoints that take 14 bits back to a byte, which lfg_resample_light uploads.  Needs no context and no
    GPU.  Raises LfgError, with the code as `.code`."""
    forward, threshold = np.zeros(256, np.uint16), np.zeros(255, np.uint16)
    rc = load().lfg_light_tables(int(light), forward.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)),
                                 threshold.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)))
    if rc != 0:
        err = LfgError(f"lfg_light_tables failed ({rc}): LIGHT_GAMMA has no tables, and no other light is known")
        err.code = rc
        raise err
    return forward, threshold


def upscale_edge_positions(n_in: int, n_out: int):
    """(base[n_out] int32, frac[n_out] uint8) of lfg_upscale_edge_positions: the texel left of (above) each output sample of one
    axis and the sample's distance from it in 256ths, which lfg_upscale_edge uploads.  Needs no context and no GPU.  Raises
    LfgError, with the code as `.code`."""
    n_in, n_out = int(n_in), int(n_out)
    rows = n_out if 0 < n_out < 2 ** 31 else 0
    base, frac = np.zeros(rows, np.int32), np.zeros(rows, np.uint8)
    rc = load().lfg_upscale_edge_positions(n_in if 0 < n_in < 2 ** 32 else 0, rows, base.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                           frac.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    if rc != 0:
        err = LfgError(f"lfg_upscale_edge_positions failed ({rc}): a size of 0, or of 2^31 samples or more")
        err.code = rc
        raise err
    return base, frac


def upscale_edge_shapes() -> np.ndarray:
    """(16, 33, 5) int16 of lfg_upscale_edge_shapes: (A, B, C, lob, clp) per direction and edge strength.  Needs no context and
    no GPU."""
    t = np.zeros((16, 33, 5), np.int16)
    rc = load().lfg_upscale_edge_shapes(t.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)))
    if rc != 0:
        raise LfgError(f"lfg_upscale_edge_shapes failed ({rc})")
    return t


def deband_draw(seed: int, x: int, y: int, iterations: int, radius: int):
    """(offsets[8] int32, noise_bytes[3] int32) of lfg_deband_draw: ox, oy of each of lfg_deband's iterations at pixel (x, y)
    (zeros past `iterations`) and the three noise bytes.  Needs no context and no GPU.  Raises LfgError where the call refuses."""
    offsets, noise = (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 3)()
    rc = load().lfg_deband_draw(int(seed) & 0xFFFFFFFF, int(x) & 0xFFFFFFFF, int(y) & 0xFFFFFFFF, int(iterations), int(radius), offsets, noise)
    if rc != 0:
        raise LfgError(f"lfg_deband_draw failed ({rc}): iterations outside 1 .. 4 or radius outside 1 .. 32")
    return np.array(offsets, np.int32), np.array(noise, np.int32)


def sampling_weights() -> np.ndarray:
    """(64, 4) int16 of lfg_sampling_weights: the bicubic fetch's weights per phase.  Needs no context and no GPU."""
    w = np.zeros((64, 4), np.int16)
    rc = load().lfg_sampling_weights(w.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)))
    if rc != 0:
        raise LfgError(f"lfg_sampling_weights failed ({rc})")
    return w


def load() -> ctypes.CDLL:
    """Load liblinuxfg_hip.so and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LfgError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)")
        # HIP gives a process four hardware queues unless told otherwise, and streams beyond that share them: three lanes, a
        # communication stream and a framework's own stream are five -- two lanes on one queue run in turn (measured on the MI355X:
        # 3,684 -> 2,750 frames/s for every context of a process but its first; NOTES_r05.md section 7).  Read by the HIP runtime at
        # its first call, so this has effect only if nothing in the process has touched the GPU yet; an explicit setting wins.
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


class Ring:
    """lfg_ring (Context.ring_create): transfers between pinned slots and frames, ordered against the lane selected at the call."""

    def __init__(self, ctx: "Context", handle, slot_bytes: int):
        self.ctx, self.h, self.slot_bytes = ctx, handle, slot_bytes

    def acquire(self):
        """(the slot's bytes as a uint8 array (no copy), its index); blocks while the slot's last transfer runs."""
        p, slot = _vp(), _u32()
        self.ctx._check(self.ctx.lib.lfg_ring_acquire(self.h, ctypes.byref(p), ctypes.byref(slot)), "lfg_ring_acquire")
        return np.ctypeslib.as_array((ctypes.c_uint8 * self.slot_bytes).from_address(p.value)), int(slot.value)

    def upload(self, slot: int, dst: Frame):
        self.ctx._check(self.ctx.lib.lfg_ring_upload(self.h, int(slot), ctypes.byref(dst)), "lfg_ring_upload")

    def download(self, slot: int, src: Frame):
        self.ctx._check(self.ctx.lib.lfg_ring_download(self.h, int(slot), ctypes.byref(src)), "lfg_ring_download")

    def wait(self, slot: int):
        self.ctx._check(self.ctx.lib.lfg_ring_wait(self.h, int(slot)), "lfg_ring_wait")

    def fence_slot(self, slot: int):
        self.ctx._check(self.ctx.lib.lfg_ring_fence_slot(self.h, int(slot)), "lfg_ring_fence_slot")

    def destroy(self):
        if self.h:
            self.ctx.lib.lfg_ring_destroy(self.h)
            self.h = None


class Context:
    """One GPU, one stream (lfg_context).  Mirrors the reference's VulkanContext + FrameManager calls."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self.lib = load()
        h = _vp()
        rc = self.lib.lfg_context_create(device, ctypes.byref(h))
        if rc != 0:
            raise LfgError(f"lfg_context_create failed ({rc}): {self.lib.lfg_last_error(None).decode()}")
        self.h = h
        self._frames: list[Frame] = []
        if stream is not None:
            self.set_stream(stream)

    # -- plumbing
    def _check(self, rc: int, what: str):
        if rc != 0:
            raise LfgError(f"{what} failed ({rc}): {self.lib.lfg_last_error(self.h).decode()}")

    def close(self):
        if getattr(self, "h", None):
            for f in self._frames:
                self.lib.lfg_frame_destroy(self.h, ctypes.byref(f))
            self._frames.clear()
            self.lib.lfg_context_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream: int | None):
        self._check(self.lib.lfg_context_set_stream(self.h, _vp(stream or 0)), "lfg_context_set_stream")

    def get_stream(self) -> int:
        """The hipStream_t the selected lane's calls run on, as an integer: its own, or the one it has adopted."""
        return int(self.lib.lfg_context_get_stream(self.h) or 0)

    def sync(self):
        self._check(self.lib.lfg_sync(self.h), "lfg_sync")

    # lanes: several frames in flight on one GPU (include/linuxfg_hip.h)
    def lanes(self, count: int):
        self._check(self.lib.lfg_lanes(self.h, int(count)), "lfg_lanes")

    def lane_count(self) -> int:
        return int(self.lib.lfg_lane_count(self.h))

    def lane_current(self) -> int:
        return int(self.lib.lfg_lane_current(self.h))

    def lane_select(self, lane: int):
        self._check(self.lib.lfg_lane_select(self.h, int(lane)), "lfg_lane_select")

    def lane_mark(self):
        self._check(self.lib.lfg_lane_mark(self.h), "lfg_lane_mark")

    def lane_sync(self):
        """The host waits for the selected lane alone."""
        self._check(self.lib.lfg_lane_sync(self.h), "lfg_lane_sync")

    def lane_wait(self, other: int):
        self._check(self.lib.lfg_lane_wait(self.h, int(other)), "lfg_lane_wait")

    # -- frames
    def create_frame(self, width: int, height: int, fmt: int = FORMAT_RGBA8) -> Frame:
        f = Frame()
        self._check(self.lib.lfg_frame_create(self.h, width, height, fmt, ctypes.byref(f)), "lfg_frame_create")
        self._frames.append(f)
        return f

    def destroy_frame(self, f: Frame):
        self.lib.lfg_frame_destroy(self.h, ctypes.byref(f))
        self._frames = [g for g in self._frames if g is not f]

    @staticmethod
    def wrap(device_ptr: int, width: int, height: int, fmt: int = FORMAT_RGBA8, pitch: int | None = None) -> Frame:
        f = Frame()
        rc = load().lfg_frame_wrap(_vp(device_ptr), width, height, pitch or width * _BPP[fmt], fmt, ctypes.byref(f))
        if rc != 0:
            raise LfgError(f"lfg_frame_wrap failed ({rc})")
        return f

    def upload(self, f: Frame, host: np.ndarray):
        a = np.ascontiguousarray(host)
        self._check(self.lib.lfg_frame_upload(self.h, ctypes.byref(f), a.ctypes.data_as(_vp), a.nbytes), "lfg_frame_upload")
        self.sync()                      # `a` is pageable and may be a temporary

    def download(self, f: Frame) -> np.ndarray:
        if f.format == FORMAT_RGBA8:
            out = np.empty((f.height, f.width, 4), np.uint8)
        elif f.format == FORMAT_MV_S16X2_Q2:
            out = np.empty((f.height, f.width, 2), np.int16)
        else:
            out = np.empty((f.height, f.width, 2), np.int8)
        self._check(self.lib.lfg_frame_download(self.h, ctypes.byref(f), out.ctypes.data_as(_vp), out.nbytes), "lfg_frame_download")
        self.sync()
        return out

    def frame_from(self, host: np.ndarray, fmt: int = FORMAT_RGBA8) -> Frame:
        """A new frame holding `host`: (H, W, 4) uint8, (H, W, 2) int8 for FORMAT_MV_S8X2 or (H, W, 2) int16 for
        FORMAT_MV_S16X2_Q2."""
        if fmt == FORMAT_MV_S16X2_Q2 and (host.dtype != np.int16 or host.shape[2:] != (2,)):
            raise LfgError(f"frame_from: FORMAT_MV_S16X2_Q2 takes (H, W, 2) int16, not {host.shape} {host.dtype}")
        f = self.create_frame(host.shape[1], host.shape[0], fmt)
        self.upload(f, host)
        return f

    def copy(self, src: Frame, dst: Frame):
        self._check(self.lib.lfg_frame_copy(self.h, ctypes.byref(src), ctypes.byref(dst)), "lfg_frame_copy")

    # -- staging (pinned host memory)
    def staging_create(self, nbytes: int) -> np.ndarray:
        """lfg_staging_create: ``nbytes`` of pinned host memory as a uint8 array (no copy); release it with
        staging_destroy(array)."""
        p = _vp()
        self._check(self.lib.lfg_staging_create(self.h, nbytes, ctypes.byref(p)), "lfg_staging_create")
        a = np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(p.value))
        self._staging = getattr(self, "_staging", {})
        self._staging[a.ctypes.data] = p.value
        return a

    def staging_destroy(self, a: np.ndarray):
        self.lib.lfg_staging_destroy(self.h, _vp(self._staging.pop(a.ctypes.data)))

    def upload_async(self, f: Frame, host: np.ndarray):
        """lfg_frame_upload without the wait: ``host`` must be pinned and stay alive until sync()."""
        self._check(self.lib.lfg_frame_upload(self.h, ctypes.byref(f), host.ctypes.data_as(_vp), host.nbytes), "lfg_frame_upload")

    def download_async(self, f: Frame, host: np.ndarray):
        self._check(self.lib.lfg_frame_download(self.h, ctypes.byref(f), host.ctypes.data_as(_vp), host.nbytes), "lfg_frame_download")

    def ring_create(self, slots: int, slot_bytes: int) -> "Ring":
        """lfg_ring_create: a ring of pinned slots with a copy stream of its own.  Destroy it before the context."""
        r = _vp()
        self._check(self.lib.lfg_ring_create(self.h, int(slots), int(slot_bytes), ctypes.byref(r)), "lfg_ring_create")
        return Ring(self, r, int(slot_bytes))

    def mv_export_rgba32f(self, mv: Frame) -> np.ndarray:
        """The reference's rgba32f motion-vector image, vec4(mv.x, mv.y, 0, 1) per pixel, as (H, W, 4) float32."""
        tmp = self.create_frame(mv.width * 4, mv.height)          # W*H*16 bytes of device memory
        self._check(self.lib.lfg_mv_export_rgba32f(self.h, ctypes.byref(mv), _vp(tmp.data)), "lfg_mv_export_rgba32f")
        raw = self.download(tmp)
        self.destroy_frame(tmp)
        return raw.reshape(mv.height, mv.width * 16).view(np.float32).reshape(mv.height, mv.width, 4)

    # -- stages (enqueue only)
    def scale(self, src: Frame, dst: Frame):
        self._check(self.lib.lfg_scale(self.h, ctypes.byref(src), ctypes.byref(dst)), "lfg_scale")

    def motion(self, prev: Frame, curr: Frame, mv: Frame, block_size: int = 8, search_radius: float = 16.0):
        self._check(self.lib.lfg_motion(self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(mv),
                                        block_size, search_radius), "lfg_motion")

    def set_motion_mode(self, mode: int):
        """0 = prefiltered (default), 1 = exact kernel only; results are identical."""
        self._check(self.lib.lfg_set_motion_mode(self.h, mode), "lfg_set_motion_mode")

    def motion_pyramid(self, prev: Frame, curr: Frame, mv: Frame, levels: int = 2, coarse_radius: int = 16, refine_radius: int = 2):
        """Coarse-to-fine block matcher (lfg_motion_pyramid): the same vector format as motion(), a range of
        coarse_radius * 2^levels + refine_radius * (2^levels - 1) pixels at a cost independent of the content."""
        self._check(self.lib.lfg_motion_pyramid(self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(mv),
                                                int(levels), int(coarse_radius), int(refine_radius)), "lfg_motion_pyramid")

    def set_motion_estimator(self, estimator: int):
        """ESTIMATOR_FULL_SEARCH (default) or ESTIMATOR_PYRAMID for interpolate_frames[_multi]."""
        self._check(self.lib.lfg_set_motion_estimator(self.h, int(estimator)), "lfg_set_motion_estimator")

    def set_semantics(self, semantics: int):
        """0 = the shaders as written (parity contract), 1 = opt-in "intended" tie-break and motion-vector units."""
        self._check(self.lib.lfg_set_semantics(self.h, semantics), "lfg_set_semantics")

    def motion_last_stats(self):
        """(tiles, tiles that fell back to the exact kernel, mean candidates recorded per pixel elsewhere)."""
        t, f, m = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_double()
        self._check(self.lib.lfg_motion_last_stats(self.h, ctypes.byref(t), ctypes.byref(f), ctypes.byref(m)), "lfg_motion_last_stats")
        return t.value, f.value, m.value

    def motion_open_segments(self):
        """(segments the prefilter left to the resolve kernel, segments of the frame) of the last prefiltered lfg_motion."""
        a, b = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self.lib.lfg_motion_open_segments(self.h, ctypes.byref(a), ctypes.byref(b)), "lfg_motion_open_segments")
        return a.value, b.value

    def motion_hand_over_stats(self):
        """(entries of the run-time queue the last prefiltered lfg_motion asked for, entries the queue is laid out for)."""
        a, b = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self.lib.lfg_motion_hand_over_stats(self.h, ctypes.byref(a), ctypes.byref(b)), "lfg_motion_hand_over_stats")
        return a.value, b.value

    def motion_lean_stats(self):
        """(the selected lane's last lfg_motion went through the lean kernel, tiles listed for it, tiles in which it left work)."""
        u, t, l = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self.lib.lfg_motion_lean_stats(self.h, ctypes.byref(u), ctypes.byref(t), ctypes.byref(l)), "lfg_motion_lean_stats")
        return bool(u.value), t.value, l.value

    def motion_strip_stats(self):
        """(pixel rows whose left or right band, pixel columns whose top or bottom band the strip kernel decided in the last lfg_motion)."""
        a, b = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self.lib.lfg_motion_strip_stats(self.h, ctypes.byref(a), ctypes.byref(b)), "lfg_motion_strip_stats")
        return a.value, b.value

    def motion_prediction_stats(self):
        """(calls whose verdict came back, of which launched on a wrong guess about: the lean kernel, the persistent grid, the
        second pass) since the context was created, all lanes together (lfg_motion_prediction_stats)."""
        v = [ctypes.c_uint64() for _ in range(4)]
        self._check(self.lib.lfg_motion_prediction_stats(self.h, *[ctypes.byref(x) for x in v]), "lfg_motion_prediction_stats")
        return tuple(int(x.value) for x in v)

    def motion_workspace_size(self, width: int, height: int) -> int:
        """Bytes the prefiltered motion path keeps for frames of this size (per lane)."""
        n = ctypes.c_uint64()
        self._check(self.lib.lfg_motion_workspace_size(self.h, width, height, ctypes.byref(n)), "lfg_motion_workspace_size")
        return n.value

    def scale_last_kernel(self) -> int:
        """Which kernel the context's last scale or interpolate_scale launched: 0 generic, 1 exact 2x, 2 fused interpolate -> 2x; -1 none yet."""
        return int(self.lib.lfg_scale_last_kernel(self.h))

    def motion_last_variant(self) -> int:
        """Which variant of the persistent kernel the context's last lfg_motion launched: 0 the default, 1 the one for moderate sensor noise."""
        return int(self.lib.lfg_motion_last_variant(self.h))

    def motion_plan(self):
        """(rim split, persistent workgroups) of the prefiltered motion path on this context (lfg_motion_plan)."""
        a, b = ctypes.c_int(), ctypes.c_int()
        self._check(self.lib.lfg_motion_plan(self.h, ctypes.byref(a), ctypes.byref(b)), "lfg_motion_plan")
        return a.value, b.value

    def interpolate(self, prev: Frame, curr: Frame, mv: Frame, out: Frame, factor: float = 0.5):
        self._check(self.lib.lfg_interpolate(self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(mv),
                                             ctypes.byref(out), factor), "lfg_interpolate")

    def interpolate_frames(self, prev: Frame, curr: Frame, out: Frame, factor: float = 0.5):
        self._check(self.lib.lfg_interpolate_frames(self.h, ctypes.byref(prev), ctypes.byref(curr),
                                                    ctypes.byref(out), factor), "lfg_interpolate_frames")

    @staticmethod
    def _multi_args(outs, factors):
        n = len(outs)
        if n != len(factors):
            raise ValueError("one output frame per factor")
        return (_FP * n)(*[ctypes.pointer(o) for o in outs]), (ctypes.c_float * n)(*factors), n

    def interpolate_multi(self, prev: Frame, curr: Frame, mv: Frame, outs, factors):
        """One pass over prev / curr / mv, one generated frame per factor (lfg_interpolate_multi)."""
        po, pf, n = self._multi_args(outs, factors)
        self._check(self.lib.lfg_interpolate_multi(self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(mv), po, pf, n),
                    "lfg_interpolate_multi")

    def interpolate_frames_multi(self, prev: Frame, curr: Frame, outs, factors):
        po, pf, n = self._multi_args(outs, factors)
        self._check(self.lib.lfg_interpolate_frames_multi(self.h, ctypes.byref(prev), ctypes.byref(curr), po, pf, n),
                    "lfg_interpolate_frames_multi")

    def interpolate_compensated(self, prev: Frame, curr: Frame, mv: Frame, out: Frame, factor: float = 0.5,
                                match_sad: int = DEFAULT_MATCH_SAD):
        """Motion-compensated interpolation (lfg_interpolate_compensated): the vectors projected to time `factor`, both
        frames fetched along them, holes filled from the background-most neighbour."""
        self._check(self.lib.lfg_interpolate_compensated(self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(mv),
                                                         ctypes.byref(out), factor, int(match_sad)), "lfg_interpolate_compensated")

    def interpolate_compensated_multi(self, prev: Frame, curr: Frame, mv: Frame, outs, factors, match_sad: int = DEFAULT_MATCH_SAD):
        """lfg_interpolate_compensated_multi: one generated frame per factor, each equal to the single call."""
        po, pf, n = self._multi_args(outs, factors)
        self._check(self.lib.lfg_interpolate_compensated_multi(self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(mv),
                                                               po, pf, n, int(match_sad)), "lfg_interpolate_compensated_multi")

    def set_interpolator(self, interpolator: int, match_sad: int = DEFAULT_MATCH_SAD):
        """INTERPOLATOR_SHADER (default) or INTERPOLATOR_COMPENSATED for interpolate_frames[_multi]."""
        self._check(self.lib.lfg_set_interpolator(self.h, int(interpolator), int(match_sad)), "lfg_set_interpolator")

    # -- static-overlay protection.  A mask is caller-owned device memory: create_mask keeps it in an RGBA8 frame of
    # _MASK_ROW bytes per row, so upload() and download() move it (mask_from / download_mask).
    _MASK_ROW = 4096

    def create_mask(self, width: int, height: int, pitch: int | None = None, offset: int = 0, fill: int = 0):
        """(the frame that owns the memory, the lfg_mask that describes it): rows `pitch` (default: width) bytes apart, the first
        `offset` bytes into the allocation; every byte of the allocation set to `fill`."""
        pitch = width if pitch is None else int(pitch)
        rows = -(-(offset + pitch * height) // self._MASK_ROW)
        f = self.frame_from(np.full((rows, self._MASK_ROW // 4, 4), fill, np.uint8))
        return f, Mask(f.data + offset, width, height, pitch)

    def mask_from(self, host: np.ndarray, pitch: int | None = None, offset: int = 0, fill: int = 0):
        """create_mask holding `host` (H, W) uint8; the row padding and the bytes in front of the mask hold `fill`."""
        h, w = host.shape
        f, m = self.create_mask(w, h, pitch, offset, fill)
        raw = np.full(f.height * self._MASK_ROW, fill, np.uint8)
        rows = raw[offset:offset + m.pitch * h].reshape(h, m.pitch)
        rows[:, :w] = host
        self.upload(f, raw.reshape(f.height, -1, 4))
        return f, m

    def download_mask(self, f: Frame, m: Mask):
        """(the mask's rows with their padding (H, pitch), every byte of the allocation) of a mask made by create_mask."""
        raw = self.download(f).reshape(-1)
        offset = m.data - f.data
        return raw[offset:offset + m.pitch * m.height].reshape(m.height, m.pitch), raw

    def static_mask(self, prev: Frame, curr: Frame, mask: Mask, tolerance: int = 0):
        """lfg_static_mask: 255 where the pair's four channel differences sum to at most `tolerance`, else 0."""
        self._check(self.lib.lfg_static_mask(self.h, ctypes.byref(prev), ctypes.byref(curr), int(tolerance), ctypes.byref(mask)),
                    "lfg_static_mask")

    def interpolate_compensated_masked(self, prev: Frame, curr: Frame, mv: Frame, mask: Mask, out: Frame, factor: float = 0.5,
                                       match_sad: int = DEFAULT_MATCH_SAD):
        """lfg_interpolate_compensated_masked: interpolate_compensated that keeps the mask's static pixels where they are."""
        self._check(self.lib.lfg_interpolate_compensated_masked(self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(mv),
                                                                ctypes.byref(mask), ctypes.byref(out), factor, int(match_sad)),
                    "lfg_interpolate_compensated_masked")

    def interpolate_compensated_masked_multi(self, prev: Frame, curr: Frame, mv: Frame, mask: Mask, outs, factors,
                                             match_sad: int = DEFAULT_MATCH_SAD):
        """lfg_interpolate_compensated_masked_multi: one generated frame per factor, each equal to the single call."""
        po, pf, n = self._multi_args(outs, factors)
        self._check(self.lib.lfg_interpolate_compensated_masked_multi(self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(mv),
                                                                      ctypes.byref(mask), po, pf, n, int(match_sad)),
                    "lfg_interpolate_compensated_masked_multi")

    def set_static_protection(self, tolerance: int):
        """-1 (default: off) or 0..1020: with INTERPOLATOR_COMPENSATED, interpolate_frames[_multi] make the pair's static mask
        (lfg_static_mask with this tolerance) and run the masked interpolation in the compensated one's place."""
        self._check(self.lib.lfg_set_static_protection(self.h, int(tolerance)), "lfg_set_static_protection")

    def extrapolate_compensated(self, prev: Frame, curr: Frame, mv: Frame, out: Frame, ahead: float = 1.0,
                                match_sad: int = DEFAULT_MATCH_SAD):
        """Motion-compensated extrapolation (lfg_extrapolate_compensated): the frame at time 1 + `ahead`, curr's content
        projected forward along its vectors and curr alone fetched along them."""
        self._check(self.lib.lfg_extrapolate_compensated(self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(mv),
                                                         ctypes.byref(out), ahead, int(match_sad)), "lfg_extrapolate_compensated")

    def extrapolate_compensated_multi(self, prev: Frame, curr: Frame, mv: Frame, outs, aheads, match_sad: int = DEFAULT_MATCH_SAD):
        """lfg_extrapolate_compensated_multi: one generated frame per `ahead`, each equal to the single call."""
        po, pf, n = self._multi_args(outs, aheads)
        self._check(self.lib.lfg_extrapolate_compensated_multi(self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(mv),
                                                               po, pf, n, int(match_sad)), "lfg_extrapolate_compensated_multi")

    def set_generation(self, generation: int):
        """GENERATION_INTERPOLATE (default) or GENERATION_EXTRAPOLATE: with INTERPOLATOR_COMPENSATED, interpolate_frames[_multi]
        read each factor as an `ahead` and run the extrapolation in the compensated interpolation's place."""
        self._check(self.lib.lfg_set_generation(self.h, int(generation)), "lfg_set_generation")

    def motion_consistency(self, a: Frame, b: Frame, tolerance: int, out: Mask):
        """The forward-backward check (lfg_motion_consistency): out(q) = 255 where q + a(q) is inside and b there is -a(q)
        within `tolerance` in L1, else 0.  (fwd, bwd) answers for curr's grid, (bwd, fwd) for prev's."""
        self._check(self.lib.lfg_motion_consistency(self.h, ctypes.byref(a), ctypes.byref(b), int(tolerance), ctypes.byref(out)),
                    "lfg_motion_consistency")

    def interpolate_compensated_bidirectional(self, prev: Frame, curr: Frame, fwd: Frame, bwd: Frame, out: Frame, factor: float = 0.5,
                                              match_sad: int = DEFAULT_MATCH_SAD, tolerance: int = 1):
        """Bidirectional compensated interpolation (lfg_interpolate_compensated_bidirectional): fwd as motion(prev, curr) and
        bwd as motion(curr, prev) write them; a vector projects only where the other field confirms it, from both grids."""
        self._check(self.lib.lfg_interpolate_compensated_bidirectional(
            self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(fwd), ctypes.byref(bwd), ctypes.byref(out), factor,
            int(match_sad), int(tolerance)), "lfg_interpolate_compensated_bidirectional")

    def interpolate_compensated_bidirectional_multi(self, prev: Frame, curr: Frame, fwd: Frame, bwd: Frame, outs, factors,
                                                    match_sad: int = DEFAULT_MATCH_SAD, tolerance: int = 1):
        """lfg_interpolate_compensated_bidirectional_multi: one generated frame per factor, each equal to the single call."""
        po, pf, n = self._multi_args(outs, factors)
        self._check(self.lib.lfg_interpolate_compensated_bidirectional_multi(
            self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(fwd), ctypes.byref(bwd), po, pf, n, int(match_sad),
            int(tolerance)), "lfg_interpolate_compensated_bidirectional_multi")

    def set_bidirectional(self, tolerance: int):
        """-1 (default): off.  0 .. 64: with INTERPOLATOR_COMPENSATED, GENERATION_INTERPOLATE and static protection off,
        interpolate_frames[_multi] measure the pair both ways and run the bidirectional interpolation with this tolerance."""
        self._check(self.lib.lfg_set_bidirectional(self.h, int(tolerance)), "lfg_set_bidirectional")

    def hole_fill_plane(self, keys: Frame, plane: Frame, reach: int, pass_static: bool = False):
        """The fill plane of a key image (lfg_hole_fill_plane): both RGBA8 frames hold one 32-bit word per pixel (upload and
        download them as (H, W, 4) uint8 views of uint32 arrays).  plane(x, y) = the smallest walk-order key of the nearest
        donors within `reach` in the four axis directions, the hole word where there is none."""
        self._check(self.lib.lfg_hole_fill_plane(self.h, ctypes.byref(keys), int(reach), int(bool(pass_static)), ctypes.byref(plane)),
                    "lfg_hole_fill_plane")

    def set_hole_reach(self, reach: int):
        """-1 (default): off, the 16-pixel hole walk.  1 .. HOLE_REACH_MAX: the compensated, masked and bidirectional
        interpolations fill their holes from a fill plane of this reach; extrapolation and the shader interpolator ignore it."""
        self._check(self.lib.lfg_set_hole_reach(self.h, int(reach)), "lfg_set_hole_reach")

    def motion_refine(self, prev: Frame, curr: Frame, mv_in: Frame, mv_out: Frame, radius: int = 1):
        """Per-pixel vector refinement (lfg_motion_refine): each pixel takes, of the vectors of mv_in at it and 4 or 8 px
        around it, the one that fits its (2 radius + 1)^2 window best."""
        self._check(self.lib.lfg_motion_refine(self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(mv_in),
                                               ctypes.byref(mv_out), int(radius)), "lfg_motion_refine")

    def set_vector_refinement(self, radius: int):
        """-1 (default: off) or 0..2: lfg_motion_refine with that radius between the estimator and the interpolator of
        interpolate_frames[_multi]."""
        self._check(self.lib.lfg_set_vector_refinement(self.h, int(radius)), "lfg_set_vector_refinement")

    def frame_halve(self, src: Frame, dst: Frame):
        """lfg_frame_halve: dst, ceil(W / 2) x ceil(H / 2), is the rounded 2 x 2 mean of src (the pyramid's level rule)."""
        self._check(self.lib.lfg_frame_halve(self.h, ctypes.byref(src), ctypes.byref(dst)), "lfg_frame_halve")

    def motion_expand(self, prev: Frame, curr: Frame, mv_low: Frame, mv_out: Frame, radius: int = 1):
        """lfg_motion_expand: a W x H field from the ceil(W / 2) x ceil(H / 2) field mv_low.  Each pixel takes the doubled vector
        of the 3 x 3 coarse neighbours above it that fits its (2 radius + 1)^2 window best, then the best of its +-1 steps."""
        self._check(self.lib.lfg_motion_expand(self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(mv_low),
                                               ctypes.byref(mv_out), int(radius)), "lfg_motion_expand")

    def motion_subpel(self, prev: Frame, curr: Frame, mv_in: Frame, mvq_out: Frame, radius: int = 1):
        """lfg_motion_subpel: the FORMAT_MV_S16X2_Q2 field mvq_out from the integer field mv_in.  Each pixel takes the best of the
        nine half-pixel steps around 4 * mv_in, then of the nine quarter-pixel steps around that, by its (2 radius + 1)^2 window."""
        self._check(self.lib.lfg_motion_subpel(self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(mv_in),
                                               ctypes.byref(mvq_out), int(radius)), "lfg_motion_subpel")

    def interpolate_compensated_subpel(self, prev: Frame, curr: Frame, mvq: Frame, out: Frame, factor: float = 0.5,
                                       match_sad: int = DEFAULT_MATCH_SAD):
        """lfg_interpolate_compensated_subpel: interpolate_compensated along quarter-pixel vectors (FORMAT_MV_S16X2_Q2)."""
        self._check(self.lib.lfg_interpolate_compensated_subpel(self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(mvq),
                                                                ctypes.byref(out), factor, int(match_sad)), "lfg_interpolate_compensated_subpel")

    def interpolate_compensated_subpel_multi(self, prev: Frame, curr: Frame, mvq: Frame, outs, factors, match_sad: int = DEFAULT_MATCH_SAD):
        """lfg_interpolate_compensated_subpel_multi: one generated frame per factor, each equal to the single call."""
        po, pf, n = self._multi_args(outs, factors)
        self._check(self.lib.lfg_interpolate_compensated_subpel_multi(self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(mvq),
                                                                      po, pf, n, int(match_sad)), "lfg_interpolate_compensated_subpel_multi")

    def set_subpixel_vectors(self, radius: int):
        """lfg_set_subpixel_vectors: -1 (default) off; 0 .. 2, where interpolate_frames[_multi] would run the plain compensated
        call with the walk they run motion_subpel with that radius and interpolate_compensated_subpel[_multi] in its place."""
        self._check(self.lib.lfg_set_subpixel_vectors(self.h, int(radius)), "lfg_set_subpixel_vectors")

    def interpolate_compensated_sampled(self, prev: Frame, curr: Frame, mv: Frame, out: Frame, factor: float = 0.5,
                                        match_sad: int = DEFAULT_MATCH_SAD, sampling: int = SAMPLING_BICUBIC):
        """lfg_interpolate_compensated_sampled: interpolate_compensated (mv FORMAT_MV_S8X2) or interpolate_compensated_subpel (mv
        FORMAT_MV_S16X2_Q2) with the fetch `sampling`: SAMPLING_BILINEAR is that call itself, SAMPLING_BICUBIC the 4 x 4 fetch."""
        self._check(self.lib.lfg_interpolate_compensated_sampled(self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(mv),
                                                                 ctypes.byref(out), factor, int(match_sad), int(sampling)),
                    "lfg_interpolate_compensated_sampled")

    def interpolate_compensated_sampled_multi(self, prev: Frame, curr: Frame, mv: Frame, outs, factors, match_sad: int = DEFAULT_MATCH_SAD,
                                              sampling: int = SAMPLING_BICUBIC):
        """lfg_interpolate_compensated_sampled_multi: one generated frame per factor, each equal to the single call."""
        po, pf, n = self._multi_args(outs, factors)
        self._check(self.lib.lfg_interpolate_compensated_sampled_multi(self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(mv),
                                                                       po, pf, n, int(match_sad), int(sampling)),
                    "lfg_interpolate_compensated_sampled_multi")

    def set_sampling(self, sampling: int):
        """lfg_set_sampling: SAMPLING_BILINEAR (default) or SAMPLING_BICUBIC, where interpolate_frames[_multi] would run the plain
        compensated call with the walk or the sub-pixel one; under every other setting it is stored and has no effect."""
        self._check(self.lib.lfg_set_sampling(self.h, int(sampling)), "lfg_set_sampling")

    def sampling_effective(self) -> int:
        """lfg_sampling_effective: what the next interpolate_frames[_multi] call would fetch with."""
        return int(self.lib.lfg_sampling_effective(self.h))

    def set_half_resolution_motion(self, radius: int):
        """-1 (default: off) or 0..2: interpolate_frames[_multi] run the selected estimator on both frames halved and
        lfg_motion_expand with that radius in its place."""
        self._check(self.lib.lfg_set_half_resolution_motion(self.h, int(radius)), "lfg_set_half_resolution_motion")

    # -- scene-cut detection.  A record is 24 bytes of device memory: here a 6 x 1 RGBA8 frame, so upload() and download()
    # move it (write_pair_record / read_pair_record).
    def create_pair_record(self) -> Frame:
        return self.create_frame(ctypes.sizeof(PairStats) // 4, 1)

    def write_pair_record(self, record: Frame, pixels: int, matched: int, sad_sum: int):
        self.upload(record, np.array([pixels, matched, sad_sum], np.uint64).view(np.uint8).reshape(1, -1, 4))

    def read_pair_record(self, record: Frame):
        """(pixels, matched, sad_sum) of a record in device memory; waits for the context."""
        return tuple(int(v) for v in self.download(record).reshape(-1).view(np.uint64))

    def pair_match(self, prev: Frame, curr: Frame, mv: Frame, record: Frame, match_sad: int = DEFAULT_MATCH_SAD):
        """Pair statistics (lfg_pair_match): how many pixels pass the compensated interpolator's match gate under the
        vectors `mv`, and the sum of their SADs, written into `record` (create_pair_record)."""
        self._check(self.lib.lfg_pair_match(self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(mv), int(match_sad),
                                            _vp(record.data)), "lfg_pair_match")

    def cut_fallback(self, prev: Frame, curr: Frame, record: Frame, min_matched_permille: int, outs, factors):
        """lfg_cut_fallback: where `record` says the pair is a cut, every output becomes prev (factor < 0.5) or curr;
        otherwise nothing is written.  The decision is taken on the device."""
        po, pf, n = self._multi_args(outs, factors)
        self._check(self.lib.lfg_cut_fallback(self.h, ctypes.byref(prev), ctypes.byref(curr), _vp(record.data),
                                              int(min_matched_permille), po, pf, n), "lfg_cut_fallback")

    def set_cut_detection(self, min_matched_permille: int):
        """-1 (default: off) or 0..1000: interpolate_frames[_multi] measure each pair (lfg_pair_match on the vectors they
        use) and show a source frame instead of a generated one where fewer than that many pixels per thousand match."""
        self._check(self.lib.lfg_set_cut_detection(self.h, int(min_matched_permille)), "lfg_set_cut_detection")

    def last_pair_stats(self):
        """((pixels, matched, sad_sum), cut) of the selected lane's last call with cut detection on (lfg_last_pair_stats)."""
        s, cut = PairStats(), ctypes.c_int()
        self._check(self.lib.lfg_last_pair_stats(self.h, ctypes.byref(s), ctypes.byref(cut)), "lfg_last_pair_stats")
        return s.as_tuple(), bool(cut.value)

    # -- frame comparison.  A record is 2,088 bytes of device memory: here a 522 x 1 RGBA8 frame, as the pair record above.
    def create_diff_record(self) -> Frame:
        return self.create_frame(ctypes.sizeof(FrameDiffStats) // 4, 1)

    def frame_diff(self, a: Frame, b: Frame, record: Frame, channel_mask: int = 0xF, accumulate: bool = False):
        """Frame comparison (lfg_frame_diff): the squared differences per channel and the histogram of the largest
        difference over the channels of `channel_mask`, written into `record` (create_diff_record) or added to it."""
        self._check(self.lib.lfg_frame_diff(self.h, ctypes.byref(a), ctypes.byref(b), int(channel_mask), int(accumulate),
                                            _vp(record.data)), "lfg_frame_diff")

    def read_diff_record(self, record: Frame):
        """(pixels, sse tuple, hist tuple) of a record in device memory; waits for the context."""
        words = [int(v) for v in self.download(record).reshape(-1).view(np.uint64)]
        return words[0], tuple(words[1:5]), tuple(words[5:])

    # -- level matching.  A histogram record is 8,200 bytes of device memory and a map 1,560: here 2,050 x 1 and 390 x 1 RGBA8
    # frames, as the records above.
    def create_histogram_record(self) -> Frame:
        return self.create_frame(ctypes.sizeof(FrameHistogramStats) // 4, 1)

    def write_histogram_record(self, record: Frame, pixels: int, hist):
        """`hist` is 4 x 256 counts."""
        words = np.concatenate([np.array([pixels], np.uint64), np.asarray(hist, np.uint64).reshape(-1)])
        self.upload(record, words.view(np.uint8).reshape(1, -1, 4))

    def read_histogram_record(self, record: Frame):
        """(pixels, hist as a 4 x 256 uint64 array) of a record in device memory; waits for the context."""
        words = self.download(record).reshape(-1).view(np.uint64)
        return int(words[0]), words[1:].reshape(4, 256).copy()

    def frame_histogram(self, f: Frame, record: Frame, accumulate: bool = False):
        """Per-channel histogram of a frame (lfg_frame_histogram), written into `record` (create_histogram_record) or added to it."""
        self._check(self.lib.lfg_frame_histogram(self.h, ctypes.byref(f), int(accumulate), _vp(record.data)), "lfg_frame_histogram")

    def create_levels_map(self) -> Frame:
        return self.create_frame(ctypes.sizeof(LevelsMap) // 4, 1)

    def levels_match(self, hist_from: Frame, hist_to: Frame, level_map: Frame, min_shift16: int = 0):
        """The pair of level maps that carries `hist_from`'s levels to `hist_to`'s of equal rank and back (lfg_levels_match),
        built on the device into `level_map` (create_levels_map)."""
        self._check(self.lib.lfg_levels_match(self.h, _vp(hist_from.data), _vp(hist_to.data), int(min_shift16), _vp(level_map.data)),
                    "lfg_levels_match")

    def read_levels_map(self, level_map: Frame) -> dict:
        """A map in device memory as a dict of pixels, shift_sum, active, reserved and the 3 x 256 forward and inverse tables;
        waits for the context."""
        raw = self.download(level_map).reshape(-1)
        head = raw[:24]
        return {"pixels": int(head[:8].view(np.uint64)[0]), "shift_sum": int(head[8:16].view(np.uint64)[0]),
                "active": int(head[16:20].view(np.uint32)[0]), "reserved": int(head[20:24].view(np.uint32)[0]),
                "forward": raw[24:24 + 768].reshape(3, 256).copy(), "inverse": raw[24 + 768:24 + 1536].reshape(3, 256).copy()}

    def levels_apply(self, src: Frame, dst: Frame, level_map: Frame, mode: int = LEVELS_FORWARD, factor: float = 0.0):
        """A map through every pixel (lfg_levels_apply): LEVELS_FORWARD, or LEVELS_AT with the frame's time in [0, 1].  `dst` may
        be `src`."""
        self._check(self.lib.lfg_levels_apply(self.h, ctypes.byref(src), ctypes.byref(dst), _vp(level_map.data), int(mode),
                                              ctypes.c_float(factor)), "lfg_levels_apply")

    def set_level_matching(self, min_shift16: int):
        """-1 (default: off) or 0..4080: interpolate_frames[_multi] level prev onto curr before every stage where the pair's
        histograms are a mean of min_shift16 / 16 levels apart, and take the generated frames to the levels of their time."""
        self._check(self.lib.lfg_set_level_matching(self.h, int(min_shift16)), "lfg_set_level_matching")

    def last_level_match(self):
        """(shift_sum, pixels, active) of the selected lane's last call with level matching on (lfg_last_level_match)."""
        s, p, a = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
        self._check(self.lib.lfg_last_level_match(self.h, ctypes.byref(s), ctypes.byref(p), ctypes.byref(a)), "lfg_last_level_match")
        return int(s.value), int(p.value), bool(a.value)

    # -- structural similarity.  A record is 568 bytes of device memory: here a 142 x 1 RGBA8 frame.
    def create_ssim_record(self) -> Frame:
        return self.create_frame(ctypes.sizeof(FrameSsimStats) // 4, 1)

    def frame_ssim(self, a: Frame, b: Frame, record: Frame, channel_mask: int = 0xF, accumulate: bool = False):
        """Integer SSIM (lfg_frame_ssim) over 8 x 8 windows at stride 4: the sum of Q per channel, the histogram of the smallest
        Q over the channels of `channel_mask` and the worst window, written into `record` (create_ssim_record) or added to it."""
        self._check(self.lib.lfg_frame_ssim(self.h, ctypes.byref(a), ctypes.byref(b), int(channel_mask), int(accumulate),
                                            _vp(record.data)), "lfg_frame_ssim")

    def read_ssim_record(self, record: Frame):
        """(windows, sum tuple of 4 signed, hist tuple of 65, worst) of a record in device memory; waits for the context."""
        raw = self.download(record).reshape(-1)
        words = [int(v) for v in raw.view(np.uint64)]
        return words[0], tuple(int(v) for v in raw.view(np.int64)[1:5]), tuple(words[5:70]), words[70]

    # -- NV12 input and output.  The planes are caller-owned device memory; create_nv12 keeps both in one MV_S8X2 frame of
    # W/2 x 3H/2 (W bytes per row: H rows of luma, then H/2 rows of pairs), so upload() and download() move them.
    def create_nv12(self, width: int, height: int):
        """(the frame that owns the memory, the lfg_nv12 that describes it): tightly packed planes, luma first."""
        if width % 2 or height % 2 or width <= 0 or height <= 0:
            raise ValueError("NV12 wants an even width and height")
        f = self.create_frame(width // 2, height * 3 // 2, FORMAT_MV_S8X2)
        return f, Nv12(f.data, f.data + width * height, width, height, width, width)

    def nv12_from(self, y: np.ndarray, uv: np.ndarray):
        """create_nv12 holding the luma plane y (H, W) and the pairs uv (H/2, W/2, 2), both uint8."""
        h, w = y.shape
        f, planes = self.create_nv12(w, h)
        self.upload(f, np.concatenate([y.reshape(-1), uv.reshape(-1)]).view(np.int8).reshape(h * 3 // 2, w // 2, 2))
        return f, planes

    def download_nv12(self, f: Frame):
        """(y, uv) of a frame made by create_nv12."""
        w, h = f.width * 2, f.height * 2 // 3
        raw = self.download(f).view(np.uint8).reshape(-1)
        return raw[:w * h].reshape(h, w), raw[w * h:].reshape(h // 2, w // 2, 2)

    def nv12_to_rgba(self, planes: Nv12, out: Frame, matrix: int = YUV_BT709, yuv_range: int = YUV_LIMITED, siting: int = CHROMA_LEFT):
        """lfg_nv12_to_rgba: the NV12 planes as an RGBA8 frame of the same size (A = 255); one launch on the selected lane."""
        self._check(self.lib.lfg_nv12_to_rgba(self.h, ctypes.byref(planes), ctypes.byref(out), int(matrix), int(yuv_range), int(siting)),
                    "lfg_nv12_to_rgba")

    def rgba_to_nv12(self, src: Frame, planes: Nv12, matrix: int = YUV_BT709, yuv_range: int = YUV_LIMITED, siting: int = CHROMA_LEFT):
        """lfg_rgba_to_nv12: an RGBA8 frame into NV12 planes of the same size (alpha ignored); one launch on the selected lane."""
        self._check(self.lib.lfg_rgba_to_nv12(self.h, ctypes.byref(src), ctypes.byref(planes), int(matrix), int(yuv_range), int(siting)),
                    "lfg_rgba_to_nv12")

    def sharpen(self, src: Frame, dst: Frame, strength: int):
        """lfg_sharpen: `src` sharpened into `dst` (both RGBA8, one size, no overlap), strength 0 .. MAX_SHARPEN, limited to
        the range of each pixel and its four neighbours; for presented frames only, never for one a motion stage reads."""
        self._check(self.lib.lfg_sharpen(self.h, ctypes.byref(src), ctypes.byref(dst), int(strength)), "lfg_sharpen")

    def deband(self, src: Frame, dst: Frame, iterations: int = 1, threshold: int = 4, radius: int = 16, grain: int = 0, seed: int = 0):
        """lfg_deband: `src` debanded into `dst` (both RGBA8, one size, no overlap): 1 .. 4 iterations of a four-tap average at
        a random offset within radius * i, accepted within threshold / i quarter levels, then grain and the dither back to 8
        bits; `seed` is the presented-frame counter.  For presented frames only, never for one a motion stage reads."""
        self._check(self.lib.lfg_deband(self.h, ctypes.byref(src), ctypes.byref(dst), int(iterations), int(threshold), int(radius),
                                        int(grain), int(seed) & 0xFFFFFFFF), "lfg_deband")

    def denoise_temporal(self, curr: Frame, refs, mvs, dst: Frame, radius: int = 1, tolerance: int = 32, strength: int = 192,
                         limit: int = 255):
        """lfg_denoise_temporal: `curr` mixed into `dst` with one or two reference frames `refs`, each displaced by its field of
        `mvs` (MV_S8X2 on curr's grid, as motion(ref, curr) writes it), where the (2 radius + 1)^2 window fits within
        `tolerance` per texel; no output byte leaves curr +- limit.  One launch on the selected lane."""
        if len(refs) != len(mvs):
            raise LfgError(f"denoise_temporal: {len(refs)} references and {len(mvs)} fields")
        n = len(refs)
        ref_ptrs, mv_ptrs = (_FP * n)(*[ctypes.pointer(f) for f in refs]), (_FP * n)(*[ctypes.pointer(f) for f in mvs])
        self._check(self.lib.lfg_denoise_temporal(self.h, ctypes.byref(curr), ref_ptrs, mv_ptrs, n, ctypes.byref(dst), int(radius),
                                                  int(tolerance), int(strength), int(limit)), "lfg_denoise_temporal")

    def resample(self, src: Frame, dst: Frame, filt: int):
        """lfg_resample: `src` resampled into `dst` (both RGBA8, any sizes, no overlap) under one of FILTER_*, anti-aliased where
        an axis shrinks; one launch, timed under STAGE_SCALE."""
        self._check(self.lib.lfg_resample(self.h, ctypes.byref(src), ctypes.byref(dst), int(filt)), "lfg_resample")

    def upscale_edge(self, src: Frame, dst: Frame):
        """lfg_upscale_edge: `src` upscaled into `dst` (both RGBA8, `dst` at least as large on each axis, no overlap) by the
        edge-adaptive 12-tap kernel; every output byte stays within its 2 x 2 bracket.  One launch on the selected lane."""
        self._check(self.lib.lfg_upscale_edge(self.h, ctypes.byref(src), ctypes.byref(dst)), "lfg_upscale_edge")

    def resample_antiring(self, src: Frame, dst: Frame, filt: int, strength: int):
        """lfg_resample_antiring: lfg_resample with each upscaling pass held to the range of the two source samples that bracket
        the output position, mixed with the plain result by strength 0 .. 64; lfg_resample itself where no axis grows,
        at strength 0 and under FILTER_NEAREST."""
        self._check(self.lib.lfg_resample_antiring(self.h, ctypes.byref(src), ctypes.byref(dst), int(filt), int(strength)),
                    "lfg_resample_antiring")

    def resample_light(self, src: Frame, dst: Frame, filt: int, light: int):
        """lfg_resample_light: lfg_resample with the colour channels' sums formed in linear (LIGHT_LINEAR) or sigmoidal
        (LIGHT_SIGMOID, no axis may shrink) light; lfg_resample itself under LIGHT_GAMMA and under FILTER_NEAREST."""
        self._check(self.lib.lfg_resample_light(self.h, ctypes.byref(src), ctypes.byref(dst), int(filt), int(light)), "lfg_resample_light")

    def set_fused_motion_interpolate(self, on: bool):
        """lfg_interpolate_frames in the north-star order: the motion kernels write the generated frame themselves."""
        self._check(self.lib.lfg_set_fused_motion_interpolate(self.h, int(on)), "lfg_set_fused_motion_interpolate")

    def set_fused_interpolate_scale(self, on: bool):
        self._check(self.lib.lfg_set_fused_interpolate_scale(self.h, int(on)), "lfg_set_fused_interpolate_scale")

    def interpolate_scale(self, prev: Frame, curr: Frame, mv: Frame, out: Frame, factor: float = 0.5):
        """interpolate at input resolution and upscale, one call (one kernel when out is exactly 2x the inputs)."""
        self._check(self.lib.lfg_interpolate_scale(self.h, ctypes.byref(prev), ctypes.byref(curr), ctypes.byref(mv),
                                                   ctypes.byref(out), factor), "lfg_interpolate_scale")

    def selftest_sqrt(self, lo_bits: int, hi_bits: int) -> int:
        n = ctypes.c_uint64()
        self._check(self.lib.lfg_selftest_sqrt(self.h, lo_bits, hi_bits, ctypes.byref(n)), "lfg_selftest_sqrt")
        return n.value

    # -- multi-GPU: the shared previous frame (RCCL behind the C-ABI)
    @staticmethod
    def comm_unique_id() -> bytes:
        """128 bytes made by ONE rank; hand them to the others (torch.distributed store, file, ...)."""
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        rc = load().lfg_comm_unique_id(buf)
        if rc != 0:
            raise LfgError(f"lfg_comm_unique_id failed ({rc}): is librccl.so available?")
        return buf.raw

    def comm_init(self, nranks: int, rank: int, comm_id: bytes):
        if len(comm_id) != COMM_ID_BYTES:
            raise ValueError(f"communicator id must be {COMM_ID_BYTES} bytes")
        buf = ctypes.create_string_buffer(comm_id, COMM_ID_BYTES)
        self._check(self.lib.lfg_comm_init(self.h, nranks, rank, buf), "lfg_comm_init")

    def comm_ranks(self) -> int:
        """Ranks of this context's communicator (0 without one)."""
        return int(self.lib.lfg_comm_ranks(self.h))

    def comm_rank(self) -> int:
        return int(self.lib.lfg_comm_rank(self.h))

    def broadcast_frame(self, f: Frame, root: int = 0):
        self._check(self.lib.lfg_broadcast_frame(self.h, ctypes.byref(f), root), "lfg_broadcast_frame")

    def comm_wait(self):
        self._check(self.lib.lfg_comm_wait(self.h), "lfg_comm_wait")

    def comm_sync(self):
        """The host waits for every broadcast issued so far."""
        self._check(self.lib.lfg_comm_sync(self.h), "lfg_comm_sync")

    def comm_reserved_cus(self) -> int:
        """CUs the library's own streams leave to the communicator (0 without one)."""
        return int(self.lib.lfg_comm_reserved_cus(self.h))

    def comm_cu_mask(self, words: int = 8) -> list[int]:
        """The CU mask (32-bit words, bit i = CU i usable) a caller-supplied compute stream should be created with."""
        buf = (_u32 * words)()
        self._check(self.lib.lfg_comm_cu_mask(self.h, buf, words), "lfg_comm_cu_mask")
        return [int(x) for x in buf]

    def comm_probe(self, workgroups: int = 8, microseconds: int = 50, every_lane: bool = True):
        """Diagnostic: a kernel of RCCL's device kernel's footprint where a broadcast would run (csrc/comm_probe.hip)."""
        self._check(self.lib.lfg_comm_probe(self.h, workgroups, microseconds, int(every_lane)), "lfg_comm_probe")

    def comm_probe_ms(self) -> float:
        """Device milliseconds of the last probe from ready to done (waits for it)."""
        ms = ctypes.c_float()
        self._check(self.lib.lfg_comm_probe_ms(self.h, ctypes.byref(ms)), "lfg_comm_probe_ms")
        return float(ms.value)

    def broadcast_frame_lane(self, f: Frame, root: int = 0):
        """lfg_broadcast_frame ordered behind the selected lane only (the caller has ordered that lane behind the frame's readers)."""
        self._check(self.lib.lfg_broadcast_frame_lane(self.h, ctypes.byref(f), root), "lfg_broadcast_frame_lane")

    def comm_destroy(self):
        self._check(self.lib.lfg_comm_destroy(self.h), "lfg_comm_destroy")

    # -- measurement
    def profile_enable(self, on: bool = True):
        self._check(self.lib.lfg_profile_enable(self.h, int(on)), "lfg_profile_enable")

    def profile_reset(self):
        self._check(self.lib.lfg_profile_reset(self.h), "lfg_profile_reset")

    def profile_get(self, stage: int):
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        self._check(self.lib.lfg_profile_get(self.h, stage, ctypes.byref(ms), ctypes.byref(n)), "lfg_profile_get")
        return ms.value, n.value
