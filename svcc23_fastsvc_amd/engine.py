"""ctypes binding of the C ABI in ``include/fastsvc_hip.h`` (``libfastsvc_hip.so``).

PyTorch is used for plumbing only: device memory (weight blob, workspace, outputs) comes from its
caching allocator and kernels are enqueued on its current HIP stream.  There is NO CPU fallback:
if the shared library is missing or the tensors are not on a GPU, this module raises.
"""
from __future__ import annotations

import ctypes
import json
import math
import os
from typing import Dict, Mapping, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .synth import GeneratorConfig

_LIB = None
# FASTSVC_HIP_LIB: load another build of the same ABI (tools/timeline.py points it at the stamped
# diagnostic library); there is no fallback of any kind - a missing library is an error
_LIB_PATH = os.environ.get("FASTSVC_HIP_LIB") or \
    os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfastsvc_hip.so")
MAX_STAGES = 8
# launch shapes measured once on an MI355X by tools/tune_shapes.py (fastsvc_autotune winners for
# the BASELINE.json workloads); other (B, F) fall back to the static cost model or model.autotune
# activation storage of a plan: name -> fastsvc_plan_set_storage code / the dtype of the workspace taps
STORAGE_CODES = {"float32": 0, "bfloat16": 1, "float16": 2}
STORAGE_DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
DTYPE_CODES = {dt: STORAGE_CODES[name] for name, dt in STORAGE_DTYPES.items()}       # the C side's storage code of a tensor
TUNED_TABLE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned_mi355x.json")

# every symbol include/fastsvc_hip.h declares (checked by tests/test_boundary.py)
ABI_SYMBOLS = (
    "fastsvc_abi_version", "fastsvc_last_error", "fastsvc_plan_create", "fastsvc_plan_destroy",
    "fastsvc_plan_set_storage", "fastsvc_plan_get_storage",
    "fastsvc_weight_blob_bytes", "fastsvc_pack_weights", "fastsvc_workspace_bytes",
    "fastsvc_pack_device_scratch_bytes", "fastsvc_pack_device_launch_count", "fastsvc_pack_weights_device",
    "fastsvc_forward", "fastsvc_forward_grouped", "fastsvc_norm_group_scratch_bytes", "fastsvc_norm_group_stats",
    "fastsvc_forward_running", "fastsvc_norm_carry_bytes", "fastsvc_norm_running_scratch_bytes", "fastsvc_norm_running_stats",
    "fastsvc_forward_running_decay", "fastsvc_norm_running_stats_decay",
    "fastsvc_autotune", "fastsvc_tuned_count", "fastsvc_tuned_get", "fastsvc_tuned_set",
    "fastsvc_forward_profile", "fastsvc_workspace_tap", "fastsvc_forward_launch_count",
    "fastsvc_flops_per_sample", "fastsvc_signal_scratch_bytes", "fastsvc_signal_generate",
    "fastsvc_stream_prepare", "fastsvc_stream_release", "fastsvc_split_half", "fastsvc_plan_set_workspace_mode",
    "fastsvc_loudness_frames", "fastsvc_loudness_scratch_bytes", "fastsvc_loudness_extract",
    "fastsvc_gather_padded", "fastsvc_gather_time_major", "fastsvc_pcm16_pack",
    "fastsvc_pcm16_pack_checked", "fastsvc_output_check",
    "fastsvc_collate_launch_count", "fastsvc_collate_crops",
    "fastsvc_fanout_launch_count", "fastsvc_fanout_assemble",
    "fastsvc_window_launch_count", "fastsvc_window_assemble", "fastsvc_window_stitch",
    "fastsvc_stream_launch_count", "fastsvc_stream_push", "fastsvc_stream_assemble", "fastsvc_stream_check",
    "fastsvc_stream_loudness_scratch_bytes", "fastsvc_stream_loudness",
    "fastsvc_stream_f0", "fastsvc_stream_f0_running", "fastsvc_f0_lags", "fastsvc_f0_extract",
    "fastsvc_f0_candidates", "fastsvc_f0_track_scratch_bytes", "fastsvc_f0_track", "fastsvc_stream_f0_tracked",
    "fastsvc_stft_loss_scratch_bytes", "fastsvc_stft_loss_forward", "fastsvc_stft_loss_backward",
    "fastsvc_conv1d_forward", "fastsvc_conv1d_backward_weight", "fastsvc_conv1d_backward_weight_scratch_bytes",
    "fastsvc_film_norm_forward", "fastsvc_film_norm_backward", "fastsvc_weight_norm_forward", "fastsvc_weight_norm_backward",
    "fastsvc_gconv1d_supported", "fastsvc_gconv1d_forward", "fastsvc_gconv1d_backward_data",
    "fastsvc_gconv1d_backward_weight_scratch_bytes", "fastsvc_gconv1d_backward_weight",
)


class FastSVCError(RuntimeError):
    pass


class _Config(ctypes.Structure):
    _fields_ = [
        ("in_channels", ctypes.c_int32),
        ("n_stages", ctypes.c_int32),
        ("mid_channels", ctypes.c_int32 * MAX_STAGES),
        ("upsampling_scales", ctypes.c_int32 * MAX_STAGES),
        ("out_channels", ctypes.c_int32),
        ("spk_emb_size", ctypes.c_int32),
        ("use_spk_emb", ctypes.c_int32),
    ]


class _LaunchRecord(ctypes.Structure):
    _fields_ = [("layer", ctypes.c_char * 64), ("kernel", ctypes.c_char * 40),
                ("flops", ctypes.c_double), ("bytes", ctypes.c_double), ("ms", ctypes.c_float), ("x2_path", ctypes.c_int32)]


class _Tensor(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("data", ctypes.POINTER(ctypes.c_float)), ("numel", ctypes.c_int64)]


def library_path() -> str:
    return _LIB_PATH


def load_library():
    """dlopen the in-tree gfx950 library; raise (never fall back) when it is absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_LIB_PATH):
        raise FastSVCError(
            f"{_LIB_PATH} not found: build it with `python -m svcc23_fastsvc_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for this path.")
    lib = ctypes.CDLL(_LIB_PATH)
    vp, sz, i32, i64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32, ctypes.c_int64
    lib.fastsvc_abi_version.restype = ctypes.c_int
    lib.fastsvc_last_error.restype = ctypes.c_char_p
    lib.fastsvc_plan_create.argtypes = [ctypes.POINTER(_Config), ctypes.POINTER(vp)]
    lib.fastsvc_plan_create.restype = ctypes.c_int
    lib.fastsvc_plan_destroy.argtypes = [vp]
    lib.fastsvc_plan_destroy.restype = None
    lib.fastsvc_plan_set_storage.argtypes = [vp, i32]
    lib.fastsvc_plan_set_storage.restype = ctypes.c_int
    lib.fastsvc_plan_get_storage.argtypes = [vp]
    lib.fastsvc_plan_get_storage.restype = ctypes.c_int
    lib.fastsvc_weight_blob_bytes.argtypes = [vp]
    lib.fastsvc_weight_blob_bytes.restype = sz
    lib.fastsvc_pack_weights.argtypes = [vp, ctypes.POINTER(_Tensor), i32, vp]
    lib.fastsvc_pack_weights.restype = ctypes.c_int
    lib.fastsvc_pack_device_scratch_bytes.argtypes = [vp]
    lib.fastsvc_pack_device_scratch_bytes.restype = sz
    lib.fastsvc_pack_device_launch_count.argtypes = [vp]
    lib.fastsvc_pack_device_launch_count.restype = ctypes.c_int
    lib.fastsvc_pack_weights_device.argtypes = [vp, ctypes.POINTER(_Tensor), i32, vp, vp, sz, vp]
    lib.fastsvc_pack_weights_device.restype = ctypes.c_int
    lib.fastsvc_workspace_bytes.argtypes = [vp, i32, i32]
    lib.fastsvc_workspace_bytes.restype = sz
    lib.fastsvc_forward.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, sz, vp]
    lib.fastsvc_forward.restype = ctypes.c_int
    lib.fastsvc_norm_group_scratch_bytes.argtypes = [vp, i32, i32]
    lib.fastsvc_norm_group_scratch_bytes.restype = sz
    lib.fastsvc_forward_grouped.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, sz, vp, sz, vp]
    lib.fastsvc_forward_grouped.restype = ctypes.c_int
    lib.fastsvc_norm_group_stats.argtypes = [vp, i32, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, sz, vp]
    lib.fastsvc_norm_group_stats.restype = ctypes.c_int
    lib.fastsvc_norm_carry_bytes.argtypes = [vp]
    lib.fastsvc_norm_carry_bytes.restype = sz
    lib.fastsvc_norm_running_scratch_bytes.argtypes = [vp, i32, i32]
    lib.fastsvc_norm_running_scratch_bytes.restype = sz
    lib.fastsvc_forward_running.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp] + [vp] * 6 + [vp, sz, vp, sz, vp, sz, vp]
    lib.fastsvc_forward_running.restype = ctypes.c_int
    lib.fastsvc_norm_running_stats.argtypes = [vp, i32, i32, i32, i32, vp, i32] + [vp] * 6 + [vp, vp, vp, sz, vp]
    lib.fastsvc_norm_running_stats.restype = ctypes.c_int
    lib.fastsvc_forward_running_decay.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp] + [vp] * 9 + [vp, sz, vp, sz, vp, sz, vp]
    lib.fastsvc_forward_running_decay.restype = ctypes.c_int
    lib.fastsvc_norm_running_stats_decay.argtypes = [vp, i32, i32, i32, i32, vp, i32] + [vp] * 9 + [vp, vp, vp, sz, vp]
    lib.fastsvc_norm_running_stats_decay.restype = ctypes.c_int
    lib.fastsvc_loudness_frames.argtypes = [i32, i32]
    lib.fastsvc_loudness_frames.restype = i32
    lib.fastsvc_loudness_scratch_bytes.argtypes = [i32, i32, i32]
    lib.fastsvc_loudness_scratch_bytes.restype = sz
    lib.fastsvc_loudness_extract.argtypes = [vp, vp, vp, i32, i32, i32, ctypes.c_float, vp]
    lib.fastsvc_loudness_extract.restype = ctypes.c_int
    lib.fastsvc_stft_loss_scratch_bytes.argtypes = [i32, i32, i32, vp, vp]
    lib.fastsvc_stft_loss_scratch_bytes.restype = sz
    lib.fastsvc_stft_loss_forward.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.fastsvc_stft_loss_forward.restype = ctypes.c_int
    lib.fastsvc_stft_loss_backward.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.fastsvc_stft_loss_backward.restype = ctypes.c_int
    lib.fastsvc_conv1d_forward.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.fastsvc_conv1d_forward.restype = ctypes.c_int
    lib.fastsvc_conv1d_backward_weight_scratch_bytes.argtypes = [i32, i32, i32, i32, i32]
    lib.fastsvc_conv1d_backward_weight_scratch_bytes.restype = sz
    lib.fastsvc_conv1d_backward_weight.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    lib.fastsvc_conv1d_backward_weight.restype = ctypes.c_int
    lib.fastsvc_gconv1d_supported.argtypes = [i32] * 6
    lib.fastsvc_gconv1d_supported.restype = ctypes.c_int
    lib.fastsvc_gconv1d_forward.argtypes = [vp, vp, vp, vp] + [i32] * 8 + [ctypes.c_float, vp]
    lib.fastsvc_gconv1d_forward.restype = ctypes.c_int
    lib.fastsvc_gconv1d_backward_data.argtypes = [vp, vp, vp, vp] + [i32] * 8 + [ctypes.c_float, vp]
    lib.fastsvc_gconv1d_backward_data.restype = ctypes.c_int
    lib.fastsvc_gconv1d_backward_weight_scratch_bytes.argtypes = [i32, i32, i32]
    lib.fastsvc_gconv1d_backward_weight_scratch_bytes.restype = sz
    lib.fastsvc_gconv1d_backward_weight.argtypes = [vp, vp, vp, vp, vp, vp] + [i32] * 8 + [ctypes.c_float, vp]
    lib.fastsvc_gconv1d_backward_weight.restype = ctypes.c_int
    lib.fastsvc_film_norm_forward.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, ctypes.c_float, ctypes.c_float, vp]
    lib.fastsvc_film_norm_forward.restype = ctypes.c_int
    lib.fastsvc_film_norm_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, ctypes.c_float, vp]
    lib.fastsvc_film_norm_backward.restype = ctypes.c_int
    lib.fastsvc_weight_norm_forward.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp]
    lib.fastsvc_weight_norm_forward.restype = ctypes.c_int
    lib.fastsvc_weight_norm_backward.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.fastsvc_weight_norm_backward.restype = ctypes.c_int
    lib.fastsvc_split_half.argtypes = [vp, i64, vp, vp, vp]
    lib.fastsvc_split_half.restype = None
    lib.fastsvc_stream_prepare.argtypes = [vp]
    lib.fastsvc_stream_prepare.restype = ctypes.c_int
    lib.fastsvc_stream_release.argtypes = [vp]
    lib.fastsvc_stream_release.restype = ctypes.c_int
    lib.fastsvc_gather_padded.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i32), vp, i32, i32, i32, vp]
    lib.fastsvc_gather_padded.restype = ctypes.c_int
    lib.fastsvc_gather_time_major.argtypes = [vp, i64, ctypes.POINTER(i64), ctypes.POINTER(i32), vp, i32, i32, i32, vp]
    lib.fastsvc_gather_time_major.restype = ctypes.c_int
    lib.fastsvc_pcm16_pack.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i64), vp, i64, i32, i32, vp]
    lib.fastsvc_pcm16_pack.restype = ctypes.c_int
    lib.fastsvc_pcm16_pack_checked.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i64), vp, i64, vp, i32, i32, vp]
    lib.fastsvc_pcm16_pack_checked.restype = ctypes.c_int
    lib.fastsvc_output_check.argtypes = [vp, ctypes.POINTER(i32), vp, i32, i32, vp]
    lib.fastsvc_output_check.restype = ctypes.c_int
    lib.fastsvc_collate_launch_count.argtypes = [i32]
    lib.fastsvc_collate_launch_count.restype = ctypes.c_int
    lib.fastsvc_collate_crops.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, i32, ctypes.POINTER(i64), ctypes.POINTER(i32),
                                          ctypes.POINTER(i32), ctypes.POINTER(i32), vp, vp, vp, vp, vp] + [i32] * 6 + [vp]
    lib.fastsvc_collate_crops.restype = ctypes.c_int
    lib.fastsvc_fanout_launch_count.argtypes = [i32]
    lib.fastsvc_fanout_launch_count.restype = ctypes.c_int
    lib.fastsvc_fanout_assemble.argtypes = [vp, i64, vp, i64, vp, i64, i32] + [ctypes.POINTER(i64)] * 3 + [ctypes.POINTER(i32)] + \
        [vp, vp, vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i32), vp, vp, vp, vp] + [i32] * 5 + [vp]
    lib.fastsvc_fanout_assemble.restype = ctypes.c_int
    lib.fastsvc_window_launch_count.argtypes = [i32]
    lib.fastsvc_window_launch_count.restype = ctypes.c_int
    lib.fastsvc_window_assemble.argtypes = [vp, i64, vp, vp, i64, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i32),
                                            vp, vp, vp, i32, i32, i32, i32, vp]
    lib.fastsvc_window_assemble.restype = ctypes.c_int
    lib.fastsvc_window_stitch.argtypes = [vp, i32, i32] + [ctypes.POINTER(i32)] * 3 + [i32] + [ctypes.POINTER(i32)] * 2 + \
        [ctypes.POINTER(i64)] * 2 + [vp, i64, ctypes.POINTER(i64), vp, vp, i64, ctypes.POINTER(i32), vp, i32, vp]
    lib.fastsvc_window_stitch.restype = ctypes.c_int
    lib.fastsvc_stream_launch_count.argtypes = [i32]
    lib.fastsvc_stream_launch_count.restype = ctypes.c_int
    lib.fastsvc_stream_push.argtypes = [vp, i64, i32, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i64), ctypes.POINTER(i64),
                                        ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_uint64), vp, vp, vp, vp] + \
        [i32] * 5 + [ctypes.c_float] * 3 + [vp]
    lib.fastsvc_stream_push.restype = ctypes.c_int
    lib.fastsvc_stream_assemble.argtypes = [vp, vp, vp, i32, i32, ctypes.POINTER(i64), ctypes.POINTER(i32), ctypes.POINTER(i64),
                                            ctypes.POINTER(i32), vp, vp, vp, i32, i32, i32, i32, vp]
    lib.fastsvc_stream_assemble.restype = ctypes.c_int
    lib.fastsvc_stream_check.argtypes = [vp, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32), vp, i64, i32, i32,
                                         ctypes.POINTER(i32), ctypes.POINTER(i32), vp, vp]
    lib.fastsvc_stream_check.restype = ctypes.c_int
    lib.fastsvc_stream_loudness_scratch_bytes.argtypes = [i32, i32]
    lib.fastsvc_stream_loudness_scratch_bytes.restype = sz
    lib.fastsvc_stream_loudness.argtypes = [vp, vp, vp, vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i64), ctypes.POINTER(i32),
                                            ctypes.POINTER(i64), ctypes.POINTER(i32), ctypes.POINTER(i32), i32, i32, i32, i32,
                                            ctypes.c_float, vp]
    lib.fastsvc_stream_loudness.restype = ctypes.c_int
    lib.fastsvc_stream_f0.argtypes = [vp, vp, vp, vp, vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i64), ctypes.POINTER(i32),
                                      ctypes.POINTER(i64), ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_uint64),
                                      ctypes.POINTER(ctypes.c_double), i32, i32, i32, i32] + [ctypes.c_float] * 6 + [vp]
    lib.fastsvc_stream_f0.restype = ctypes.c_int
    lib.fastsvc_stream_f0_running.argtypes = [vp, vp, vp, vp, vp, vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i64),
                                              ctypes.POINTER(i32), ctypes.POINTER(i64), ctypes.POINTER(i32), ctypes.POINTER(i32),
                                              ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double),
                                              ctypes.POINTER(ctypes.c_double), i32, i32, i32, i32] + [ctypes.c_float] * 6 + [vp]
    lib.fastsvc_stream_f0_running.restype = ctypes.c_int
    lib.fastsvc_f0_lags.argtypes = [ctypes.c_float] * 3 + [ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.fastsvc_f0_lags.restype = ctypes.c_int
    lib.fastsvc_f0_extract.argtypes = [vp, vp, i32, i32, i32] + [ctypes.c_float] * 4 + [vp]
    lib.fastsvc_f0_extract.restype = ctypes.c_int
    lib.fastsvc_f0_candidates.argtypes = [vp, vp, i32, i32, i32] + [ctypes.c_float] * 4 + [vp]
    lib.fastsvc_f0_candidates.restype = ctypes.c_int
    lib.fastsvc_f0_track_scratch_bytes.argtypes = [i32, i32]
    lib.fastsvc_f0_track_scratch_bytes.restype = i64
    lib.fastsvc_f0_track.argtypes = [vp, vp, vp, i32, i32, i32, ctypes.c_float, i32] + [ctypes.c_double] * 4 + [vp]
    lib.fastsvc_f0_track.restype = ctypes.c_int
    lib.fastsvc_stream_f0_tracked.argtypes = [vp] * 9 + [i32, ctypes.POINTER(i32), ctypes.POINTER(i64), ctypes.POINTER(i32),
                                              ctypes.POINTER(i64), ctypes.POINTER(i32), ctypes.POINTER(i32),
                                              ctypes.POINTER(i32), ctypes.POINTER(i64), ctypes.POINTER(i32),
                                              ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double),
                                              ctypes.POINTER(ctypes.c_double), i32, i32, i32, i32] + [ctypes.c_float] * 4 + \
        [i32] + [ctypes.c_double] * 4 + [ctypes.c_float] * 2 + [vp]
    lib.fastsvc_stream_f0_tracked.restype = ctypes.c_int
    lib.fastsvc_autotune.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, sz, vp, ctypes.POINTER(i32)]
    lib.fastsvc_autotune.restype = ctypes.c_int
    lib.fastsvc_tuned_count.argtypes = [vp]
    lib.fastsvc_tuned_count.restype = ctypes.c_int
    lib.fastsvc_tuned_get.argtypes = [vp, i32, ctypes.c_char_p, ctypes.POINTER(i32 * 5)]
    lib.fastsvc_tuned_get.restype = ctypes.c_int
    lib.fastsvc_tuned_set.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(i32 * 5)]
    lib.fastsvc_tuned_set.restype = ctypes.c_int
    lib.fastsvc_forward_profile.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, sz, vp,
                                            ctypes.POINTER(_LaunchRecord), i32, ctypes.POINTER(i32)]
    lib.fastsvc_forward_profile.restype = ctypes.c_int
    lib.fastsvc_workspace_tap.argtypes = [vp, i32, i32, ctypes.c_char_p, ctypes.POINTER(sz),
                                          ctypes.POINTER(i64), ctypes.POINTER(i64 * 3)]
    lib.fastsvc_workspace_tap.restype = ctypes.c_int
    lib.fastsvc_plan_set_workspace_mode.argtypes = [vp, i32]
    lib.fastsvc_plan_set_workspace_mode.restype = ctypes.c_int
    lib.fastsvc_forward_launch_count.argtypes = [vp, i32]
    lib.fastsvc_forward_launch_count.restype = ctypes.c_int
    lib.fastsvc_flops_per_sample.argtypes = [vp]
    lib.fastsvc_flops_per_sample.restype = ctypes.c_double
    lib.fastsvc_signal_scratch_bytes.argtypes = [i32, i32]
    lib.fastsvc_signal_scratch_bytes.restype = sz
    lib.fastsvc_signal_generate.argtypes = [vp, vp, vp, i32, i32, i32, ctypes.c_float, ctypes.c_float,
                                            ctypes.c_float, ctypes.POINTER(i32), i32, ctypes.c_uint64, vp]
    lib.fastsvc_signal_generate.restype = ctypes.c_int
    if lib.fastsvc_abi_version() != 1:
        raise FastSVCError("libfastsvc_hip.so ABI version mismatch")
    _LIB = lib
    return lib


def _ptr(t):
    """A tensor's device address as the library takes it; ``None`` is the null pointer."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _ints(ctype, values):
    """The ctypes array of ``ctype`` (``c_int32``, ``c_int64``) that holds ``int(v)`` of every value; an array a caller
    made once, of that type, passes through."""
    if isinstance(values, ctypes.Array) and values._type_ is ctype:
        return values
    return (ctype * len(values))(*[int(v) for v in values])


def _gpu_tensors(who: str, like, specs) -> None:
    """What the wrapper ``who`` asks of its tensors, ``specs = (name, tensor, dtype, dim), ...`` in the order they are
    checked: each on a GPU (``FastSVCError``: no CPU fallback), then of its dtype and rank, contiguous and on the device
    of ``like`` (``ValueError``) - a tensor that was checked before, or the first of ``specs``."""
    for name, t, dtype, dim in specs:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise FastSVCError(f"{who} needs GPU tensors (no CPU fallback); {name} is on " + str(getattr(t, "device", type(t))))
        if t.dtype != dtype or not t.is_contiguous() or t.device != like.device or t.dim() != dim:
            raise ValueError(f"{name} must be a contiguous {dim}-D {dtype} tensor on {like.device}")


def gather_padded(rows: Sequence[torch.Tensor], width: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Assemble a zero-padded batch from B device tensors of shape (C, len_b) (len_b <= width; float32, unit stride
    along time, any row pitch - views of larger tensors are fine): -> (B, C, width).  One HIP launch per 64
    utterances on the current stream (fastsvc_gather_padded, csrc/fastsvc_stage.hip); fails loudly off the GPU."""
    lib = load_library()
    B = len(rows)
    if B == 0:
        raise ValueError("gather_padded needs at least one utterance")
    first = rows[0]
    if not first.is_cuda:
        raise FastSVCError("gather_padded needs GPU tensors (no CPU fallback); got " + str(first.device))
    C = int(first.shape[0])
    for t in rows:
        if t.dim() != 2 or t.shape[0] != C or t.dtype != torch.float32 or t.device != first.device or \
                (t.shape[1] > 1 and t.stride(1) != 1) or t.shape[1] > width:
            raise ValueError(f"gather_padded: every utterance must be a float32 (C={C}, len <= {width}) tensor with unit "
                             f"time stride on {first.device}; got {tuple(t.shape)} {t.dtype} strides {t.stride()}")
    if out is None:
        out = torch.empty((B, C, width), dtype=torch.float32, device=first.device)
    elif tuple(out.shape) != (B, C, width) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != first.device:
        raise ValueError(f"out must be a contiguous float32 {(B, C, width)} tensor on {first.device}")
    src = (ctypes.c_void_p * B)(*[t.data_ptr() for t in rows])
    lens = (ctypes.c_int32 * B)(*[int(t.shape[1]) for t in rows])
    pitches = (ctypes.c_int32 * B)(*[int(t.stride(0)) if t.shape[0] > 1 else max(int(t.shape[1]), 1) for t in rows])
    with torch.cuda.device(first.device):
        stream = torch.cuda.current_stream(first.device).cuda_stream
        _check(lib, lib.fastsvc_gather_padded(src, lens, pitches, ctypes.c_void_p(out.data_ptr()), B, C, width,
                                              ctypes.c_void_p(stream)), "fastsvc_gather_padded")
    return out


def gather_time_major(packed: torch.Tensor, offsets: Sequence[int], lens: Sequence[int], C: int, width: int,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Assemble a zero-padded channel-major batch from time-major blocks: utterance b is the contiguous (lens[b], C)
    float32 block that starts ``offsets[b]`` elements into ``packed`` (a 1-D device tensor - the dump layout, blocks back to
    back) -> (B, C, width), transposed, every column >= lens[b] zero.  No alignment or % 4 requirement.  One HIP launch per
    64 utterances on the current stream (fastsvc_gather_time_major, csrc/fastsvc_decodeio.hip); fails loudly off the GPU."""
    lib = load_library()
    if not isinstance(packed, torch.Tensor) or not packed.is_cuda:
        raise FastSVCError("gather_time_major needs a GPU tensor (no CPU fallback); got " +
                           str(getattr(packed, "device", type(packed))))
    B, C, width = len(lens), int(C), int(width)
    if B == 0 or len(offsets) != B:
        raise ValueError("gather_time_major needs at least one utterance and one offset per length")
    if packed.dim() != 1 or packed.dtype != torch.float32 or not packed.is_contiguous():
        raise ValueError("packed must be a contiguous 1-D float32 tensor")
    if out is None:
        out = torch.empty((B, C, width), dtype=torch.float32, device=packed.device)
    elif tuple(out.shape) != (B, C, width) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != packed.device:
        raise ValueError(f"out must be a contiguous float32 {(B, C, width)} tensor on {packed.device}")
    offs, ls = _ints(ctypes.c_int64, offsets), _ints(ctypes.c_int32, lens)
    with torch.cuda.device(packed.device):
        stream = torch.cuda.current_stream(packed.device).cuda_stream
        _check(lib, lib.fastsvc_gather_time_major(_ptr(packed), packed.numel(), offs, ls, _ptr(out), B, C, width,
                                                  ctypes.c_void_p(stream)), "fastsvc_gather_time_major")
    return out


def _report_tensor(report, B: int, device) -> torch.Tensor:
    if not isinstance(report, torch.Tensor) or not report.is_cuda:
        raise FastSVCError("the report must be a GPU tensor (no CPU fallback); got " + str(getattr(report, "device", type(report))))
    if tuple(report.shape) != (B, 4) or report.dtype != torch.int32 or not report.is_contiguous() or report.device != device:
        raise ValueError(f"report must be a contiguous int32 {(B, 4)} tensor on {device}")
    return report


def output_check(y: torch.Tensor, lens: Sequence[int], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """What a PCM-16 conversion of ``y`` would hide, per row: -> (B, 4) int32 on the device, row b the
    ``fastsvc_row_report`` of ``y[b, :lens[b]]`` - non-finite samples, finite samples whose PCM-16 value saturates, the
    bit pattern of the largest finite ``|y|`` (float32), 0.  ``report_arrays`` decodes a downloaded one;
    ``decode.output_report`` is the host's version.  ``y`` as for ``pcm16_pack``; ``out``: a (B, 4) int32 tensor to
    overwrite.  One memset and one HIP launch per 64 rows on the current stream (fastsvc_output_check); fails loudly
    off the GPU."""
    lib = load_library()
    if not isinstance(y, torch.Tensor) or not y.is_cuda:
        raise FastSVCError("output_check needs a GPU tensor (no CPU fallback); got " + str(getattr(y, "device", type(y))))
    if y.dim() == 3 and y.shape[1] == 1:
        y = y[:, 0]
    if y.dim() != 2 or y.dtype != torch.float32 or not y.is_contiguous() or y.shape[0] != len(lens) or y.shape[0] == 0:
        raise ValueError(f"y must be a contiguous float32 (B, width) tensor with one length per row; got {tuple(y.shape)} {y.dtype}")
    B, width = int(y.shape[0]), int(y.shape[1])
    report = torch.empty((B, 4), dtype=torch.int32, device=y.device) if out is None else _report_tensor(out, B, y.device)
    ls = _ints(ctypes.c_int32, lens)
    with torch.cuda.device(y.device):
        stream = torch.cuda.current_stream(y.device).cuda_stream
        _check(lib, lib.fastsvc_output_check(_ptr(y), ls, _ptr(report), B, width, ctypes.c_void_p(stream)), "fastsvc_output_check")
    return report


def report_arrays(report) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """A downloaded (B, 4) int32 report (``output_check``, ``pcm16_pack(report=)``; tensor or array) ->
    ``(nonfinite, clipped, max_abs)``: int32, int32 and - column 2 reinterpreted - float32 arrays of B entries."""
    if isinstance(report, torch.Tensor):
        report = report.detach().cpu().numpy()
    r = np.ascontiguousarray(report, dtype=np.int32).reshape(-1, 4)
    return r[:, 0].copy(), r[:, 1].copy(), r[:, 2].copy().view(np.float32)


def pcm16_pack(y: torch.Tensor, lens: Sequence[int], offsets: Optional[Sequence[int]] = None,
               out: Optional[torch.Tensor] = None, report: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PCM-16 of a batch of waveforms, packed: row b of ``y`` (B, width) or (B, 1, width), float32 on the device, valid for
    ``lens[b]`` samples, goes to ``out[offsets[b]: offsets[b] + lens[b]]`` (1-D int16; default offsets: the rows back to
    back, default out: a new tensor of sum(lens) samples).  The values are ``decode.to_pcm16``'s bit for bit (float64
    product, round half to even, saturated; NaN -> 0); samples of ``out`` outside the rows are left as they are.  One HIP
    launch per 64 rows on the current stream (fastsvc_pcm16_pack, csrc/fastsvc_decodeio.hip); fails loudly off the GPU.

    ``report``: a (B, 4) int32 device tensor; when given, the checked entry point runs instead
    (fastsvc_pcm16_pack_checked: the same bytes into ``out`` from the same pass, plus one memset) and overwrites it with
    the rows' ``fastsvc_row_report`` (see ``output_check``)."""
    lib = load_library()
    if not isinstance(y, torch.Tensor) or not y.is_cuda:
        raise FastSVCError("pcm16_pack needs a GPU tensor (no CPU fallback); got " + str(getattr(y, "device", type(y))))
    if y.dim() == 3 and y.shape[1] == 1:
        y = y[:, 0]
    if y.dim() != 2 or y.dtype != torch.float32 or not y.is_contiguous() or y.shape[0] != len(lens) or y.shape[0] == 0:
        raise ValueError(f"y must be a contiguous float32 (B, width) tensor with one length per row; got {tuple(y.shape)} {y.dtype}")
    B, width = int(y.shape[0]), int(y.shape[1])
    lens = [int(v) for v in lens]
    if offsets is None:
        offsets = [0] * B
        for b in range(1, B):
            offsets[b] = offsets[b - 1] + lens[b - 1]
    elif len(offsets) != B:
        raise ValueError("pcm16_pack needs one offset per row")
    if out is None:
        out = torch.empty(max(int(o) + n for o, n in zip(offsets, lens)), dtype=torch.int16, device=y.device)
    elif out.dim() != 1 or out.dtype != torch.int16 or not out.is_contiguous() or out.device != y.device:
        raise ValueError(f"out must be a contiguous 1-D int16 tensor on {y.device}")
    if report is not None:
        _report_tensor(report, B, y.device)
    if out.numel() == 0:
        if report is not None:
            report.zero_()
        return out
    offs, ls = _ints(ctypes.c_int64, offsets), _ints(ctypes.c_int32, lens)
    with torch.cuda.device(y.device):
        stream = torch.cuda.current_stream(y.device).cuda_stream
        if report is not None:
            _check(lib, lib.fastsvc_pcm16_pack_checked(_ptr(y), ls, offs, _ptr(out), out.numel(), _ptr(report), B, width,
                                                       ctypes.c_void_p(stream)), "fastsvc_pcm16_pack_checked")
            return out
        _check(lib, lib.fastsvc_pcm16_pack(_ptr(y), ls, offs, _ptr(out), out.numel(), B, width, ctypes.c_void_p(stream)),
               "fastsvc_pcm16_pack")
    return out


def collate_launch_count(B: int) -> int:
    """Launches one ``collate_crops`` of B rows enqueues: one per 64 rows."""
    return int(load_library().fastsvc_collate_launch_count(int(B)))


def collate_crops(wave: torch.Tensor, lft: torch.Tensor, ppg: torch.Tensor, f0: torch.Tensor, emb: Optional[torch.Tensor],
                  frame_off: Sequence[int], n_frames: Sequence[int], utt: Sequence[int], start: Sequence[int],
                  D: int, hop: int, frames: int, ctx: int = 0, out: Optional[Sequence[Optional[torch.Tensor]]] = None):
    """Cut a training batch out of a resident corpus: the reference Collater's slices (train_fastsvc.py:500-543), bit for
    bit, by ONE HIP launch per 64 rows on the current stream (fastsvc_collate_crops, csrc/fastsvc_collate.hip).

    ``wave``, ``lft``, ``ppg``, ``f0`` are the packed 1-D float32 device buffers of the store (utterance u: ``n_frames[u]``
    frames from frame ``frame_off[u]``; ppg time-major (n, D), wave / lft ``hop`` samples per frame), ``emb`` (U, S) or None.
    Row b is utterance ``utt[b]`` from frame ``start[b]``, ``ctx <= start[b] <= n_frames - frames - ctx``.  Returns
    ``(y (B, 1, T), lft (B, 1, T), ppg (B, D, frames + 2 ctx), f0 (B, 1, frames), emb (B, S) or None)``; ``out``: the same
    five, contiguous float32 tensors to write into (views of larger buffers are fine).  Anything out of range raises
    ``ValueError`` before a launch; fails loudly off the GPU."""
    lib = load_library()
    for name, t in (("wave", wave), ("lft", lft), ("ppg", ppg), ("f0", f0)) + ((("emb", emb),) if emb is not None else ()):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise FastSVCError(f"collate_crops needs GPU tensors (no CPU fallback); {name} is on " +
                               str(getattr(t, "device", type(t))))
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != wave.device or t.dim() != (2 if name == "emb" else 1):
            raise ValueError(f"{name} must be a contiguous float32 {'(U, S)' if name == 'emb' else '1-D'} tensor on {wave.device}")
    if lft.numel() != wave.numel():
        raise ValueError("wave and lft must hold the same number of samples")
    B, U = len(utt), len(n_frames)
    D, hop, frames, ctx = int(D), int(hop), int(frames), int(ctx)
    if B == 0 or len(start) != B or U == 0 or len(frame_off) != U:
        raise ValueError("collate_crops needs at least one row, one start per row and one offset per stored utterance")
    if emb is not None and emb.shape[0] != U:
        raise ValueError(f"emb must hold one row per stored utterance ({U}), got {tuple(emb.shape)}")
    S = int(emb.shape[1]) if emb is not None else 0
    T, W = frames * hop, frames + 2 * ctx
    shapes = [(B, 1, T), (B, 1, T), (B, D, W), (B, 1, frames), (B, S)]
    if out is None:
        out = [None] * 5
    outs = []
    for i, shp in enumerate(shapes):
        t = out[i] if i < len(out) else None
        if i == 4 and emb is None:
            outs.append(None)
        elif t is None:
            outs.append(torch.empty(shp, dtype=torch.float32, device=wave.device))
        elif not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise FastSVCError("collate_crops needs GPU tensors (no CPU fallback) for out")
        elif tuple(t.shape) != shp or t.dtype != torch.float32 or not t.is_contiguous() or t.device != wave.device:
            raise ValueError(f"out[{i}] must be a contiguous float32 {shp} tensor on {wave.device}")
        else:
            outs.append(t)
    # (a session hands in the ctypes arrays it made once: a corpus has thousands of entries, a batch a few dozen)
    offs, nfr = _ints(ctypes.c_int64, frame_off), _ints(ctypes.c_int32, n_frames)
    us, st = _ints(ctypes.c_int32, utt), _ints(ctypes.c_int32, start)
    with torch.cuda.device(wave.device):
        stream = torch.cuda.current_stream(wave.device).cuda_stream
        _check(lib, lib.fastsvc_collate_crops(_ptr(wave), _ptr(lft), wave.numel(), _ptr(ppg), ppg.numel(), _ptr(f0), f0.numel(),
                                              _ptr(emb), U, offs, nfr, us, st, *[_ptr(t) for t in outs],
                                              B, D, S, hop, frames, ctx, ctypes.c_void_p(stream)), "fastsvc_collate_crops")
    return tuple(outs)


def fanout_launch_count(R: int) -> int:
    """Launches one ``fanout_assemble`` of R rows enqueues: one per 64 rows."""
    return int(load_library().fastsvc_fanout_launch_count(int(R)))


def fanout_assemble(ppg: torch.Tensor, lft: torch.Tensor, f0: torch.Tensor, ppg_off: Sequence[int], lft_off: Sequence[int],
                    f0_off: Sequence[int], n_frames: Sequence[int], utt: Sequence[int], spk: Sequence[int],
                    C: int, hop: int, width: int, src_stats: Optional[torch.Tensor] = None,
                    spk_stats: Optional[torch.Tensor] = None, spk_emb: Optional[torch.Tensor] = None, n_spk: Optional[int] = None,
                    out: Optional[Sequence[Optional[torch.Tensor]]] = None):
    """Assemble a decode batch whose rows are (utterance, target speaker) pairs out of a resident session's packed
    buffers, by ONE HIP launch per 64 rows on the current stream (fastsvc_fanout_assemble, csrc/fastsvc_fanout.hip).

    ``ppg``, ``lft``, ``f0`` are packed 1-D float32 device buffers; utterance u has ``n_frames[u]`` frames, its time-major
    (n, C) ppg block at element ``ppg_off[u]``, its n * hop lft samples at ``lft_off[u]`` and its n f0 values at
    ``f0_off[u]``.  Row r is utterance ``utt[r]`` for speaker ``spk[r]``.  Returns ``(ppg (R, C, width), lft (R, 1, width *
    hop), f0 (R, 1, width), emb (R, E) or None)``: ppg with ``gather_time_major``'s bits, lft with ``gather_padded``'s, f0
    moved from ``src_stats[utt]`` to ``spk_stats[spk]`` (device float64 tables (U, 2) and (S, 2) of [mean, std];
    ``decode.F0Statistics.convert`` in double precision, within one float32 ulp; unvoiced and padded frames exactly 0;
    copied bit for bit when either table is None) and row ``spk`` of ``spk_emb`` (S, E) (None: no embedding is returned).
    ``n_spk``: the number of speakers when neither table is given (default: 1 + max(spk)).  ``out``: the same four,
    contiguous float32 tensors to write into.  Anything out of range raises ``ValueError`` before a launch; fails loudly
    off the GPU."""
    lib = load_library()
    named = [("ppg", ppg, torch.float32, 1), ("lft", lft, torch.float32, 1), ("f0", f0, torch.float32, 1)]
    named += [(n, t, torch.float64, 2) for n, t in (("src_stats", src_stats), ("spk_stats", spk_stats)) if t is not None]
    if spk_emb is not None:
        named.append(("spk_emb", spk_emb, torch.float32, 2))
    _gpu_tensors("fanout_assemble", ppg, named)
    R, U = len(utt), len(n_frames)
    C, hop, width = int(C), int(hop), int(width)
    if R == 0 or len(spk) != R or U == 0 or len(ppg_off) != U or len(lft_off) != U or len(f0_off) != U:
        raise ValueError("fanout_assemble needs at least one row, one speaker per row and three offsets per stored utterance")
    if src_stats is not None and tuple(src_stats.shape) != (U, 2):
        raise ValueError(f"src_stats must be ({U}, 2), got {tuple(src_stats.shape)}")
    tables = [int(t.shape[0]) for t in (spk_stats, spk_emb) if t is not None]
    if spk_stats is not None and spk_stats.shape[1] != 2:
        raise ValueError(f"spk_stats must be (S, 2), got {tuple(spk_stats.shape)}")
    if n_spk is None:
        n_spk = tables[0] if tables else 1 + max(int(v) for v in spk)
    n_spk = int(n_spk)
    if any(n != n_spk for n in tables):
        raise ValueError(f"spk_stats and spk_emb must hold one row per speaker ({n_spk})")
    E = int(spk_emb.shape[1]) if spk_emb is not None else 0
    shapes = [(R, C, width), (R, 1, width * hop), (R, 1, width), (R, E)]
    if out is None:
        out = [None] * 4
    outs = []
    for i, shp in enumerate(shapes):
        t = out[i] if i < len(out) else None
        if i == 3 and spk_emb is None:
            outs.append(None)
        elif t is None:
            outs.append(torch.empty(shp, dtype=torch.float32, device=ppg.device))
        elif not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise FastSVCError("fanout_assemble needs GPU tensors (no CPU fallback) for out")
        elif tuple(t.shape) != shp or t.dtype != torch.float32 or not t.is_contiguous() or t.device != ppg.device:
            raise ValueError(f"out[{i}] must be a contiguous float32 {shp} tensor on {ppg.device}")
        else:
            outs.append(t)
    # (a session hands in the ctypes arrays it made once)
    po, lo, fo = (_ints(ctypes.c_int64, v) for v in (ppg_off, lft_off, f0_off))
    nfr, us, ss = (_ints(ctypes.c_int32, v) for v in (n_frames, utt, spk))
    with torch.cuda.device(ppg.device):
        stream = torch.cuda.current_stream(ppg.device).cuda_stream
        _check(lib, lib.fastsvc_fanout_assemble(_ptr(ppg), ppg.numel(), _ptr(lft), lft.numel(), _ptr(f0), f0.numel(), U,
                                                po, lo, fo, nfr, _ptr(src_stats), _ptr(spk_stats), _ptr(spk_emb), n_spk, us, ss,
                                                *[_ptr(t) for t in outs], R, C, E, hop, width, ctypes.c_void_p(stream)),
               "fastsvc_fanout_assemble")
    return tuple(outs)


def window_launch_count(R: int) -> int:
    """Launches one ``window_assemble`` (or ``window_stitch``) of R rows enqueues: one per 64 rows."""
    return int(load_library().fastsvc_window_launch_count(int(R)))


def window_assemble(ppg: torch.Tensor, lft: torch.Tensor, sine: torch.Tensor, ppg_off: Sequence[int], sig_off: Sequence[int],
                    n_frames: Sequence[int], C: int, hop: int, width: int,
                    out: Optional[Sequence[Optional[torch.Tensor]]] = None):
    """Assemble a decode batch whose rows are SLICES of utterances - the windows of ``DecodeSession.convert_windowed`` -
    out of packed buffers, by ONE HIP launch per 64 rows on the current stream (fastsvc_window_assemble,
    csrc/fastsvc_window.hip).

    ``ppg``, ``lft``, ``sine`` are packed 1-D float32 device buffers, ``lft`` and ``sine`` of one size and layout.  Row r is
    ``n_frames[r]`` frames: the time-major (n, C) ppg slice at element ``ppg_off[r]`` and the n * hop samples of ``lft`` and
    ``sine`` at element ``sig_off[r]``.  Returns ``(ppg (R, C, width), lft (R, 1, width * hop), sine (R, 1, width * hop))``:
    the ppg slice transposed (``gather_time_major``'s bits), the samples copied bit for bit, everything past a row's
    length exactly zero.  No alignment requirement on the offsets.  ``out``: the same three, contiguous float32 tensors to
    write into.  Anything out of range raises ``ValueError`` before a launch; fails loudly off the GPU."""
    lib = load_library()
    for name, t in (("ppg", ppg), ("lft", lft), ("sine", sine)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise FastSVCError(f"window_assemble needs GPU tensors (no CPU fallback); {name} is on " +
                               str(getattr(t, "device", type(t))))
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != ppg.device or t.dim() != 1:
            raise ValueError(f"{name} must be a contiguous 1-D float32 tensor on {ppg.device}")
    if lft.numel() != sine.numel():
        raise ValueError("lft and sine must hold the same number of samples")
    R = len(n_frames)
    C, hop, width = int(C), int(hop), int(width)
    if R == 0 or len(ppg_off) != R or len(sig_off) != R:
        raise ValueError("window_assemble needs at least one row and two offsets per row")
    shapes = [(R, C, width), (R, 1, width * hop), (R, 1, width * hop)]
    if out is None:
        out = [None] * 3
    outs = []
    for i, shp in enumerate(shapes):
        t = out[i] if i < len(out) else None
        if t is None:
            outs.append(torch.empty(shp, dtype=torch.float32, device=ppg.device))
        elif not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise FastSVCError("window_assemble needs GPU tensors (no CPU fallback) for out")
        elif tuple(t.shape) != shp or t.dtype != torch.float32 or not t.is_contiguous() or t.device != ppg.device:
            raise ValueError(f"out[{i}] must be a contiguous float32 {shp} tensor on {ppg.device}")
        else:
            outs.append(t)
    po, so, nfr = _ints(ctypes.c_int64, ppg_off), _ints(ctypes.c_int64, sig_off), _ints(ctypes.c_int32, n_frames)
    with torch.cuda.device(ppg.device):
        stream = torch.cuda.current_stream(ppg.device).cuda_stream
        _check(lib, lib.fastsvc_window_assemble(_ptr(ppg), ppg.numel(), _ptr(lft), _ptr(sine), lft.numel(), po, so, nfr,
                                                *[_ptr(t) for t in outs], R, C, hop, width, ctypes.c_void_p(stream)),
               "fastsvc_window_assemble")
    return tuple(outs)


# a side of a window row in ``window_stitch`` (include/fastsvc_hip.h)
STITCH_NONE, STITCH_STAGE, STITCH_FROM_STAGE, STITCH_FROM_Y, STITCH_SKIP = range(5)


def window_stitch(y: torch.Tensor, n_samples: Sequence[int], core_lo: Sequence[int], core_hi: Sequence[int], half: int,
                  left_mode: Sequence[int], right_mode: Sequence[int], left_src: Sequence[int], right_src: Sequence[int],
                  dst_off: Sequence[int], stage: Optional[torch.Tensor] = None, out_pcm: Optional[torch.Tensor] = None,
                  out_float: Optional[torch.Tensor] = None, utt: Optional[Sequence[int]] = None,
                  report: Optional[torch.Tensor] = None) -> None:
    """Cross-fade the window rows ``y`` (B, width) or (B, 1, width), float32 on the device, into packed destinations:
    row r writes one contiguous run to element ``dst_off[r]`` of ``out_pcm`` (1-D int16) and / or ``out_float`` (1-D
    float32, the same length).  The arguments are those of ``fastsvc_window_stitch`` (include/fastsvc_hip.h), which
    ``decode.stitch_layout`` computes: the core ``[core_lo[r], core_hi[r])`` of the row in samples, ``half`` = half a fade
    zone in samples, a mode per side (``STITCH_*``) with the zone's source in ``stage`` (1-D float32, kept between the
    calls of one pass) or in ``y``.  The values are ``decode.stitch_windows``' (float64 cross-fade) and ``to_pcm16``'s, bit
    for bit.  ``report``: an (n_utts, 4) int32 device tensor the written samples are ACCUMULATED into at row ``utt[r]``
    (clear it before an utterance's first window).  One HIP launch per 64 rows on the current stream
    (csrc/fastsvc_window.hip); anything out of range raises ``ValueError`` before a launch; fails loudly off the GPU."""
    lib = load_library()
    if not isinstance(y, torch.Tensor) or not y.is_cuda:
        raise FastSVCError("window_stitch needs a GPU tensor (no CPU fallback); got " + str(getattr(y, "device", type(y))))
    if y.dim() == 3 and y.shape[1] == 1:
        y = y[:, 0]
    B = len(n_samples)
    if y.dim() != 2 or y.dtype != torch.float32 or not y.is_contiguous() or y.shape[0] != B or B == 0:
        raise ValueError(f"y must be a contiguous float32 (B, width) tensor with one length per row; got {tuple(y.shape)} {y.dtype}")
    per_row = (core_lo, core_hi, left_mode, right_mode, left_src, right_src, dst_off) + ((utt,) if report is not None else ())
    if any(v is None or len(v) != B for v in per_row):
        raise ValueError("window_stitch needs one entry per row in every row array")
    if out_pcm is None and out_float is None:
        raise ValueError("window_stitch needs out_pcm or out_float")
    n_dst = None
    for name, t, dtype in (("out_pcm", out_pcm, torch.int16), ("out_float", out_float, torch.float32), ("stage", stage, torch.float32)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise FastSVCError(f"window_stitch needs GPU tensors (no CPU fallback); {name} is on " + str(getattr(t, "device", type(t))))
        if t.dim() != 1 or t.dtype != dtype or not t.is_contiguous() or t.device != y.device:
            raise ValueError(f"{name} must be a contiguous 1-D {dtype} tensor on {y.device}")
        if name != "stage":
            if n_dst is not None and n_dst != t.numel():
                raise ValueError("out_pcm and out_float must hold the same number of samples")
            n_dst = t.numel()
    n_utts = 0
    if report is not None:
        n_utts = int(report.shape[0]) if isinstance(report, torch.Tensor) and report.dim() == 2 else 0
        _report_tensor(report, n_utts, y.device)
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    ptr = lambda t: _ptr(t) if t is not None and t.numel() else None      # (an empty tensor goes in as the null pointer)  # noqa: E731
    with torch.cuda.device(y.device):
        stream = torch.cuda.current_stream(y.device).cuda_stream
        _check(lib, lib.fastsvc_window_stitch(ptr(y), B, int(y.shape[1]), _ints(i32, n_samples), _ints(i32, core_lo),
                                              _ints(i32, core_hi), int(half), _ints(i32, left_mode), _ints(i32, right_mode),
                                              _ints(i64, left_src), _ints(i64, right_src),
                                              ptr(stage), stage.numel() if stage is not None else 0, _ints(i64, dst_off),
                                              ptr(out_pcm), ptr(out_float), n_dst,
                                              _ints(i32, utt) if report is not None else None, ptr(report), n_utts,
                                              ctypes.c_void_p(stream)), "fastsvc_window_stitch")


def stream_launch_count(R: int) -> int:
    """Launches one ``stream_push`` of R streams (that append something) or ``stream_assemble`` of R rows enqueues: one
    per 64."""
    return int(load_library().fastsvc_stream_launch_count(int(R)))


STREAM_MAX_PUSH = 1024      # frames of one chunk the push kernel takes (their phase prefixes live in LDS)


def _stream_rings(who: str, ppg_ring, lft_ring, exc_ring):
    """The three rings of ``decode.StreamSession``: (n_streams, cap, C), (n_streams, cap * hop) twice -> (n_streams, cap, C, hop)."""
    for name, t in (("ppg_ring", ppg_ring), ("lft_ring", lft_ring), ("exc_ring", exc_ring)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise FastSVCError(f"{who} needs GPU tensors (no CPU fallback); {name} is on " + str(getattr(t, "device", type(t))))
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != ppg_ring.device:
            raise ValueError(f"{name} must be a contiguous float32 tensor on {ppg_ring.device}")
    if ppg_ring.dim() != 3 or lft_ring.dim() != 2 or exc_ring.shape != lft_ring.shape or lft_ring.shape[0] != ppg_ring.shape[0]:
        raise ValueError("the rings must be (n_streams, cap, C), (n_streams, cap * hop) and (n_streams, cap * hop)")
    n_streams, cap, C = (int(v) for v in ppg_ring.shape)
    if cap < 4 or cap % 4 or lft_ring.shape[1] % cap or lft_ring.shape[1] == 0:
        raise ValueError(f"the rings' capacity must be a multiple of 4 frames and divide the sample rings, got {cap}")
    return n_streams, cap, C, int(lft_ring.shape[1]) // cap


def stream_push(upload: torch.Tensor, streams: Sequence[int], n: Sequence[int], up_off: Sequence[int], pos: Sequence[int],
                first: Sequence[int], parity: Sequence[int], seed: Sequence[int], ppg_ring: torch.Tensor, lft_ring: torch.Tensor,
                exc_ring: Optional[torch.Tensor], phase: Optional[torch.Tensor], max_push: int, sample_rate: float,
                sine_amp: float, noise_amp: float) -> None:
    """Append chunks to the rings of live streams and synthesise their excitation, by ONE HIP launch per 64 streams on
    the current stream (fastsvc_stream_push, csrc/fastsvc_stream.hip; none when every chunk is empty).

    Entry i appends ``n[i]`` frames (``0 <= n[i] <= max_push``) to stream ``streams[i]`` (each at most once), which held
    ``pos[i]`` frames: from element ``up_off[i]`` of ``upload`` (1-D float32 on the device) the time-major ppg ``n x C``,
    then f0 ``n``, then lft ``n x hop``.  ``ppg_ring (n_streams, cap, C)``, ``lft_ring`` / ``exc_ring (n_streams, cap *
    hop)``: frame p of a stream at index ``p % cap``.  ``phase (n_streams, 2)`` float64: the push reads entry
    ``parity[i]`` (or starts at 0 when ``first[i]``) and writes entry ``parity[i] ^ 1``.  ``seed[i]`` keys the noise
    together with the absolute sample index.  ``exc_ring=None`` (and ``phase=None``): the slices hold NO f0 - ppg ``n x
    C``, then ``n x hop`` samples for ``lft_ring`` - and nothing is synthesised (``StreamSession(f0="audio")``, whose
    excitation ``stream_f0`` makes when the frames are final).  Anything out of range raises ``ValueError`` before a launch
    and changes nothing; fails loudly off the GPU."""
    lib = load_library()
    synth = exc_ring is not None
    if not synth and phase is not None:
        raise ValueError("stream_push without an exc_ring synthesises nothing: it takes no phase")
    n_streams, cap, C, hop = _stream_rings("stream_push", ppg_ring, lft_ring, exc_ring if synth else lft_ring)
    _gpu_tensors("stream_push", ppg_ring, (("upload", upload, torch.float32, 1),) + ((("phase", phase, torch.float64, 2),) if synth else ()))
    if synth and tuple(phase.shape) != (n_streams, 2):
        raise ValueError(f"phase must be ({n_streams}, 2), got {tuple(phase.shape)}")
    per_frame = C + (1 if synth else 0) + hop
    S = len(streams)
    max_push = int(max_push)
    if S == 0 or any(len(v) != S for v in (n, up_off, pos, first, parity, seed)):
        raise ValueError("stream_push needs at least one stream and one entry per stream in every array")
    if not 1 <= max_push <= min(cap, STREAM_MAX_PUSH):
        raise ValueError(f"max_push must be in [1, min(cap {cap}, {STREAM_MAX_PUSH})], got {max_push}")
    if len(set(int(s) for s in streams)) != S:
        raise ValueError("stream_push takes every stream at most once per call")
    for i in range(S):
        s, k, o = int(streams[i]), int(n[i]), int(up_off[i])
        if not 0 <= s < n_streams:
            raise ValueError(f"stream {s} outside [0, {n_streams})")
        if not 0 <= k <= max_push:
            raise ValueError(f"stream {s}: {k} frames, outside [0, max_push {max_push}]")
        if o < 0 or o + k * per_frame > upload.numel():
            raise ValueError(f"stream {s}: its slice [{o}, +{k * per_frame}) leaves the upload buffer of {upload.numel()} elements")
        if int(pos[i]) < 0:
            raise ValueError(f"stream {s}: position {int(pos[i])} out of range")
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    seeds = _ints(ctypes.c_uint64, [int(x) & 0xFFFFFFFFFFFFFFFF for x in seed])
    with torch.cuda.device(ppg_ring.device):
        stream = torch.cuda.current_stream(ppg_ring.device).cuda_stream
        _check(lib, lib.fastsvc_stream_push(_ptr(upload), upload.numel(), S, _ints(i32, streams), _ints(i32, n), _ints(i64, up_off),
                                            _ints(i64, pos), _ints(i32, [1 if v else 0 for v in first]),
                                            _ints(i32, [int(v) & 1 for v in parity]), seeds,
                                            _ptr(ppg_ring), _ptr(lft_ring), _ptr(exc_ring), _ptr(phase), n_streams, cap, max_push, C, hop,
                                            ctypes.c_float(float(sample_rate)), ctypes.c_float(float(sine_amp)),
                                            ctypes.c_float(float(noise_amp)), ctypes.c_void_p(stream)), "fastsvc_stream_push")


def stream_assemble(ppg_ring: torch.Tensor, lft_ring: torch.Tensor, exc_ring: torch.Tensor, pos: Sequence[int],
                    streams: Sequence[int], first_frame: Sequence[int], n_frames: Sequence[int], width: int,
                    out: Optional[Sequence[Optional[torch.Tensor]]] = None):
    """Assemble a decode batch whose rows are cut from the rings of live streams, by ONE HIP launch per 64 rows on the
    current stream (fastsvc_stream_assemble, csrc/fastsvc_stream.hip).  Row r is the ``n_frames[r]`` frames from frame
    ``first_frame[r]`` of stream ``streams[r]``, read modulo the rings' capacity; ``pos[s]`` is how many frames stream s
    holds.  Returns ``window_assemble``'s three: ``(ppg (R, C, width), lft (R, 1, width * hop), sine (R, 1, width *
    hop))``, everything past a row's length exactly zero.  ``out``: the same three, to write into.  A row outside the
    retained frames ``[pos - cap, pos)`` of its stream, or anything else out of range, raises ``ValueError`` before a
    launch; fails loudly off the GPU."""
    lib = load_library()
    n_streams, cap, C, hop = _stream_rings("stream_assemble", ppg_ring, lft_ring, exc_ring)
    R, width = len(n_frames), int(width)
    if R == 0 or len(streams) != R or len(first_frame) != R or len(pos) != n_streams or width < 1:
        raise ValueError("stream_assemble needs at least one row, a stream and a first frame per row, and a position per stream")
    for r in range(R):
        s, f, k = int(streams[r]), int(first_frame[r]), int(n_frames[r])
        if not 0 <= s < n_streams:
            raise ValueError(f"row {r}: stream {s} outside [0, {n_streams})")
        if not 0 <= k <= min(width, cap):
            raise ValueError(f"row {r} has {k} frames, outside [0, min(width {width}, cap {cap})]")
        p = int(pos[s])
        if f < 0 or f < p - cap or f + k > p:
            raise ValueError(f"row {r}: frames [{f}, {f + k}) are not retained by stream {s}, which holds [{max(0, p - cap)}, {p})")
    shapes = [(R, C, width), (R, 1, width * hop), (R, 1, width * hop)]
    if out is None:
        out = [None] * 3
    outs = []
    for i, shp in enumerate(shapes):
        t = out[i] if i < len(out) else None
        if t is None:
            outs.append(torch.empty(shp, dtype=torch.float32, device=ppg_ring.device))
        elif not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise FastSVCError("stream_assemble needs GPU tensors (no CPU fallback) for out")
        elif tuple(t.shape) != shp or t.dtype != torch.float32 or not t.is_contiguous() or t.device != ppg_ring.device:
            raise ValueError(f"out[{i}] must be a contiguous float32 {shp} tensor on {ppg_ring.device}")
        else:
            outs.append(t)
    ps, ff = _ints(ctypes.c_int64, pos), _ints(ctypes.c_int64, first_frame)
    st, nfr = _ints(ctypes.c_int32, streams), _ints(ctypes.c_int32, n_frames)
    with torch.cuda.device(ppg_ring.device):
        stream = torch.cuda.current_stream(ppg_ring.device).cuda_stream
        _check(lib, lib.fastsvc_stream_assemble(_ptr(ppg_ring), _ptr(lft_ring), _ptr(exc_ring), n_streams, cap, ps, st, ff, nfr,
                                                *[_ptr(t) for t in outs], R, C, hop, width, ctypes.c_void_p(stream)),
               "fastsvc_stream_assemble")
    return tuple(outs)


def stream_check(y: torch.Tensor, span_lo: Sequence[int], span_hi: Sequence[int], carry: Optional[torch.Tensor] = None,
                 slots: Optional[Sequence[int]] = None, entries: Optional[Sequence[int]] = None, entry_doubles: int = 0,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """What the window rows of a live-stream forward CONTRIBUTE, per row: -> (B, 4) int32 on the device, row r the
    ``fastsvc_row_report`` of ``y[r, span_lo[r]:span_hi[r]]`` (``decode.stream_check_spans`` gives the spans) - the bits
    ``output_check`` gives for that span as a row of its own - and, in the fourth word, the number of non-finite doubles
    among the ``entry_doubles`` doubles of entry ``entries[r]`` (0 or 1; -1: none, the word is 0) of slot ``slots[r]``'s
    record in ``carry``, a contiguous 2-D device tensor with one record per row (the running InstanceNorm carry of
    ``Model.forward(norm_running=)``: pass the entry the forward just wrote, ``parity ^ 1``).  ``y`` (B, width) or
    (B, 1, width), float32, contiguous; any ``0 <= lo <= hi <= width``.  ``out``: a (B, 4) int32 tensor to overwrite; every
    call overwrites with plain stores (no memset, no atomics).  One HIP launch per 64 rows on the current stream
    (fastsvc_stream_check, csrc/fastsvc_stream_check.hip); a bad span, slot or entry raises ``ValueError`` before
    anything is enqueued; fails loudly off the GPU."""
    lib = load_library()
    if not isinstance(y, torch.Tensor) or not y.is_cuda:
        raise FastSVCError("stream_check needs a GPU tensor (no CPU fallback); got " + str(getattr(y, "device", type(y))))
    if y.dim() == 3 and y.shape[1] == 1:
        y = y[:, 0]
    if y.dim() != 2 or y.dtype != torch.float32 or not y.is_contiguous() or y.shape[0] == 0 or \
            len(span_lo) != y.shape[0] or len(span_hi) != y.shape[0]:
        raise ValueError(f"y must be a contiguous float32 (B, width) tensor with one span per row; got {tuple(y.shape)} {y.dtype}")
    B, width = int(y.shape[0]), int(y.shape[1])
    if (slots is None) != (entries is None) or (entries is not None and (len(slots) != B or len(entries) != B)):
        raise ValueError("stream_check needs slots and entries together, one of each per row")
    carry_bytes = n_slots = 0
    if carry is not None:
        if not isinstance(carry, torch.Tensor) or not carry.is_cuda:
            raise FastSVCError("stream_check needs a GPU tensor (no CPU fallback) for carry")
        if carry.dim() != 2 or not carry.is_contiguous() or carry.device != y.device:
            raise ValueError(f"carry must be a contiguous 2-D tensor on {y.device}, one record per row")
        n_slots, carry_bytes = int(carry.shape[0]), int(carry.shape[1]) * carry.element_size()
    report = torch.empty((B, 4), dtype=torch.int32, device=y.device) if out is None else _report_tensor(out, B, y.device)
    lo, hi = _ints(ctypes.c_int32, span_lo), _ints(ctypes.c_int32, span_hi)
    sl = None if slots is None else _ints(ctypes.c_int32, slots)
    en = None if entries is None else _ints(ctypes.c_int32, entries)
    with torch.cuda.device(y.device):
        stream = torch.cuda.current_stream(y.device).cuda_stream
        _check(lib, lib.fastsvc_stream_check(_ptr(y), B, width, lo, hi, _ptr(carry), carry_bytes, int(entry_doubles), n_slots,
                                             sl, en, _ptr(report), ctypes.c_void_p(stream)), "fastsvc_stream_check")
    return report


STREAM_LOUDNESS_MAX_FRAMES = 2048      # frames of one stream a stream_loudness call finalises


def stream_loudness_scratch_bytes(n_streams: int, max_frames: int) -> int:
    """Bytes of the scratch ``stream_loudness`` needs for ``n_streams`` slots that finalise at most ``max_frames`` frames
    each per call: their power rows and maxima."""
    return int(load_library().fastsvc_stream_loudness_scratch_bytes(int(n_streams), int(max_frames)))


def stream_loudness(audio_ring: torch.Tensor, lft_ring: torch.Tensor, peak: torch.Tensor, scratch: torch.Tensor,
                    streams: Sequence[int], first_frame: Sequence[int], n: Sequence[int], seen: Sequence[int],
                    ended: Sequence[int], parity: Sequence[int], cap: int, max_frames: int, sample_rate: float) -> None:
    """The A-weighted log loudness of the frames of live streams that have become final, from their audio rings into
    their lft rings, by TWO HIP launches per 64 streams on the current stream (fastsvc_stream_loudness,
    csrc/fastsvc_stream_loudness.hip; none when every ``n[i]`` is 0).

    ``audio_ring`` and ``lft_ring`` are ``(n_streams, cap * hop)``: sample p of a stream's audio at index ``p % (cap *
    hop)`` (``stream_push`` appends it, handed the audio ring as its lft ring), the loudness of frame f at frame index ``f
    % cap``.  Entry i finalises the ``n[i]`` frames (``0 <= n[i] <= max_frames``) from ``first_frame[i]`` of stream
    ``streams[i]`` (each at most once), of which ``seen[i]`` frames have arrived; ``ended[i]``: they are the stream's last,
    with reflection at its end.  ``peak (n_streams, 2)`` float32 carries the running maximum the 80 dB floor hangs under:
    the call reads entry ``parity[i]`` (or starts from 0 when ``first_frame[i] == 0``) and writes entry ``parity[i] ^ 1``.
    ``scratch``: ``stream_loudness_scratch_bytes(n_streams, max_frames)`` bytes.  Anything out of range raises
    ``ValueError`` before a launch and changes nothing; fails loudly off the GPU."""
    lib = load_library()
    _gpu_tensors("stream_loudness", audio_ring, (("audio_ring", audio_ring, torch.float32, 2), ("lft_ring", lft_ring, torch.float32, 2),
                                                 ("peak", peak, torch.float32, 2), ("scratch", scratch, torch.uint8, 1)))
    n_streams, cap, max_frames = int(audio_ring.shape[0]), int(cap), int(max_frames)
    if cap < 4 or cap % 4 or audio_ring.shape[1] == 0 or audio_ring.shape[1] % cap or lft_ring.shape != audio_ring.shape:
        raise ValueError(f"the rings must both be (n_streams, cap * hop) with cap {cap} a multiple of 4, got "
                         f"{tuple(audio_ring.shape)} and {tuple(lft_ring.shape)}")
    hop = int(audio_ring.shape[1]) // cap
    if tuple(peak.shape) != (n_streams, 2):
        raise ValueError(f"peak must be ({n_streams}, 2), got {tuple(peak.shape)}")
    if not 1 <= max_frames <= min(cap, STREAM_LOUDNESS_MAX_FRAMES):
        raise ValueError(f"max_frames must be in [1, min(cap {cap}, {STREAM_LOUDNESS_MAX_FRAMES})], got {max_frames}")
    if scratch.numel() < stream_loudness_scratch_bytes(n_streams, max_frames):
        raise ValueError(f"scratch holds {scratch.numel()} bytes, {stream_loudness_scratch_bytes(n_streams, max_frames)} are needed")
    S = len(streams)
    if S == 0 or any(len(v) != S for v in (first_frame, n, seen, ended, parity)):
        raise ValueError("stream_loudness needs at least one stream and one entry per stream in every array")
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    with torch.cuda.device(audio_ring.device):
        stream = torch.cuda.current_stream(audio_ring.device).cuda_stream
        _check(lib, lib.fastsvc_stream_loudness(_ptr(audio_ring), _ptr(lft_ring), _ptr(peak), _ptr(scratch), S, _ints(i32, streams),
                                                _ints(i64, first_frame), _ints(i32, n), _ints(i64, seen),
                                                _ints(i32, [1 if v else 0 for v in ended]),
                                                _ints(i32, [int(v) & 1 for v in parity]), n_streams, cap, max_frames, hop,
                                                ctypes.c_float(float(sample_rate)), ctypes.c_void_p(stream)),
               "fastsvc_stream_loudness")


F0_MAX_LAG = 1024           # the largest lag: half the 2048-sample frame


def f0_lags(sample_rate: float, f0_floor: float = 70.0, f0_ceil: float = 340.0) -> Tuple[int, int]:
    """The lags the YIN estimator searches, ``(tau_min, tau_max) = (floor(sr / f0_ceil), ceil(sr / f0_floor))`` with the
    three taken as float32 (what the kernels get): (70, 343) at 24 kHz with the defaults.  ``ValueError`` unless ``1 <=
    tau_min <= tau_max <= 1024`` - the frame is 2048 samples and the difference function sums over ``2048 - tau_max``.  Host
    arithmetic only: fastsvc_f0_lags (csrc/fastsvc_f0.hip) computes the same two and refuses the same."""
    sr, lo, hi = (float(np.float32(v)) for v in (sample_rate, f0_floor, f0_ceil))
    if not (sr > 0.0 and lo > 0.0 and hi >= lo and sr / lo < 1e6):
        raise ValueError(f"F0 search range needs sample_rate > 0 and 0 < f0_floor <= f0_ceil, got {sample_rate}, {f0_floor}, {f0_ceil}")
    tau_min, tau_max = int(math.floor(sr / hi)), int(math.ceil(sr / lo))
    if tau_min < 1 or tau_max > F0_MAX_LAG or tau_min > tau_max:
        raise ValueError(f"F0 lags [{tau_min}, {tau_max}] outside [1, {F0_MAX_LAG}]: f0_ceil {f0_ceil} above the sample rate, or "
                         f"f0_floor {f0_floor} below sample_rate / {F0_MAX_LAG}")
    return tau_min, tau_max


def _stream_f0_args(who: str, audio_ring, f0_ring, f0s_ring, exc_ring, phase, streams, first_frame, n, seen, ended, parity, seed,
                    stats, cap: int, max_frames: int, sample_rate: float, f0_floor: float, f0_ceil: float):
    """What ``stream_f0`` and ``stream_f0_running`` check on the host, and the arguments the two entry points share from ``S``
    to ``stats`` and from ``n_streams`` to ``hop``: -> (S .. stats as ctypes, (n_streams, cap, max_frames, hop))."""
    _gpu_tensors(who, audio_ring, (("audio_ring", audio_ring, torch.float32, 2), ("f0_ring", f0_ring, torch.float32, 2),
                                   ("f0s_ring", f0s_ring, torch.float32, 2), ("exc_ring", exc_ring, torch.float32, 2),
                                   ("phase", phase, torch.float64, 2)))
    n_streams, cap, max_frames = int(audio_ring.shape[0]), int(cap), int(max_frames)
    if cap < 4 or cap % 4 or audio_ring.shape[1] == 0 or audio_ring.shape[1] % cap or exc_ring.shape != audio_ring.shape:
        raise ValueError(f"audio_ring and exc_ring must both be (n_streams, cap * hop) with cap {cap} a multiple of 4, got "
                         f"{tuple(audio_ring.shape)} and {tuple(exc_ring.shape)}")
    hop = int(audio_ring.shape[1]) // cap
    if tuple(f0_ring.shape) != (n_streams, cap) or tuple(f0s_ring.shape) != (n_streams, cap) or tuple(phase.shape) != (n_streams, 2):
        raise ValueError(f"f0_ring and f0s_ring must be ({n_streams}, {cap}) and phase ({n_streams}, 2)")
    if not 1 <= max_frames <= min(cap, STREAM_LOUDNESS_MAX_FRAMES):
        raise ValueError(f"max_frames must be in [1, min(cap {cap}, {STREAM_LOUDNESS_MAX_FRAMES})], got {max_frames}")
    f0_lags(sample_rate, f0_floor, f0_ceil)
    S = len(streams)
    if S == 0 or any(len(v) != S for v in (first_frame, n, seen, ended, parity, seed, stats)):
        raise ValueError(f"{who} needs at least one stream and one entry per stream in every array")
    flat = []
    for st in stats:
        flat += [float("nan")] * 4 if st is None else [float(v) for v in st]
    if len(flat) != 4 * S:
        raise ValueError("stats entries are (m0, s0, m1, s1) or None")
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    per = (S, _ints(i32, streams), _ints(i64, first_frame), _ints(i32, n), _ints(i64, seen),
           _ints(i32, [1 if v else 0 for v in ended]), _ints(i32, [int(v) & 1 for v in parity]),
           _ints(ctypes.c_uint64, [int(x) & 0xFFFFFFFFFFFFFFFF for x in seed]), (ctypes.c_double * len(flat))(*flat))
    return per, (n_streams, cap, max_frames, hop)


def stream_f0(audio_ring: torch.Tensor, f0_ring: torch.Tensor, f0s_ring: torch.Tensor, exc_ring: torch.Tensor, phase: torch.Tensor,
              streams: Sequence[int], first_frame: Sequence[int], n: Sequence[int], seen: Sequence[int], ended: Sequence[int],
              parity: Sequence[int], seed: Sequence[int], stats: Sequence[Optional[Sequence[float]]], cap: int, max_frames: int,
              sample_rate: float, f0_floor: float, f0_ceil: float, threshold: float, sine_amp: float, noise_amp: float) -> None:
    """The F0 (YIN, ``f0_extract``'s function frame by frame), its Gaussian log-F0 shift and the excitation of the frames of
    live streams that have become final, from their audio rings, by TWO HIP launches per 64 streams on the current stream
    (fastsvc_stream_f0, csrc/fastsvc_stream_f0.hip; none when every ``n[i]`` is 0).

    ``audio_ring`` and ``exc_ring`` are ``(n_streams, cap * hop)``, ``f0_ring`` (raw) and ``f0s_ring`` (shifted) ``(n_streams,
    cap)``: frame f at index ``f % cap``.  Entry i takes the ``n[i]`` frames from ``first_frame[i]`` of stream ``streams[i]``
    with ``seen[i]`` frames arrived and ``ended[i]`` - ``stream_loudness``'s entries.  ``stats[i]``: ``(m0, s0, m1, s1)``, the
    source's and the target's mean and std of log F0, or None for no shift.  ``phase (n_streams, 2)`` float64: read at entry
    ``parity[i]`` (or started at 0 when ``first_frame[i] == 0``), written at ``parity[i] ^ 1``; ``seed[i]`` keys the noise with
    the absolute sample index.  Anything out of range raises ``ValueError`` before a launch and changes nothing; fails loudly
    off the GPU."""
    lib = load_library()
    per, dims = _stream_f0_args("stream_f0", audio_ring, f0_ring, f0s_ring, exc_ring, phase, streams, first_frame, n, seen, ended,
                                parity, seed, stats, cap, max_frames, sample_rate, f0_floor, f0_ceil)
    with torch.cuda.device(audio_ring.device):
        stream = torch.cuda.current_stream(audio_ring.device).cuda_stream
        _check(lib, lib.fastsvc_stream_f0(_ptr(audio_ring), _ptr(f0_ring), _ptr(f0s_ring), _ptr(exc_ring), _ptr(phase), *per, *dims,
                                          ctypes.c_float(float(sample_rate)), ctypes.c_float(float(f0_floor)),
                                          ctypes.c_float(float(f0_ceil)), ctypes.c_float(float(threshold)),
                                          ctypes.c_float(float(sine_amp)), ctypes.c_float(float(noise_amp)), ctypes.c_void_p(stream)),
               "fastsvc_stream_f0")


def stream_f0_running(audio_ring: torch.Tensor, f0_ring: torch.Tensor, f0s_ring: torch.Tensor, exc_ring: torch.Tensor,
                      phase: torch.Tensor, record: Optional[torch.Tensor], streams: Sequence[int], first_frame: Sequence[int],
                      n: Sequence[int], seen: Sequence[int], ended: Sequence[int], parity: Sequence[int], seed: Sequence[int],
                      stats: Sequence[Optional[Sequence[float]]], running: Sequence[Optional[Sequence[float]]], cap: int,
                      max_frames: int, sample_rate: float, f0_floor: float, f0_ceil: float, threshold: float, sine_amp: float,
                      noise_amp: float) -> None:
    """``stream_f0`` for a call in which a stream runs source statistics (``decode.RunningF0Stats``): THREE HIP launches per 64
    streams of which one has them, two otherwise (fastsvc_stream_f0_running, csrc/fastsvc_stream_f0.hip).

    Everything is ``stream_f0``'s, plus ``running[i]``: ``(m_p, s_p, n0, g, m_t, s_t)`` - the prior's mean, std and weight in
    frames, the decay per voiced frame and the target's mean and std - or None for an entry that runs none (``stats[i]`` then
    says what it gets; an entry has one kind or neither), and ``record (n_streams, 2, 4)`` float64, per stream two entries of
    ``(w, S1, S2, voiced frames)``: read at entry ``parity[i]`` (or started from zeros when ``first_frame[i] == 0``), written at
    ``parity[i] ^ 1``, like ``phase``.  The rule is in include/fastsvc_hip.h.  Anything out of range - a missing record, ``s_p <=
    0``, ``n0 <= 0``, ``g`` outside (0, 1], a value that is not finite - raises ``ValueError`` before a launch and changes
    nothing; fails loudly off the GPU."""
    lib = load_library()
    per, dims = _stream_f0_args("stream_f0_running", audio_ring, f0_ring, f0s_ring, exc_ring, phase, streams, first_frame, n, seen,
                                ended, parity, seed, stats, cap, max_frames, sample_rate, f0_floor, f0_ceil)
    if record is not None:                           # (none is the library's to refuse)
        _gpu_tensors("stream_f0_running", audio_ring, (("record", record, torch.float64, 3),))
        if tuple(record.shape) != (dims[0], 2, 4):
            raise ValueError(f"record must be ({dims[0]}, 2, 4), got {tuple(record.shape)}")
    flat = []
    for ru in running:
        flat += [float("nan")] * 6 if ru is None else [float(v) for v in ru]
    if len(flat) != 6 * per[0]:
        raise ValueError("running entries are (m_p, s_p, n0, g, m_t, s_t) or None, one per stream")
    with torch.cuda.device(audio_ring.device):
        stream = torch.cuda.current_stream(audio_ring.device).cuda_stream
        _check(lib, lib.fastsvc_stream_f0_running(_ptr(audio_ring), _ptr(f0_ring), _ptr(f0s_ring), _ptr(exc_ring), _ptr(phase),
                                                  _ptr(record), *per, (ctypes.c_double * len(flat))(*flat), *dims,
                                                  ctypes.c_float(float(sample_rate)), ctypes.c_float(float(f0_floor)),
                                                  ctypes.c_float(float(f0_ceil)), ctypes.c_float(float(threshold)),
                                                  ctypes.c_float(float(sine_amp)), ctypes.c_float(float(noise_amp)),
                                                  ctypes.c_void_p(stream)),
               "fastsvc_stream_f0_running")


def stream_f0_tracked(audio_ring: torch.Tensor, cand_ring: torch.Tensor, bp_ring: torch.Tensor, f0_ring: torch.Tensor,
                      f0s_ring: torch.Tensor, exc_ring: torch.Tensor, phase: torch.Tensor, record: Optional[torch.Tensor],
                      track_record: torch.Tensor, streams: Sequence[int], first_frame: Sequence[int], n: Sequence[int],
                      seen: Sequence[int], ended: Sequence[int], parity: Sequence[int], track_parity: Sequence[int],
                      emit_first: Sequence[int], emit_n: Sequence[int], seed: Sequence[int],
                      stats: Sequence[Optional[Sequence[float]]], running: Optional[Sequence[Optional[Sequence[float]]]], cap: int,
                      max_frames: int, sample_rate: float, f0_floor: float, f0_ceil: float, cand_threshold: float, lag: int,
                      lag_bias: float, jump: float, switch: float, unvoiced: float, sine_amp: float, noise_amp: float) -> None:
    """``stream_f0_running`` with fixed-lag Viterbi tracking (``decode.F0Track``; fastsvc_stream_f0_tracked,
    csrc/fastsvc_stream_f0.hip): the newly final frames ``[first_frame[i], + n[i])`` get their candidates into ``cand_ring
    (n_streams, cap, 4, 2)`` float32 and advance the recurrence, whose state lives in ``track_record (n_streams, 2, 8)``
    float64 (entry ``track_parity[i]`` read, the other written) and whose backpointers in ``bp_ring (n_streams, cap, 8)`` uint8;
    the frames ``[emit_first[i], + emit_n[i])`` get the tracked raw F0, the shift (``stats`` / ``running`` with ``record``, which
    may both be None) and the excitation.  The rule is in include/fastsvc_hip.h.  Anything out of range raises ``ValueError``
    before a launch and changes nothing; fails loudly off the GPU."""
    lib = load_library()
    who = "stream_f0_tracked"
    per, dims = _stream_f0_args(who, audio_ring, f0_ring, f0s_ring, exc_ring, phase, streams, first_frame, n, seen, ended, parity,
                                seed, stats, cap, max_frames, sample_rate, f0_floor, f0_ceil)
    S, n_streams = per[0], dims[0]
    _gpu_tensors(who, audio_ring, (("cand_ring", cand_ring, torch.float32, 4), ("bp_ring", bp_ring, torch.uint8, 3),
                                   ("track_record", track_record, torch.float64, 3)))
    if tuple(cand_ring.shape) != (n_streams, cap, 4, 2) or tuple(bp_ring.shape) != (n_streams, cap, 8) or \
            tuple(track_record.shape) != (n_streams, 2, 8):
        raise ValueError(f"cand_ring must be ({n_streams}, {cap}, 4, 2), bp_ring ({n_streams}, {cap}, 8) and track_record "
                         f"({n_streams}, 2, 8)")
    if any(len(v) != S for v in (track_parity, emit_first, emit_n)):
        raise ValueError(f"{who} needs one entry per stream in every array")
    flat = None
    if running is not None:
        _gpu_tensors(who, audio_ring, (("record", record, torch.float64, 3),))
        if tuple(record.shape) != (n_streams, 2, 4):
            raise ValueError(f"record must be ({n_streams}, 2, 4), got {tuple(record.shape)}")
        flat = []
        for ru in running:
            flat += [float("nan")] * 6 if ru is None else [float(v) for v in ru]
        if len(flat) != 6 * S:
            raise ValueError("running entries are (m_p, s_p, n0, g, m_t, s_t) or None, one per stream")
        flat = (ctypes.c_double * len(flat))(*flat)
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    with torch.cuda.device(audio_ring.device):
        stream = torch.cuda.current_stream(audio_ring.device).cuda_stream
        _check(lib, lib.fastsvc_stream_f0_tracked(
            _ptr(audio_ring), _ptr(cand_ring), _ptr(bp_ring), _ptr(f0_ring), _ptr(f0s_ring), _ptr(exc_ring), _ptr(phase),
            _ptr(record) if running is not None else None, _ptr(track_record), *per[:7],
            _ints(i32, [int(v) & 1 for v in track_parity]), _ints(i64, emit_first), _ints(i32, emit_n), per[7], per[8], flat, *dims,
            ctypes.c_float(float(sample_rate)), ctypes.c_float(float(f0_floor)), ctypes.c_float(float(f0_ceil)),
            ctypes.c_float(float(cand_threshold)), int(lag), float(lag_bias), float(jump), float(switch), float(unvoiced),
            ctypes.c_float(float(sine_amp)), ctypes.c_float(float(noise_amp)), ctypes.c_void_p(stream)), "fastsvc_stream_f0_tracked")


def check_norm_groups(norm_groups, lens: Sequence[int]):
    """Validate ``norm_groups = (group, own_lo, own_hi)`` - three sequences of B ints, as ``fastsvc_forward_grouped`` takes
    them - against the rows' frame counts ``lens``, on the host (the library gets device arrays it cannot check): row b
    owns the frames ``[own_lo[b], own_hi[b])`` with ``0 <= own_lo < own_hi <= lens[b]``, and ``group[b]`` is the index of
    the first row of b's group, so ``group[b] <= b`` and ``group[group[b]] == group[b]``.  Returns the three as lists of
    ints; ``ValueError`` names the first row that breaks a rule."""
    try:
        group, own_lo, own_hi = ([int(v) for v in seq] for seq in norm_groups)
    except (TypeError, ValueError):
        raise ValueError("norm_groups must be (group, own_lo, own_hi), three sequences of ints") from None
    B = len(lens)
    if len(group) != B or len(own_lo) != B or len(own_hi) != B:
        raise ValueError(f"norm_groups must hold {B} entries each, got {len(group)}, {len(own_lo)}, {len(own_hi)}")
    for b in range(B):
        if not 0 <= own_lo[b] < own_hi[b] <= int(lens[b]):
            raise ValueError(f"row {b}: owned frames [{own_lo[b]}, {own_hi[b]}) must satisfy 0 <= own_lo < own_hi <= "
                             f"{int(lens[b])}, the row's frame count")
        if not 0 <= group[b] <= b:
            raise ValueError(f"row {b}: group[{b}] = {group[b]} must be the index of the first row of its group, so in [0, {b}]")
        if group[group[b]] != group[b]:
            raise ValueError(f"row {b}: group[{b}] = {group[b]} is not the first row of a group (group[{group[b]}] = "
                             f"{group[group[b]]})")
    return group, own_lo, own_hi


class _NormOverride(NamedTuple):         # what replaces a forward's InstanceNorm statistics (Plan.forward), validated
    kind: str                          # "grouped" (norm_groups) or "running" (norm_running)
    rows: tuple                        # 3 (group, own_lo, own_hi) or 6 (slot, own_lo, own_hi, prior, reset, parity) lists of B ints
    decay: Optional[tuple]             # running only: (decay, weight, bound), lists of B floats, or None


def _norm_stats_args(who: str, u, lens, len_mul, stats):
    """What ``norm_group_stats`` and ``norm_running_stats`` ask of ``u``, ``lens``, ``len_mul`` and ``stats``; returns
    ``(B, C, ld, len_mul, frame counts)``, the frame counts ``lens`` or, without, the full ``ld // len_mul`` of every row."""
    if not isinstance(u, torch.Tensor) or not u.is_cuda:
        raise FastSVCError(who + " needs GPU tensors (no CPU fallback); got " + str(getattr(u, "device", type(u))))
    if u.dim() != 3 or u.dtype not in DTYPE_CODES or not u.is_contiguous():
        raise ValueError(f"u must be a contiguous (B, C, ld) float32 / bfloat16 / float16 tensor; got {tuple(u.shape)} {u.dtype}")
    B, C, ld = u.shape
    len_mul = int(len_mul)
    if len_mul < 1 or ld % len_mul:
        raise ValueError(f"the pitch {ld} must be a multiple of len_mul {len_mul}")
    if lens is not None and (len(lens) != B or min(lens) < 1 or max(lens) * len_mul > ld):
        raise ValueError(f"lens must hold {B} frame counts in [1, {ld // len_mul}]")
    if not isinstance(stats, torch.Tensor) or stats.device != u.device or stats.dtype != torch.float64 or \
            tuple(stats.shape) != (B, C, 2) or not stats.is_contiguous():
        raise ValueError(f"stats must be a contiguous float64 {(B, C, 2)} tensor on {u.device}")
    return B, C, ld, len_mul, lens if lens is not None else [ld // len_mul] * B


def norm_group_stats(u: torch.Tensor, lens: Optional[Sequence[int]], len_mul: int, norm_groups, stats: torch.Tensor) -> torch.Tensor:
    """InstanceNorm sums of one tensor pooled over groups of rows (``fastsvc_norm_group_stats``,
    csrc/fastsvc_normgroup.hip): ``u`` (B, C, ld) float32, bfloat16 or float16 on the device, row b valid for ``lens[b] *
    len_mul`` columns (``None``: ``ld``), ``norm_groups = (group, own_lo, own_hi)`` in frames.  ``stats`` (B, C, 2)
    float64 receives, for every row that is not alone in its group owning all its frames, the group's sums over the owned
    columns times ``lens[b] * len_mul / N`` - ``decode.pool_norm_sums``' values; the other rows' entries are left
    untouched.  Two launches on the current stream.  Returns ``stats``."""
    lib = load_library()
    B, C, ld, len_mul, lens_host = _norm_stats_args("norm_group_stats", u, lens, len_mul, stats)
    group, own_lo, own_hi = check_norm_groups(norm_groups, lens_host)
    dev = u.device
    ints = torch.tensor([group, own_lo, own_hi] + ([[int(v) for v in lens]] if lens is not None else []), dtype=torch.int32).to(dev)
    scratch = torch.empty(B * C * (-(-ld // 2048)) * 16, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _check(lib, lib.fastsvc_norm_group_stats(_ptr(u), DTYPE_CODES[u.dtype], B, C, ld, _ptr(ints[3]) if lens is not None else None,
                                                 len_mul, _ptr(ints[0]), _ptr(ints[1]), _ptr(ints[2]), _ptr(stats), _ptr(scratch),
                                                 scratch.numel(), ctypes.c_void_p(stream)), "fastsvc_norm_group_stats")
    return stats


def check_norm_running(norm_running, lens: Sequence[int], n_slots: Optional[int] = None):
    """Validate ``norm_running = (slot, own_lo, own_hi, prior, reset, parity)`` - six sequences of B ints, as
    ``fastsvc_forward_running`` takes them - against the rows' frame counts ``lens``, on the host (the library gets device
    arrays it cannot check, and it FOLLOWS ``slot``).  Row b is a window of the stream in carry slot ``slot[b]`` with the
    core ``[own_lo[b], own_hi[b])``, ``0 <= own_lo < own_hi <= lens[b]``, and ``prior[b] >= own_lo[b]`` frames of the
    stream in front of the core; a ``reset`` row (the first window a stream runs in its slot) has ``prior == own_lo`` and
    is the first row of its slot in the batch.  Slots ascend through the batch (``slot[b] <= slot[b + 1]``, ``0 <= slot <
    n_slots``), so a slot's rows are neighbours; they are in window order - ``prior[b + 1] == prior[b] + own_hi[b] -
    own_lo[b]`` - and carry one ``parity`` (0 or 1).  Returns the six as lists of ints; ``ValueError`` names the first row
    that breaks a rule."""
    try:
        slot, own_lo, own_hi, prior, reset, parity = ([int(v) for v in seq] for seq in norm_running)
    except (TypeError, ValueError):
        raise ValueError("norm_running must be (slot, own_lo, own_hi, prior, reset, parity), six sequences of ints") from None
    B = len(lens)
    if any(len(a) != B for a in (slot, own_lo, own_hi, prior, reset, parity)):
        raise ValueError(f"norm_running must hold {B} entries each, got " +
                         ", ".join(str(len(a)) for a in (slot, own_lo, own_hi, prior, reset, parity)))
    for b in range(B):
        if not 0 <= own_lo[b] < own_hi[b] <= int(lens[b]):
            raise ValueError(f"row {b}: core frames [{own_lo[b]}, {own_hi[b]}) must satisfy 0 <= own_lo < own_hi <= "
                             f"{int(lens[b])}, the row's frame count")
        if slot[b] < 0 or (n_slots is not None and slot[b] >= int(n_slots)):
            raise ValueError(f"row {b}: slot {slot[b]} is not one of the carry's" + ("" if n_slots is None else f" {int(n_slots)}"))
        if prior[b] < own_lo[b]:
            raise ValueError(f"row {b}: prior {prior[b]} must be at least own_lo {own_lo[b]} (the left context lies in earlier cores)")
        if prior[b] + int(lens[b]) - own_lo[b] >= 2 ** 31:
            raise ValueError(f"row {b}: prior {prior[b]} is out of range")
        if parity[b] not in (0, 1):
            raise ValueError(f"row {b}: parity must be 0 or 1, got {parity[b]}")
        if reset[b] and prior[b] != own_lo[b]:
            raise ValueError(f"row {b}: a reset row starts its stream, so prior must equal own_lo {own_lo[b]}, got {prior[b]}")
        if b and slot[b] < slot[b - 1]:
            raise ValueError(f"row {b}: slots must ascend through the batch, {slot[b]} follows {slot[b - 1]}")
        if b and slot[b] == slot[b - 1]:
            if reset[b]:
                raise ValueError(f"row {b}: only the first row of slot {slot[b]} in the batch may be a reset row")
            if parity[b] != parity[b - 1]:
                raise ValueError(f"row {b}: the rows of slot {slot[b]} must carry one parity")
            if prior[b] != prior[b - 1] + own_hi[b - 1] - own_lo[b - 1]:
                raise ValueError(f"row {b}: the rows of slot {slot[b]} must be in window order: prior {prior[b]} should be "
                                 f"{prior[b - 1] + own_hi[b - 1] - own_lo[b - 1]}, the frames up to the end of row {b - 1}'s core")
    return slot, own_lo, own_hi, prior, [1 if v else 0 for v in reset], parity


def check_norm_decay(decay, weight, bound, running, lengths: Sequence[int]):
    """Validate the three per-row float arrays of a forgetting horizon (``fastsvc_forward_running_decay``) against the rows
    ``running = (slot, own_lo, own_hi, prior, reset, parity)`` (``check_norm_running`` has passed them) and their frame
    counts ``lengths``, on the host: B entries each, everything finite, ``0 < decay[b] <= 1``, ``weight[b] >= lengths[b] -
    own_lo[b]`` (the row's own core and look-ahead count in full) and ``bound[b] >= weight[b]`` (no column weighs more
    than one).  Returns the three as lists of floats; ``ValueError`` names the first row that breaks a rule."""
    try:
        decay, weight, bound = ([float(v) for v in seq] for seq in (decay, weight, bound))
    except (TypeError, ValueError):
        raise ValueError("norm_decay must be (decay, weight, bound), three sequences of floats") from None
    own_lo = [int(v) for v in running[1]]
    B = len(lengths)
    if any(len(a) != B for a in (decay, weight, bound, own_lo)):
        raise ValueError(f"norm_decay must hold {B} entries each, like the rows, got {len(decay)}, {len(weight)}, {len(bound)}")
    isfinite = math.isfinite
    for b, (d, w, bd) in enumerate(zip(decay, weight, bound)):
        if not (isfinite(d) and isfinite(w) and isfinite(bd)):
            raise ValueError(f"row {b}: decay, weight and bound must be finite, got {d}, {w}, {bd}")
        if not 0.0 < d <= 1.0:
            raise ValueError(f"row {b}: decay must be in (0, 1], got {d}")
        if w < int(lengths[b]) - own_lo[b]:
            raise ValueError(f"row {b}: weight {w} is less than the {int(lengths[b]) - own_lo[b]} frames of the row's own core "
                             f"and look-ahead")
        if bd < w:
            raise ValueError(f"row {b}: bound {bd} must be at least weight {w}")
    return decay, weight, bound


def norm_running_stats(u: torch.Tensor, lens: Optional[Sequence[int]], len_mul: int, norm_running, carry: torch.Tensor,
                       stats: torch.Tensor, decay=None) -> torch.Tensor:
    """Running InstanceNorm sums of one tensor with one norm point's carry (``fastsvc_norm_running_stats``,
    csrc/fastsvc_normgroup.hip): ``u`` (B, C, ld) float32, bfloat16 or float16 on the device, row b valid for ``lens[b] *
    len_mul`` columns (``None``: ``ld``), ``norm_running = (slot, own_lo, own_hi, prior, reset, parity)`` in frames
    (``check_norm_running``).  ``carry`` (n_slots, 2, C, 2) float64: entry ``parity`` of a slot's record is read (not for a
    reset row), entry ``parity ^ 1`` receives the slot's new carry - the caller flips its parity.  ``stats`` (B, C, 2)
    float64 receives ``decode.pool_running_sums``' values for every row that is not a pass-through row (reset, ``own_lo ==
    0``); those rows' entries are left untouched.  ``decay = (decay, weight, bound)``, three sequences of B floats
    (``check_norm_decay``): the fold of a forgetting horizon, ``fastsvc_norm_running_stats_decay`` - the sum is multiplied
    by ``decay[q]`` in front of every row's core and ``N = weight[b] * len_mul``.  Two launches on the current stream.
    Returns ``stats``."""
    lib = load_library()
    B, C, ld, len_mul, lens_host = _norm_stats_args("norm_running_stats", u, lens, len_mul, stats)
    if not isinstance(carry, torch.Tensor) or carry.device != u.device or carry.dtype != torch.float64 or carry.dim() != 4 or \
            tuple(carry.shape[1:]) != (2, C, 2) or carry.shape[0] < 1 or not carry.is_contiguous():
        raise ValueError(f"carry must be a contiguous float64 (n_slots, 2, {C}, 2) tensor on {u.device}")
    arrays = check_norm_running(norm_running, lens_host, carry.shape[0])
    dev = u.device
    ints = torch.tensor(list(arrays) + ([[int(v) for v in lens]] if lens is not None else []), dtype=torch.int32).to(dev)
    scratch = torch.empty(B * C * (-(-ld // 2048)) * 32, dtype=torch.uint8, device=dev)
    lens_ptr = _ptr(ints[6]) if lens is not None else None
    name, dbl = "fastsvc_norm_running_stats", []
    if decay is not None:
        if len(decay) != 3:
            raise ValueError("decay must be (decay, weight, bound), three sequences of floats")
        name, dbl = name + "_decay", torch.tensor(check_norm_decay(*decay, arrays, lens_host), dtype=torch.float64).to(dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _check(lib, getattr(lib, name)(_ptr(u), DTYPE_CODES[u.dtype], B, C, ld, lens_ptr, len_mul, *[_ptr(ints[i]) for i in range(6)],
                                       *[_ptr(d) for d in dbl], _ptr(carry), _ptr(stats), _ptr(scratch), scratch.numel(),
                                       ctypes.c_void_p(stream)), name)
    return stats


def _check(lib, rc: int, what: str):
    if rc != 0:
        msg = lib.fastsvc_last_error().decode("utf-8", "replace")
        if msg.endswith("split it"):                 # (the forward's limit on one utterance: say what does the splitting)
            from .synth import TOO_LONG_HINT
            msg += TOO_LONG_HINT
        if rc == -1:
            raise ValueError(f"{what}: {msg}")
        raise FastSVCError(f"{what} failed ({rc}): {msg}")


class Plan:
    """Host-only plan (layer table + blob / workspace layout) for one generator configuration."""

    def __init__(self, cfg: GeneratorConfig, load_shipped_table: bool = True, storage: str = "float32",
                 compact_workspace: bool = False):
        """``storage``: "float32" (default, the parity path), "bfloat16" - every workspace tensor is
        stored as bf16 (half the HBM traffic of the narrow layers, half the workspace; fp32 arithmetic;
        bf16-activation accuracy, frame counts must be multiples of 4) - or "float16": the same tensors as IEEE
        binary16 (bfloat16's bytes and kernels' shapes, 11 significand bits instead of 8; unscaled, so every workspace
        tensor must stay below 65504 in magnitude - see fastsvc_plan_set_storage in include/fastsvc_hip.h).
        ``compact_workspace``: intermediates of different stages share buffers (about 40 % less memory for long
        batches); the ``tap`` of a shared buffer then holds the last stage's tensor only."""
        if storage not in STORAGE_CODES:
            raise ValueError("storage must be 'float32', 'bfloat16' or 'float16'")
        self.storage = storage
        self.cfg = cfg
        self.lib = load_library()
        if cfg.n_stages > MAX_STAGES or len(cfg.upsampling_scales) != cfg.n_stages:
            raise ValueError("mid_channels / upsampling_scales must have equal length <= 8")
        c = _Config()
        c.in_channels = cfg.in_channels
        c.n_stages = cfg.n_stages
        for i in range(cfg.n_stages):
            c.mid_channels[i] = cfg.mid_channels[i]
            c.upsampling_scales[i] = cfg.upsampling_scales[i]
        c.out_channels = cfg.out_channels
        c.spk_emb_size = cfg.spk_emb_size
        c.use_spk_emb = 1 if cfg.use_spk_emb else 0
        handle = ctypes.c_void_p()
        _check(self.lib, self.lib.fastsvc_plan_create(ctypes.byref(c), ctypes.byref(handle)), "fastsvc_plan_create")
        self._h = handle
        if storage != "float32":
            _check(self.lib, self.lib.fastsvc_plan_set_storage(handle, STORAGE_CODES[storage]), "fastsvc_plan_set_storage")
            # (bfloat16 launches look their shapes up under "<layer>|<B>|<T>|b": separate entries of the same table;
            # float16 launches under "...|h" first, then under "...|b")
        self.compact_workspace = bool(compact_workspace)
        if compact_workspace:
            _check(self.lib, self.lib.fastsvc_plan_set_workspace_mode(handle, 1), "fastsvc_plan_set_workspace_mode")
        self.last_autotune_trials = 0
        self.pad_odd_lengths = True          # float32 storage: run F % 4 != 0 batches padded (see padded_frames)
        if load_shipped_table:
            self.load_tuned_file(TUNED_TABLE_PATH, missing_ok=True)

    # ---- launch-shape table (fastsvc_autotune winners) ----
    def config_signature(self) -> str:
        c = self.cfg
        return "in%d_mid%s_up%s_out%d_spk%d" % (c.in_channels, "-".join(map(str, c.mid_channels)),
                                                "-".join(map(str, c.upsampling_scales)), c.out_channels,
                                                c.spk_emb_size if c.use_spk_emb else 0)

    def tuned_shapes(self) -> dict:
        """{"<layer>|<B>|<T>": [NW, WM, WN, tiles_per_workgroup, algorithm]} currently held by the plan."""
        out = {}
        key = ctypes.create_string_buffer(96)
        shape = (ctypes.c_int32 * 5)()
        for i in range(int(self.lib.fastsvc_tuned_count(self._h))):
            _check(self.lib, self.lib.fastsvc_tuned_get(self._h, i, key, ctypes.byref(shape)), "fastsvc_tuned_get")
            out[key.value.decode()] = [int(v) for v in shape]
        return out

    def load_tuned(self, table: Mapping[str, Sequence[int]]) -> int:
        for k, v in table.items():
            v = list(v) + [0] * (5 - len(v))                  # older 4-entry tables: algorithm 0
            shape = (ctypes.c_int32 * 5)(*[int(x) for x in v])
            _check(self.lib, self.lib.fastsvc_tuned_set(self._h, k.encode(), ctypes.byref(shape)), "fastsvc_tuned_set")
        return len(table)

    def keep_last_block_output(self, B: int, F: int) -> None:
        """By default ``conv_last`` rides on the last block's final launch and the block's C-channel output is not
        written.  This keeps the two launches for batches of this shape (launch-table entry with algorithm 0
        under ``conv_last|B|T``), so that the ``up.<n-1>.out`` workspace tap holds the tensor."""
        T = F
        for sc in self.cfg.upsampling_scales:
            T *= int(sc)
        # (a float16 plan reads "|h" first and "|b" where there is none: its own entry, in case a tuning run wrote one)
        self.load_tuned({f"conv_last|{B}|{T}{sfx}": [1, 1, 4, 1, 0]
                         for sfx in ("", "|b") + (("|h",) if self.storage == "float16" else ())})

    def fuse_block_heads(self, B: int, F: int, fused: bool = True) -> None:
        """The head of an up block - ``conv_first`` and the two stretched convs behind it - can run as ONE launch
        (kernel mode 8, float32 storage, rows a multiple of 4 long: the tensor ``a`` between them never leaves LDS).
        It costs about what the three launches cost, so it runs only where the launch table holds algorithm 3 under
        ``up.<i>.head|B|T_in``; this sets those entries for a batch shape (``fused=False``: algorithm 0, the three
        launches whatever a loaded table says - the ``up.<i>.a`` taps then hold the tensor)."""
        T = F
        table = {}
        for i, sc in enumerate(self.cfg.upsampling_scales):
            table[f"up.{i}.head|{B}|{T}"] = [2, 1, 4, 1, 3 if fused else 0]
            T *= int(sc)
        self.load_tuned(table)

    def keep_block_heads_separate(self, B: int, F: int) -> None:
        self.fuse_block_heads(B, F, fused=False)
        self.keep_residual_convs_separate(B, F)

    def keep_residual_convs_separate(self, B: int, F: int) -> None:
        """By default the stretched residual conv of an up block is folded into the block's d = 3 conv (launch
        ``up.<i>.d3x``: the tensor ``xr`` is never written).  This keeps the two launches for batches of this shape
        (algorithm 0 under ``up.<i>.d3x|B|T_out``), so that the ``up.<i>.xr`` workspace taps hold the tensor."""
        T = F
        table = {}
        for i, sc in enumerate(self.cfg.upsampling_scales):
            T *= int(sc)
            table[f"up.{i}.d3x|{B}|{T}"] = [2, 1, 4, 1, 0]
            table[f"up.{i}.d3x|{B}|{T}|b"] = [2, 1, 4, 1, 0]
            if self.storage == "float16":
                table[f"up.{i}.d3x|{B}|{T}|h"] = [2, 1, 4, 1, 0]
        self.load_tuned(table)

    def load_tuned_file(self, path: str, missing_ok: bool = False) -> int:
        """Load this configuration's section of a tuned-shape JSON file (tools/tune_shapes.py)."""
        if not os.path.exists(path):
            if missing_ok:
                return 0
            raise FileNotFoundError(path)
        with open(path) as f:
            doc = json.load(f)
        return self.load_tuned(doc.get("tables", {}).get(self.config_signature(), {}))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self.lib.fastsvc_plan_destroy(h)
            self._h = None

    @property
    def arithmetic(self) -> str:
        """The type the path computes in, for bench.py's `dtype` (FASTSVC_HX=0 selects the f32-input MFMA kernels
        everywhere; by default every k=3 convolution whose rows are a multiple of 4 long runs on the
        half-precision MFMA kernels of csrc/fastsvc_hx.hip)."""
        hx = os.environ.get("FASTSVC_HX", "1") != "0"
        if self.storage == "float32":
            return ("f32 (conv products as split-binary16 pairs on the f16 MFMA, x*w = xh*wh + xh*wl + xl*wh with f32 "
                    "accumulation; weights scaled per output channel and activations per tensor and utterance by exact "
                    "powers of two into binary16's range, undone in the epilogue: fp32-class, 4e-6 of the f32-MFMA path, "
                    "held over 2^-20..2^8 input / weight scales by tests/test_dynamic_range_gpu.py)") if hx else "f32"
        if self.storage == "float16":
            return ("f16 (binary16 MFMA products, f32 accumulate, binary16 activation storage, unscaled)" if hx
                    else "f32 arithmetic, binary16 activation storage")
        return ("bf16 (bf16 MFMA products, f32 accumulate, bf16 activation storage)" if hx
                else "f32 arithmetic, bf16 activation storage")

    @property
    def blob_bytes(self) -> int:
        return int(self.lib.fastsvc_weight_blob_bytes(self._h))

    @property
    def flops_per_sample(self) -> float:
        return float(self.lib.fastsvc_flops_per_sample(self._h))

    def launch_count(self, with_spk: bool = True) -> int:
        return int(self.lib.fastsvc_forward_launch_count(self._h, 1 if with_spk else 0))

    def prepare_stream(self, device=None) -> None:
        """Create the helper streams / events of the current HIP stream of `device` ahead of the first
        forward on it (so that forward allocates nothing)."""
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            _check(self.lib, self.lib.fastsvc_stream_prepare(ctypes.c_void_p(stream)), "fastsvc_stream_prepare")

    def release_stream(self, stream=None, device=None) -> bool:
        """Free the helper streams / events the library holds for `stream` (a torch.cuda.Stream; default: the
        current one) - to be called before a short-lived stream that ran forwards is dropped."""
        with torch.cuda.device(device):
            st = (stream or torch.cuda.current_stream(device)).cuda_stream
            return bool(self.lib.fastsvc_stream_release(ctypes.c_void_p(st)))

    def workspace_bytes(self, B: int, F: int) -> int:
        return int(self.lib.fastsvc_workspace_bytes(self._h, B, F))

    def norm_group_scratch_bytes(self, B: int, F: int) -> int:
        """Bytes of device scratch one forward with ``norm_groups`` needs for its partial sums."""
        return int(self.lib.fastsvc_norm_group_scratch_bytes(self._h, B, F))

    def norm_carry_bytes(self) -> int:
        """Bytes of ONE slot's carry record for ``norm_running``: both parity entries of every norm point's C x 2 doubles."""
        return int(self.lib.fastsvc_norm_carry_bytes(self._h))

    def norm_running_scratch_bytes(self, B: int, F: int) -> int:
        """Bytes of device scratch one forward with ``norm_running`` needs for its partial sums."""
        return int(self.lib.fastsvc_norm_running_scratch_bytes(self._h, B, F))

    def padded_frames(self, F: int) -> int:
        """Frame count the library actually runs for an F-frame batch: the next multiple of 4 (the padded batch is run
        as a ragged one).  bfloat16 and float16 storage need it; float32 storage takes any F, but rows that are not a multiple of
        4 long (F-rate and 2F-rate tensors) send their layers to the slower gathered kernels - 64 x 1499 frames took
        27.0 ms against 22.5 ms for 64 x 1500 (tools/ragged_check.py) - so `Plan.forward` pads there too."""
        return F + ((-F) % 4)

    def pack_prefetch(self, state_dict: Mapping[str, object]):
        """Start the device-to-host copy of a state dict's device tensors (one gather, one asynchronous copy into a
        page-locked buffer, one event on the current stream) and return a handle for ``pack(..., prefetched=handle)``.
        A training step calls this right behind the optimizer update: the copy and the host-side packing then overlap
        whatever the GPU is given next instead of draining the stream first."""
        items = list(state_dict.items())
        on_dev = [i for i, (_, v) in enumerate(items) if isinstance(v, torch.Tensor) and v.device.type != "cpu"]
        if not on_dev:
            return None
        flat = torch.cat([items[i][1].detach().reshape(-1).to(torch.float32) for i in on_dev])
        buf = getattr(self, "_pinned_params", None)
        if buf is None or buf.numel() < flat.numel():
            buf = self._pinned_params = torch.empty(flat.numel(), dtype=torch.float32, pin_memory=True)
        buf[: flat.numel()].copy_(flat, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(flat.device))
        return {"event": ev, "host": buf[: flat.numel()], "numels": [items[i][1].numel() for i in on_dev], "keep": flat}

    def pack(self, state_dict: Mapping[str, object], reuse_pinned: bool = False, prefetched=None) -> torch.Tensor:
        """Fold weight-norm and pack a state dict (either key layout) into the kernel blob.

        Returns a CPU float32 tensor of ``blob_bytes`` bytes (upload or broadcast it).  Device tensors are gathered
        with ONE device-to-host copy (a training step re-packs after every optimizer update: 251 separate copies were
        a third of that).  ``reuse_pinned``: return this plan's page-locked staging buffer (overwritten by the next
        such call) - for callers that upload it right away."""
        items = list(state_dict.items())
        host = [None] * len(items)
        on_dev = [i for i, (_, v) in enumerate(items) if isinstance(v, torch.Tensor) and v.device.type != "cpu"]
        if on_dev:
            if prefetched is not None and prefetched["numels"] == [items[i][1].numel() for i in on_dev]:
                prefetched["event"].synchronize()            # the copy issued by pack_prefetch (same tensors, same order)
                flat = prefetched["host"].numpy()
            else:
                flat = torch.cat([items[i][1].detach().reshape(-1).to(torch.float32) for i in on_dev]).cpu().numpy()
            o = 0
            for i in on_dev:
                n = items[i][1].numel()
                host[i] = flat[o:o + n]
                o += n
        keep = []
        arr = (_Tensor * len(items))()
        for i, (k, v) in enumerate(items):
            if host[i] is not None:
                a = host[i]
            else:
                if isinstance(v, torch.Tensor):
                    v = v.detach().to("cpu", torch.float32).contiguous().numpy()
                a = np.ascontiguousarray(np.asarray(v, dtype=np.float32))
            name = k.encode("utf-8")
            keep.append((a, name))
            arr[i].name = name
            arr[i].data = a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
            arr[i].numel = a.size
        if reuse_pinned:
            if getattr(self, "_pinned_blob", None) is None:
                self._pinned_blob = torch.empty(self.blob_bytes // 4, dtype=torch.float32,
                                                pin_memory=torch.cuda.is_available())
            blob = self._pinned_blob
        else:
            blob = torch.empty(self.blob_bytes // 4, dtype=torch.float32)
        rc = self.lib.fastsvc_pack_weights(self._h, arr, len(items), ctypes.c_void_p(blob.data_ptr()))
        if rc == -2:
            raise KeyError(self.lib.fastsvc_last_error().decode())
        _check(self.lib, rc, "fastsvc_pack_weights")
        return blob

    @property
    def pack_device_scratch_bytes(self) -> int:
        return int(self.lib.fastsvc_pack_device_scratch_bytes(self._h))

    @property
    def pack_device_launches(self) -> int:
        """Launches one ``pack_device`` enqueues (kernels + one table copy + one memset)."""
        return int(self.lib.fastsvc_pack_device_launch_count(self._h))

    def pack_device(self, state_dict: Mapping[str, torch.Tensor], out: Optional[torch.Tensor] = None,
                    scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``pack`` for parameters that are already on the GPU: the same bytes, written by HIP kernels
        (csrc/fastsvc_pack.hip) into a device blob, asynchronously on the current stream - no weight crosses the host
        link in either direction.  Every value must be a float32 CUDA tensor on one device (non-contiguous ones are made
        contiguous); anything else raises ``FastSVCError`` - there is no fallback to the host packer.  ``out``: a
        contiguous device tensor of ``blob_bytes`` bytes to write into (the blob of earlier forwards on the stream is
        fine); returned as it is.  ``scratch``: a uint8 device tensor of at least ``pack_device_scratch_bytes`` bytes, any
        contents (default: one per device and stream, kept by the plan).  ``KeyError`` for a missing or mis-sized tensor,
        like ``pack``."""
        items = list(state_dict.items())
        if not items:
            raise KeyError("empty state dict")
        dev = None
        for k, v in items:
            if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype != torch.float32:
                raise FastSVCError(f"pack_device needs float32 GPU tensors (no CPU fallback: use pack); {k} is "
                                   f"{getattr(v, 'dtype', type(v))} on {getattr(v, 'device', 'the host')}")
            if dev is None:
                dev = v.device
            elif v.device != dev:
                raise FastSVCError(f"pack_device: {k} is on {v.device}, expected {dev}")
        nbytes = self.blob_bytes
        if out is None:
            out = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        elif not isinstance(out, torch.Tensor) or out.device != dev or not out.is_contiguous() or \
                out.numel() * out.element_size() != nbytes:
            raise ValueError(f"out must be a contiguous tensor of {nbytes} bytes on {dev}")
        tensors = [v.detach() if v.is_contiguous() else v.detach().contiguous() for _, v in items]
        # the ctypes table is rebuilt only when a tensor moved (a training loop packs the same parameters every step)
        key = tuple((t.data_ptr(), t.numel()) for t in tensors)
        cached = getattr(self, "_pack_device_args", None)
        if cached is None or cached[0] != key or cached[1] != [k for k, _ in items]:
            arr = (_Tensor * len(items))()
            names = [k.encode("utf-8") for k, _ in items]
            for i, t in enumerate(tensors):
                arr[i].name = names[i]
                arr[i].data = ctypes.cast(ctypes.c_void_p(t.data_ptr()), ctypes.POINTER(ctypes.c_float))
                arr[i].numel = t.numel()
            cached = self._pack_device_args = (key, [k for k, _ in items], arr, names)
        arr = cached[2]
        need = self.pack_device_scratch_bytes
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            if scratch is None:
                # one per (device, stream): packs of one plan on different streams must not share it
                pool = self.__dict__.setdefault("_pack_device_scratch", {})
                skey = (str(dev), int(stream))
                if skey not in pool:
                    if len(pool) >= 4:
                        pool.pop(next(iter(pool)))
                    pool[skey] = torch.empty(need, dtype=torch.uint8, device=dev)
                scratch = pool[skey]
            elif scratch.device != dev or scratch.dtype != torch.uint8 or not scratch.is_contiguous() or scratch.numel() < need:
                raise ValueError(f"scratch must be a contiguous uint8 tensor of at least {need} bytes on {dev}")
            rc = self.lib.fastsvc_pack_weights_device(self._h, arr, len(items), ctypes.c_void_p(out.data_ptr()),
                                                      ctypes.c_void_p(scratch.data_ptr()), scratch.numel(), ctypes.c_void_p(stream))
        if rc == -2:
            raise KeyError(self.lib.fastsvc_last_error().decode())
        _check(self.lib, rc, "fastsvc_pack_weights_device")
        self._pack_device_keep = tensors             # (contiguous copies: alive until the next pack on this plan)
        return out

    def tap_info(self, name: str, B: int, F: int) -> Tuple[int, int, Tuple[int, int, int]]:
        off = ctypes.c_size_t()
        numel = ctypes.c_int64()
        shape = (ctypes.c_int64 * 3)()
        _check(self.lib, self.lib.fastsvc_workspace_tap(self._h, B, F, name.encode(), ctypes.byref(off),
                                                        ctypes.byref(numel), ctypes.byref(shape)),
               "fastsvc_workspace_tap")
        return int(off.value), int(numel.value), (int(shape[0]), int(shape[1]), int(shape[2]))

    def tap(self, name: str, B: int, F: int, workspace: torch.Tensor) -> torch.Tensor:
        """View of a named intermediate inside ``workspace`` (valid after a forward)."""
        off, numel, shape = self.tap_info(name, B, F)
        if name.endswith(".stats"):
            return workspace[off: off + numel * 8].view(torch.float64).view(shape)
        if self.storage != "float32" and name != "sig" and not name.endswith(".spk"):
            return workspace[off: off + numel * 2].view(STORAGE_DTYPES[self.storage]).view(shape)
        return workspace[off: off + numel * 4].view(torch.float32).view(shape)

    _LENS_SLOTS = 32

    def _stage_lengths(self, lens_host: torch.Tensor, B: int, dev) -> torch.Tensor:
        """Frame counts -> device through a RING of page-locked slots owned by the plan.  A fresh pinned tensor per
        call looked harmless, but the host runs many batches ahead of the GPU: the pinned allocator cannot recycle a
        block whose copy has not run yet, so every forward of a pass over ragged batches paid a hipHostMalloc
        (≈ 3 ms each, serialised with the device: 187 ms instead of 145 ms for the 13 batches of cfg4var).  A slot is
        reused only after its copy has completed (event; the host waits only if it is 32 batches ahead)."""
        ring = getattr(self, "_lens_ring", None)
        if ring is None or ring["buf"].shape[1] < B:
            ring = {"buf": torch.empty((self._LENS_SLOTS, max(64, B)), dtype=torch.int32, pin_memory=True),
                    "ev": [None] * self._LENS_SLOTS, "i": 0}
            self._lens_ring = ring
        slot = ring["i"] % self._LENS_SLOTS
        ring["i"] += 1
        if ring["ev"][slot] is not None:
            ring["ev"][slot].synchronize()
        src = ring["buf"][slot, :B]
        src.copy_(lens_host)
        out = src.to(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        ring["ev"][slot] = ev
        return out

    def forward(self, blob: torch.Tensor, ppg: torch.Tensor, sine: torch.Tensor, lft: torch.Tensor,
                spk_emb: Optional[torch.Tensor], out: Optional[torch.Tensor] = None,
                workspace: Optional[torch.Tensor] = None, profile: Optional[list] = None,
                autotune: bool = False, lengths=None, norm_groups=None,
                norm_scratch: Optional[torch.Tensor] = None, norm_running=None,
                norm_carry: Optional[torch.Tensor] = None, norm_decay=None) -> torch.Tensor:
        """Enqueue one forward on the current HIP stream of ``ppg.device``; returns (B, O, T).

        ``lengths`` (B frame counts, 1 <= n <= F; sequence or int tensor) makes the batch ragged:
        inputs stay padded to F, utterance b is computed exactly as if run alone with lengths[b]
        frames and ``out[b, :, lengths[b]*hop:]`` is zero.

        ``norm_groups = (group, own_lo, own_hi)`` (three sequences of B ints, ``check_norm_groups``) pools the InstanceNorm
        statistics over groups of rows (``fastsvc_forward_grouped``): row b owns the frames ``[own_lo[b], own_hi[b])`` and is
        normalised by the mean and variance of the owned frames of all rows whose ``group`` entry equals its own.  Rows alone
        in their group that own all their frames run exactly as without it.  Not with ``profile`` or ``autotune``.
        ``norm_scratch``: a uint8 device tensor of at least ``norm_group_scratch_bytes(B, padded_frames(F))`` bytes for the
        partial sums (allocated per call when missing).

        ``norm_running = (slot, own_lo, own_hi, prior, reset, parity)`` (six sequences of B ints, ``check_norm_running``)
        with ``norm_carry``, a contiguous 2-D device tensor of one record per slot (``norm_carry_bytes()`` bytes a row, or
        more), makes the rows windows of live streams (``fastsvc_forward_running``): each is normalised by the statistics
        of every frame of its stream up to its right edge, the sums of earlier windows read from the slot's record, entry
        ``parity``, and the new ones written to entry ``parity ^ 1`` - the CALLER flips a slot's parity after the call.
        Not with ``norm_groups``, ``profile`` or ``autotune``; ``norm_scratch`` then needs
        ``norm_running_scratch_bytes(B, padded_frames(F))`` bytes.  Without ``spk_emb`` nothing is normalised and nothing
        carried.  ``norm_decay = (decay, weight, bound)`` (three sequences of B floats, ``check_norm_decay``; only with
        ``norm_running``) forgets the carried sums exponentially (``fastsvc_forward_running_decay``): the slot's sums are
        multiplied by ``decay[b]`` in front of row b's core and the row is normalised over ``weight[b]`` frames; the six
        int arrays and these three travel to the device in one upload.

        With ``profile`` (a list) the launches are bracketed by hipEvents on that stream, the
        stream is synchronised and one dict per kernel launch is appended to the list.
        With ``autotune`` every convolution first times its candidate launch shapes for this
        (B, F) and the plan remembers the fastest (cf. ``cudnn.benchmark``); synchronises."""
        cfg = self.cfg
        ppg, sine, lft, spk_emb = self._check_inputs(blob, ppg, sine, lft, spk_emb)
        dev, (B, _, F) = ppg.device, ppg.shape
        T = F * cfg.hop
        override = self._norm_override(B, F, dev, lengths, profile is not None or autotune, norm_groups, norm_running,
                                       norm_carry, norm_decay)
        if F % 4 != 0 and profile is None and (self.storage != "float32" or self.pad_odd_lengths):
            return self._forward_padded(blob, ppg, sine, lft, spk_emb, out, workspace, autotune, lengths, override,
                                        norm_scratch, norm_carry)
        lens_dev = None
        if lengths is not None:
            if autotune:
                raise ValueError("autotune times full-length batches: call it without lengths")
            if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
                # already on the device: used as is (int32, B entries; range checked by the caller - reading it back
                # here would synchronise)
                if lengths.device != dev or lengths.numel() != B:
                    raise ValueError(f"lengths must hold {B} frame counts on {dev}")
                lens_dev = lengths.reshape(-1).to(torch.int32).contiguous()
            else:
                lens_host = torch.as_tensor(lengths, dtype=torch.int64, device="cpu").reshape(-1)
                if lens_host.numel() != B or int(lens_host.min()) < 1 or int(lens_host.max()) > F:
                    raise ValueError(f"lengths must hold {B} frame counts in [1, {F}]")
                # through page-locked memory: a pageable source makes the copy block the host until it is done
                # (the header promises a forward that never synchronises)
                lens_dev = self._stage_lengths(lens_host, B, dev)
        need = self.workspace_bytes(B, F)
        if workspace is None or workspace.numel() < need:
            workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        if out is None:
            out = torch.empty((B, cfg.out_channels, T), dtype=torch.float32, device=dev)
        elif out.dtype != torch.float32 or tuple(out.shape) != (B, cfg.out_channels, T) or out.device != dev or \
                not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 {(B, cfg.out_channels, T)} tensor on {dev}")
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            tensors = (self._h, _ptr(blob), _ptr(ppg), _ptr(sine), _ptr(lft), _ptr(spk_emb), _ptr(out), B, F)
            lens_p, ws = _ptr(lens_dev), (_ptr(workspace), workspace.numel())
            if autotune:
                ntr = ctypes.c_int32(0)
                rc = self.lib.fastsvc_autotune(*tensors, *ws, stream, ctypes.byref(ntr))
                self.last_autotune_trials = int(ntr.value)
            elif override is not None and spk_emb is not None:
                grouped = override.kind == "grouped"
                need = self.norm_group_scratch_bytes(B, F) if grouped else self.norm_running_scratch_bytes(B, F)
                if norm_scratch is None or norm_scratch.numel() * norm_scratch.element_size() < need or norm_scratch.device != dev:
                    norm_scratch = torch.empty(need, dtype=torch.uint8, device=dev)
                scratch = (_ptr(norm_scratch), norm_scratch.numel() * norm_scratch.element_size())
                if override.decay is None:               # 3 (grouped) or 6 (running) arrays of B ints in one upload ...
                    host = torch.tensor(override.rows, dtype=torch.int32).reshape(-1)
                else:                                    # (... the doubles behind the 6 B ints - an even count, so 8-byte aligned)
                    packed = np.empty(12 * B, dtype=np.int32)
                    packed[:6 * B] = np.asarray(override.rows, dtype=np.int32).reshape(-1)
                    packed[6 * B:].view(np.float64)[:] = np.asarray(override.decay, dtype=np.float64).reshape(-1)
                    host = torch.from_numpy(packed)
                up = self._stage_lengths(host, host.numel(), dev)
                rows_p = [ctypes.c_void_p(up[i * B:].data_ptr()) for i in range(len(override.rows))]
                if grouped:
                    rc = self.lib.fastsvc_forward_grouped(*tensors, lens_p, *rows_p, *ws, *scratch, stream)
                else:
                    carry = (_ptr(norm_carry), norm_carry.shape[1] * norm_carry.element_size())
                    if override.decay is None:
                        rc = self.lib.fastsvc_forward_running(*tensors, lens_p, *rows_p, *carry, *ws, *scratch, stream)
                    else:
                        decay_p = [ctypes.c_void_p(up[(6 + 2 * i) * B:].data_ptr()) for i in range(3)]
                        rc = self.lib.fastsvc_forward_running_decay(*tensors, lens_p, *rows_p, *decay_p, *carry, *ws, *scratch, stream)
                workspace = (workspace, up, norm_scratch, norm_carry)
            elif profile is None:
                rc = self.lib.fastsvc_forward(*tensors, lens_p, *ws, stream)
            else:
                recs = (_LaunchRecord * 256)()
                n = ctypes.c_int32(0)
                rc = self.lib.fastsvc_forward_profile(*tensors, lens_p, *ws, stream, recs, 256, ctypes.byref(n))
                if rc == 0:
                    for i in range(n.value):
                        profile.append(dict(layer=recs[i].layer.decode(), kernel=recs[i].kernel.decode(),
                                            flops=recs[i].flops, bytes=recs[i].bytes, ms=recs[i].ms,
                                            x2_path=("", "element", "gather")[recs[i].x2_path]))
        _check(self.lib, rc, "fastsvc_forward")
        self._last_workspace = (workspace, lens_dev)      # keep alive until the stream has consumed them
        return out

    def _check_inputs(self, blob, ppg, sine, lft, spk_emb):
        """The tensors of one forward against the plan's config and each other; returns the four inputs as contiguous float32."""
        cfg = self.cfg
        if not ppg.is_cuda:
            raise FastSVCError("FastSVC HIP path needs GPU tensors (no CPU fallback); got " + str(ppg.device))
        dev = ppg.device
        for name, t in (("sine", sine), ("lft", lft), ("spk_emb", spk_emb), ("blob", blob)):
            if t is not None and t.device != dev:
                raise ValueError(f"{name} is on {t.device}, expected {dev}")
        if ppg.dim() != 3 or ppg.shape[1] != cfg.in_channels:
            raise ValueError(f"ppg must be (B, {cfg.in_channels}, F), got {tuple(ppg.shape)}")
        B, _, F = ppg.shape
        T = F * cfg.hop
        for name, t in (("sine", sine), ("lft", lft)):
            if tuple(t.shape) != (B, 1, T):
                raise ValueError(f"{name} must be (B, 1, F*{cfg.hop}) = {(B, 1, T)}, got {tuple(t.shape)}")
        if spk_emb is not None and tuple(spk_emb.shape) != (B, cfg.spk_emb_size):
            raise ValueError(f"spk_emb must be {(B, cfg.spk_emb_size)}, got {tuple(spk_emb.shape)}")
        return tuple(None if t is None else t.to(torch.float32).contiguous() for t in (ppg, sine, lft, spk_emb))

    def _norm_override(self, B: int, F: int, dev, lengths, timed: bool, norm_groups, norm_running, norm_carry, norm_decay):
        """``norm_groups`` or ``norm_running`` (+ ``norm_carry``, ``norm_decay``) of one forward, validated on the host
        against the rows' frame counts; a ``_NormOverride`` record, or None when the call has neither."""
        def lens_host(name: str, what: str):
            if timed:
                raise ValueError(f"{name} runs neither profiled nor under autotune")
            if isinstance(lengths, torch.Tensor):
                raise ValueError(f"{name} needs lengths on the host (the {what} are checked against them)")
            return [F] * B if lengths is None else [int(v) for v in lengths]
        grouped = None
        if norm_groups is not None:
            grouped = _NormOverride("grouped", check_norm_groups(norm_groups, lens_host("norm_groups", "owned ranges")), None)
        if norm_running is None:
            if norm_carry is not None or norm_decay is not None:
                raise ValueError(("norm_carry" if norm_carry is not None else "norm_decay") + " goes with norm_running")
            return grouped
        if grouped is not None:
            raise ValueError("norm_running and norm_groups exclude each other")
        lens = lens_host("norm_running", "cores")
        row = 0 if not isinstance(norm_carry, torch.Tensor) or norm_carry.dim() != 2 else norm_carry.shape[1] * norm_carry.element_size()
        if row < self.norm_carry_bytes() or row % 8 or norm_carry.device != dev or not norm_carry.is_contiguous():
            raise ValueError(f"norm_running needs norm_carry: a contiguous (n_slots, k) tensor on {dev} with rows of at least "
                             f"norm_carry_bytes() = {self.norm_carry_bytes()} bytes, a multiple of 8")
        rows = check_norm_running(norm_running, lens, norm_carry.shape[0])
        if norm_decay is not None:
            if len(norm_decay) != 3:
                raise ValueError("norm_decay must be (decay, weight, bound), three sequences of floats")
            norm_decay = check_norm_decay(*norm_decay, rows, lens)
        return _NormOverride("running", rows, norm_decay)

    def _forward_padded(self, blob, ppg, sine, lft, spk_emb, out, workspace, autotune, lengths, override, norm_scratch,
                        norm_carry) -> torch.Tensor:
        """bfloat16 / float16 storage moves 4 time steps per access at the frame rate, so the library wants F % 4 == 0 (three
        of four real utterances are not); float32 storage runs such rows on its slower kernels.  Pad to the next multiple and
        run the padded batch as a ragged one - `lengths` makes every utterance exactly what it would be alone at its own
        length.  The caller's workspace is used when it holds the padded batch (size it with `workspace_bytes(B,
        padded_frames(F))`); the padded inputs live in one reused staging set.  Autotuning tunes the padded shape (launch
        shapes are keyed by the padded row lengths)."""
        cfg, dev, (B, _, F) = self.cfg, ppg.device, ppg.shape
        Fp, hop = self.padded_frames(F), cfg.hop
        T = F * hop
        if lengths is not None and not (isinstance(lengths, torch.Tensor) and lengths.is_cuda):
            lh = torch.as_tensor(lengths, dtype=torch.int64, device="cpu").reshape(-1)
            if lh.numel() != B or int(lh.min()) < 1 or int(lh.max()) > F:        # (against the caller's F, not the padded one)
                raise ValueError(f"lengths must hold {B} frame counts in [1, {F}]")
        if workspace is not None and workspace.numel() < self.workspace_bytes(B, Fp):
            raise ValueError(f"workspace too small for the padded batch: size it with workspace_bytes({B}, padded_frames({F}) = {Fp})")
        # one staging set per (shape, device, STREAM): forwards of one plan on different streams must not share it
        key = (B, Fp, str(dev), int(torch.cuda.current_stream(dev).cuda_stream))
        sets = self.__dict__.setdefault("_pad_sets", {})
        if key not in sets:
            if len(sets) >= 8:
                sets.pop(next(iter(sets)))
            sets[key] = [torch.zeros((B, cfg.in_channels, Fp), dtype=torch.float32, device=dev),
                         torch.zeros((B, 1, Fp * hop), dtype=torch.float32, device=dev),
                         torch.zeros((B, 1, Fp * hop), dtype=torch.float32, device=dev),
                         torch.empty((B, cfg.out_channels, Fp * hop), dtype=torch.float32, device=dev), F]
        pp, ps, pl, py, lastF = sets[key]
        pp[..., :F].copy_(ppg); ps[..., :T].copy_(sine); pl[..., :T].copy_(lft)
        if lastF > F:                                    # a longer batch used this set: its tail is not padding
            pp[..., F:lastF].zero_(); ps[..., T:lastF * hop].zero_(); pl[..., T:lastF * hop].zero_()
        sets[key][4] = F
        if autotune:
            if lengths is not None:
                raise ValueError("autotune times full-length batches: call it without lengths")
            self.forward(blob, pp, ps, pl, spk_emb, out=py, workspace=workspace, autotune=True)
        kind, rows, decay = override or (None, None, None)
        self.forward(blob, pp, ps, pl, spk_emb, out=py, workspace=workspace, lengths=[F] * B if lengths is None else lengths,
                     norm_groups=rows if kind == "grouped" else None, norm_running=rows if kind == "running" else None,
                     norm_scratch=norm_scratch, norm_carry=norm_carry, norm_decay=decay)
        return py[..., :T].contiguous() if out is None else out.copy_(py[..., :T])
