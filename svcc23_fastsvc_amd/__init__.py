"""MI355X-native FastSVC generator forward (gfx950 HIP kernels behind the reference's
``harana.models.FastSVCGenerator`` surface).  See DESIGN.md / INTEGRATION.md."""
from .synth import GeneratorConfig, FULL_CONFIG, TINY_CONFIG  # noqa: F401
from .engine import FastSVCError, Plan, load_library, library_path, gather_padded, gather_time_major, pcm16_pack, output_check, report_arrays, collate_crops, fanout_assemble, fanout_launch_count, window_assemble, window_stitch, window_launch_count, stream_push, stream_assemble, stream_check, stream_launch_count, stream_f0, stream_f0_running, stream_f0_tracked, f0_lags, check_norm_groups, norm_group_stats, check_norm_running, norm_running_stats, check_norm_decay  # noqa: F401
from .generator import FastSVCGenerator, install_into_harana  # noqa: F401
from .signal import SignalGenerator  # noqa: F401
from .loudness import loudness_extract  # noqa: F401
from .f0 import f0_extract, f0_candidates, f0_track  # noqa: F401
from .stft_loss import MultiResolutionSTFTLoss  # noqa: F401
from .train_session import TrainSession, CropSampler  # noqa: F401

__all__ = ["FastSVCGenerator", "SignalGenerator", "loudness_extract", "f0_extract", "f0_candidates", "f0_track", "MultiResolutionSTFTLoss", "GeneratorConfig", "Plan", "FastSVCError", "install_into_harana",
           "load_library", "library_path", "gather_padded", "gather_time_major", "pcm16_pack", "output_check", "report_arrays", "collate_crops", "fanout_assemble", "fanout_launch_count", "window_assemble", "window_stitch", "window_launch_count", "stream_push", "stream_assemble", "stream_check", "stream_launch_count", "stream_f0", "stream_f0_running", "stream_f0_tracked", "f0_lags", "check_norm_groups", "norm_group_stats", "check_norm_running", "norm_running_stats", "check_norm_decay", "TrainSession", "CropSampler", "FULL_CONFIG", "TINY_CONFIG"]
