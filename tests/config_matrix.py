"""Generator configurations other than the yaml one, each chosen for a kernel route it reaches.  Shared by
tests/golden/make_golden.py (`live_configs`: the live reference's output for each, which pins the oracle there) and
the tests (tests/test_oracle_golden.py, tests/test_config_matrix_gpu.py).

C below is an up block's width (mid_channels[i]) and S its stretch factor (upsampling_scales[i]).  The routes follow
from the plan's gates: the channel tile per C (choose_mw: 48 channels where C % 48 == 0 or C > 32, else 32), the
stretch factors that have a fused residual instance for that tile (conv_hx_x2_ok: 48-channel tiles S = 2 / 4, one
32-channel chunk S = 5), and the row rate of each tensor relative to the frame rate in a ragged batch.
"""
from svcc23_fastsvc_amd import synth as S

CONFIGS = {
    "s2_second": (
        dict(in_channels=144, mid_channels=[192, 96, 48, 24], upsampling_scales=[2, 2, 4, 5], out_channels=1,
             spk_emb_size=512, use_spk_emb=True),
        "S = 2 at C = 96 in up.1, whose residual operand runs at twice the frame rate (ragged rows end at 2 mod 4)"),
    "s3_narrow": (
        dict(in_channels=48, mid_channels=[96, 48, 24, 24], upsampling_scales=[2, 2, 3, 5], out_channels=1,
             spk_emb_size=32, use_spk_emb=True),
        "S = 3 (no fused residual instance), S = 2 at C = 48 behind a x2 operand, hop 60"),
    "s5_wide": (
        dict(in_channels=144, mid_channels=[192, 96, 48, 24], upsampling_scales=[2, 4, 5, 4], out_channels=2,
             spk_emb_size=512, use_spk_emb=True),
        "S = 5 at C = 48 and S = 4 at C = 24 (separate residual launches), decimating pair at scale 4, two outputs"),
    "odd_widths": (
        dict(in_channels=100, mid_channels=[192, 72, 40, 24], upsampling_scales=[4, 2, 2, 5], out_channels=1,
             spk_emb_size=64, use_spk_emb=False),
        "partial 48-channel groups (72, 40), C_in = 100 (not a multiple of 8 or 32) into a 192-channel conv, "
        "S = 2 behind x4 / x8 operands, no speaker"),
    "three_stage": (
        dict(in_channels=144, mid_channels=[96, 48, 24], upsampling_scales=[4, 4, 5], out_channels=1,
             spk_emb_size=512, use_spk_emb=True),
        "three stages (the whole-stage conditioning launches key on the stage count)"),
}

NAMES = tuple(CONFIGS)

# live_configs.npz: weights / inputs regenerate from these seeds (synth.py), B x F frames per case
SEED_W, SEED_X, B, F = 611, 612, 2, 9


def config(name) -> S.GeneratorConfig:
    return S.GeneratorConfig.from_kwargs(**CONFIGS[name][0])


def speaker_modes(name):
    """(True,) = with a speaker embedding; a generator built with use_spk_emb also runs without one."""
    return (True, False) if config(name).use_spk_emb else (False,)
