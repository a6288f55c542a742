"""Host logic of the windowed decode (decode.window_plan / window_batches / stitch_windows / stitch_layout /
receptive_field_frames), without a GPU.  The receptive field is checked against the float64 oracle: with that much
context the speakerless generator's output on a window's core IS the whole-utterance output."""
import numpy as np
import pytest
import torch

import config_matrix as CM
from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd import synth as S


# ---------------------------------------------------------------------------------------------------- window_plan
@pytest.mark.parametrize("context", [0, 8, 40])
@pytest.mark.parametrize("core", [4, 32])
def test_window_plan_geometry(core, context):
    frames = [1, 3, 4, 31, 32, 33, 100]
    rows = Dc.window_plan(frames, core, context)
    for u, F in enumerate(frames):
        mine = [r for r in rows if r[0] == u]
        K = -(-F // core)
        assert len(mine) == K
        # the cores partition [0, F), in order
        assert mine[0][3] == 0 and mine[-1][4] == F
        for k, (_, in_lo, in_hi, lo, hi) in enumerate(mine):
            assert (lo, hi) == (k * core, min((k + 1) * core, F)) and lo < hi
            # reads: the core plus the context, clipped to the utterance
            assert (in_lo, in_hi) == (max(0, lo - context), min(F, hi + context))
            assert 0 <= in_lo <= lo and hi <= in_hi <= F
        if K == 1:
            assert mine == [(u, 0, F, 0, F)]             # one row, the whole utterance
    assert [r[0] for r in rows] == sorted(r[0] for r in rows)


def test_window_plan_rejects_sizes_that_are_not_multiples_of_4():
    for core, context in ((0, 0), (6, 0), (8, 2), (8, -4), (3, 0)):
        with pytest.raises(ValueError):
            Dc.window_plan([10], core, context)
    with pytest.raises(ValueError):
        Dc.window_plan([10, 0], 8, 0)


def test_window_batches_share_batches_across_utterances():
    frames = [100, 7, 64, 33]
    rows = Dc.window_plan(frames, 32, 8)
    batches = Dc.window_batches(rows, max_batch=4, pad_tolerance=0.125)
    lens = [r[2] - r[1] for r in rows]
    assert batches == Dc.bucket_ragged(range(len(rows)), lens, 4, 0.125)
    assert sorted(r for b in batches for r in b) == list(range(len(rows)))
    assert any(len({rows[r][0] for r in b}) > 1 for b in batches)          # windows of several utterances in one batch
    for b in batches:
        assert len(b) <= 4 and min(lens[r] for r in b) >= 0.875 * lens[b[0]]


# ------------------------------------------------------------------------------------------------- stitch_windows
def _random_rows(rng, frames, core, context, hop):
    rows = Dc.window_plan(frames, core, context)
    return rows, [rng.standard_normal((r[2] - r[1]) * hop) for r in rows]


def test_stitch_without_a_fade_is_concatenation_bit_for_bit():
    rng = np.random.default_rng(1)
    hop = 6
    rows, ys = _random_rows(rng, [33, 8, 100], 32, 8, hop)
    out = Dc.stitch_windows(ys, rows, hop, 0)
    for u, F in enumerate([33, 8, 100]):
        want = np.concatenate([ys[r][(row[3] - row[1]) * hop: (row[4] - row[1]) * hop]
                               for r, row in enumerate(rows) if row[0] == u])
        assert out[u].dtype == np.float64 and out[u].shape == (F * hop,)
        assert np.array_equal(out[u].view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("fade", [2, 8])
def test_stitch_fade_weights(fade):
    """A constant stays the constant (the two weights sum to 1); window k-1 = 0 and window k = 1 shows the weight itself:
    (j + 0.5) / fh inside the zone, 0 before and 1 after, strictly inside (0, 1); samples outside the zones are the
    owning window's."""
    hop, core, context = 5, 8, 4
    frames = [29, 8, 17]                                 # 29: a last window of 5 frames; 17: of 1 frame (shorter than half a zone)
    rows = Dc.window_plan(frames, core, context)
    const = [np.full((r[2] - r[1]) * hop, 0.25) for r in rows]
    for y in Dc.stitch_windows(const, rows, hop, fade):
        assert np.all(y == 0.25)                         # (exact for a power of two: (1 - w) + w rounds to 1)
    for y in Dc.stitch_windows([c * 1.2 for c in const], rows, hop, fade):
        assert np.all(np.abs(y - 0.3) <= 2.0 ** -53)     # (otherwise to the last bit: the two products round)
    ks = [(r[3] // core) for r in rows]
    steps = [np.full((r[2] - r[1]) * hop, float(k)) for r, k in zip(rows, ks)]
    fh = fade * hop
    for u, y in enumerate(Dc.stitch_windows(steps, rows, hop, fade)):
        T = frames[u] * hop
        want = np.empty(T)
        for t in range(T):
            k = min(int(t // (core * hop)), -(-frames[u] // core) - 1)
            want[t] = k
            for b in range(1, -(-frames[u] // core)):
                z0 = b * core * hop - fh // 2
                if z0 <= t < z0 + fh:
                    w = (t - z0 + 0.5) / fh
                    assert 0.0 < w < 1.0
                    want[t] = (1.0 - w) * (b - 1) + w * b
        assert np.array_equal(y, want), u
    # the rule's PCM-16 is to_pcm16's on the float64 values
    rng = np.random.default_rng(2)
    ys = [rng.standard_normal(len(c)) for c in const]
    st = Dc.stitch_windows(ys, rows, hop, fade)
    assert np.array_equal(Dc.to_pcm16(st[0]), np.clip(np.rint(st[0] * 32767.0), -32768, 32767).astype(np.int16))


def test_stitch_rejects_bad_fades():
    hop = 4
    rows, ys = _random_rows(np.random.default_rng(3), [40], 8, 4, hop)
    Dc.stitch_windows(ys, rows, hop, 8)                  # min(core, 2 context) = 8 is allowed
    for fade in (1, 3, 7, -2, 10, 12):                   # not even; above min(core, 2 context)
        with pytest.raises(ValueError):
            Dc.stitch_windows(ys, rows, hop, fade)
    rows, ys = _random_rows(np.random.default_rng(3), [40], 8, 0, hop)
    Dc.stitch_windows(ys, rows, hop, 0)
    with pytest.raises(ValueError):
        Dc.stitch_windows(ys, rows, hop, 2)              # no context: nothing to fade over
    rows, ys = _random_rows(np.random.default_rng(3), [40], 4, 8, hop)
    with pytest.raises(ValueError):
        Dc.stitch_windows(ys, rows, hop, 6)              # longer than the core
    with pytest.raises(ValueError):
        Dc._check_window_sizes(8, 4, 10)                 # (the rule the session applies before anything runs)


def test_stitch_layout_writes_every_sample_once_and_pairs_every_zone():
    """Whatever the batches, every utterance sample is in exactly one row's run; a zone is resolved by exactly one of its
    two rows - from the other's staged slot when that one runs in an earlier batch, from y when both share a batch."""
    hop, core, context, fade = 4, 8, 4, 6
    frames = [29, 8, 17, 64]
    rows = Dc.window_plan(frames, core, context)
    for max_batch, order in ((3, 1), (64, 1), (2, -1)):
        batches = Dc.window_batches(rows, max_batch, 0.125)[::order]
        layout, stage_elems = Dc.stitch_layout(rows, batches, hop, fade)
        seen = [np.zeros(f * hop, int) for f in frames]
        slots = {}
        for k, (chunk, lay) in enumerate(zip(batches, layout)):
            assert lay["width"] == max(rows[r][2] - rows[r][1] for r in chunk) * hop and lay["half"] == fade * hop // 2
            ends = []
            for j, r in enumerate(chunk):
                u, lo, hi = lay["runs"][j]
                assert u == rows[r][0] == lay["utt"][j]
                seen[u][lo:hi] += 1
                assert lay["dst_off"][j] % 8 == 0 and all(lay["dst_off"][j] >= e for e in ends)
                ends.append(lay["dst_off"][j] + hi - lo)
                for side in ("left", "right"):
                    mode, src = lay[side + "_mode"][j], lay[side + "_src"][j]
                    if mode in (1, 2):
                        assert 0 <= src and src + fade * hop <= stage_elems
                        slots.setdefault(src, []).append((mode, k))
                    if mode == 3:
                        nb = chunk.index(r + 1 if side == "right" else r - 1)
                        assert src // lay["width"] == nb
            assert lay["total"] >= max(ends)
        assert all((s == 1).all() for s in seen)
        for src, uses in slots.items():                  # staged in an earlier batch than it is read
            assert sorted(m for m, _ in uses) == [1, 2]
            assert dict(uses)[1] < dict(uses)[2]
        if max_batch == 64:
            assert stage_elems == 0 or len(batches) > 1
    layout, stage_elems = Dc.stitch_layout(rows, Dc.window_batches(rows, 3, 0.125), hop, 0)
    assert stage_elems == 0 and all(set(lay["left_mode"] + lay["right_mode"]) == {0} for lay in layout)


# ----------------------------------------------------------------------------------------- receptive_field_frames
def _oracle_window_error(cfg, R_ctx, F, lo, hi, seed_w=611, seed_x=612):
    """max |window oracle - whole oracle| on the core [lo, hi), relative to max(1, |ref|max): the window is run alone on
    the frames [lo - R_ctx, hi + R_ctx) of the utterance, without a speaker embedding, float64."""
    from oracle import fastsvc_oracle as O
    w = S.fold_weight_norm(S.synth_state_dict(cfg, seed_w))
    b = S.synth_batch(cfg, 1, F, seed_x)
    hop = cfg.hop
    run = lambda a, e: O.forward_dedup(w, cfg.upsampling_scales, b.ppg[:, :, a:e], b.sine[:, :, a * hop: e * hop],   # noqa: E731
                                       b.lft[:, :, a * hop: e * hop], None, dtype=torch.float64).numpy()
    whole = run(0, F)
    a, e = max(0, lo - R_ctx), min(F, hi + R_ctx)
    win = run(a, e)
    ref = whole[..., lo * hop: hi * hop]
    got = win[..., (lo - a) * hop: (hi - a) * hop]
    return float(np.abs(got - ref).max()) / max(1.0, float(np.abs(whole).max()))


def test_receptive_field_of_the_recipe_generator_is_exact_and_not_over_reported():
    cfg = S.FULL_CONFIG
    R = Dc.receptive_field_frames(cfg)
    assert R <= 40
    assert R == Dc.receptive_field_frames(S.GeneratorConfig.from_kwargs(use_spk_emb=False))
    at_R = _oracle_window_error(cfg, R, 160, 64, 96)
    short = _oracle_window_error(cfg, R - 8, 160, 64, 96)
    print(f"R = {R}: window error {at_R:.3e} at R, {short:.3e} at R - 8")
    assert at_R <= 1e-9
    assert short > 1e-6


@pytest.mark.parametrize("name", ["tiny"] + list(CM.NAMES))
def test_receptive_field_of_other_configurations(name):
    cfg = S.TINY_CONFIG if name == "tiny" else CM.config(name)
    R = Dc.receptive_field_frames(cfg)
    assert 1 <= R <= 64
    err = _oracle_window_error(cfg, R, 2 * R + 24, R + 4, R + 20)         # 4 frames of real input beyond the window
    print(f"{name}: R = {R}, window error {err:.3e}")
    assert err <= 1e-9


def test_forward_limit_is_the_one_the_library_states():
    assert S.max_forward_frames(S.FULL_CONFIG) == 69905                  # T >= 11 184 811 samples is refused at hop 160
    assert (S.max_forward_frames(S.FULL_CONFIG) + 1) * 160 >= 11184811 > S.max_forward_frames(S.FULL_CONFIG) * 160
