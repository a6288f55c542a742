"""CPU tests of the forgetting horizon of StreamSession(norm="running", horizon=H): the float64 statement of the decayed fold
(decode.pool_running_sums with decay) against the weighted population taken directly, however the windows fall into
forwards; the host arithmetic of the horizon (decode.running_horizon_rows) against its closed forms; the host validation
(engine.check_norm_decay, decode.check_horizon); and, on the float64 reference (tests/running_horizon_ref.py), what
forgetting buys after a change of level."""
import math

import numpy as np
import pytest
import torch

from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd import synth as S
from svcc23_fastsvc_amd.engine import check_norm_decay


# ------------------------------------------------------------------------------------------------ pool_running_sums
MUL, CHUNK = 3, 16          # columns per frame; columns per partial sum (small: most ranges have several chunks)
P_CORE, P_CONTEXT, P_H = 8, 4, 12.0


def _forward(xs, rows, carry, forget):
    """One forward over `rows` = [(slot, k, in_lo, in_hi, lo, hi)] (slot order, a slot's windows ascending) of the streams
    xs[slot] (C, F MUL): the arrays as StreamSession builds them, the chunk sums of every row, the pool.  forget[(slot, k)]
    = (decay, weight) in frames, or None for the call without a horizon."""
    core = [Dc.chunk_sums(xs[s][:, a * MUL: e * MUL], (lo - a) * MUL, (hi - a) * MUL, CHUNK) for s, _, a, e, lo, hi in rows]
    look = [Dc.chunk_sums(xs[s][:, a * MUL: e * MUL], (hi - a) * MUL, (e - a) * MUL, CHUNK) for s, _, a, e, lo, hi in rows]
    extra = {} if forget is None else dict(decay=[forget[r[:2]][0] for r in rows], weight=[forget[r[:2]][1] for r in rows])
    return Dc.pool_running_sums(core, look, lens=[e - a for _, _, a, e, _, _ in rows], slot=[r[0] for r in rows],
                                own_lo=[lo - a for _, _, a, _, lo, _ in rows], prior=[r[4] for r in rows],
                                reset=[int(r[1] == 0) for r in rows], carry=carry, **extra)


def _run(xs, plans, cuts, forget):
    """The streams' windows in forwards: forward j takes windows cuts[j][s] .. cuts[j + 1][s] - 1 of every stream s.  Returns
    {(slot, k): stats}, and the final carry."""
    carry = {s: np.full((xs[s].shape[0], 2), np.nan) for s in range(len(xs))}       # (a reset row never looks)
    stats = {}
    for before, after in zip(cuts, cuts[1:]):
        rows = [(s, k) + tuple(plans[s][k][1:]) for s in range(len(xs)) for k in range(before[s], after[s])]
        if not rows:
            continue
        st, carry = _forward(xs, rows, carry, forget)
        stats.update({(r[0], r[1]): v for r, v in zip(rows, st)})
    return stats, carry


def _same_bits(a, b):
    return (a is None and b is None) or np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_decayed_pool_is_the_weighted_population_however_windows_fall_into_forwards():
    """Two streams of 75 and 53 frames (3 columns a frame, 5 channels; 10 and 7 windows), core 8, context 4, horizon 12,
    chunks of 16 columns: the rows of both in one forward, one window per forward, and four random splits.  Every window
    k > 0 has the mean and biased variance of the WEIGHTED population - a frame of core j < k with the product of the decays
    of the cores j + 1 .. k, its own core and look-ahead with weight 1 - to 1e-12, its weight being the weights' sum; window
    0 is a pass-through row; the carry is the weighted sum of all cores; every split gives the SAME BITS, carry included;
    and with decay 1 and weight N the bits are those of the call without them."""
    rng = np.random.default_rng(23)
    frames = [75, 53]
    xs = [rng.standard_normal((5, F * MUL)) * (3.0, 0.2)[i] + (1.5, -4.0)[i] for i, F in enumerate(frames)]
    plans = [Dc.window_plan([F], P_CORE, P_CONTEXT) for F in frames]
    n = [len(p) for p in plans]
    assert min(n) >= 6
    forget, plain_w, decays = {}, {}, {}
    for s in range(2):
        d, w, bd, _ = Dc.running_horizon_rows([p[1:] for p in plans[s]], P_H, None, P_CORE)
        d1, w1, _, _ = Dc.running_horizon_rows([p[1:] for p in plans[s]], None, None, P_CORE)
        for k in range(n[s]):
            forget[(s, k)], plain_w[(s, k)], decays[(s, k)] = (d[k], w[k]), (d1[k], w1[k]), d[k]
            assert d1[k] == 1.0 and w1[k] == plans[s][k][2] and bd[k] >= w[k]
    splits = {"one forward": [[0, 0], n], "window by window": [[min(j, n[0]), min(j, n[1])] for j in range(max(n) + 1)]}
    for t in range(4):
        cuts = [sorted(rng.integers(0, n[s] + 1, size=3).tolist()) for s in range(2)]
        splits[f"random {t}"] = [[0, 0]] + [[cuts[0][j], cuts[1][j]] for j in range(3)] + [n]
    results = {name: _run(xs, plans, cuts, forget) for name, cuts in splits.items()}
    stats, carry = results["one forward"]
    assert sorted(stats) == [(s, k) for s in range(2) for k in range(n[s])]

    def frame_weights(s, k, upto):
        """Per frame of [0, upto): the weight it has at window k of stream s."""
        w = np.ones(upto)
        for j in range(k):
            w[plans[s][j][3]: plans[s][j][4]] = math.prod(decays[(s, i)] for i in range(j + 1, k + 1))
        return w

    for (s, k), st in stats.items():
        _, a, e, lo, hi = plans[s][k]
        if k == 0:
            assert st is None                            # window 0 owns its whole row: the producer's statistics stay
            continue
        w = np.repeat(frame_weights(s, k, e), MUL)
        seen = xs[s][:, : e * MUL]
        np.testing.assert_allclose(forget[(s, k)][1] * MUL, w.sum(), rtol=1e-13, atol=0)
        L = (e - a) * MUL
        mean = st[:, 0] / L
        var = st[:, 1] / L - mean ** 2
        wmean = (seen * w).sum(axis=1) / w.sum()
        np.testing.assert_allclose(mean, wmean, rtol=1e-12, atol=0)
        np.testing.assert_allclose(var, (seen ** 2 * w).sum(axis=1) / w.sum() - wmean ** 2, rtol=1e-12, atol=0)
    for s in range(2):
        w = np.repeat(frame_weights(s, n[s] - 1, frames[s]), MUL)
        want = np.stack([(xs[s] * w).sum(axis=1), (xs[s] ** 2 * w).sum(axis=1)], axis=-1)
        np.testing.assert_allclose(carry[s], want, rtol=1e-12, atol=0)
    for name, (st2, carry2) in results.items():
        for key, v in stats.items():
            assert _same_bits(v, st2[key]), (name, key)
        for s in range(2):
            assert _same_bits(carry[s], carry2[s]), (name, s)
    # decay 1 and weight N: the existing call's bits
    old, old_carry = _run(xs, plans, splits["random 0"], None)
    new, new_carry = _run(xs, plans, splits["random 0"], plain_w)
    assert all(_same_bits(old[key], new[key]) for key in old) and all(_same_bits(old_carry[s], new_carry[s]) for s in range(2))
    assert not _same_bits(old[(0, 3)], stats[(0, 3)])
    with pytest.raises(ValueError, match="go together"):
        Dc.pool_running_sums([], [], [], [], [], [], [], {}, decay=[])


def test_decayed_pool_by_hand():
    """One channel, one slot, three windows of two-frame cores, decay 0.5: window 0 (pass-through) leaves the carry (4, 16);
    window 1 halves it, adds its core (6, 36) - the new carry (8, 44) - and its look-ahead (2, 4): (10, 48) over w = 0.5 * 2
    + 2 = 3 frames and one of look-ahead, 4 of its own 4 frames; window 2 halves again and adds (1, 1): (5, 23) over w = 0.5 *
    3 + 2 = 3.5 frames, of its own 7.  In one forward, and cut behind window 0."""
    c = lambda *v: np.array(v, dtype=np.float64).reshape(-1, 1, 2)                      # noqa: E731
    core = [c(4, 16), c(1, 6, 5, 30), c(1, 1)]
    look = [c(9, 9), c(2, 4), np.zeros((0, 1, 2))]
    args = dict(lens=[3, 4, 7], slot=[0, 0, 0], own_lo=[0, 1, 5], prior=[0, 2, 4], reset=[1, 0, 0])
    decay, weight = [1.0, 0.5, 0.5], [3.0, 4.0, 3.5]
    stats, carry = Dc.pool_running_sums(core, look, carry={0: np.array([[np.nan, np.nan]])}, decay=decay, weight=weight, **args)
    assert stats[0] is None
    np.testing.assert_array_equal(stats[1], [[10.0, 48.0]])
    np.testing.assert_array_equal(stats[2], [[10.0, 46.0]])
    np.testing.assert_array_equal(carry[0], [[5.0, 23.0]])
    head = {key: v[:1] for key, v in args.items()}
    tail = {key: v[1:] for key, v in args.items()}
    tail["reset"] = [0, 0]
    st0, carry0 = Dc.pool_running_sums(core[:1], look[:1], carry={0: np.array([[np.nan, np.nan]])}, decay=decay[:1],
                                       weight=weight[:1], **head)
    np.testing.assert_array_equal(carry0[0], [[4.0, 16.0]])
    st1, carry1 = Dc.pool_running_sums(core[1:], look[1:], carry=carry0, decay=decay[1:], weight=weight[1:], **tail)
    assert st0 == [None]
    np.testing.assert_array_equal(st1[0], stats[1])
    np.testing.assert_array_equal(st1[1], stats[2])
    np.testing.assert_array_equal(carry1[0], carry[0])


# --------------------------------------------------------------------------------------------- running_horizon_rows
def test_horizon_rows_against_their_closed_forms():
    """Core 32, context 36, H = 64.  w_k = sum_{j <= k} 32 e^{-(k - j) / 2} rises towards 32 / (1 - e^{-1/2}) and, after
    10 000 windows, has reached it to 1e-12 without passing it; fed window by window it is the same float as fed at once.
    A short last core decays by exp(-c / H) with ITS c.  The left context of 36 frames reaches two cores back: wmin =
    e^{-64 / 64} from window 2 on, e^{-32 / 64} for window 1 (whose context ends at frame 0, in core 0), 1 for window 0."""
    core, context, H = 32, 36, 64.0
    K = 10_000
    F = K * core + 20
    rows = [r[1:] for r in Dc.window_plan([F], core, context)]
    assert len(rows) == K + 1 and rows[-1][3] - rows[-1][2] == 20
    decay, weight, bound, w_all = Dc.running_horizon_rows(rows, H, None, core)
    lam = math.exp(-core / H)
    limit = core / (1.0 - lam)
    w = None
    for k, row in enumerate(rows[:K]):
        (d,), (wt,), (bd,), w_next = Dc.running_horizon_rows([row], H, w, core)
        assert (d, wt, bd) == (decay[k], weight[k], bound[k])
        assert k == 0 or w < w_next <= limit or w_next == w          # (monotone until it stands still)
        w = w_next
        assert d == (1.0 if k == 0 else lam) and wt == w + (row[1] - row[3])
    assert w <= limit and abs(w - limit) <= 1e-12 * limit
    (d,), (wt,), (bd,), w_last = Dc.running_horizon_rows(rows[K:], H, w)        # the short last window ALONE needs `core` ...
    assert d == math.exp(-20 / H) and w_last == d * w + 20 and w_last == w_all
    (d2,), (wt2,), (bd2,), _ = Dc.running_horizon_rows(rows[K:], H, w, core)
    assert (d2, wt2) == (d, wt) == (decay[K], weight[K]) and wt == w_last         # (no look-ahead at the end)
    assert bd2 == bound[K] == wt2 / math.exp(-(20 + 32) / H)                       # ... for wmin: core j ends 52 frames back
    assert all(b >= x for b, x in zip(bound, weight))
    assert bound[0] == weight[0] == 68.0 and decay[0] == 1.0
    assert bound[1] == weight[1] / math.exp(-32 / H)
    for k in (2, 3, 500, K - 1):
        assert bound[k] == weight[k] / math.exp(-64 / H), k
    # without a horizon: today's rule
    d, wt, bd, w = Dc.running_horizon_rows(rows[:4], None, None, core)
    assert d == [1.0] * 4 and wt == bd == [float(r[1]) for r in rows[:4]] and w == 128.0
    with pytest.raises(ValueError, match="w_prev"):
        Dc.running_horizon_rows(rows[1:2], H, None, core)
    with pytest.raises(ValueError, match="not a window"):
        Dc.running_horizon_rows([(0, 40, 8, 40)], H, 8.0, 16)


# ------------------------------------------------------------------------------------------------------- validation
def test_norm_decay_and_horizon_are_validated_on_the_host():
    lens = [68, 72, 8]
    #          slot       own_lo     own_hi       prior       reset      parity
    running = ([0, 0, 1], [0, 4, 0], [32, 36, 8], [0, 32, 0], [1, 0, 1], [1, 1, 0])
    ok = ([1.0, 0.5, 1.0], [68.0, 68.0, 8.0], [68.0, 100.0, 8.0])
    assert check_norm_decay(*ok, running, lens) == ok
    assert check_norm_decay(np.array(ok[0]), ok[1], tuple(ok[2]), running, lens) == ok

    def bad(i, b, v):
        arrays = [list(a) for a in ok]
        arrays[i][b] = v
        return arrays
    for args, what in (
            (bad(0, 1, 0.0), "row 1: decay"),
            (bad(0, 1, -0.5), "row 1: decay"),
            (bad(0, 2, 1.0000001), "row 2: decay"),
            (bad(0, 0, float("nan")), "row 0: .* finite"),
            (bad(1, 1, float("inf")), "row 1: .* finite"),
            (bad(2, 2, float("nan")), "row 2: .* finite"),
            (bad(1, 1, 67.5), "row 1: weight"),                    # less than the 72 - 4 frames of the row's own
            (bad(1, 2, 7.0), "row 2: weight"),
            (bad(2, 1, 67.9), "row 1: bound"),
            ([ok[0][:2], ok[1], ok[2]], "3 entries"),
            ([ok[0], ok[1], ok[2] + [1.0]], "3 entries"),
            ([None, ok[1], ok[2]], "three sequences"),
            ([ok[0], ["x", 1, 2], ok[2]], "three sequences"),
    ):
        with pytest.raises(ValueError, match=what):
            check_norm_decay(*args, running, lens)
    assert Dc.check_horizon(None, 32) is None and Dc.check_horizon(32, 32) == 32.0 and Dc.check_horizon(64.5, 32) == 64.5
    for h in (31.9, 0, -64, float("inf"), float("nan"), "a"):
        with pytest.raises(ValueError, match="horizon"):
            Dc.check_horizon(h, 32)


# ---------------------------------------------------------------------------------------------- the reference property
CORE, CONTEXT, FADE = 32, 36, 8
JUMP, GAIN, TOTAL = 160, 4.0, 320
# measured on the float64 reference (the test prints both): 1.03e-1 with horizon 64 against 3.73e-1 without, a ratio of
# 0.275; the bound is that ratio moved half-way to 1
RATIO = 0.637


def level_jump_stream(cfg, F=TOTAL, seed=612):
    """The 160-frame test stream's generator at F frames with every feature - ppg, lft, the excitation's amplitude - times
    4 from frame 160 on: a speaker who moves to the microphone."""
    b = S.synth_batch(cfg, 1, F, seed)
    hop = cfg.hop
    ppg, sine, lft = b.ppg.copy(), b.sine.copy(), b.lft.copy()
    ppg[:, :, JUMP:] *= GAIN
    sine[:, :, JUMP * hop:] *= GAIN
    lft[:, :, JUMP * hop:] *= GAIN
    return b, ppg, sine, lft


def test_forgetting_after_a_change_of_level():
    """On the float64 oracle, the recipe generator with weights seed 611, core 32, context 36, fade 8, 320 frames whose
    features are four times louder from frame 160 on.  The yardstick is the whole-utterance oracle of the loud part alone,
    frames [160 - 36, 320); compared over each of the last three cores (frames 224 .. 320), worst core against worst core,
    relative to max(1, |yardstick|max).  Measured: without a horizon the three cores are 3.73e-1, 2.87e-1 and 2.66e-1 away -
    half the population is still the quiet part - with horizon 64 they are 5.41e-2, 7.50e-2 and 1.03e-1: a ratio of 0.275,
    asserted as at most RATIO = 0.637.  horizon=None is tests/running_norm_ref.py's reference bit for bit, and window 0,
    which has no carry to forget, is norm="window"'s in all of them."""
    from oracle import fastsvc_oracle as O
    from running_horizon_ref import stream_reference
    from running_norm_ref import stream_reference as old_reference
    cfg = S.FULL_CONFIG
    hop = cfg.hop
    wf = S.fold_weight_norm(S.synth_state_dict(cfg, 611))
    assert Dc.receptive_field_frames(cfg) <= CONTEXT
    b, ppg, sine, lft = level_jump_stream(cfg)
    emb = b.spk_emb[0]
    t0 = JUMP - CONTEXT
    loud = O.forward_dedup(wf, cfg.upsampling_scales, ppg[:, :, t0:], sine[:, :, t0 * hop:], lft[:, :, t0 * hop:], emb[None],
                           dtype=torch.float64).numpy()[0, 0]
    mag = max(1.0, float(np.abs(loud).max()))
    runs, errs = {}, {}
    for name, H in (("none", None), ("64", 64.0)):
        runs[name], rows = stream_reference(wf, cfg.upsampling_scales, ppg, sine, lft, emb, CORE, CONTEXT, FADE, "running", H)
        assert runs[name].shape == (TOTAL * hop,) and len(rows) == 10 and np.isfinite(runs[name]).all()
        errs[name] = [float(np.abs(runs[name][lo * hop: hi * hop] - loud[(lo - t0) * hop: (hi - t0) * hop]).max()) / mag
                      for _, _, _, lo, hi in rows[-3:]]
        print(f"STREAM-HORIZON reference, horizon {name}: last three cores " + " ".join(f"{e:.3e}" for e in errs[name]))
    e_none, e_h = max(errs["none"]), max(errs["64"])
    print(f"STREAM-HORIZON reference: worst {e_h:.4e} with horizon 64, {e_none:.4e} without, ratio {e_h / e_none:.4f}")
    assert e_h <= RATIO * e_none, (e_h, e_none)
    # horizon=None is the reference without one, bit for bit
    old, _ = old_reference(wf, cfg.upsampling_scales, ppg, sine, lft, emb, CORE, CONTEXT, FADE, "running")
    assert np.array_equal(old.view(np.uint64), runs["none"].view(np.uint64))
    # window 0's core, short of the half fade zone it shares with window 1: no carry yet, nothing to forget (a stream of
    # 96 frames has the same window 0, frames [0, 68))
    own = (CORE - FADE // 2) * hop
    win, _ = stream_reference(wf, cfg.upsampling_scales, ppg[:, :, :96], sine[:, :, :96 * hop], lft[:, :, :96 * hop], emb,
                              CORE, CONTEXT, FADE, "window")
    for name in runs:
        assert np.array_equal(runs[name][:own].view(np.uint64), win[:own].view(np.uint64)), name
