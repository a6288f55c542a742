"""CPU tests of the host side of StreamSession(norm="running"): the float64 statement of the running pool of
csrc/fastsvc_normgroup.hip (decode.pool_running_sums) against a brute-force concatenation, however the windows fall into
forwards; the host validation of norm_running (engine.check_norm_running); and the property that makes the mode worth
having, on the float64 reference (tests/running_norm_ref.py): late windows of a stream are closer to the whole-utterance
result than per-window statistics leave them."""
import numpy as np
import pytest
import torch

from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd import synth as S
from svcc23_fastsvc_amd.engine import check_norm_running


# ------------------------------------------------------------------------------------------------ pool_running_sums
MUL, CHUNK = 3, 16          # columns per frame; columns per partial sum (small: most ranges have several chunks)


def _forward(xs, rows, carry):
    """One forward over `rows` = [(slot, k, in_lo, in_hi, lo, hi)] (slot order, a slot's windows ascending) of the streams
    xs[slot] (C, F MUL): the six arrays as StreamSession builds them, the chunk sums of every row, the pool."""
    core = [Dc.chunk_sums(xs[s][:, a * MUL: e * MUL], (lo - a) * MUL, (hi - a) * MUL, CHUNK) for s, _, a, e, lo, hi in rows]
    look = [Dc.chunk_sums(xs[s][:, a * MUL: e * MUL], (hi - a) * MUL, (e - a) * MUL, CHUNK) for s, _, a, e, lo, hi in rows]
    return Dc.pool_running_sums(core, look, lens=[e - a for _, _, a, e, _, _ in rows], slot=[r[0] for r in rows],
                                own_lo=[lo - a for _, _, a, _, lo, _ in rows], prior=[r[4] for r in rows],
                                reset=[int(r[1] == 0) for r in rows], carry=carry)


def _run(xs, plans, cuts):
    """The streams' windows in forwards: forward j takes windows cuts[j][s] .. cuts[j + 1][s] - 1 of every stream s.  Returns
    {(slot, k): stats}, and the final carry."""
    carry = {s: np.full((xs[s].shape[0], 2), np.nan) for s in range(len(xs))}       # (a reset row never looks)
    stats = {}
    for before, after in zip(cuts, cuts[1:]):
        rows = [(s, k) + tuple(plans[s][k][1:]) for s in range(len(xs)) for k in range(before[s], after[s])]
        if not rows:
            continue
        st, carry = _forward(xs, rows, carry)
        stats.update({(r[0], r[1]): v for r, v in zip(rows, st)})
    return stats, carry


def test_running_pool_is_the_prefix_statistics_however_windows_fall_into_forwards():
    """Two streams of 75 and 37 frames (3 columns a frame, 5 channels), core 8, context 4, chunks of 16 columns: the rows of
    both in one forward, one window per forward, and four random splits.  Every window k > 0 gets the mean and variance of
    its stream's columns [0, in_hi MUL) to 1e-12; window 0 is a pass-through row; and because the rule is one left fold -
    carry, earlier cores, own core, look-ahead - every split gives the SAME BITS, carry included."""
    rng = np.random.default_rng(11)
    frames = [75, 37]
    xs = [rng.standard_normal((5, F * MUL)) * (3.0, 0.2)[i] + (1.5, -4.0)[i] for i, F in enumerate(frames)]
    plans = [Dc.window_plan([F], 8, 4) for F in frames]
    n = [len(p) for p in plans]
    splits = {"one forward": [[0, 0], n], "window by window": [[min(j, n[0]), min(j, n[1])] for j in range(max(n) + 1)]}
    for t in range(4):
        cuts = [sorted(rng.integers(0, n[s] + 1, size=3).tolist()) for s in range(2)]
        splits[f"random {t}"] = [[0, 0]] + [[cuts[0][j], cuts[1][j]] for j in range(3)] + [n]
    results = {name: _run(xs, plans, cuts) for name, cuts in splits.items()}
    stats, carry = results["one forward"]
    assert sorted(stats) == [(s, k) for s in range(2) for k in range(n[s])]
    for (s, k), st in stats.items():
        _, a, e, lo, hi = plans[s][k]
        if k == 0:
            assert st is None                            # window 0 owns its whole row: the producer's statistics stay
            continue
        L = (e - a) * MUL
        mean = st[:, 0] / L
        var = st[:, 1] / L - mean ** 2
        seen = xs[s][:, : e * MUL]
        np.testing.assert_allclose(mean, seen.mean(axis=1), rtol=1e-12, atol=0)
        np.testing.assert_allclose(var, seen.var(axis=1), rtol=1e-12, atol=0)
    for s in range(2):
        want = np.stack([xs[s].sum(axis=1), (xs[s] ** 2).sum(axis=1)], axis=-1)
        np.testing.assert_allclose(carry[s], want, rtol=1e-12, atol=0)         # the cores tile the stream
    for name, (st2, carry2) in results.items():
        for key, v in stats.items():
            assert (v is None and st2[key] is None) or np.array_equal(v.view(np.uint64), st2[key].view(np.uint64)), (name, key)
        for s in range(2):
            assert np.array_equal(carry[s].view(np.uint64), carry2[s].view(np.uint64)), (name, s)


def test_running_pool_by_hand():
    """Slot 3 with two rows in the batch and a carry, slot 5 reset with own_lo > 0 (not a pass-through row), an empty
    look-ahead."""
    c = lambda *v: np.array(v, dtype=np.float64).reshape(-1, 1, 2)                      # noqa: E731
    core = [c(1, 10, 2, 20), c(4, 40), c(100, 1000)]
    look = [c(8, 80), np.zeros((0, 1, 2)), c(200, 2000)]
    stats, carry = Dc.pool_running_sums(core, look, lens=[12, 6, 9], slot=[3, 3, 5], own_lo=[4, 2, 1], prior=[20, 24, 1],
                                        reset=[0, 0, 1], carry={3: np.array([[0.5, 5.0]]), 5: np.array([[np.nan, np.nan]])})
    np.testing.assert_array_equal(stats[0], np.array([[11.5, 115.0]]) * 12 / 28)     # 0.5 + 1 + 2 + 8, N = 20 + 12 - 4
    np.testing.assert_array_equal(stats[1], np.array([[7.5, 75.0]]) * 6 / 28)        # 0.5 + 1 + 2 + 4, N = 24 + 6 - 2
    np.testing.assert_array_equal(stats[2], np.array([[300.0, 3000.0]]) * 9 / 9)     # reset: the NaN carry is not read
    np.testing.assert_array_equal(carry[3], [[7.5, 75.0]])
    np.testing.assert_array_equal(carry[5], [[100.0, 1000.0]])


# ------------------------------------------------------------------------------------------------------- validation
def test_norm_running_is_validated_on_the_host():
    lens = [68, 72, 8]
    #      slot       own_lo     own_hi       prior       reset      parity
    ok = ([0, 0, 1], [0, 4, 0], [32, 36, 8], [0, 32, 0], [1, 0, 1], [1, 1, 0])
    assert check_norm_running(ok, lens, 2) == ok
    assert check_norm_running(ok, lens) == ok

    def bad(i, b, v):
        arrays = [list(a) for a in ok]
        arrays[i][b] = v
        return tuple(arrays)
    for args, what in (
            (bad(2, 1, 73), "row 1: core"),                        # own_hi past the row's length
            (bad(1, 1, 36), "row 1: core"),                        # own_lo == own_hi
            (bad(1, 0, -1), "row 0: core"),                        # negative own_lo
            (bad(3, 1, 3), "row 1: prior"),                        # own_lo > prior
            (bad(3, 2, 4), "row 2: a reset row"),                  # reset with prior != own_lo
            (bad(0, 2, 2), "row 2: slot"),                         # not one of the carry's two
            (bad(0, 0, -1), "row 0: slot"),
            (bad(0, 0, 1), "row 1: slots must ascend"),
            (bad(5, 1, 0), "row 1: .* one parity"),
            (bad(5, 2, 2), "row 2: parity"),
            (bad(4, 1, 1), "row 1: a reset row"),                  # (prior 32 != own_lo 4) ...
            (bad(3, 1, 28), "row 1: .* window order"),             # prior does not continue row 0's core
            ((ok[0][:2],) + ok[1:], "3 entries"),
            ((None,) + ok[1:], "six sequences"),
            (ok[:5], "six sequences"),
    ):
        with pytest.raises(ValueError, match=what):
            check_norm_running(args, lens, 2)
    with pytest.raises(ValueError, match="row 1: only the first row"):     # ... and a reset row in mid-slot
        check_norm_running(([0, 0], [0, 4], [32, 36], [0, 4], [1, 1], [0, 0]), [68, 72], 1)


# ---------------------------------------------------------------------------------------------- the reference property
CORE, CONTEXT, FADE = 32, 36, 8


def _rel(got, ref):
    return float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))


def test_running_statistics_bring_late_windows_closer_to_the_whole_utterance():
    """On the float64 oracle, the recipe generator with weights seed 611, core 32, context 36, fade 8.

    160 frames (batch seed 612): over each of the last three cores, the error against the whole-utterance oracle under the
    running reference is at most HALF of what per-window statistics leave (measured where the rule was proposed: 2.3e-2
    against 8.3e-2, worst core against worst core), and window 0's core is identical in both.
    52 frames (seed 613): window 0 already sees everything (and window 1, with the carry, too) - the whole-utterance
    oracle to 1e-12."""
    from oracle import fastsvc_oracle as O
    from running_norm_ref import stream_reference
    cfg = S.FULL_CONFIG
    hop = cfg.hop
    wf = S.fold_weight_norm(S.synth_state_dict(cfg, 611))
    assert Dc.receptive_field_frames(cfg) <= CONTEXT
    b = S.synth_batch(cfg, 1, 160, 612)
    emb = b.spk_emb[0]
    whole = O.forward_dedup(wf, cfg.upsampling_scales, b.ppg, b.sine, b.lft, emb[None], dtype=torch.float64).numpy()[0, 0]
    run, rows = stream_reference(wf, cfg.upsampling_scales, b.ppg, b.sine, b.lft, emb, CORE, CONTEXT, FADE, "running")
    win, _ = stream_reference(wf, cfg.upsampling_scales, b.ppg, b.sine, b.lft, emb, CORE, CONTEXT, FADE, "window")
    assert run.shape == win.shape == whole.shape == (160 * hop,) and len(rows) == 5
    mag = max(1.0, float(np.abs(whole).max()))
    errs = {}
    for name, y in (("running", run), ("window", win)):
        errs[name] = [float(np.abs(y[lo * hop: hi * hop] - whole[lo * hop: hi * hop]).max()) / mag for _, _, _, lo, hi in rows]
        print(f"STREAM-NORM reference, {name}: per core " + " ".join(f"{e:.2e}" for e in errs[name]))
    assert max(errs["running"][-3:]) <= 0.5 * max(errs["window"][-3:]), errs
    # window 0's core, short of the half fade zone it shares with window 1
    own = (CORE - FADE // 2) * hop
    assert np.array_equal(run[:own], win[:own])
    b = S.synth_batch(cfg, 1, 52, 613)
    whole = O.forward_dedup(wf, cfg.upsampling_scales, b.ppg, b.sine, b.lft, emb[None], dtype=torch.float64).numpy()[0, 0]
    run, rows = stream_reference(wf, cfg.upsampling_scales, b.ppg, b.sine, b.lft, emb, CORE, CONTEXT, FADE, "running")
    assert rows[0][1:3] == (0, 52) and len(rows) == 2
    err = _rel(run, whole)
    print(f"STREAM-NORM reference, 52 frames: {err:.2e} to the whole-utterance oracle")
    assert err <= 1e-12, err
