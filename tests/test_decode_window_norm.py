"""CPU tests of the host side of convert_windowed(norm="utterance"): batches that hold whole utterances
(decode.grouped_window_batches), the float64 statement of the pool-and-scatter rule of csrc/fastsvc_normgroup.hip
(decode.pool_norm_sums) and the host validation of norm_groups (engine.check_norm_groups)."""
import numpy as np
import pytest

from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd.engine import check_norm_groups


# ------------------------------------------------------------------------------------------ grouped_window_batches
FRAMES, CORE, CONTEXT = [160, 52, 8, 70], 16, 8


def test_grouped_batches_hold_whole_utterances():
    rows = Dc.window_plan(FRAMES, CORE, CONTEXT)
    batches = Dc.grouped_window_batches(rows, 16)
    assert sorted(r for chunk in batches for r in chunk) == list(range(len(rows)))       # every row exactly once
    assert all(1 <= len(chunk) <= 16 for chunk in batches)
    where = {r: k for k, chunk in enumerate(batches) for r in chunk}
    for u in range(len(FRAMES)):
        mine = [r for r in range(len(rows)) if rows[r][0] == u]
        assert len({where[r] for r in mine}) == 1, u                                       # one batch
        chunk = batches[where[mine[0]]]
        j = chunk.index(mine[0])
        assert chunk[j: j + len(mine)] == mine, u                                          # adjacent and ascending
        assert [rows[r][3] for r in mine] == sorted(rows[r][3] for r in mine)
    # first-fit, most windows first: 10 + 5 + 1 share the first batch of 16, the 4 windows of utterance 1 open the next
    assert [sorted({rows[r][0] for r in chunk}) for chunk in batches] == [[0, 2, 3], [1]]
    # a stitch layout takes this batching as any other
    layout, _ = Dc.stitch_layout(rows, batches, 160, 8)
    assert [lay["width"] for lay in layout] == [max(rows[r][2] - rows[r][1] for r in chunk) * 160 for chunk in batches]


def test_grouped_batches_refuse_an_utterance_that_does_not_fit():
    rows = Dc.window_plan(FRAMES, CORE, CONTEXT)
    with pytest.raises(ValueError, match=r"utterance 0 has 10 windows but max_batch is 4.*larger core or a larger max_batch"):
        Dc.grouped_window_batches(rows, 4)
    assert Dc.grouped_window_batches(rows, 10)                                             # exactly fits


# --------------------------------------------------------------------------------------------------- pool_norm_sums
def _cut(x, rows, mul):
    """Per-row owned sums of x (C, T) cut by window_plan rows: (s1, s2, owned, lens), columns = frames x mul."""
    s1 = np.stack([x[:, lo * mul: hi * mul].sum(axis=1) for _, _, _, lo, hi in rows])
    s2 = np.stack([(x[:, lo * mul: hi * mul] ** 2).sum(axis=1) for _, _, _, lo, hi in rows])
    return s1, s2, [(hi - lo) * mul for _, _, _, lo, hi in rows], [(e - a) * mul for _, a, e, _, _ in rows]


def test_pooled_sums_give_the_whole_tensors_mean_and_variance_in_every_row():
    rng = np.random.default_rng(5)
    mul = 3
    xs = [rng.standard_normal((5, 37 * mul)) * 3.0 + 1.5, rng.standard_normal((5, 37 * mul)) * 0.2 - 4.0]
    rows = Dc.window_plan([37], 8, 4)
    assert len(rows) == 5 and len({e - a for _, a, e, _, _ in rows}) > 1                   # rows of different lengths
    parts = [_cut(x, rows, mul) for x in xs]                                               # two utterances in one call
    s1 = np.concatenate([p[0] for p in parts])
    s2 = np.concatenate([p[1] for p in parts])
    owned = parts[0][2] + parts[1][2]
    lens = parts[0][3] + parts[1][3]
    group = [0] * 5 + [5] * 5
    q1, q2 = Dc.pool_norm_sums(s1, s2, owned, lens, group)
    for b in range(10):
        x = xs[b // 5]
        mean = q1[b] / lens[b]
        var = q2[b] / lens[b] - mean ** 2
        np.testing.assert_allclose(mean, x.mean(axis=1), rtol=1e-12, atol=0)
        np.testing.assert_allclose(var, x.var(axis=1), rtol=1e-12, atol=0)


def test_a_singleton_row_that_owns_everything_keeps_its_sums():
    rng = np.random.default_rng(6)
    s1, s2 = rng.standard_normal((3, 4)), rng.random((3, 4))
    # row 1 is alone and whole; rows 0 and 2 form a group
    q1, q2 = Dc.pool_norm_sums(s1, s2, owned=[6, 9, 3], lens=[8, 9, 5], group=[0, 1, 0])
    assert np.array_equal(q1[1], s1[1]) and np.array_equal(q2[1], s2[1])
    np.testing.assert_allclose(q1[0], (s1[0] + s1[2]) * 8 / 9, rtol=1e-15)
    np.testing.assert_allclose(q2[2], (s2[0] + s2[2]) * 5 / 9, rtol=1e-15)
    # alone but not whole: its own sums rescaled to its length
    q1, _ = Dc.pool_norm_sums(s1, s2, owned=[6, 4, 3], lens=[8, 9, 5], group=[0, 1, 0])
    np.testing.assert_allclose(q1[1], s1[1] * 9 / 4, rtol=1e-15)


# ------------------------------------------------------------------------------------------------------- validation
def test_norm_groups_are_validated_on_the_host():
    lens = [8, 8, 5]
    assert check_norm_groups(([0, 0, 2], [0, 4, 0], [4, 8, 5]), lens) == ([0, 0, 2], [0, 4, 0], [4, 8, 5])
    for bad, what in (
            (([0, 0, 2], [0, 4, 0], [4, 9, 5]), "row 1: owned"),           # own_hi past the row's length
            (([0, 0, 2], [0, 4, 5], [4, 8, 5]), "row 2: owned"),           # own_lo == own_hi
            (([0, 0, 2], [-1, 4, 0], [4, 8, 5]), "row 0: owned"),          # negative own_lo
            (([0, 2, 2], [0, 4, 0], [4, 8, 5]), "row 1: group"),           # group[b] > b
            (([0, 0, 1], [0, 4, 0], [4, 8, 5]), "row 2: group"),           # group[group[b]] != group[b]
            (([0, -1, 2], [0, 4, 0], [4, 8, 5]), "row 1: group"),
            (([0, 0], [0, 4, 0], [4, 8, 5]), "3 entries"),
            ((None, [0, 4, 0], [4, 8, 5]), "three sequences"),
    ):
        with pytest.raises(ValueError, match=what):
            check_norm_groups(bad, lens)


def test_convert_windowed_refuses_an_unknown_norm():
    class _Closed:
        _closed, n = False, 1
        model = signal_generator = None
        device, hop, frames, channels = "cpu", 160, [8], 4
    with pytest.raises(ValueError, match="norm must be"):
        Dc.DecodeSession.convert_windowed(_Closed(), core=8, context=4, fade=0, norm="batch")
