"""Host-side tests (no GPU) of checked live streams: StreamSession's new constructor arguments, the span a window row is
judged on (decode.stream_check_spans) against a brute-force search through decode.stitch_windows, and the rows a
flagged row takes along into a fallback run (decode.stream_rerun_rows)."""
import numpy as np
import pytest

from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd import synth as S


def test_check_args_resolve_checked_and_fallback():
    cfg, hop = S.FULL_CONFIG, 160
    got = Dc.StreamSession._check_args(cfg, hop)
    assert got["checked"] is False and got["fallback"] == ("bfloat16",)
    got = Dc.StreamSession._check_args(cfg, hop, checked=True, fallback="float32")          # a string is one name
    assert got["checked"] is True and got["fallback"] == ("float32",)
    got = Dc.StreamSession._check_args(cfg, hop, checked=1, fallback=["bfloat16", "float32"])
    assert got["checked"] is True and got["fallback"] == ("bfloat16", "float32")
    assert Dc.StreamSession._check_args(cfg, hop, checked=True, fallback=())["fallback"] == ()
    for bad in ("float64", ("bfloat16", "half"), ["bf16"]):
        with pytest.raises(ValueError, match="fallback storage must be one of"):
            Dc.StreamSession._check_args(cfg, hop, checked=True, fallback=bad)
    with pytest.raises(ValueError, match="fallback storage must be one of"):                 # (also when nothing is checked)
        Dc.StreamSession._check_args(cfg, hop, fallback="float8")


HOP, CORE, CONTEXT = 4, 4, 2


def _plan(frames):
    """window_plan's rule for one utterance, written out: the sessions' sizes are multiples of 4 (window_plan checks
    that), the rule and stitch_windows are not bound to them, and a context of 2 frames keeps the brute force small."""
    return [(0, max(0, lo - CONTEXT), min(frames, lo + CORE + CONTEXT), lo, min(frames, lo + CORE)) for lo in range(0, frames, CORE)]


def _stream_rows(plan):
    """window_plan's rows (u, in_lo, in_hi, lo, hi) of ONE utterance as the StreamRows a session would run."""
    return [Dc.StreamRow(0, k, in_lo, in_hi, lo, hi, k == len(plan) - 1) for k, (_, in_lo, in_hi, lo, hi) in enumerate(plan)]


@pytest.mark.parametrize("fade", [2, 0])
@pytest.mark.parametrize("frames", [1, 4, 5, 13])
def test_spans_are_exactly_the_samples_that_reach_the_stitched_stream(frames, fade):
    """Every sample of every window row, one at a time, set to NaN: stitch_windows' result has a NaN iff the sample lies
    in the row's span."""
    plan = _plan(frames)
    assert len(plan) == -(-frames // CORE)
    half = fade * HOP // 2
    lo, hi = Dc.stream_check_spans(_stream_rows(plan), HOP, half)
    rng = np.random.default_rng(frames)
    ys = [rng.standard_normal((r[2] - r[1]) * HOP) for r in plan]
    assert np.isfinite(Dc.stitch_windows(ys, plan, HOP, fade)[0]).all()
    inside = outside = 0
    for r, y in enumerate(ys):
        assert 0 <= lo[r] <= hi[r] <= y.size
        for j in range(y.size):
            keep = y[j]
            y[j] = np.nan
            reaches = bool(np.isnan(Dc.stitch_windows(ys, plan, HOP, fade)[0]).any())
            y[j] = keep
            assert reaches == (lo[r] <= j < hi[r]), (r, j, lo[r], hi[r])
            inside += reaches
            outside += not reaches
    # every sample of the stream comes from one row, or - in a fade zone - from two
    zones = sum(min(2 * half, frames * HOP - (plan[k][4] * HOP - half)) for k in range(len(plan) - 1))
    assert inside == frames * HOP + zones
    assert (outside > 0) == (len(plan) > 1)


def test_spans_take_plain_tuples_of_a_session_in_any_mix():
    rows = [Dc.StreamRow(2, 0, 0, 6, 0, 4, False), Dc.StreamRow(2, 1, 2, 8, 4, 8, False), Dc.StreamRow(0, 3, 10, 13, 12, 13, True)]
    assert Dc.stream_check_spans(rows, 4, 4) == ([0, 4, 4], [20, 24, 12])
    assert Dc.stream_check_spans(rows, 4, 0) == ([0, 8, 8], [16, 24, 12])


def test_rerun_rows_are_the_flagged_rows_stream_mates_in_order():
    def row(s, k):
        return Dc.StreamRow(s, k, 0, 8, 0, 4, False)
    rows = [row(0, 3), row(0, 4), row(1, 0), row(2, 7), row(2, 8), row(2, 9), row(5, 1)]
    assert Dc.stream_rerun_rows(rows, []) == []
    assert Dc.stream_rerun_rows(rows, [2]) == [2]
    assert Dc.stream_rerun_rows(rows, [1]) == [0, 1]
    assert Dc.stream_rerun_rows(rows, [4]) == [3, 4, 5]
    assert Dc.stream_rerun_rows(rows, [6, 0]) == [0, 1, 6]
    assert Dc.stream_rerun_rows(rows, [5, 3, 4]) == [3, 4, 5]
    assert Dc.stream_rerun_rows(rows, range(len(rows))) == list(range(len(rows)))
    # a stream interleaved with another (no session orders rows like this, the rule holds anyway)
    mixed = [row(0, 0), row(1, 0), row(0, 1), row(1, 1)]
    assert Dc.stream_rerun_rows(mixed, [2]) == [0, 2]
