"""CPU tests of the loudness of live streams from raw audio (decode.StreamSession(loudness="audio")): when
a frame is final, that the windows a stream runs are still its window plan whatever the pushes, that the rings sized by
stream_loudness_ring_frames never lose a frame or a sample that is still needed, and the float64 reference
(tests/stream_loudness_ref.py) against the whole-file oracle - equal when frame 0 holds the peak, far from it on a signal
that rises."""
import numpy as np
import pytest

import stream_loudness_ref as R
from oracle import loudness_oracle as LO
from svcc23_fastsvc_amd import decode as Dc

HOPS = (64, 160, 256, 1024, 2048)


@pytest.mark.parametrize("hop", HOPS)
def test_final_frames_are_those_whose_last_sample_arrived(hop):
    """Frame f reads samples up to f hop + 1023: before the end it is final once seen hop >= f hop + 1024, at the end
    every frame is.  The lag is ceil(1024 / hop) - 1: 6 at hop 160."""
    lag = Dc.stream_loudness_lag(hop)
    assert lag == -(-1024 // hop) - 1 and Dc.stream_loudness_lag(160) == 6
    for seen in range(0, 3 * lag + 40):
        brute = sum(1 for f in range(seen) if f * hop + 1024 <= seen * hop)
        assert Dc.stream_final_frames(seen, False, hop) == brute == max(0, seen - lag), (hop, seen)
        assert Dc.stream_final_frames(seen, True, hop) == seen
    with pytest.raises(ValueError):
        Dc.stream_loudness_lag(0)


def _schedule(rng, F, max_push):
    """Pushes of 0..max_push frames that add up to F."""
    out, left = [], F
    while left:
        out.append(min(int(rng.integers(0, max_push + 1)), left))
        left -= out[-1]
    return out


@pytest.mark.parametrize("F", [1, 5, 40, 100])
@pytest.mark.parametrize("hop", [160, 256, 2048])
def test_rows_are_the_window_plan_whatever_the_pushes(F, hop):
    """stream_ready_rows over the FINAL frames: concatenated over a stream's pushes - the end arriving with the last chunk
    or alone after it - the rows are window_plan([F], core, context)."""
    rng = np.random.default_rng(F * 7 + hop)
    for core, context, max_push in ((32, 36, 48), (8, 4, 3), (4, 0, 1), (16, 8, 40)):
        plan = [r[1:] for r in Dc.window_plan([F], core, context)]
        for trial in range(6):
            sched = _schedule(rng, F, max_push)
            alone = trial % 2 == 1                       # (the end comes in a push of its own)
            seen = done = 0
            rows = []
            for i, n in enumerate(sched + ([0] if alone else [])):
                seen += n
                ended = i == len(sched) - (0 if alone else 1)
                ready = Dc.stream_ready_rows(Dc.stream_final_frames(seen, ended, hop), ended, core, context, done)
                done += len(ready)
                rows += ready
            assert rows == plan, (core, context, max_push, sched)


@pytest.mark.parametrize("hop", [64, 160, 256, 1024])
@pytest.mark.parametrize("core,context,max_push", [(4, 0, 1), (4, 0, 3), (8, 4, 2), (32, 36, 48), (16, 8, 40), (4, 4, 64)])
def test_the_rings_keep_every_frame_and_sample_still_needed(hop, core, context, max_push):
    """A model of the rings under random push schedules: ring position p % len remembers WHICH sample / frame it holds.
    Every frame that becomes final finds all the samples it reads in the audio ring (reflection at 0 and at the end
    included), every window that runs finds all its frames in the frame rings - ppg and excitation, written as they
    arrive, and lft, written as frames become final.  (4, 0, 1) at hop 64 and 160 is sized by the SAMPLE bound, (32, 36, 48)
    by the frame bound."""
    lag = Dc.stream_loudness_lag(hop)
    cap = Dc.stream_loudness_ring_frames(core, context, max_push, hop)
    frames_bound = Dc.stream_ring_frames(core, context, max_push + lag)
    samples_bound = -(-((max_push + lag) * hop + 1024) // hop)
    assert cap % 4 == 0 and max(frames_bound, samples_bound) <= cap < max(frames_bound, samples_bound) + 4
    if (core, context, max_push) == (4, 0, 1) and hop <= 160:
        assert samples_bound > frames_bound
    if (core, context, max_push) == (32, 36, 48):
        assert frames_bound > samples_bound
    rng = np.random.default_rng(hop + core)
    for F in (1, lag, lag + 1, 3 * cap + 5):
        if F < 1:
            continue
        T = F * hop
        audio = np.full(cap * hop, -1, np.int64)         # the absolute sample index a ring position holds
        arrived = np.full(cap, -1, np.int64)             # ... the frame of ppg / excitation
        lft = np.full(cap, -1, np.int64)                 # ... the frame of loudness
        seen = final = done = 0
        sched = _schedule(rng, F, max_push)
        for i, n in enumerate(sched):
            ended = i == len(sched) - 1
            p = np.arange(seen * hop, (seen + n) * hop)
            audio[p % (cap * hop)] = p
            f = np.arange(seen, seen + n)
            arrived[f % cap] = f
            seen += n
            new_final = Dc.stream_final_frames(seen, ended, hop)
            assert new_final - final <= max_push + lag
            for f in range(final, new_final):
                idx = f * hop - 1024 + np.arange(2048)
                if ended:                                # np.pad(..., "reflect") at both ends, repeatedly for T < 1025
                    idx = np.pad(np.arange(T), 2048 + T, mode="reflect")[idx + 2048 + T] if T > 1 else np.zeros(2048, np.int64)
                else:
                    idx = np.abs(idx)
                    idx = idx[1:] if idx[0] >= seen * hop else idx      # (element 0 has window weight 0: never read past the ring)
                assert idx.min() >= 0 and idx.max() < seen * hop
                assert np.array_equal(audio[idx % (cap * hop)], idx), (F, f, sched)
            f = np.arange(final, new_final)
            lft[f % cap] = f
            final = new_final
            for in_lo, in_hi, _, _ in Dc.stream_ready_rows(final, ended, core, context, done):
                f = np.arange(in_lo, in_hi)
                assert np.array_equal(arrived[f % cap], f) and np.array_equal(lft[f % cap], f), (F, in_lo, in_hi, sched)
                done += 1
        assert final == seen == F and done == -(-F // core)


@pytest.mark.parametrize("hop", [160, 256])
def test_reference_is_the_whole_file_oracle_when_frame_0_holds_the_peak(hop):
    """Frame 0 louder than every other frame (the whole-file function's extra frame F included): the running maximum is
    the utterance's from the start, and the reference is the whole-file oracle - to 1e-9 against its float64 arithmetic,
    and exactly once rounded to the float32 the oracle returns."""
    F = 24
    y = R.peak_first_signal(F, hop)
    P = LO.stft_power(y, hop)
    assert P.shape == (1025, F + 1) and P[:, 0].max() >= 1.1 * P[:, 1:].max()
    ref = R.stream_loudness_frames(y, R.SR, hop)
    db = np.maximum(10.0 * np.log10(np.maximum(1e-10, P)), 10.0 * np.log10(P.max()) - 80.0)
    db = db + LO.a_weighting(np.linspace(0.0, R.SR / 2.0, 1025))[:, None]
    whole64 = np.log(np.mean(10.0 ** (db / 20.0), axis=0) + 1e-5)[:F]
    whole = LO.loudness_extract(y, R.SR, hop)
    assert whole.shape == ((F + 1) * hop,) and np.array_equal(whole[::hop][:F], whole64.astype(np.float32))
    assert np.abs(ref - whole64).max() <= 1e-9
    assert np.array_equal(ref.astype(np.float32), whole[::hop][:F])
    assert np.array_equal(R.stream_loudness(y, R.SR, hop), np.repeat(ref, hop))


@pytest.mark.parametrize("hop", [160, 256])
def test_reference_is_causal_on_a_signal_that_rises(hop):
    """The sine that is 100 times louder from the middle on: before the jump the running floor lies far below the
    whole-file one, and the reference differs from the whole-file oracle by more than 1 in log loudness; where the running
    maximum has reached the utterance's, the two agree."""
    F = 24
    y = R.rising_signal(F, hop)
    ref = R.stream_loudness_frames(y, R.SR, hop)
    whole = LO.loudness_extract(y, R.SR, hop)[::hop][:F].astype(np.float64)
    d = np.abs(ref - whole)
    print(f"STREAM LOUDNESS oracle hop {hop}: |causal - whole file| per frame", " ".join(f"{v:.3g}" for v in d))
    assert d.max() > 1.0 and d[: F // 2 - 1024 // hop - 1].min() > 0.5
    assert d[F // 2 + 1024 // hop + 1:].max() <= 1e-2
    # ... and it does not look ahead: the frames in front of a later change of the audio keep their values
    z = y.copy()
    z[(F - 4) * hop:] *= 3.0
    keep = F - 4 - 1024 // hop - 1
    assert np.array_equal(R.stream_loudness_frames(z, R.SR, hop)[:keep], ref[:keep])
