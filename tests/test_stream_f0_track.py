"""CPU tests of the fixed-lag Viterbi F0 tracker (decode.F0Track, decode.f0_track_rule): the rule on the host
against the float64 reference tests/stream_f0_track_ref.py, which is written from the definition alone; what tracking buys on
a noise burst and on sub-harmonic modulations and that it changes nothing on clean signals; the fixed-lag properties; the
float32 model of the candidates against float64 (the GPU test's margins); and the host helpers of a tracked StreamSession -
the tracked frames, the ring bound under random push schedules, latencies, refusals.

The signals are the issue's as stated: per-frame reference YIN loses 4 of 97 frames on the burst and 4 and 8 on the two gated
modulations (the conditions hold without adjusting an amplitude), the tracked reference none at a look-ahead of 4 and 8."""
import numpy as np
import pytest

import stream_f0_ref as R
import stream_f0_track_ref as Q
from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd import synth as S

TAU_MAX = R.lags()[1]


@pytest.fixture(scope="module")
def refs():
    """name -> (audio, true frequency, hop, per-frame reference F0, reference candidates (F, 4, 2) float64): the tracker's
    own signals at hop 256, stream_f0_ref.f0_signals() at hop 160.  Computed once."""
    out = {}
    for name, (y, true) in Q.track_signals().items():
        hop = 256 if true else 160
        per, _, cands = Q.track_audio(y, hop)
        out[name] = (y, true, hop, per, cands)
    return out


def _rule(cands, lag=8, **kw):
    track = Dc.F0Track(lag=lag, **kw)
    return Dc.f0_track_rule(cands, TAU_MAX, R.SR, track, R.THRESHOLD)


# ------------------------------------------------------------------------------------------------- rule against reference

@pytest.mark.parametrize("lag", [0, 4, 8, 64])
def test_the_rule_equals_the_reference_exactly(refs, lag):
    for name, (_, _, _, _, cands) in refs.items():
        want = Q.track(cands, TAU_MAX, lag=lag)
        got = _rule(cands, lag)
        assert got.dtype == np.float64 and np.array_equal(got, want), name
        c32 = cands.astype(np.float32)                  # (float32 candidates, as the device has them: float32 out)
        got32 = _rule(c32, lag)
        assert got32.dtype == np.float32 and np.array_equal(got32, Q.track(c32, TAU_MAX, lag=lag)), name


def test_other_costs_and_zero_costs(refs):
    """Costs of zero are legal: no NaN (an absent state is never priced), still the reference's bits."""
    cands = refs["burst"][4]
    for kw in (dict(jump=0.0), dict(switch=0.0), dict(lag_bias=0.0), dict(jump=0.0, switch=0.0, lag_bias=0.0),
               dict(jump=3.0, switch=0.05, lag_bias=1.0)):
        got = _rule(cands, 8, **kw)
        assert np.isfinite(got).all()
        assert np.array_equal(got, Q.track(cands, TAU_MAX, lag=8, **kw)), kw
    with pytest.raises(ValueError):
        Dc.f0_track_rule(cands[:, :3], TAU_MAX, R.SR, Dc.F0Track(), R.THRESHOLD)


# --------------------------------------------------------------------------------------------------- what tracking buys

@pytest.mark.parametrize("name,lost", [("burst", 4), ("sub0.3", 4), ("sub0.6", 8)])
def test_tracking_recovers_the_frames_per_frame_yin_loses(refs, name, lost):
    """CONDITION: per-frame reference YIN has at least 4 bad frames (unvoiced, or more than 1 % off).  GATE: the tracked
    reference at lag 4 and 8 has none.  Measured: 4 -> 0, 4 -> 0, 8 -> 0."""
    y, true, hop, per, cands = refs[name]
    assert len(per) == 97 and y.dtype == np.float32
    bad = Q.bad_frames(per, true)
    print(f"{name}: per-frame YIN loses {bad} of {len(per)} frames")
    assert bad >= 4 and bad == lost
    for lag in (4, 8):
        tracked = Q.track(cands, TAU_MAX, lag=lag)
        print(f"{name}: tracked at lag {lag} loses {Q.bad_frames(tracked, true)}")
        assert Q.bad_frames(tracked, true) == 0, lag


def test_a_strong_modulation_is_reported_not_gated():
    """(a, lo, hi) = (1.0, 0.47, 0.53): per-frame YIN loses 12 frames, the tracker still 8 (DESIGN.md 4.10 reports it)."""
    y = Q.subharmonic_signal(1.0, 0.47, 0.53)
    per, tracked, _ = Q.track_audio(y, 256)
    print(f"sub1: per-frame {Q.bad_frames(per, Q.SUB_F0)}, tracked {Q.bad_frames(tracked, Q.SUB_F0)}")
    assert len(per) == len(tracked) == 97 and np.isfinite(tracked).all()      # (the figures are printed, not gated)


def test_clean_signals_keep_their_per_frame_value(refs):
    """tone110, tone339, glide, noise, zeros at hop 160, lag 8: tracked equals per-frame on EVERY frame, bit for bit in
    float64; nothing is NaN or inf.  At the edges of a voiced stretch voicing has hysteresis: on `gap` 11 of 61 frames around
    the silence are voiced that per-frame YIN calls unvoiced, on tone70.5 (at the floor of the range) 5 of 31 - and no frame
    the other way."""
    for name in ("tone110", "tone339", "glide", "noise", "zeros"):
        _, _, hop, per, cands = refs[name]
        tracked = _rule(cands, 8)
        assert hop == 160 and np.isfinite(tracked).all() and np.array_equal(tracked, per), name
    for name, more in (("gap", 11), ("tone70.5", 5)):
        _, _, _, per, cands = refs[name]
        tracked = _rule(cands, 8)
        assert np.isfinite(tracked).all()
        assert int(((tracked > 0) & (per == 0)).sum()) == more and not ((tracked == 0) & (per > 0)).any(), name
        both = (tracked > 0) & (per > 0)
        assert np.array_equal(tracked[both], per[both])


# ------------------------------------------------------------------------------------------------- fixed-lag properties

@pytest.mark.parametrize("lag", [0, 3, 8])
def test_frame_f_is_a_function_of_the_frames_up_to_f_plus_lag(refs, lag):
    for name in ("burst", "sub0.6", "gap"):
        cands = refs[name][4]
        whole = _rule(cands, lag)
        for f in range(0, len(cands), 5):
            assert _rule(cands[: f + lag + 1], lag)[f] == whole[f], (name, f)
            assert Q.track(cands[: f + lag + 1], TAU_MAX, lag=lag)[f] == whole[f]


def test_a_lag_of_all_frames_is_plain_viterbi(refs):
    for name in ("burst", "gap", "glide"):
        cands = refs[name][4][:60]
        plain = Q.f0_of(cands, Q.viterbi_states(cands, TAU_MAX))
        assert np.array_equal(_rule(cands, 60), plain) and np.array_equal(_rule(cands, 64), plain), name
    assert not np.array_equal(_rule(refs["burst"][4], 0), _rule(refs["burst"][4], 8))


# ------------------------------------------------------------------------------------------ the selection of the candidates

def test_the_reference_keeps_the_four_smallest_with_ties_to_the_smaller_lag():
    """A hand-made d' with seven local minima under the threshold: the four smallest d' are kept, of two equal ones the
    smaller lag, in ascending lag; one above the threshold and one at a plateau's right end are no candidates; the last lag
    needs no right neighbour.  The margin of a kept one reaches to the fifth-best."""
    tau_min, tau_max = 2, 40
    dn = np.full(tau_max + 1, 0.9)
    for t, v in ((5, 0.30), (9, 0.10), (13, 0.20), (17, 0.20), (21, 0.05), (25, 0.20), (29, 0.45), (33, 0.60), (40, 0.15)):
        dn[t] = v
    dn[36], dn[37] = 0.4, 0.4                            # a plateau: 36 falls and does not rise - a minimum; 37 does not fall
    c = Q.candidates(dn, tau_min, tau_max, 0.5)
    assert c.minima.tolist() == [5, 9, 13, 17, 21, 25, 29, 36, 40]
    assert c.lags == [9, 13, 21, 40]                     # 0.05, 0.10, 0.15 and the FIRST of the three 0.20
    assert c.pairs[:, 1].tolist() == [0.10, 0.20, 0.05, 0.15]
    assert c.margin[1] == 0.0 and abs(c.margin[0] - 0.10) < 1e-12        # (the fifth-best is 0.20, at lag 17)
    assert c.pairs[3, 0] == 40.0 and abs(c.pairs[0, 0] - 9.0) < 1e-12    # (no parabola at the range's end; a symmetric one)
    few = Q.candidates(np.where(np.arange(tau_max + 1) == 9, 0.1, 0.9), tau_min, tau_max, 0.5)
    assert few.lags == [9] and few.margin[0] == pytest.approx(0.4) and np.isinf(few.pairs[1:, 1]).all()
    c32 = Q.candidates(dn.astype(np.float32), tau_min, tau_max, 0.5)
    assert c32.lags == c.lags and c32.pairs.dtype == np.float32


def test_wide_signals_offer_more_than_four_minima():
    """Searched down to 24 Hz the wide signals have frames with more than four local minima, so a fifth-best exists and the
    selection matters: what tests/test_f0_candidates_gpu.py relies on."""
    for name, (y, hop) in (("tone339", (Q.wide_signals()["tone339"], 256)), ("glide", (Q.wide_signals()["glide"], 160))):
        _, cs, dns = Q.audio_candidates(y, hop, f0_floor=Q.WIDE_FLOOR)
        most = max(len(c.minima) for c in cs)
        assert most >= 8 and sum(len(c.minima) > 4 for c in cs) >= len(cs) // 2, (name, most)
        for c, dn in zip(cs, dns):                       # (kept: the four smallest of the minima, in ascending lag)
            assert len(c.lags) == min(4, len(c.minima)) and c.lags == sorted(c.lags) and set(c.lags) <= set(c.minima.tolist())
            rest = [t for t in c.minima.tolist() if t not in c.lags]
            if rest:
                assert max(dn[t] for t in c.lags) <= min(dn[t] for t in rest) < 0.5
                assert min(c.margin) <= min(dn[t] for t in rest) - max(dn[t] for t in c.lags) + 1e-15


# ------------------------------------------------------------------------------------- the float32 model of the candidates

def test_the_float32_model_keeps_the_measured_bounds():
    """A SAMPLE of the measurement behind the bounds of tests/test_f0_candidates_gpu.py (the whole of it is
    ``python tests/stream_f0_track_ref.py``: every frame of Q.measured_cases(), minutes): every 8th frame of the burst, a
    modulation, tone70.5 and gap at hop 256 and of the wide signals (f0_floor 24: more than four minima a frame) - the float32
    model of the kernel's d' gives the reference's candidates, none lost or gained, within the figures measured over all
    frames: 4.56e-6 for d', 5.42e-7 for s, 7.36e-4 lags for tau_hat (f0_floor 24 alone: 2.68e-6, 3.47e-7, 1.76e-4)."""
    sig = R.f0_signals()
    narrow = [(y, 256, R.F0_FLOOR) for y in (Q.burst_signal(), Q.subharmonic_signal(0.6, 0.47, 0.53), sig["tone70.5"], sig["gap"])]
    wide = [(y, 256, Q.WIDE_FLOOR) for y in Q.wide_signals().values()]
    for cases, (dn, s_, tau), most in ((narrow, (4.56e-6, 5.42e-7, 7.36e-4), 1), (wide, (2.68e-6, 3.47e-7, 1.76e-4), 8)):
        m = Q.measure_float32_model(cases, every=8)
        assert m["dn"] <= dn and m["s"] <= s_ and m["tau"] <= tau, m
        assert m["lost"] == 0.0 and m["gained"] == 0 and m["most"] >= most, m


# ---------------------------------------------------------------------------------------------------------- host helpers

def test_tracked_frames():
    assert [Dc.stream_tracked_frames(f, False, 8) for f in (0, 5, 8, 9, 40)] == [0, 0, 0, 1, 32]
    assert [Dc.stream_tracked_frames(f, True, 8) for f in (0, 5, 40)] == [0, 5, 40]
    assert Dc.stream_tracked_frames(7, False, 0) == 7


def _schedule(rng, F, max_push):
    out, left = [], F
    while left:
        out.append(min(int(rng.integers(0, max_push + 1)), left))
        left -= out[-1]
    return out


@pytest.mark.parametrize("hop", [64, 160, 1024])
@pytest.mark.parametrize("track_lag", [0, 8, 64])
@pytest.mark.parametrize("core,context,max_push", [(4, 0, 1), (8, 4, 2), (32, 36, 48), (4, 4, 64)])
def test_the_rings_keep_every_frame_the_tracker_and_the_windows_need(hop, track_lag, core, context, max_push):
    """test_stream_f0.py's model of the rings with the tracker's: candidates and backpointers are written as frames become
    final, the tracked F0 and the excitation as frames are EMITTED - every frame once, in order, its trace reading the
    backpointers of the frames up to min(f + lag, final - 1) and its own candidates - and every window, ready by the tracked
    frames, finds all its frames in every ring.  A stream may end in a push that brings nothing."""
    lag = Dc.stream_loudness_lag(hop)
    cap = Dc.stream_track_ring_frames(core, context, max_push, hop, track_lag)
    frames_bound = Dc.stream_ring_frames(core, context, max_push + lag + track_lag)
    samples_bound = -(-((max_push + lag) * hop + 1024) // hop)
    assert cap % 4 == 0 and max(frames_bound, samples_bound) <= cap < max(frames_bound, samples_bound) + 4
    assert Dc.stream_track_ring_frames(core, context, max_push, hop, 0) == Dc.stream_loudness_ring_frames(core, context, max_push, hop)
    rng = np.random.default_rng(hop + core + track_lag)
    for F in (1, track_lag, lag + track_lag + 1, 3 * cap + 5):
        if F < 1:
            continue
        ppg = np.full(cap, -1, np.int64)
        rings = {k: np.full(cap, -1, np.int64) for k in ("lft", "cand", "back", "f0", "exc")}
        emitted = []
        seen = final = tracked = done = 0
        sched = _schedule(rng, F, max_push) + [0]        # (the end comes alone, with an empty push)
        for i, n in enumerate(sched):
            ended = i == len(sched) - 1
            f = np.arange(seen, seen + n)
            ppg[f % cap] = f
            seen += n
            new_final = Dc.stream_final_frames(seen, ended, hop)
            new = np.arange(final, new_final)
            assert len(new) <= max_push + lag
            for k in ("lft", "cand", "back"):
                rings[k][new % cap] = new
            final = new_final
            upto = Dc.stream_tracked_frames(final, ended, track_lag)
            emit = np.arange(tracked, upto)
            assert len(emit) <= max_push + lag + track_lag <= cap and final - tracked <= cap
            for f in emit:
                e = min(f + track_lag, final - 1)
                g = np.arange(f, e + 1)
                assert np.array_equal(rings["back"][g % cap], g) and rings["cand"][f % cap] == f, (F, f, sched)
            rings["f0"][emit % cap] = emit
            rings["exc"][emit % cap] = emit
            emitted += emit.tolist()
            tracked = upto
            for in_lo, in_hi, _, _ in Dc.stream_ready_rows(tracked, ended, core, context, done):
                f = np.arange(in_lo, in_hi)
                assert in_hi <= tracked and np.array_equal(ppg[f % cap], f), (F, in_lo, in_hi, sched)
                for k in ("lft", "exc"):
                    assert np.array_equal(rings[k][f % cap], f), (k, F, in_lo, in_hi, sched)
                done += 1
        assert emitted == list(range(F)) and tracked == final == seen == F and done == -(-F // core)


def _cfg():
    return S.GeneratorConfig(in_channels=8, mid_channels=(16, 8, 8, 4), upsampling_scales=(2, 4, 4, 5), out_channels=1,
                             spk_emb_size=16, use_spk_emb=True)


def test_session_arguments_and_latencies():
    """StreamSession._check_args, with no device: f0_track needs f0="audio" and an F0Track; the ring and the latencies grow
    by the tracker's lag; f0_track=None resolves to what it did."""
    cfg = _cfg()
    hop = cfg.hop
    kw = dict(core=8, context=4, fade=4, max_push=12, loudness="audio", f0="audio")
    base = Dc.StreamSession._check_args(cfg, hop, **kw)
    assert base["f0_track"] is None and base["track_lag"] == 0
    assert base["cap"] == Dc.stream_loudness_ring_frames(8, 4, 12, hop)
    for lag in (0, 8, 64):
        a = Dc.StreamSession._check_args(cfg, hop, f0_track=Dc.F0Track(lag=lag), **kw)
        assert a["track_lag"] == lag and a["lag"] == base["lag"] == 6
        assert a["cap"] == Dc.stream_track_ring_frames(8, 4, 12, hop, lag) >= base["cap"]
        same = ("core", "context", "fade", "max_push", "lag", "channels", "_slice", "f0_threshold")
        assert {k: a[k] for k in same} == {k: base[k] for k in same}

        class _Session:                                  # (the latency properties read these four)
            core, context, lag, track_lag = a["core"], a["context"], a["lag"], a["track_lag"]
        assert Dc.StreamSession.latency_frames.fget(_Session) == 8 + 4 + 6 + lag
        assert Dc.StreamSession.latency_frames_max.fget(_Session) == 16 + 4 + 6 + lag
    for bad in (dict(kw, f0="given"), dict(core=8, context=4, fade=4), dict(kw, loudness="given", f0="given")):
        with pytest.raises(ValueError, match="f0_track"):
            Dc.StreamSession._check_args(cfg, hop, f0_track=Dc.F0Track(), **bad)
    for not_a_track in (8, "viterbi", dict(lag=8)):
        with pytest.raises(ValueError, match="F0Track"):
            Dc.StreamSession._check_args(cfg, hop, f0_track=not_a_track, **kw)
    # (a call finalises at most 2048 frames of a stream: at hop 1 the loudness lag is 1023, and 1024 + 1023 fit without a tracker)
    Dc.StreamSession._check_args(cfg, 1, **dict(kw, max_push=1024))
    with pytest.raises(ValueError, match="the tracker's lag must be at most 2048"):
        Dc.StreamSession._check_args(cfg, 1, f0_track=Dc.F0Track(lag=64), **dict(kw, max_push=1024))
    assert Dc.StreamSession._check_args(cfg, hop, **kw) == base          # (nothing was left behind by the refusals)


def test_f0_track_is_validated_and_immutable():
    t = Dc.F0Track()
    assert (t.lag, t.cand_threshold, t.lag_bias, t.jump, t.switch, t.unvoiced) == (8, 0.5, 0.2, 1.0, 0.3, None)
    assert Dc.F0_CANDIDATES == 4
    assert Dc.F0Track(lag=0).lag == 0 and Dc.F0Track(lag=64).lag == 64 and Dc.F0Track(unvoiced=0).unvoiced == 0.0
    assert Dc.F0Track(lag=np.int64(5)).lag == 5 and hash(Dc.F0Track()) == hash(Dc.F0Track(lag=8))
    with pytest.raises(Exception):
        t.lag = 3
    for bad in (dict(lag=-1), dict(lag=65), dict(lag=2.5), dict(lag="x"), dict(cand_threshold=0.0), dict(cand_threshold=-1.0),
                dict(jump=-0.1), dict(switch=float("nan")), dict(lag_bias=float("inf")), dict(unvoiced=-1.0),
                dict(unvoiced=float("nan")), dict(jump=None)):
        with pytest.raises(ValueError):
            Dc.F0Track(**bad)
    assert Dc.F0Track() == t                             # (still usable after each)
