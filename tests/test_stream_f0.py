"""CPU tests of the F0 of live streams from raw audio (decode.StreamSession(f0="audio")): the float64
reference of the estimator (tests/stream_f0_ref.py) on synthetic audio, the float32 model of the kernel's arithmetic against
it - where the margins of the GPU tests come from - a host model of the rings and the finalisation order, and what
check_stream_chunks refuses in the new mode."""
import numpy as np
import pytest

import stream_f0_ref as R
from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd.engine import f0_lags

HOPS = (160, 256)

# Measured on the CPU with the reference, hop 160 and 256 (the figures DESIGN.md 4.10 quotes):
#   steady tones, interior frames: largest relative error 8.8e-5 (339 Hz; 2.1e-6 at 70.5 Hz)      -> gated at 2e-4, below 1 %
#   glide 110 -> 220 Hz in 0.4 s, interior frames, against the frequency at the frame's centre: 0.79 %  -> gated at 1 %
#   1e-3 white noise and digital silence: unvoiced on every frame, d' finite everywhere
TONE_BOUND = 2e-4
GLIDE_BOUND = 1e-2
# float32 model against the reference, all 498 frames of the signals at both hops: max |d'_32 - d'_64| = 4.6e-6, every
# decision and lag equal, largest relative F0 difference 1.07e-7.  The GPU tests use four times these.
DN_F32 = 4.6e-6
F0_F32 = 1.07e-7


@pytest.fixture(scope="module")
def picks():
    """{(name, hop): (audio, [(Pick, d') per frame])}: the reference on every signal, computed once."""
    out = {}
    for name, y in R.f0_signals().items():
        for hop in HOPS:
            out[name, hop] = (y, [R.yin_frame(R.frame(y, f, hop), full=True) for f in range(1 + len(y) // hop)])
    return out


def test_lags_and_their_limits():
    assert f0_lags(24000) == (70, 343) == R.lags()
    assert f0_lags(24000, 23.5, 340.0)[1] == 1022
    for bad in ((24000, 23.0, 340.0), (24000, 70.0, 48000.0), (24000, 340.0, 70.0), (24000, 0.0, 340.0), (0, 70.0, 340.0)):
        with pytest.raises(ValueError):
            f0_lags(*bad)


@pytest.mark.parametrize("hop", HOPS)
def test_reference_on_steady_tones(picks, hop):
    worst = 0.0
    for freq in R.TONES:
        y, ref = picks[f"tone{freq:g}", hop]
        inter = R.interior_frames(len(y), hop)
        assert len(inter) >= 8
        err = max(abs(ref[f][0].f0 - freq) / freq for f in inter)
        print(f"STREAM F0 reference hop {hop}: tone {freq} Hz relative error {err:.3g}")
        worst = max(worst, err)
    assert worst <= TONE_BOUND < 1e-2


@pytest.mark.parametrize("hop", HOPS)
def test_reference_on_the_glide(picks, hop):
    y, ref = picks["glide", hop]
    freq = R.glide_freq()
    inter = R.interior_frames(len(y), hop)
    assert all(ref[f][0].f0 > 0 for f in inter)
    err = max(abs(ref[f][0].f0 - freq[f * hop]) / freq[f * hop] for f in inter)
    print(f"STREAM F0 reference hop {hop}: glide relative error {err:.3g}")
    assert err <= GLIDE_BOUND


@pytest.mark.parametrize("hop", HOPS)
def test_reference_voicing(picks, hop):
    """Noise and zeros are unvoiced on every frame; nothing anywhere is NaN or inf; voiced -> silence -> voiced follows the
    audio: the frames that lie wholly in the silence are unvoiced, the frames wholly in a tone are at 150 Hz."""
    for (name, h), (y, ref) in picks.items():
        if h != hop:
            continue
        assert all(np.isfinite(d).all() and np.isfinite(p.f0) for p, d in ref), name
        if name in ("noise", "zeros"):
            assert all(p.f0 == 0.0 for p, _ in ref), name
    y, ref = picks["gap", hop]
    for f, (p, _) in enumerate(ref):
        lo, hi = f * hop - 1024, f * hop + 1024
        if lo >= 3200 and hi <= 6400:
            assert p.f0 == 0.0, f
        if (lo >= 0 and hi <= 3200) or (lo >= 6400 and hi <= 9600):
            assert abs(p.f0 - 150.0) <= 150.0 * TONE_BOUND, f


@pytest.mark.parametrize("hop", HOPS)
def test_float32_model_against_the_reference(picks, hop):
    """The float32 arithmetic of the kernel, modelled in numpy, on a third of the frames: d' within DN_F32 of the
    reference's, the same decision and lag on every frame, F0 within F0_F32; and at most 5 % of ALL frames have a reference
    margin below 4 DN_F32 - the frames the GPU test may leave out."""
    low = total = 0
    for (name, h), (y, ref) in picks.items():
        if h != hop:
            continue
        total += len(ref)
        low += sum(1 for p, _ in ref if p.margin < 4 * DN_F32)
        for f in range(0, len(ref), 3):
            (p, d), (q, e) = ref[f], R.yin_frame_f32(R.frame(y, f, hop), full=True)
            assert np.abs(d - e.astype(np.float64)).max() <= DN_F32, (name, f)
            assert (p.f0 > 0) == (q.f0 > 0) and p.tau == q.tau, (name, f)
            if p.f0 > 0:
                assert abs(p.f0 - q.f0) <= F0_F32 * p.f0, (name, f)
    print(f"STREAM F0 reference hop {hop}: {low} of {total} frames have a margin below {4 * DN_F32:.3g}")
    assert low <= 0.05 * total


def test_value_depends_on_the_frame_alone_and_never_on_its_first_sample():
    """x[0] is never read: frame 0's is sample 1024 by reflection, which a live stream whose hop divides 1024 has not
    received when the frame is final."""
    y = R.voiced_stream(12, 256, seed=1)
    x = R.frame(y, 0, 256)
    z = x.copy()
    z[0] = 123.0
    assert R.yin_frame(x) == R.yin_frame(z) and R.yin_frame(x).f0 > 0
    assert R.yin_frame_f32(x) == R.yin_frame_f32(z)


# ----------------------------------------------------------------------------------------- rings and finalisation order

def _schedule(rng, F, max_push):
    """Pushes of 0..max_push frames that add up to F."""
    out, left = [], F
    while left:
        out.append(min(int(rng.integers(0, max_push + 1)), left))
        left -= out[-1]
    return out


@pytest.mark.parametrize("hop", [64, 160, 256, 1024])
@pytest.mark.parametrize("core,context,max_push", [(4, 0, 1), (4, 0, 3), (8, 4, 2), (32, 36, 48), (16, 8, 40), (4, 4, 64)])
def test_every_frame_is_finalised_once_in_order_before_any_window_reads_it(hop, core, context, max_push):
    """test_stream_loudness.py's model of the rings with the f0 and excitation rings added: ppg is written as frames
    arrive; lft, raw f0, shifted f0 and the EXCITATION as frames become final - the excitation step after the f0 step of the
    same call, reading the shifted f0 it wrote.  Every frame is finalised exactly once, in order (the phase recurrence
    needs that), from samples the audio ring still holds - x[0] left out, as the estimator leaves it out - and every window
    finds all its frames in all five frame rings."""
    lag = Dc.stream_loudness_lag(hop)
    cap = Dc.stream_loudness_ring_frames(core, context, max_push, hop)
    rng = np.random.default_rng(hop + core)
    for F in (1, lag, lag + 1, 3 * cap + 5):
        if F < 1:
            continue
        T = F * hop
        audio = np.full(cap * hop, -1, np.int64)         # the absolute sample index a ring position holds
        ppg = np.full(cap, -1, np.int64)                 # ... the frame, per frame ring
        rings = {k: np.full(cap, -1, np.int64) for k in ("lft", "f0", "f0s", "exc")}
        finalised = []
        phase_at = 0                                     # the frame the carried phase stands in front of
        seen = final = done = 0
        sched = _schedule(rng, F, max_push)
        for i, n in enumerate(sched):
            ended = i == len(sched) - 1
            p = np.arange(seen * hop, (seen + n) * hop)
            audio[p % (cap * hop)] = p
            f = np.arange(seen, seen + n)
            ppg[f % cap] = f
            seen += n
            new_final = Dc.stream_final_frames(seen, ended, hop)
            assert new_final - final <= max_push + lag <= cap
            new = np.arange(final, new_final)
            for f in new:                                # launch 1: one block per frame, in any order
                idx = f * hop - 1024 + np.arange(1, 2048)                      # (x[0] is never read)
                idx = R.reflect_index(idx, T) if ended else np.abs(idx)
                assert idx.min() >= 0 and idx.max() < seen * hop
                assert np.array_equal(audio[idx % (cap * hop)], idx), (F, f, sched)
            rings["lft"][new % cap] = new
            rings["f0"][new % cap] = new
            rings["f0s"][new % cap] = new
            if len(new):                                 # launch 2: the recurrence over the call's frames, from the carried phase
                assert phase_at == new[0]
                assert np.array_equal(rings["f0s"][new % cap], new)
                rings["exc"][new % cap] = new
                phase_at = int(new[-1]) + 1
            finalised += new.tolist()
            final = new_final
            for in_lo, in_hi, _, _ in Dc.stream_ready_rows(final, ended, core, context, done):
                f = np.arange(in_lo, in_hi)
                assert in_hi <= final
                assert np.array_equal(ppg[f % cap], f), (F, in_lo, in_hi, sched)
                for k, r in rings.items():
                    assert np.array_equal(r[f % cap], f), (k, F, in_lo, in_hi, sched)
                done += 1
        assert finalised == list(range(F)) and final == seen == F and done == -(-F // core)


# -------------------------------------------------------------------------------------------------- check_stream_chunks

def test_check_stream_chunks_in_the_new_mode():
    C, hop = 6, 160
    rng = np.random.default_rng(0)

    def chunk(n, **extra):
        d = dict(ppg=rng.standard_normal((n, C)).astype(np.float32), audio=rng.standard_normal(n * hop).astype(np.float32))
        d.update(extra)
        return d

    ok = {3: chunk(4), 5: chunk(0)}
    parts, ids, end = Dc.check_stream_chunks(ok, [5], {3: 0, 5: 1}, C, hop, 8, "audio", "audio")
    assert ids == [3, 5] and end == [5]
    assert parts[3][0] == 4 and parts[3][2] is None and parts[3][3].shape == (4 * hop,) and parts[5][0] == 0
    assert np.array_equal(parts[3][1], ok[3]["ppg"]) and np.array_equal(parts[3][3], ok[3]["audio"])
    bad = [
        {3: chunk(4, f0=np.zeros(4, np.float32))},                       # an f0 key: the session makes it
        {3: dict(ppg=chunk(4)["ppg"])},                                  # no audio
        {3: chunk(4, lft=np.zeros(4 * hop, np.float32))},                # the other loudness mode's array
        {3: dict(ppg=np.zeros((4, C), np.float32), audio=np.zeros(4 * hop + 1, np.float32))},
        {3: chunk(9)},                                                   # more than max_push
        {7: chunk(1)},                                                   # not open
    ]
    for chunks in bad:
        before = {k: {a: np.array(v, copy=True) for a, v in ch.items()} for k, ch in chunks.items()}
        with pytest.raises(ValueError):
            Dc.check_stream_chunks(chunks, [], {3: 0, 5: 1}, C, hop, 8, "audio", "audio")
        for k, ch in chunks.items():                                     # (the parts are left as they were)
            assert set(ch) == set(before[k]) and all(np.array_equal(ch[a], before[k][a]) for a in ch)
    with pytest.raises(ValueError, match="loudness"):
        Dc.check_stream_chunks(ok, [], {3: 0, 5: 1}, C, hop, 8, "given", "audio")
    # the default keeps the present behaviour: f0 is required, and comes back
    given = {3: dict(ppg=np.zeros((2, C), np.float32), f0=np.ones(2, np.float32), audio=np.zeros(2 * hop, np.float32))}
    parts, _, _ = Dc.check_stream_chunks(given, [], {3: 0}, C, hop, 8, "audio")
    assert np.array_equal(parts[3][2], np.ones(2, np.float32))
    with pytest.raises(ValueError):
        Dc.check_stream_chunks({3: chunk(2)}, [], {3: 0}, C, hop, 8, "audio")


def test_session_arguments():
    """StreamSession._check_args, with no device: f0="audio" needs loudness="audio", the lags must fit the frame, and the
    ring sizes, lag and latencies are loudness="audio"'s."""
    from svcc23_fastsvc_amd import synth as S
    cfg = S.GeneratorConfig(in_channels=8, mid_channels=(16, 8, 8, 4), upsampling_scales=(2, 4, 4, 5), out_channels=1,
                            spk_emb_size=16, use_spk_emb=True)
    hop = cfg.hop
    base = Dc.StreamSession._check_args(cfg, hop, core=8, context=4, fade=4, loudness="audio")
    a = Dc.StreamSession._check_args(cfg, hop, core=8, context=4, fade=4, loudness="audio", f0="audio")
    assert a["f0"] == "audio" and base["f0"] == "given"
    assert {k: v for k, v in a.items() if not k.startswith("f0")} == {k: v for k, v in base.items() if not k.startswith("f0")}
    with pytest.raises(ValueError, match="loudness"):
        Dc.StreamSession._check_args(cfg, hop, core=8, context=4, fade=4, f0="audio")
    with pytest.raises(ValueError):
        Dc.StreamSession._check_args(cfg, hop, core=8, context=4, fade=4, loudness="audio", f0="audio", f0_floor=20.0)
    with pytest.raises(ValueError):
        Dc.StreamSession._check_args(cfg, hop, core=8, context=4, fade=4, loudness="audio", f0="audio", f0_threshold=0.0)
    with pytest.raises(ValueError):
        Dc.StreamSession._check_args(cfg, hop, core=8, context=4, fade=4, loudness="audio", f0="yin")
