"""GPU tests (-m gpu) of the loudness of live streams from raw audio (csrc/fastsvc_stream_loudness.hip,
decode.StreamSession(loudness="audio")): the streamed loudness against the float64 causal reference
(tests/stream_loudness_ref.py), bit for bit against loudness_extract where the running maximum is the utterance's from the
first frame, across push schedules, slots and ends; a session fed audio against a session fed its loudness; refusals; and
the default session untouched.  Tiny generators (hop 160 and 256), at most 80 frames."""
import ctypes

import numpy as np
import pytest
import torch

import stream_loudness_ref as R
import svcc23_fastsvc_amd as A
from oracle import loudness_oracle as LO
from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd import synth as S

pytestmark = pytest.mark.gpu

BOUND = 2e-3                # log loudness: the bound tests/test_loudness.py holds the whole-file kernels to
BATCHING = 2e-5             # x max(1, |ref|max): the batching invariance tests/test_decode_stream_gpu.py uses
CORE, CONTEXT, FADE, MAX_PUSH = 8, 8, 4, 12
SCALES = {160: (2, 4, 4, 5), 256: (4, 4, 4, 4)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    A.load_library()
    return torch.device("cuda:0")


class _World:
    pass


@pytest.fixture(scope="module")
def world(dev):
    """Per hop a tiny generator (8 input channels, 16-value embedding) and its signal generator (noise off), made on
    first use; ppg, f0 and an embedding for 80 frames; the whole-file oracle's and the reference's values are computed per
    test from the shared signals of tests/stream_loudness_ref.py."""
    w = _World()
    w.cache = {}
    rng = np.random.default_rng(2048)
    w.ppg = rng.standard_normal((80, 8)).astype(np.float32)
    w.f0 = rng.uniform(80.0, 400.0, 80).astype(np.float32)
    w.emb = rng.standard_normal(16).astype(np.float32)

    def get(hop):
        if hop not in w.cache:
            cfg = S.GeneratorConfig(in_channels=8, mid_channels=(16, 8, 8, 4), upsampling_scales=SCALES[hop], out_channels=1,
                                    spk_emb_size=16, use_spk_emb=True)
            assert cfg.hop == hop
            g = A.FastSVCGenerator(in_channels=8, mid_channels=[16, 8, 8, 4], upsampling_scales=list(SCALES[hop]), out_channels=1,
                                   spk_emb_size=16, use_spk_emb=True)
            g.load_state_dict({k: torch.from_numpy(v) for k, v in S.synth_state_dict(cfg, 77 + hop).items()}, strict=True)
            g.remove_weight_norm()
            sg = A.SignalGenerator(sample_rate=R.SR, hop_size=hop, sine_amp=0.1, noise_amp=0.0, signal_types=["sine"])
            w.cache[hop] = (g.eval().to(dev), sg)
        return w.cache[hop]
    w.get = get
    return w


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _chunk(w, third, a, k, hop, key="audio"):
    return {"ppg": w.ppg[a: a + k], "f0": w.f0[a: a + k], key: third[a * hop: (a + k) * hop]}


def _feed(w, s, sid, audio, sched, hop, end=True):
    """Push `audio` into stream sid in chunks of sched frames (the end with the last, or alone after it when end="alone")
    -> the pieces push returned."""
    pieces, at = [], 0
    for i, k in enumerate(sched):
        last = end is True and i == len(sched) - 1
        pieces.append(s.push({sid: _chunk(w, audio, at, k, hop)}, end=[sid] if last else ())[sid])
        at += k
    assert at * hop == audio.size
    if end == "alone":
        pieces.append(s.end([sid])[sid])
    return pieces


def _session(w, dev, hop, n_streams=1, **kw):
    model, sg = w.get(hop)
    kw = dict(dict(core=CORE, context=CONTEXT, fade=FADE, max_push=MAX_PUSH, pcm16=False, loudness="audio"), **kw)
    s = Dc.StreamSession(model, sg, dev, n_streams=n_streams, **kw)
    s._stream_trace = {}
    return s


def _traced(s, sid):
    return torch.cat(s._stream_trace["lft"][sid]).cpu().numpy()


def _streamed(w, dev, audio, sched, hop, end=True):
    """The traced loudness (F hop,) of one stream in slot 0 of a fresh session, and the samples it returned."""
    with _session(w, dev, hop) as s:
        sid = s.open(w.emb)
        pieces = _feed(w, s, sid, audio, sched, hop, end)
        return _traced(s, sid), np.concatenate(pieces)


def _split(F, k):
    return [k] * (F // k) + ([F % k] if F % k else [])


def _bound_for(dev, audio, hop):
    """The bound of the comparison with the reference: 2e-3, the whole-file kernels' own - whose error against the oracle
    on the same audio is measured and printed next to it; only if that alone exceeds 2e-3, 1.5 times it."""
    whole = A.loudness_extract(torch.from_numpy(audio).to(dev), R.SR, hop).cpu().numpy()
    err = float(np.abs(whole - LO.loudness_extract(audio, R.SR, hop)).max())
    print(f"STREAM LOUDNESS hop {hop}: whole-file kernels against the whole-file oracle on this audio {err:.3e}")
    return BOUND if err <= BOUND else 1.5 * err


@pytest.mark.parametrize("hop", [160, 256])
def test_streamed_loudness_is_the_causal_reference(dev, world, hop):
    """Two streams in slots 0 and 1 fed different audio - the sine that is 100 times louder from the middle on, with two
    noise seeds, the second stream half as loud - in different chunkings: 24 frames whose running maximum takes 18
    (hop 160) values.  The traced loudness against the float64 causal reference."""
    F = 24
    audio = [R.rising_signal(F, hop, 0), (0.5 * R.rising_signal(F, hop, 1)).astype(np.float32)]
    P = LO.stft_power(audio[0], hop)[:, :F]
    assert len(np.unique(np.maximum.accumulate(P.max(axis=0)))) >= 16
    bound = max(_bound_for(dev, a, hop) for a in audio)
    scheds = [_split(F, 5), _split(F, 7)]
    with _session(world, dev, hop, n_streams=2) as s:
        ids = [s.open(world.emb), s.open(world.emb)]
        assert [s._ids[i] for i in ids] == [0, 1] and s.lag == Dc.stream_loudness_lag(hop)
        at = [0, 0]
        for i in range(max(len(sc) for sc in scheds)):
            chunks, end = {}, []
            for j in range(2):
                if i < len(scheds[j]):
                    chunks[ids[j]] = _chunk(world, audio[j], at[j], scheds[j][i], hop)
                    at[j] += scheds[j][i]
                    if i == len(scheds[j]) - 1:
                        end.append(ids[j])
            s.push(chunks, end)
        got = [_traced(s, i) for i in ids]
    for j in range(2):
        ref = R.stream_loudness(audio[j], R.SR, hop)
        assert got[j].shape == ref.shape == (F * hop,) and got[j].dtype == np.float32
        err = float(np.abs(got[j] - ref).max())
        print(f"STREAM LOUDNESS hop {hop} stream {j}: streamed against the causal reference {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (j, err)
        assert np.all(got[j].reshape(F, hop) == got[j].reshape(F, hop)[:, :1])       # (a frame's value, hop times)
    # the definition IS the causal one: in front of the jump it is far from the whole-file kernels' value
    whole = A.loudness_extract(torch.from_numpy(audio[0]).to(dev), R.SR, hop).cpu().numpy()[: F * hop]
    assert np.abs(got[0] - whole).max() > 1.0


@pytest.mark.parametrize("hop", [160, 256])
def test_streamed_loudness_is_loudness_extract_bit_for_bit_when_frame_0_holds_the_peak(dev, world, hop):
    """A burst in the first 128 samples: on the oracle frame 0's peak power is >= 1.1 x every other frame's (the
    whole-file function's frame F included), so float32 rounding cannot move the argmax, the running maximum is the
    utterance's from frame 0 on, and the streamed loudness equals loudness_extract of the whole audio bit for bit."""
    F = 24
    y = R.peak_first_signal(F, hop)
    P = LO.stft_power(y, hop)
    assert P[:, 0].max() >= 1.1 * P[:, 1:].max()
    got, _ = _streamed(world, dev, y, _split(F, 5), hop)
    whole = A.loudness_extract(torch.from_numpy(y).to(dev), R.SR, hop).cpu().numpy()
    assert whole.shape == ((F + 1) * hop,) and got.shape == (F * hop,)
    assert np.array_equal(_bits(got), _bits(whole[: F * hop]))


def test_push_schedules_and_slots_give_the_same_bits(dev, world):
    """60 frames of the rising signal, hop 160: frame by frame, in pushes of 7, in pushes of max_push with empty pushes
    between, with the end in a push of its own; in slot 0 and in slot 1 after another stream ended there.  The traced
    loudness has the same bits every time, and so many frames that the rings (cap frames) wrap."""
    hop, F = 160, 60
    y = R.rising_signal(F, hop, 3)
    base, _ = _streamed(world, dev, y, [1] * F, hop)
    assert base.shape == (F * hop,)
    with_gaps = [k for n in _split(F, MAX_PUSH) for k in (n, 0)][:-1]
    for name, sched, end in (("7s", _split(F, 7), True), ("max_push and empty", with_gaps, True), ("end alone", _split(F, 7), "alone")):
        got, _ = _streamed(world, dev, y, sched, hop, end)
        assert np.array_equal(_bits(got), _bits(base)), name
    with _session(world, dev, hop, n_streams=2) as s:
        assert s.cap < F
        keep = s.open(world.emb)                          # (slot 0 stays busy)
        other = s.open(world.emb)
        _feed(world, s, other, (0.3 * R.rising_signal(17, hop, 4)).astype(np.float32), _split(17, 7), hop)
        sid = s.open(world.emb)
        assert s._ids[sid] == 1 and s._ids[keep] == 0
        _feed(world, s, sid, y, _split(F, 7), hop)
        assert np.array_equal(_bits(_traced(s, sid)), _bits(base))


@pytest.mark.parametrize("hop", [160, 256])
def test_ends(dev, world, hop):
    """Streams that end after 1, lag and lag + 1 frames - nothing was final before the end, or one frame was - and one
    whose last chunk is empty: every frame is produced, with reflection at both ends (repeated at F = 1, where the audio
    is shorter than half a frame), equals the reference, and exactly F hop samples come back."""
    lag = Dc.stream_loudness_lag(hop)
    for F, sched in ((1, [1]), (lag, _split(lag, 4)), (lag + 1, _split(lag + 1, 4)), (11, [6, 5, 0])):
        y = R.rising_signal(F, hop, 10 + F)
        bound = _bound_for(dev, y, hop) if F * hop >= 2 else BOUND
        got, out = _streamed(world, dev, y, sched, hop)
        ref = R.stream_loudness(y, R.SR, hop)
        assert got.shape == ref.shape == (F * hop,) and out.shape == (F * hop,) and np.isfinite(out).all()
        err = float(np.abs(got - ref).max())
        print(f"STREAM LOUDNESS hop {hop} end at {F} frames: {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (F, err)


def _return_frame(t, F, core, context, fade, lag):
    """The frame whose push returns the samples of frame t, the end at frame F - 1: StreamSession's latency rule."""
    k = t // core
    r = (k + 1) * core + context - 1 + lag
    if t % core >= core - fade // 2:
        r = (k + 2) * core + context - 1 + lag
    return min(r, F - 1)


@pytest.mark.parametrize("norm", ["window", "running"])
def test_audio_session_is_the_given_session_on_its_loudness(dev, world, norm):
    """Session A takes audio, session B the loudness A traced, with the same ppg, f0, embedding and chunking (frame by
    frame): the windows are the same and only fall into different forwards, so the outputs agree within the batching
    invariance.  A returns a sample of frame t with the push that delivers frame (t // core + 1) core + context - 1 + lag
    (the last fade / 2 frames of a core one core later; everything at the end), B lag frames earlier."""
    hop, F = 160, 50
    y = R.rising_signal(F, hop, 5)
    with _session(world, dev, hop, norm=norm) as s:
        lag = s.lag
        assert lag == 6 and s.latency_frames == CORE + CONTEXT + lag and s.latency_frames_max == 2 * CORE + CONTEXT + lag
        assert s.cap == Dc.stream_loudness_ring_frames(CORE, CONTEXT, MAX_PUSH, hop)
        sid = s.open(world.emb)
        a = _feed(world, s, sid, y, [1] * F, hop)
        lft = _traced(s, sid)
        rows_a = [r[1:] for rows, _ in s._stream_trace["forwards"] for r in rows]
    with _session(world, dev, hop, norm=norm, loudness="given") as s:
        assert s.lag == 0 and s.latency_frames == CORE + CONTEXT and s.cap == Dc.stream_ring_frames(CORE, CONTEXT, MAX_PUSH)
        sid = s.open(world.emb)
        b, at = [], 0
        for i in range(F):
            b.append(s.push({sid: _chunk(world, lft, i, 1, hop, key="lft")}, end=[sid] if i == F - 1 else ())[sid])
        rows_b = [r[1:] for rows, _ in s._stream_trace["forwards"] for r in rows]
    assert rows_a == rows_b == [r[1:] for r in Dc.window_plan([F], CORE, CONTEXT)]
    ya, yb = np.concatenate(a), np.concatenate(b)
    assert ya.shape == yb.shape == (F * hop,) and np.abs(yb).max() > 1e-3
    err = float(np.abs(ya.astype(np.float64) - yb).max()) / max(1.0, float(np.abs(yb).max()))
    print(f"STREAM LOUDNESS end to end, norm {norm}: audio session against given session {err:.3e}")
    assert err <= BATCHING, err
    for pieces, lg in ((a, lag), (b, 0)):
        back = np.array([_return_frame(t, F, CORE, CONTEXT, FADE, lg) for t in range(F)])
        assert [p.size for p in pieces] == [int((back == i).sum()) * hop for i in range(F)], lg


def test_refusals(dev, world):
    """Under "audio" an lft key, a missing audio and a wrong audio shape raise ValueError, under "given" an audio key does,
    and any other value of the keyword; the next valid push returns the bytes of an undisturbed session.  The C entry
    point returns FASTSVC_E_INVALID for a null ring and for n out of range."""
    hop, F = 160, 30
    y = R.rising_signal(F, hop, 6)
    model, sg = world.get(hop)
    sched = _split(F, 7)
    with _session(world, dev, hop) as s:
        want = _feed(world, s, s.open(world.emb), y, sched, hop)
    good = _chunk(world, y, 0, 4, hop)
    with _session(world, dev, hop) as s:
        sid = s.open(world.emb)
        bad = [dict(good, lft=good["audio"]), {k: v for k, v in good.items() if k != "audio"}, dict(good, audio=good["audio"][:-1]),
               dict(good, audio=good["audio"].reshape(4, hop))]
        at = 0
        for i, k in enumerate(sched):
            with pytest.raises(ValueError):
                s.push({sid: bad[i % len(bad)]})
            got = s.push({sid: _chunk(world, y, at, k, hop)}, end=[sid] if i == len(sched) - 1 else ())[sid]
            at += k
            assert np.array_equal(_bits(got), _bits(want[i])), i
    with _session(world, dev, hop, loudness="given") as s:
        sid = s.open(world.emb)
        with pytest.raises(ValueError):
            s.push({sid: dict(good, lft=good["audio"])})                 # (lft AND audio)
        with pytest.raises(ValueError):
            s.push({sid: good})                                          # (audio instead of lft)
        assert s.push({sid: _chunk(world, y, 0, 4, hop, key="lft")})[sid].size == 0
    with pytest.raises(ValueError):
        Dc.StreamSession(model, sg, dev, loudness="raw")
    # the C entry point
    from svcc23_fastsvc_amd.engine import stream_loudness, stream_loudness_scratch_bytes
    lib = A.load_library()
    cap, mf = 16, 8
    ring, lft = torch.zeros((1, cap * hop), device=dev), torch.zeros((1, cap * hop), device=dev)
    peak = torch.zeros((1, 2), device=dev)
    scratch = torch.zeros(stream_loudness_scratch_bytes(1, mf), dtype=torch.uint8, device=dev)
    assert scratch.numel() == mf * 1026 * 4

    def call(ring_ptr, n):
        i32, i64 = (ctypes.c_int32 * 1), (ctypes.c_int64 * 1)
        return lib.fastsvc_stream_loudness(ring_ptr, lft.data_ptr(), peak.data_ptr(), scratch.data_ptr(), 1, i32(0), i64(0), i32(n),
                                           i64(16), i32(0), i32(0), 1, cap, mf, hop, ctypes.c_float(24000.0), None)
    assert call(None, 4) == -1 and call(ring.data_ptr(), mf + 1) == -1 and call(ring.data_ptr(), -1) == -1
    for kw in (dict(n=[mf + 1]), dict(streams=[1]), dict(n=[8], seen=[8]), dict(first_frame=[12], seen=[40], n=[1])):
        args = dict(dict(streams=[0], first_frame=[0], n=[4], seen=[16], ended=[0], parity=[0]), **kw)
        with pytest.raises(ValueError):                                  # (too many; no such stream; not final; left the ring)
            stream_loudness(ring, lft, peak, scratch, cap=cap, max_frames=mf, sample_rate=24000.0, **args)
    torch.cuda.synchronize()
    assert not lft.cpu().numpy().any() and not peak.cpu().numpy().any()  # nothing ran
    assert call(ring.data_ptr(), 4) == 0                                 # (silence: the value of an empty spectrum)
    torch.cuda.synchronize()
    v = lft.cpu().numpy().reshape(cap, hop)
    assert np.all(v[:4] == v[0, 0]) and np.isfinite(v[0, 0]) and v[0, 0] != 0 and not v[4:].any()


def test_default_session_is_untouched(dev, world):
    """loudness="given" is the session of before: the ring and the forwards of a session built without the keyword, and
    the same bytes."""
    hop, F = 160, 40
    model, sg = world.get(hop)
    lft = R.stream_loudness(R.rising_signal(F, hop, 8), R.SR, hop).astype(np.float32)
    outs = []
    for kw in (dict(), dict(loudness="given")):
        with Dc.StreamSession(model, sg, dev, core=CORE, context=CONTEXT, fade=FADE, max_push=MAX_PUSH, pcm16=False, **kw) as s:
            assert s.cap == Dc.stream_ring_frames(CORE, CONTEXT, MAX_PUSH) == 36 and s.loudness == "given" and s._audio is None
            assert (s.latency_frames, s.latency_frames_max) == (CORE + CONTEXT, 2 * CORE + CONTEXT)
            sid = s.open(world.emb)
            pieces, at = [], 0
            for i, k in enumerate(_split(F, 7)):
                pieces.append(s.push({sid: _chunk(world, lft, at, k, hop, key="lft")}, end=[sid] if at + k == F else ())[sid])
                at += k
            outs.append((np.concatenate(pieces), s.forwards))
    assert outs[0][1] == outs[1][1] == 4 and outs[0][0].shape == (F * hop,)
    assert np.array_equal(_bits(outs[0][0]), _bits(outs[1][0]))
