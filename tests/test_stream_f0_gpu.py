"""GPU tests (-m gpu) of the F0 of live streams from raw audio (csrc/fastsvc_f0.hip, csrc/fastsvc_stream_f0.hip,
decode.StreamSession(f0="audio")): f0_extract against the float64 reference (tests/stream_f0_ref.py), the streamed F0 bit
for bit against f0_extract across push schedules, slots, ends and the ring's wrap, the excitation against SignalGenerator,
the F0 shift against F0Statistics.convert, a session that makes its F0 against one that is fed it, and refusals.  Tiny
generators (hop 160 and 256), at most 3 slots and 60 frames."""
import ctypes

import numpy as np
import pytest
import torch

import stream_f0_ref as R
import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd import synth as S

pytestmark = pytest.mark.gpu

# Measured on the CPU (tests/test_stream_f0.py holds the float32 model of the kernel to these): the largest float32-to-float64
# difference of d' on the signals of stream_f0_ref.f0_signals() is 4.6e-6, of a voiced frame's F0 1.07e-7 relative.
MARGIN = 4 * 4.6e-6         # a reference decision nearer than this to flipping is not compared (at most 5 % of all frames)
F0_BOUND = 4 * 1.07e-7      # relative, on voiced frames
CORE, CONTEXT, FADE = 8, 8, 4
SCALES = {160: (2, 4, 4, 5), 256: (4, 4, 4, 4)}
HOPS = (160, 256)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    A.load_library()
    return torch.device("cuda:0")


class _World:
    pass


@pytest.fixture(scope="module")
def world(dev):
    """Per hop a tiny generator (8 input channels, 16-value embedding) and signal generators (noise off / on), made on
    first use; ppg and an embedding for 60 frames; whole-file F0 of a stream's audio, computed once per audio."""
    w = _World()
    w.models, w.sgs, w.whole = {}, {}, {}
    rng = np.random.default_rng(4096)
    w.ppg = rng.standard_normal((60, 8)).astype(np.float32)
    w.ppg_wide = rng.standard_normal((60, 48)).astype(np.float32)
    w.emb = rng.standard_normal(16).astype(np.float32)

    def model(hop, wide=False):
        """wide: widths that are multiples of 24, which the 2-byte activation storages need."""
        if (hop, wide) not in w.models:
            cin, mid = (48, (96, 48, 24, 24)) if wide else (8, (16, 8, 8, 4))
            cfg = S.GeneratorConfig(in_channels=cin, mid_channels=mid, upsampling_scales=SCALES[hop], out_channels=1,
                                    spk_emb_size=16, use_spk_emb=True)
            assert cfg.hop == hop
            g = A.FastSVCGenerator(in_channels=cin, mid_channels=list(mid), upsampling_scales=list(SCALES[hop]), out_channels=1,
                                   spk_emb_size=16, use_spk_emb=True)
            g.load_state_dict({k: torch.from_numpy(v) for k, v in S.synth_state_dict(cfg, 77 + hop).items()}, strict=True)
            g.remove_weight_norm()
            w.models[hop, wide] = g.eval().to(dev)
        return w.models[hop, wide]

    def sg(hop, noise=0.0):
        if (hop, noise) not in w.sgs:
            w.sgs[hop, noise] = A.SignalGenerator(sample_rate=R.SR, hop_size=hop, sine_amp=0.1, noise_amp=noise, signal_types=["sine"])
        return w.sgs[hop, noise]

    def whole(F, hop, seed):
        """(audio, f0_extract of it [:F]) of voiced_stream(F, hop, seed)."""
        if (F, hop, seed) not in w.whole:
            y = R.voiced_stream(F, hop, seed)
            f0 = A.f0_extract(torch.from_numpy(y).to(dev), R.SR, hop).cpu().numpy()
            assert f0.shape == (F + 1,) and f0.dtype == np.float32
            w.whole[F, hop, seed] = (y, f0[:F])
        return w.whole[F, hop, seed]
    w.model, w.sg, w.whole_f0 = model, sg, whole
    return w


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _split(F, k):
    return [k] * (F // k) + ([F % k] if F % k else [])


def _chunk(w, audio, a, k, hop, f0=None, wide=False):
    d = {"ppg": (w.ppg_wide if wide else w.ppg)[a: a + k], "audio": audio[a * hop: (a + k) * hop]}
    if f0 is not None:
        d["f0"] = f0[a: a + k]
    return d


def _session(w, dev, hop, n_streams=1, noise=0.0, wide=False, **kw):
    kw = dict(dict(core=CORE, context=CONTEXT, fade=FADE, max_push=12, pcm16=False, loudness="audio", f0="audio"), **kw)
    s = Dc.StreamSession(w.model(hop, wide), w.sg(hop, noise), dev, n_streams=n_streams, **kw)
    s._stream_trace = {}
    return s


def _feed(w, s, sid, audio, sched, hop, end=True, f0=None, wide=False):
    pieces, at = [], 0
    for i, k in enumerate(sched):
        last = end is True and i == len(sched) - 1
        pieces.append(s.push({sid: _chunk(w, audio, at, k, hop, f0, wide)}, end=[sid] if last else ())[sid])
        at += k
    assert at * hop == audio.size
    if end == "alone":
        pieces.append(s.end([sid])[sid])
    return pieces


def _traced(s, sid, key="f0"):
    return torch.cat(s._stream_trace[key][sid]).cpu().numpy()


# ------------------------------------------------------------------------------------------- 4: f0_extract vs reference

@pytest.fixture(scope="module")
def reference():
    """{(name, hop): (audio, [Pick per frame])}: the float64 reference on every signal, computed once."""
    return {(name, hop): (y, R.f0_frames(y, hop)) for name, y in R.f0_signals().items() for hop in HOPS}


@pytest.mark.parametrize("hop", HOPS)
def test_f0_extract_against_the_reference(dev, reference, hop):
    """f0_extract on the audio of the CPU tests.  MARGIN = 1.84e-5: four times the largest float32-to-float64 difference of
    d' measured on these signals (4.6e-6).  A frame whose reference decision - every comparison with the threshold up to the
    lag picked, every comparison of the walk - is nearer than MARGIN to flipping is left out; they are at most 5 % of all
    frames (a condition, also held on the CPU).  On every other frame the voicing decision is the reference's, and a voiced
    frame's F0 is within F0_BOUND = 4.28e-7 relative: four times the float32 model's largest difference (1.07e-7)."""
    total = left_out = 0
    worst = 0.0
    for (name, h), (y, ref) in reference.items():
        if h != hop:
            continue
        got = A.f0_extract(torch.from_numpy(y).to(dev), R.SR, hop).cpu().numpy()
        assert got.shape == (len(ref),) and np.isfinite(got).all(), name
        if name in ("noise", "zeros"):
            assert not got.any(), name
        for f, p in enumerate(ref):
            total += 1
            if p.margin < MARGIN:
                left_out += 1
                continue
            assert (got[f] > 0) == (p.f0 > 0), (name, f, float(got[f]), p)
            if p.f0 > 0:
                worst = max(worst, abs(float(got[f]) - p.f0) / p.f0)
    print(f"F0 hop {hop}: {left_out} of {total} frames left out; voiced frames within {worst:.3e} of the reference (bound {F0_BOUND:.3e})")
    assert left_out <= 0.05 * total
    assert worst <= F0_BOUND


def test_f0_extract_batches_and_refusals(dev):
    """Rows of a batch are utterances of their own, and the value depends on the frame alone: a batch of two gives the
    bits of two calls.  tau_max > 1024, a threshold of 0 and CPU tensors are refused."""
    y = np.stack([R.voiced_stream(20, 160, 1), R.voiced_stream(20, 160, 2)])
    both = A.f0_extract(torch.from_numpy(y).to(dev), R.SR, 160).cpu().numpy()
    for b in range(2):
        one = A.f0_extract(torch.from_numpy(y[b]).to(dev), R.SR, 160).cpu().numpy()
        assert np.array_equal(_bits(both[b]), _bits(one)) and (one > 0).sum() >= 10
    with pytest.raises(ValueError):
        A.f0_extract(torch.from_numpy(y[0]).to(dev), R.SR, 160, f0_floor=23.0)
    with pytest.raises(ValueError):
        A.f0_extract(torch.from_numpy(y[0]).to(dev), R.SR, 160, threshold=0.0)
    with pytest.raises(A.FastSVCError):
        A.f0_extract(torch.from_numpy(y[0]), R.SR, 160)
    lib = A.load_library()
    out = torch.zeros(21, device=dev)
    assert lib.fastsvc_f0_extract(None, out.data_ptr(), 1, 3200, 160, ctypes.c_float(24000.0), ctypes.c_float(70.0),
                                  ctypes.c_float(340.0), ctypes.c_float(0.15), None) == -1


# ------------------------------------------------------------------------------------- 5: streamed vs whole file, bits

IRREGULAR = [3, 0, 11, 1, 32, 6, 7]


@pytest.mark.parametrize("hop", HOPS)
def test_streamed_f0_is_f0_extract_bit_for_bit_for_every_schedule(dev, world, hop):
    """60 frames, pushed frame by frame, in 7s, in 32s (= max_push) and irregularly (an empty push among them), the end with
    the last chunk or alone: the traced raw F0 equals f0_extract of the whole audio on every frame, the reflected frames at
    the end included - and frame 0, whose x[0] has not arrived at hop 256 when it is final."""
    F = 60
    y, whole = world.whole_f0(F, hop, 0)
    assert (whole > 0).sum() >= 20 and (whole == 0).sum() >= 1
    for name, sched, end in (("1s", [1] * F, True), ("7s", _split(F, 7), True), ("32s", _split(F, 32), True),
                             ("irregular", IRREGULAR, True), ("end alone", _split(F, 7), "alone")):
        with _session(world, dev, hop, max_push=32) as s:
            sid = s.open(world.emb)
            out = np.concatenate(_feed(world, s, sid, y, sched, hop, end))
            got = _traced(s, sid)
        assert out.shape == (F * hop,) and np.isfinite(out).all()
        assert got.shape == (F,) and np.array_equal(_bits(got), _bits(whole)), name


@pytest.mark.parametrize("hop", HOPS)
def test_streamed_f0_across_the_wrap_slots_and_short_streams(dev, world, hop):
    """max_push 12: the rings hold fewer frames than the stream has, so frames straddle the wrap of the audio ring.  Three
    slots at once with streams of 3, 25 and 60 frames in different chunkings - at 3 frames T < 1024 and both reflections
    fall inside one frame - then a slot reused after its stream ended: every traced F0 is f0_extract's, bit for bit."""
    Fs, scheds = (3, 25, 60), ([3], _split(25, 7), [5, 12, 0, 1, 12, 12, 7, 11])
    data = [world.whole_f0(F, hop, 1 + j) for j, F in enumerate(Fs)]
    with _session(world, dev, hop, n_streams=3) as s:
        assert s.cap < 60 and s.cap == Dc.stream_loudness_ring_frames(CORE, CONTEXT, 12, hop)
        ids = [s.open(world.emb) for _ in Fs]
        assert [s._ids[i] for i in ids] == [0, 1, 2]
        at = [0, 0, 0]
        for i in range(max(len(sc) for sc in scheds)):
            chunks, end = {}, []
            for j in range(3):
                if i < len(scheds[j]):
                    chunks[ids[j]] = _chunk(world, data[j][0], at[j], scheds[j][i], hop)
                    at[j] += scheds[j][i]
                    if i == len(scheds[j]) - 1:
                        end.append(ids[j])
            s.push(chunks, end)
            if i == 3:                                   # (slots 0 and 1 are free again: a new stream takes slot 0)
                again = s.open(world.emb)
                assert s._ids[again] == 0
                _feed(world, s, again, data[1][0], [12, 12, 1], hop)
        for j in range(3):
            assert np.array_equal(_bits(_traced(s, ids[j])), _bits(data[j][1])), Fs[j]
        assert np.array_equal(_bits(_traced(s, again)), _bits(data[1][1]))


# --------------------------------------------------------------------------------------------------------- 6: excitation

@pytest.mark.parametrize("hop", HOPS)
def test_excitation_is_signal_generator_on_the_traced_f0(dev, world, hop):
    """noise_amp = 0: the traced excitation, finalisation after finalisation, is the device SignalGenerator's sine of the
    whole traced (shifted) F0, bit for bit - the phase carried through the parity pair."""
    F = 60
    y, _ = world.whole_f0(F, hop, 0)
    with _session(world, dev, hop) as s:
        sid = s.open(world.emb, [5.0, 0.25], [5.4, 0.3])
        _feed(world, s, sid, y, IRREGULAR[:4] + [12, 12, 12, 9], hop)
        f0s = torch.cat(s._stream_trace["f0_shifted"][sid])
        exc = _traced(s, sid, "excitation")
    want = world.sg(hop)(f0s.view(1, 1, -1)).cpu().numpy().reshape(-1)
    assert exc.shape == want.shape == (F * hop,) and np.abs(want).max() > 0.05
    assert np.array_equal(_bits(exc), _bits(want))


def test_excitation_with_noise_does_not_depend_on_schedule_or_slot(dev, world):
    hop, F = 160, 40
    y, _ = world.whole_f0(F, hop, 3)
    got = []
    for slot, sched in ((0, _split(F, 7)), (1, [1] * F)):
        with _session(world, dev, hop, n_streams=2, noise=0.003) as s:
            if slot:
                s.open(world.emb)
            sid = s.open(world.emb, seed=11)
            assert s._ids[sid] == slot
            _feed(world, s, sid, y, sched, hop)
            got.append(_traced(s, sid, "excitation"))
    assert got[0].shape == (F * hop,) and np.array_equal(_bits(got[0]), _bits(got[1]))
    with _session(world, dev, hop) as s:                 # (... and the noise is there: not the noiseless excitation)
        sid = s.open(world.emb, seed=11)
        _feed(world, s, sid, y, _split(F, 7), hop)
        assert not np.array_equal(_traced(s, sid, "excitation"), got[0])


# --------------------------------------------------------------------------------------------------------- 7: F0 shift

@pytest.mark.parametrize("hop", HOPS)
def test_shifted_f0_is_within_one_ulp_of_the_host_conversion(dev, world, hop):
    F = 60
    y, whole = world.whole_f0(F, hop, 0)
    src, trg = [5.1, 0.21], [5.45, 0.33]
    with _session(world, dev, hop) as s:
        sid = s.open(world.emb, src, trg)
        _feed(world, s, sid, y, _split(F, 7), hop)
        raw, shifted = _traced(s, sid), _traced(s, sid, "f0_shifted")
        ring = s._f0_shift[0].cpu().numpy()              # (read back from the ring: its last cap frames)
        assert np.array_equal(_bits(ring[np.arange(F - s.cap, F) % s.cap]), _bits(shifted[F - s.cap:]))
    assert np.array_equal(_bits(raw), _bits(whole))
    want = Dc.F0Statistics().convert(raw.astype(np.float64), src, trg).astype(np.float32)
    voiced = raw > 0
    assert voiced.sum() >= 20 and (~voiced).sum() >= 1
    assert not shifted[~voiced].any() and not want[~voiced].any()
    ulps = np.abs(shifted[voiced].view(np.int32).astype(np.int64) - want[voiced].view(np.int32).astype(np.int64))
    print(f"F0 shift hop {hop}: device against host, largest difference {int(ulps.max())} ulp")
    assert ulps.max() <= 1
    assert np.abs(shifted[voiced] / raw[voiced] - 1.0).min() > 0.05      # (it did shift)


# ------------------------------------------------------------------------------------------------------- 8: end to end

@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
@pytest.mark.parametrize("norm", ["window", "running"])
def test_audio_session_returns_the_bytes_of_a_session_fed_its_f0(dev, world, norm, storage):
    """No F0 statistics: a session with f0="audio" and one with f0="given", loudness="audio" that is fed the first one's
    traced raw F0, the same ppg, audio, embedding and chunking: the same int16 bytes, push by push.  (A generator whose
    widths are multiples of 24 and a stream of 48 frames: what bfloat16 storage asks of the plan and of a row.)"""
    hop, F = 160, 48
    y, _ = world.whole_f0(F, hop, 4)
    model = world.model(hop, wide=True)
    model.use_activation_storage(storage)
    try:
        with _session(world, dev, hop, norm=norm, pcm16=True, wide=True) as s:
            sid = s.open(world.emb)
            a = _feed(world, s, sid, y, _split(F, 7), hop, wide=True)
            f0 = _traced(s, sid)
            forwards = s.forwards
        with _session(world, dev, hop, norm=norm, pcm16=True, f0="given", wide=True) as s:
            sid = s.open(world.emb)
            b = _feed(world, s, sid, y, _split(F, 7), hop, f0=f0, wide=True)
            assert s.forwards == forwards
    finally:
        model.use_activation_storage("float32")
    assert sum(p.size for p in a) == F * hop and a[0].dtype == np.int16 and np.abs(np.concatenate(a)).max() > 30
    assert len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a, b))


# ---------------------------------------------------------------------------------------------------------- 9: refusals

def test_refusals_leave_the_session_usable(dev, world):
    """f0="audio" without loudness="audio", lags that do not fit the frame and an unknown mode are refused at construction;
    an f0 key, a missing audio, an lft key and a wrong shape at push - and the next valid push returns what an undisturbed
    session returns.  The C entry point refuses a null ring, too many frames and frames that are not final."""
    hop, F = 160, 30
    y, _ = world.whole_f0(F, hop, 5)
    model, sg = world.model(hop), world.sg(hop)
    for kw in (dict(f0="audio"), dict(f0="audio", loudness="given"), dict(f0="audio", loudness="audio", f0_floor=20.0),
               dict(f0="yin", loudness="audio"), dict(f0="audio", loudness="audio", f0_threshold=-1.0)):
        with pytest.raises(ValueError):
            Dc.StreamSession(model, sg, dev, core=CORE, context=CONTEXT, fade=FADE, **kw)
    sched = _split(F, 7)
    with _session(world, dev, hop) as s:
        want = _feed(world, s, s.open(world.emb), y, sched, hop)
    good = _chunk(world, y, 0, 4, hop)
    bad = [dict(good, f0=np.full(4, 100.0, np.float32)), {"ppg": good["ppg"]}, dict(good, lft=good["audio"]),
           dict(good, audio=good["audio"][:-1])]
    with _session(world, dev, hop) as s:
        sid = s.open(world.emb)
        at = 0
        for i, k in enumerate(sched):
            with pytest.raises(ValueError):
                s.push({sid: bad[i % len(bad)]})
            got = s.push({sid: _chunk(world, y, at, k, hop)}, end=[sid] if i == len(sched) - 1 else ())[sid]
            at += k
            assert np.array_equal(_bits(got), _bits(want[i])), i
    # the C entry point, through the wrapper: nothing is enqueued
    from svcc23_fastsvc_amd.engine import stream_f0
    cap = 16
    audio, exc = torch.zeros((1, cap * hop), device=dev), torch.zeros((1, cap * hop), device=dev)
    f0r, f0s, phase = torch.zeros((1, cap), device=dev), torch.zeros((1, cap), device=dev), torch.zeros((1, 2), dtype=torch.float64, device=dev)
    base = dict(streams=[0], first_frame=[0], n=[4], seen=[16], ended=[0], parity=[0], seed=[0], stats=[None])
    for kw in (dict(n=[9]), dict(streams=[1]), dict(n=[8], seen=[8]), dict(first_frame=[12], seen=[40], n=[1]),
               dict(stats=[(5.0, 0.0, 5.0, 0.3)])):
        with pytest.raises(ValueError):                  # (too many; no such stream; not final; left the ring; std 0)
            stream_f0(audio, f0r, f0s, exc, phase, cap=cap, max_frames=8, sample_rate=24000.0, f0_floor=70.0, f0_ceil=340.0,
                      threshold=0.15, sine_amp=0.1, noise_amp=0.0, **dict(base, **kw))
    with pytest.raises(ValueError):
        stream_f0(audio, f0r, f0s, exc, phase, cap=cap, max_frames=8, sample_rate=24000.0, f0_floor=20.0, f0_ceil=340.0,
                  threshold=0.15, sine_amp=0.1, noise_amp=0.0, **base)
    torch.cuda.synchronize()
    assert not exc.cpu().numpy().any() and not phase.cpu().numpy().any()
    f0r.fill_(7.0)
    stream_f0(audio, f0r, f0s, exc, phase, cap=cap, max_frames=8, sample_rate=24000.0, f0_floor=70.0, f0_ceil=340.0,
              threshold=0.15, sine_amp=0.1, noise_amp=0.0, **base)          # (silence: four unvoiced frames, nothing else)
    torch.cuda.synchronize()
    assert np.array_equal(f0r.cpu().numpy()[0], [0.0] * 4 + [7.0] * 12) and not exc.cpu().numpy().any()
