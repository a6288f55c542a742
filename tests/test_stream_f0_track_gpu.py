"""GPU tests (-m gpu) of the fixed-lag Viterbi F0 tracker (decode.F0Track; csrc/fastsvc_f0.inc, fastsvc_f0.hip: f0_track_kernel,
fastsvc_stream_f0.hip: stream_f0_cands_kernel, stream_f0_track_kernel): f0_extract(track=...) against the rule on the host
(decode.f0_track_rule) over the GPU's own candidates, bit for bit; the streamed candidates and tracked F0 against the whole-file
functions over the stream's frames, bit for bit, across push schedules, ends, short streams, hop 1024, the rings' wrap and
slots; the excitation against SignalGenerator; a tracked session against one that is fed its F0; the running statistics over
the tracked F0.  Tiny generators (hop 160, 256 and 1024), at most 3 slots and 60 frames."""
import numpy as np
import pytest
import torch

import stream_f0_ref as R
import stream_f0_track_ref as Q
import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd import synth as S

pytestmark = pytest.mark.gpu

CORE, CONTEXT, FADE = 8, 8, 4
SCALES = {160: (2, 4, 4, 5), 256: (4, 4, 4, 4), 1024: (4, 4, 8, 8)}
HOPS = (160, 256)
IRREGULAR = [5, 12, 0, 1, 12, 12, 7, 11]               # 60 frames, an empty push among them
TAU_MAX = R.lags()[1]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    A.load_library()
    return torch.device("cuda:0")


class _World:
    pass


@pytest.fixture(scope="module")
def world(dev):
    """Per hop a tiny generator (8 input channels, 16-value embedding) and a signal generator without noise, made on first
    use; ppg and an embedding for 60 frames; per (audio, tracker) the whole-file candidates and tracked F0, computed once."""
    w = _World()
    w.models, w.sgs, w.whole = {}, {}, {}
    rng = np.random.default_rng(4097)
    w.ppg = rng.standard_normal((60, 8)).astype(np.float32)
    w.emb = rng.standard_normal(16).astype(np.float32)

    def model(hop):
        if hop not in w.models:
            cfg = S.GeneratorConfig(in_channels=8, mid_channels=(16, 8, 8, 4), upsampling_scales=SCALES[hop], out_channels=1,
                                    spk_emb_size=16, use_spk_emb=True)
            assert cfg.hop == hop
            g = A.FastSVCGenerator(in_channels=8, mid_channels=[16, 8, 8, 4], upsampling_scales=list(SCALES[hop]), out_channels=1,
                                   spk_emb_size=16, use_spk_emb=True)
            g.load_state_dict({k: torch.from_numpy(v) for k, v in S.synth_state_dict(cfg, 78 + hop).items()}, strict=True)
            g.remove_weight_norm()
            w.models[hop] = g.eval().to(dev)
        return w.models[hop]

    def sg(hop):
        if hop not in w.sgs:
            w.sgs[hop] = A.SignalGenerator(sample_rate=R.SR, hop_size=hop, sine_amp=0.1, noise_amp=0.0, signal_types=["sine"])
        return w.sgs[hop]

    def whole(F, hop, seed, track=Dc.F0Track()):
        """(audio, candidates (F, 4, 2), tracked F0 (F,)) of voiced_stream(F, hop, seed): the whole-file functions over the
        stream's F frames (the file has one frame more, which a stream of F frames never has)."""
        if (F, hop, seed, track) not in w.whole:
            y = R.voiced_stream(F, hop, seed)
            cands = A.f0_candidates(torch.from_numpy(y).to(dev), R.SR, hop, cand_threshold=track.cand_threshold)[:F].contiguous()
            f0 = A.f0_track(cands, TAU_MAX, R.SR, track, R.THRESHOLD if track.unvoiced is None else track.unvoiced)
            w.whole[F, hop, seed, track] = (y, cands.cpu().numpy(), f0.cpu().numpy())
        return w.whole[F, hop, seed, track]
    w.model, w.sg, w.whole_track = model, sg, whole
    return w


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _split(F, k):
    return [k] * (F // k) + ([F % k] if F % k else [])


def _chunk(w, audio, a, k, hop, f0=None):
    d = {"ppg": w.ppg[a: a + k], "audio": audio[a * hop: (a + k) * hop]}
    if f0 is not None:
        d["f0"] = f0[a: a + k]
    return d


def _session(w, dev, hop, n_streams=1, track=Dc.F0Track(), **kw):
    kw = dict(dict(core=CORE, context=CONTEXT, fade=FADE, max_push=12, pcm16=False, loudness="audio", f0="audio", f0_track=track), **kw)
    s = Dc.StreamSession(w.model(hop), w.sg(hop), dev, n_streams=n_streams, **kw)
    s._stream_trace = {}
    return s


def _feed(w, s, sid, audio, sched, hop, end=True, f0=None):
    pieces, at = [], 0
    for i, k in enumerate(sched):
        last = end is True and i == len(sched) - 1
        pieces.append(s.push({sid: _chunk(w, audio, at, k, hop, f0)}, end=[sid] if last else ())[sid])
        at += k
    assert at * hop == audio.size
    if end == "alone":
        pieces.append(s.end([sid])[sid])
    return pieces


def _traced(s, sid, key="f0"):
    return torch.cat(s._stream_trace[key][sid]).cpu().numpy()


def _same_as_whole(s, sid, cands, f0, what):
    got_c, got_f = _traced(s, sid, "f0_candidates"), _traced(s, sid)
    assert got_c.shape == cands.shape and np.array_equal(_bits(got_c), _bits(cands)), what
    assert got_f.shape == f0.shape and np.array_equal(_bits(got_f), _bits(f0)), what


# ------------------------------------------------------------------------------------------------------------ the tracker

@pytest.mark.parametrize("lag", [0, 8, 64])
def test_f0_extract_tracked_is_the_rule_on_its_own_candidates(dev, lag):
    """f0_extract(track=F0Track(lag)) equals decode.f0_track_rule over the downloaded candidates of f0_candidates, bit for
    bit: three rows at once (a voiced stream with a silent stretch, the noise burst's first 60 frames and a sub-harmonic
    modulation's), a row of ONE frame (T < hop) and a row of 6 frames, fewer than the default lag."""
    hop = 256
    track = Dc.F0Track(lag=lag)
    T = 60 * hop
    rows = np.stack([R.voiced_stream(60, hop, 2), Q.burst_signal()[T // 2: T // 2 + T], Q.subharmonic_signal(0.6, 0.47, 0.53)[T // 2: T // 2 + T]])
    for y in (rows, rows[0, :100], rows[0, 2 * hop: 7 * hop + 17]):
        a = torch.from_numpy(np.ascontiguousarray(y)).to(dev)
        cands = A.f0_candidates(a, R.SR, hop)
        got = A.f0_extract(a, R.SR, hop, track=track)
        c, g = cands.cpu().numpy().reshape(-1, 1 + y.shape[-1] // hop, 4, 2), got.cpu().numpy().reshape(-1, 1 + y.shape[-1] // hop)
        assert c.dtype == np.float32 and g.dtype == np.float32 and np.isfinite(g).all()
        for b in range(len(c)):
            want = Dc.f0_track_rule(c[b], TAU_MAX, R.SR, track, R.THRESHOLD)
            assert want.dtype == np.float32 and np.array_equal(_bits(g[b]), _bits(want)), (y.shape, b)
        absent = np.isinf(c[..., 1])
        assert np.array_equal(absent, c[..., 0] == 0) and (c[..., 1][~absent] < 0.5).all()
    assert (g > 0).sum() >= 3                             # (the last one: six voiced frames)
    with pytest.raises(ValueError):
        A.f0_extract(a, R.SR, hop, track="viterbi")
    with pytest.raises(A.FastSVCError):
        A.f0_candidates(a.cpu(), R.SR, hop)


# -------------------------------------------------------------------------------------------------------------- streams

@pytest.mark.parametrize("hop", HOPS)
def test_streamed_track_is_the_whole_file_track_for_every_schedule(dev, world, hop):
    """60 frames pushed frame by frame, max_push (32) a push, irregularly with an empty push, the end with the last chunk
    or alone: the traced candidates are f0_candidates' and the traced F0 is f0_track's over the stream's 60 frames, bit for
    bit; everything the stream returned is its F hop samples."""
    F = 60
    y, cands, f0 = world.whole_track(F, hop, 0)
    assert (f0 > 0).sum() >= 20 and (f0 == 0).sum() >= 1
    for name, sched, end in (("1s", [1] * F, True), ("32s", _split(F, 32), True), ("irregular", IRREGULAR, True),
                             ("end alone", _split(F, 7), "alone")):
        with _session(world, dev, hop, max_push=32) as s:
            assert s.latency_frames == CORE + CONTEXT + s.lag + 8
            sid = s.open(world.emb)
            out = np.concatenate(_feed(world, s, sid, y, sched, hop, end))
            _same_as_whole(s, sid, cands, f0, name)
        assert out.shape == (F * hop,) and np.isfinite(out).all()


@pytest.mark.parametrize("hop", HOPS)
def test_streamed_track_across_the_wrap_slots_and_short_streams(dev, world, hop):
    """max_push 12: the rings hold fewer frames than the longest stream has, so the candidate and backpointer rings wrap.
    Three slots at once with streams of 2 frames (fewer than the tracker's lag and than the loudness lag: everything happens
    at the end), 25 and 60 frames in different chunkings, then a slot reused after its stream ended."""
    Fs, scheds = (2, 25, 60), ([2], _split(25, 7), IRREGULAR)
    data = [world.whole_track(F, hop, 1 + j) for j, F in enumerate(Fs)]
    with _session(world, dev, hop, n_streams=3) as s:
        assert s.cap < 60 and s.cap == Dc.stream_track_ring_frames(CORE, CONTEXT, 12, hop, 8)
        ids = [s.open(world.emb) for _ in Fs]
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
            _same_as_whole(s, ids[j], data[j][1], data[j][2], Fs[j])
        _same_as_whole(s, again, data[1][1], data[1][2], "reused slot")


@pytest.mark.parametrize("lag", [0, 3, 8])
def test_hop_1024_ends_with_nothing_newly_final(dev, world, lag):
    """At hop 1024 the loudness lag is 0: every frame is final when it arrives, and a stream that ends alone finalises
    nothing in that push - and still emits the frames the tracker held back."""
    hop, F = 1024, 12
    track = Dc.F0Track(lag=lag)
    y, cands, f0 = world.whole_track(F, hop, 6, track)
    with _session(world, dev, hop, track=track) as s:
        assert s.lag == 0 and s.track_lag == lag
        sid = s.open(world.emb)
        out = _feed(world, s, sid, y, [5, 7], hop, "alone")
        assert sum(p.size for p in out) == F * hop
        assert len(s._stream_trace["f0"][sid][-1]) == min(lag, F) or lag == 0
        _same_as_whole(s, sid, cands, f0, lag)


# ----------------------------------------------------------------------------------------------- what is made of the track

@pytest.mark.parametrize("hop", HOPS)
def test_excitation_is_signal_generator_on_the_tracked_f0(dev, world, hop):
    """noise_amp = 0: the traced excitation is the device SignalGenerator's sine of the whole shifted tracked F0, bit for
    bit - the phase is carried over the EMITTED frames - and the static shift is within one float32 ulp of the host's."""
    F = 60
    y, _, f0 = world.whole_track(F, hop, 0)
    src, trg = [5.0, 0.25], [5.4, 0.3]
    with _session(world, dev, hop) as s:
        sid = s.open(world.emb, src, trg)
        _feed(world, s, sid, y, IRREGULAR, hop)
        raw = _traced(s, sid)
        f0s = torch.cat(s._stream_trace["f0_shifted"][sid])
        exc = _traced(s, sid, "excitation")
    assert np.array_equal(_bits(raw), _bits(f0))
    want = world.sg(hop)(f0s.view(1, 1, -1)).cpu().numpy().reshape(-1)
    assert exc.shape == want.shape == (F * hop,) and np.abs(want).max() > 0.05
    assert np.array_equal(_bits(exc), _bits(want))
    host = Dc.F0Statistics().convert(raw.astype(np.float64), src, trg).astype(np.float32)
    got, v = f0s.cpu().numpy(), raw > 0
    assert not got[~v].any()
    assert np.abs(got[v].view(np.int32).astype(np.int64) - host[v].view(np.int32).astype(np.int64)).max() <= 1


@pytest.mark.parametrize("norm", ["window", "running"])
def test_tracked_session_returns_the_samples_of_a_session_fed_its_f0(dev, world, norm):
    """No F0 statistics: everything a tracked session returns, as int16, is what a session with f0="given", loudness="audio"
    returns that is fed the tracked F0 with the same ppg, audio, embedding and chunking (the windows are the same; they
    run `lag` frames later)."""
    hop, F = 160, 48
    y, _, f0 = world.whole_track(F, hop, 4)
    with _session(world, dev, hop, norm=norm, pcm16=True) as s:
        sid = s.open(world.emb)
        a = np.concatenate(_feed(world, s, sid, y, _split(F, 7), hop))
        assert np.array_equal(_bits(_traced(s, sid)), _bits(f0))
    with _session(world, dev, hop, norm=norm, pcm16=True, f0="given", track=None) as s:
        sid = s.open(world.emb)
        b = np.concatenate(_feed(world, s, sid, y, _split(F, 7), hop, f0=f0))
    assert a.dtype == np.int16 and a.shape == (F * hop,) and np.abs(a).max() > 30
    assert np.array_equal(a, b)


def test_running_statistics_see_the_tracked_f0_in_frame_order(dev, world):
    """RunningF0Stats with tracking: the traced shifted F0 is within one float32 ulp of running_f0_convert over the traced
    tracked F0, whatever the chunking; a stream with list statistics and one with none run beside it."""
    hop, F = 160, 60
    y, _, f0 = world.whole_track(F, hop, 0)
    run, trg = Dc.RunningF0Stats(prior=(5.0, 0.3), prior_frames=5.0, horizon=40.0), [5.4, 0.3]
    with _session(world, dev, hop, n_streams=3) as s:
        ids = [s.open(world.emb, run, trg), s.open(world.emb, [5.0, 0.25], trg), s.open(world.emb)]
        at = 0
        for i, k in enumerate(IRREGULAR):
            s.push({sid: _chunk(world, y, at, k, hop) for sid in ids}, end=ids if i == len(IRREGULAR) - 1 else ())
            at += k
        raw, shifted = _traced(s, ids[0]), _traced(s, ids[0], "f0_shifted")
        for sid in ids:
            assert np.array_equal(_bits(_traced(s, sid)), _bits(f0))
        assert np.array_equal(_bits(_traced(s, ids[2], "f0_shifted")), _bits(f0))
    want = Dc.running_f0_convert(raw, run, trg).astype(np.float32)
    v = raw > 0
    assert v.sum() >= 20 and not shifted[~v].any()
    ulps = np.abs(shifted[v].view(np.int32).astype(np.int64) - want[v].view(np.int32).astype(np.int64))
    print(f"running shift over the tracked F0: largest difference {int(ulps.max())} ulp")
    assert ulps.max() <= 1


def test_refusals_leave_a_tracked_session_usable(dev, world):
    """f0_track without f0="audio" and a tracker that is no F0Track are refused at construction; a refused push in the middle
    of a tracked stream changes nothing: the stream goes on to the whole-file track."""
    hop, F = 160, 30
    y, cands, f0 = world.whole_track(F, hop, 5)
    model, sg = world.model(hop), world.sg(hop)
    for kw in (dict(f0_track=Dc.F0Track()), dict(loudness="audio", f0_track=Dc.F0Track()),
               dict(loudness="audio", f0="audio", f0_track=8)):
        with pytest.raises(ValueError):
            Dc.StreamSession(model, sg, dev, core=CORE, context=CONTEXT, fade=FADE, **kw)
    good = _chunk(world, y, 0, 4, hop)
    with _session(world, dev, hop) as s:
        sid = s.open(world.emb)
        at = 0
        for i, k in enumerate(_split(F, 7)):
            with pytest.raises(ValueError):
                s.push({sid: dict(good, f0=np.full(4, 100.0, np.float32))})
            with pytest.raises(ValueError):
                s.push({sid: dict(good, audio=good["audio"][:-1])})
            s.push({sid: _chunk(world, y, at, k, hop)}, end=[sid] if at + k == F else ())
            at += k
        _same_as_whole(s, sid, cands, f0, "after refusals")


def test_the_entry_point_refuses_before_it_launches(dev):
    """fastsvc_stream_f0_tracked through its wrapper: frames to emit that are not the `lag`-behind range, too many of them, a
    lag or a cost out of range and rings of another shape are refused and nothing is enqueued; the valid call on silence
    writes four frames of absent candidates and two unvoiced tracked frames, and nothing else."""
    from svcc23_fastsvc_amd.engine import stream_f0_tracked
    hop, cap = 160, 16
    audio, exc = torch.zeros((1, cap * hop), device=dev), torch.zeros((1, cap * hop), device=dev)
    f0r, f0s, phase = torch.full((1, cap), 7.0, device=dev), torch.zeros((1, cap), device=dev), torch.zeros((1, 2), dtype=torch.float64, device=dev)
    cand, back = torch.full((1, cap, 4, 2), 3.0, device=dev), torch.zeros((1, cap, 8), dtype=torch.uint8, device=dev)
    rec = torch.zeros((1, 2, 8), dtype=torch.float64, device=dev)
    base = dict(streams=[0], first_frame=[0], n=[4], seen=[16], ended=[0], parity=[0], track_parity=[0], emit_first=[0], emit_n=[2],
                seed=[0], stats=[None], running=None)
    fixed = dict(cap=cap, max_frames=8, sample_rate=24000.0, f0_floor=70.0, f0_ceil=340.0, cand_threshold=0.5, lag=2, lag_bias=0.2,
                 jump=1.0, switch=0.3, unvoiced=0.15, sine_amp=0.1, noise_amp=0.0)

    def call(rings=None, **kw):
        a = dict(base, **{k: v for k, v in kw.items() if k in base})
        f = dict(fixed, **{k: v for k, v in kw.items() if k in fixed})
        stream_f0_tracked(audio, *(rings or (cand, back)), f0r, f0s, exc, phase, None, rec, **a, **f)
    for kw in (dict(emit_n=[3]), dict(emit_n=[1]), dict(emit_first=[1], emit_n=[2]), dict(n=[9]), dict(lag=65), dict(lag=-1),
               dict(jump=-1.0), dict(unvoiced=float("nan")), dict(cand_threshold=0.0), dict(streams=[1]), dict(n=[8], seen=[8]),
               dict(ended=[1], emit_n=[4])):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError):
        call(rings=(cand[:, :8].contiguous(), back))
    torch.cuda.synchronize()
    assert not exc.cpu().numpy().any() and not rec.cpu().numpy().any() and (cand.cpu().numpy() == 3.0).all()
    call()
    torch.cuda.synchronize()
    c = cand.cpu().numpy()[0]
    assert not c[:4, :, 0].any() and np.isinf(c[:4, :, 1]).all() and (c[4:] == 3.0).all()
    assert np.array_equal(f0r.cpu().numpy()[0], [0.0] * 2 + [7.0] * 14) and not exc.cpu().numpy().any()
    r = rec.cpu().numpy()[0]
    assert np.isinf(r[1, :4]).all() and r[1, 4] == 0.0 and not r[0].any()      # (entry 1: the costs after four unvoiced frames)
