"""GPU tests (-m gpu) of the running source F0 statistics of live streams (decode.RunningF0Stats, csrc/fastsvc_stream_f0.hip:
stream_f0_running_kernel, fastsvc_stream_f0_running): the traced shifted F0 against the float64 reference
(tests/stream_f0_stats_ref.py) run over the traced raw F0, a heavy prior against F0Statistics.convert, a call of more frames
than one tile of the kernel holds, bit-for-bit
independence of push schedules, slots, the ring's wrap and slot reuse, neighbours with list statistics or none, a session
that runs its statistics against one that is fed its shifted F0, f0_stats(id), and refusals.  The shapes are
test_stream_f0_gpu.py's: tiny generators (hop 160 and 256), at most 3 slots and 60 frames."""
import numpy as np
import pytest
import torch

import stream_f0_ref as R
import stream_f0_stats_ref as Q
import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd import engine as E
from svcc23_fastsvc_amd import synth as S

pytestmark = pytest.mark.gpu

CORE, CONTEXT, FADE = 8, 8, 4
SCALES = {160: (2, 4, 4, 5), 256: (4, 4, 4, 4)}
HOPS = (160, 256)
TRG = [5.45, 0.33]
IRREGULAR = [3, 0, 11, 1, 32, 6, 7]
# (prior, prior_frames, horizon) of the three settings; 8 voiced frames: short enough that the decay matters within 60 frames
SETTINGS = ((None, 100.0, None), ([5.1, 0.21], 10.0, None), (None, 100.0, 8.0))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    A.load_library()
    return torch.device("cuda:0")


class _World:
    pass


@pytest.fixture(scope="module")
def world(dev):
    """Per hop a tiny generator (8 input channels, 16-value embedding; wide: 48 and multiples of 24) and a noiseless signal
    generator, made on first use; ppg and an embedding for 60 frames; the streams' audio."""
    w = _World()
    w.models, w.sgs, w.audio = {}, {}, {}
    rng = np.random.default_rng(4097)
    w.ppg = rng.standard_normal((60, 8)).astype(np.float32)
    w.ppg_wide = rng.standard_normal((60, 48)).astype(np.float32)
    w.emb = rng.standard_normal(16).astype(np.float32)

    def model(hop, wide=False):
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

    def sg(hop):
        if hop not in w.sgs:
            w.sgs[hop] = A.SignalGenerator(sample_rate=R.SR, hop_size=hop, sine_amp=0.1, noise_amp=0.0, signal_types=["sine"])
        return w.sgs[hop]

    def audio(F, hop, seed):
        if (F, hop, seed) not in w.audio:
            w.audio[F, hop, seed] = R.voiced_stream(F, hop, seed)
        return w.audio[F, hop, seed]
    w.model, w.sg, w.stream_audio = model, sg, audio
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


def _session(w, dev, hop, n_streams=1, wide=False, **kw):
    kw = dict(dict(core=CORE, context=CONTEXT, fade=FADE, max_push=12, pcm16=False, loudness="audio", f0="audio"), **kw)
    s = Dc.StreamSession(w.model(hop, wide), w.sg(hop), dev, n_streams=n_streams, **kw)
    s._stream_trace = {}
    return s


def _feed(w, s, sids, audio, sched, hop, end=True, f0=None, wide=False):
    """Push the same audio to every stream of ``sids`` in the chunks ``sched`` -> {id: [what each push returned]}."""
    sids = list(sids) if isinstance(sids, (list, tuple)) else [sids]
    pieces, at = {sid: [] for sid in sids}, 0
    for i, k in enumerate(sched):
        last = end is True and i == len(sched) - 1
        out = s.push({sid: _chunk(w, audio, at, k, hop, f0, wide) for sid in sids}, end=sids if last else ())
        for sid in sids:
            pieces[sid].append(out[sid])
        at += k
    assert at * hop == audio.size
    if end == "alone":
        out = s.end(sids)
        for sid in sids:
            pieces[sid].append(out[sid])
    return pieces


def _traced(s, sid, key="f0"):
    return torch.cat(s._stream_trace[key][sid]).cpu().numpy()


def _running(prior, frames, horizon):
    return Dc.RunningF0Stats(prior, frames, horizon)


def _both_kinds(raw):
    voiced = raw > 0
    assert voiced.sum() >= 20 and (~voiced).sum() >= 1
    return voiced


# ------------------------------------------------------------------------------------------------ 1: against the reference

@pytest.mark.parametrize("hop", HOPS)
def test_shifted_f0_is_within_one_ulp_of_the_reference(dev, world, hop):
    """60 frames, the three settings as three streams of one session, fed the same audio.  The reference runs over the traced
    raw F0, so YIN's float32 stays out of it.  Every operation of the rule is float64 on both sides; device and numpy log / exp
    differ by a few float64 ulps, amplified by at most s_t / s_p sqrt(N / n0) < 10 here: ~1e-14 relative against float32's half
    ulp of 6e-8, so only a rounding tie moves the result - one float32 ulp on voiced frames, exactly 0 on unvoiced ones."""
    F = 60
    y = world.stream_audio(F, hop, 0)
    with _session(world, dev, hop, n_streams=3) as s:
        ids = [s.open(world.emb, _running(*st), TRG) for st in SETTINGS]
        _feed(world, s, ids, y, _split(F, 7), hop)
        raw = [_traced(s, i) for i in ids]
        got = [_traced(s, i, "f0_shifted") for i in ids]
    voiced = _both_kinds(raw[0])
    worst = 0
    for j, st in enumerate(SETTINGS):
        assert raw[j].shape == got[j].shape == (F,) and np.array_equal(_bits(raw[j]), _bits(raw[0]))
        c = Q.constants(TRG, *st)
        assert c[1] > 0 and c[5] / c[1] * np.sqrt((c[2] + F) / c[2]) < 10
        want = Q.running_loop(raw[j], c).out.astype(np.float32)
        assert not got[j][~voiced].any() and not want[~voiced].any()
        assert np.isfinite(got[j]).all() and (got[j][voiced] > 0).all()
        ulps = Q.ulps32(got[j][voiced], want[voiced])
        print(f"running F0 shift hop {hop}, {st}: device against the reference, largest difference {int(ulps.max())} ulp")
        worst = max(worst, int(ulps.max()))
    assert worst <= 1
    assert not np.array_equal(_bits(got[2]), _bits(got[0]))               # (the horizon of 8 frames matters within 60)
    assert np.abs(got[1][voiced] / raw[1][voiced] - 1.0).max() > 0.05     # (... and it did shift)


# --------------------------------------------------------------------------------------------------------- 2: heavy prior

@pytest.mark.parametrize("hop", HOPS)
def test_a_heavy_prior_is_the_fixed_shift_to_one_ulp(dev, world, hop):
    """prior = src with 1e15 frames: 60 frames of evidence move mu and var by ~1e-13, far below float32's half ulp, so the
    result is F0Statistics.convert(raw, src, trg) rounded to float32, up to a rounding tie."""
    F = 60
    y = world.stream_audio(F, hop, 0)
    src = [5.1, 0.21]
    with _session(world, dev, hop) as s:
        sid = s.open(world.emb, _running(src, 1e15, None), TRG)
        _feed(world, s, sid, y, _split(F, 7), hop)
        raw, got = _traced(s, sid), _traced(s, sid, "f0_shifted")
    voiced = _both_kinds(raw)
    want = Dc.F0Statistics().convert(raw.astype(np.float64), src, TRG).astype(np.float32)
    assert not got[~voiced].any()
    ulps = Q.ulps32(got[voiced], want[voiced])
    print(f"heavy prior hop {hop}: device against F0Statistics.convert, largest difference {int(ulps.max())} ulp")
    assert ulps.max() <= 1


# ------------------------------------------------------------------------------------- 2b: more frames than one tile holds

def test_a_call_of_more_than_one_tile_carries_the_state_across_tiles(dev):
    """The kernel walks a call's frames in tiles of 256 and carries (w, S1, S2) from tile to tile; the sessions above finalise
    at most 38 frames a call.  Through the wrapper: 300 frames of one stream in ONE call (a tile of 256 and one of 44), with a
    horizon, against the reference over the raw F0 the call wrote - one float32 ulp, as above - and against the same frames
    in calls of 150 + 150 and of 256 + 44 (a tile exactly full), whose record travels through the parity pair: the same bits,
    the same record."""
    hop, cap, F = 160, 320, 300
    y = torch.from_numpy(R.voiced_stream(cap, hop, 6)).to(dev).view(1, cap * hop)
    setting = ([5.1, 0.21], 10.0, 40.0)
    consts = Dc.RunningF0Stats(*setting).constants(TRG)
    fixed = dict(cap=cap, max_frames=cap, sample_rate=float(R.SR), f0_floor=70.0, f0_ceil=340.0, threshold=0.15, sine_amp=0.1,
                 noise_amp=0.0)
    runs = []
    for parts in ([F], [150, 150], [256, 44]):
        f0r, f0s = torch.zeros((1, cap), device=dev), torch.zeros((1, cap), device=dev)
        exc, phase = torch.zeros((1, cap * hop), device=dev), torch.zeros((1, 2), dtype=torch.float64, device=dev)
        rec = torch.full((1, 2, 4), float("nan"), dtype=torch.float64, device=dev)
        first = 0
        for i, k in enumerate(parts):
            E.stream_f0_running(y, f0r, f0s, exc, phase, rec, streams=[0], first_frame=[first], n=[k], seen=[cap], ended=[0],
                                parity=[i & 1], seed=[0], stats=[None], running=[consts], **fixed)
            first += k
        runs.append((f0r.cpu().numpy()[0, :F], f0s.cpu().numpy()[0, :F], rec.cpu().numpy()[0, len(parts) & 1]))
    raw, got, state = runs[0]
    voiced = raw > 0
    assert voiced.sum() >= 270 and (~voiced).sum() >= 1 and voiced[256:].sum() >= 20
    t = Q.running_loop(raw, Q.constants(TRG, *setting))
    want = t.out.astype(np.float32)
    ulps = Q.ulps32(got[voiced], want[voiced])
    print(f"300 frames in one call: device against the reference, largest difference {int(ulps.max())} ulp")
    assert ulps.max() <= 1 and not got[~voiced].any()
    # (the record: w is plain arithmetic on the host's g; d is a log near 5, a few float64 ulps - ~1e-15 - from numpy's, |d| < 1,
    # and the sums weigh at most 1 / (1 - g) = 40.5 frames: 1e-12 absolute leaves a decade)
    assert state[3] == voiced.sum() and state[0] == t.w[-1]
    assert abs(state[1] - t.s1[-1]) <= 1e-12 and abs(state[2] - t.s2[-1]) <= 1e-12
    for raw_k, got_k, state_k in runs[1:]:
        assert np.array_equal(_bits(raw_k), _bits(raw)) and np.array_equal(_bits(got_k), _bits(got))
        assert np.array_equal(state_k.view(np.uint64), state.view(np.uint64))


# ----------------------------------------------------------------------------------------------------------- 3: schedules

@pytest.mark.parametrize("hop", HOPS)
def test_the_shift_and_the_excitation_do_not_depend_on_the_schedule(dev, world, hop):
    """Frame by frame, in 7s, in 32s (= max_push), irregularly with an empty push, the end sent alone: the traced shifted F0 and
    the traced excitation are the same bits, and the excitation is the device SignalGenerator's of the whole shifted F0."""
    F = 60
    y = world.stream_audio(F, hop, 0)
    first = None
    for name, sched, end in (("1s", [1] * F, True), ("7s", _split(F, 7), True), ("32s", _split(F, 32), True),
                             ("irregular", IRREGULAR, True), ("end alone", _split(F, 7), "alone")):
        with _session(world, dev, hop, max_push=32) as s:
            sid = s.open(world.emb, _running([5.1, 0.21], 10.0, 20.0), TRG)
            _feed(world, s, sid, y, sched, hop, end)
            raw = _traced(s, sid)
            f0s = torch.cat(s._stream_trace["f0_shifted"][sid])
            exc = _traced(s, sid, "excitation")
        got = (f0s.cpu().numpy(), exc)
        if first is None:
            first = got
            _both_kinds(raw)
            want = world.sg(hop)(f0s.view(1, 1, -1)).cpu().numpy().reshape(-1)
            assert exc.shape == want.shape == (F * hop,) and np.abs(want).max() > 0.05
            assert np.array_equal(_bits(exc), _bits(want))
        assert got[0].shape == (F,) and np.array_equal(_bits(got[0]), _bits(first[0])), name
        assert np.array_equal(_bits(got[1]), _bits(first[1])), name


# -------------------------------------------------------------------------------------------------- 4: wrap, slots, reuse

@pytest.mark.parametrize("hop", HOPS)
def test_across_the_wrap_slots_and_a_reused_slot(dev, world, hop):
    """max_push 12: the rings hold fewer frames than the longest stream has.  Three slots at once with streams of 3, 25 and 60
    frames in different chunkings and settings, then slot 0 reused after its stream ended - the record is never zeroed: every
    stream's shifted F0 equals, bit for bit, the same stream run alone in slot 0 of a fresh session."""
    Fs, scheds = (3, 25, 60), ([3], _split(25, 7), [5, 12, 0, 1, 12, 12, 7, 11])
    data = [world.stream_audio(F, hop, 1 + j) for j, F in enumerate(Fs)]
    settings = [SETTINGS[2], SETTINGS[1], SETTINGS[0], ([5.3, 0.4], 3.0, 5.0)]            # (the last: the reused slot's)
    with _session(world, dev, hop, n_streams=3) as s:
        assert s.cap < 60
        ids = [s.open(world.emb, _running(*settings[j]), TRG) for j in range(3)]
        assert [s._ids[i] for i in ids] == [0, 1, 2]
        at = [0, 0, 0]
        for i in range(max(len(sc) for sc in scheds)):
            chunks, end = {}, []
            for j in range(3):
                if i < len(scheds[j]):
                    chunks[ids[j]] = _chunk(world, data[j], at[j], scheds[j][i], hop)
                    at[j] += scheds[j][i]
                    if i == len(scheds[j]) - 1:
                        end.append(ids[j])
            s.push(chunks, end)
            if i == 3:                                   # (slots 0 and 1 are free again: a new stream takes slot 0)
                again = s.open(world.emb, _running(*settings[3]), TRG)
                assert s._ids[again] == 0
                _feed(world, s, again, data[1], [12, 12, 1], hop)
        got = [_traced(s, i, "f0_shifted") for i in ids + [again]]
        raws = [_traced(s, i) for i in ids + [again]]
    assert sum((r > 0).sum() for r in raws) >= 20
    for j, (F, y) in enumerate(zip(Fs + (25,), data + [data[1]])):
        with _session(world, dev, hop) as s:
            sid = s.open(world.emb, _running(*settings[j]), TRG)
            assert s._ids[sid] == 0
            _feed(world, s, sid, y, _split(F, 9), hop)
            alone = _traced(s, sid, "f0_shifted")
        assert alone.shape == (F,) and np.array_equal(_bits(got[j]), _bits(alone)), (j, F)
        assert (alone > 0).sum() == (raws[j] > 0).sum()


# ------------------------------------------------------------------------------------------------------------ 5: neighbours

def test_neighbours_keep_their_bits_and_a_session_without_running_streams_its_entry_point(dev, world, monkeypatch):
    """A stream with list statistics, one with none and a running one, pushed together: the first two return the traced F0
    bits and the output bytes they return in a session that never had the running stream - where the new entry point is not
    called at all (the session makes fastsvc_stream_f0's launches, with its arguments), while the mixed session calls it."""
    hop, F = 160, 40
    y = world.stream_audio(F, hop, 2)
    calls = []
    real = E.stream_f0_running

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(E, "stream_f0_running", counted)
    results = []
    for mixed in (False, True):
        calls.clear()
        with _session(world, dev, hop, n_streams=3) as s:
            ids = [s.open(world.emb, [5.0, 0.25], [5.4, 0.3]), s.open(world.emb)]
            if mixed:
                ids.append(s.open(world.emb, Dc.RunningF0Stats(), TRG))
            out = _feed(world, s, ids, y, _split(F, 7), hop)
            results.append([(np.concatenate(out[i]), _traced(s, i, "f0_shifted"), _traced(s, i)) for i in ids])
        assert bool(calls) == mixed
    plain, with_running = results
    for j in range(2):
        for a, b in zip(plain[j], with_running[j]):
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), j
    assert np.array_equal(_bits(plain[1][1]), _bits(plain[1][2]))          # (no statistics: the raw F0)
    raw = with_running[2][2]
    assert not np.array_equal(_bits(with_running[2][1]), _bits(raw)) and (raw > 0).sum() >= 20


# ------------------------------------------------------------------------------------------------------------ 6: end to end

@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
@pytest.mark.parametrize("norm", ["window", "running"])
def test_a_running_session_returns_the_bytes_of_a_session_fed_its_shifted_f0(dev, world, norm, storage):
    """f0="audio" with RunningF0Stats() against f0="given", loudness="audio" opened without statistics and fed the first one's
    traced shifted F0, the same ppg, audio, embedding and chunking: the same int16 bytes, push by push (the wide generator and
    48 frames: what bfloat16 storage asks of the plan and of a row)."""
    hop, F = 160, 48
    y = world.stream_audio(F, hop, 4)
    model = world.model(hop, wide=True)
    model.use_activation_storage(storage)
    try:
        with _session(world, dev, hop, norm=norm, pcm16=True, wide=True) as s:
            sid = s.open(world.emb, Dc.RunningF0Stats(), TRG)
            a = _feed(world, s, sid, y, _split(F, 7), hop, wide=True)[sid]
            raw, f0 = _traced(s, sid), _traced(s, sid, "f0_shifted")
            forwards = s.forwards
        with _session(world, dev, hop, norm=norm, pcm16=True, f0="given", wide=True) as s:
            sid = s.open(world.emb)
            b = _feed(world, s, sid, y, _split(F, 7), hop, f0=f0, wide=True)[sid]
            assert s.forwards == forwards
    finally:
        model.use_activation_storage("float32")
    assert (raw > 0).sum() >= 20 and not np.array_equal(_bits(raw), _bits(f0))
    assert sum(p.size for p in a) == F * hop and a[0].dtype == np.int16 and np.abs(np.concatenate(a)).max() > 30
    assert len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a, b))


# -------------------------------------------------------------------------------------------------------------- 7: f0_stats

@pytest.mark.parametrize("hop", HOPS)
def test_f0_stats_reads_the_streams_record(dev, world, hop):
    """After 60 frames were pushed (the stream still open: the frames that are final are the traced ones): observed_mean and
    observed_std are F0Statistics.estimate of the traced raw F0 to 1e-10 relative - sums of at most 60 terms taken about the
    prior mean lose ~1e-13 on the variance - voiced_frames is exact, and mean and std are those the reference shifted the
    last voiced frame with, to 1e-12.  Before the first frame they are the prior's; after the end the stream is unknown."""
    F = 60
    y = world.stream_audio(F, hop, 0)
    prior, frames = [5.1, 0.21], 10.0
    with _session(world, dev, hop, n_streams=2) as s:
        s.open(world.emb)                                # (slot 0: the stream under test sits in slot 1)
        sid = s.open(world.emb, _running(prior, frames, None), TRG)
        st = s.f0_stats(sid)
        assert st["voiced_frames"] == 0 and st["weight"] == 0.0 and st["mean"] == prior[0] and abs(st["std"] - prior[1]) < 1e-15
        assert np.isnan(st["observed_mean"]) and np.isnan(st["observed_std"])
        _feed(world, s, sid, y, _split(F, 7), hop, end=False)
        raw = _traced(s, sid)
        st = s.f0_stats(sid)
        with pytest.raises(ValueError):
            s.f0_stats(0)                                # (slot 0's stream has no running statistics)
        s.end([sid])
        with pytest.raises(ValueError):
            s.f0_stats(sid)
    voiced = raw > 0
    assert raw.size < F and voiced.sum() >= 20 and (~voiced).sum() >= 1
    est = Dc.F0Statistics().estimate([raw.astype(np.float64)])
    t = Q.running_loop(raw, Q.constants(TRG, prior, frames))
    assert st["voiced_frames"] == int(voiced.sum()) and st["weight"] == float(voiced.sum())
    print(f"f0_stats hop {hop}: observed mean {abs(st['observed_mean'] / est[0] - 1):.2e}, std {abs(st['observed_std'] / est[1] - 1):.2e} "
          f"relative to estimate; mean {abs(st['mean'] / t.mean[-1] - 1):.2e}, std {abs(st['std'] / np.sqrt(t.var[-1]) - 1):.2e} to the reference")
    assert abs(st["observed_mean"] / est[0] - 1.0) <= 1e-10 and abs(st["observed_std"] / est[1] - 1.0) <= 1e-10
    assert abs(st["mean"] / t.mean[-1] - 1.0) <= 1e-12 and abs(st["std"] / np.sqrt(t.var[-1]) - 1.0) <= 1e-12


# -------------------------------------------------------------------------------------------------------------- 8: refusals

def test_refusals_leave_the_session_usable(dev, world):
    """open refuses RunningF0Stats without trg_f0_stats, and in an f0="given" session; f0_stats refuses a stream with list
    statistics; each is a ValueError between two pushes, and every push returns an undisturbed session's bytes.  Through the
    wrapper the C entry point refuses a null record, s_p = 0, n0 = 0 and g = 1.5 before anything is enqueued."""
    hop, F = 160, 30
    y = world.stream_audio(F, hop, 5)
    sched = _split(F, 7)
    with _session(world, dev, hop, n_streams=2) as s:
        sid = s.open(world.emb, Dc.RunningF0Stats(), TRG)
        want = _feed(world, s, sid, y, sched, hop)[sid]
    with _session(world, dev, hop, n_streams=2) as s:
        sid = s.open(world.emb, Dc.RunningF0Stats(), TRG)
        at = 0
        for i, k in enumerate(sched):
            with pytest.raises(ValueError):
                s.open(world.emb, Dc.RunningF0Stats())
            with pytest.raises(ValueError):
                s.open(world.emb, Dc.RunningF0Stats(), [5.4, float("nan")])
            assert s._slots[1] is None and len(s._ids) == 1
            got = s.push({sid: _chunk(world, y, at, k, hop)}, end=[sid] if i == len(sched) - 1 else ())[sid]
            at += k
            assert np.array_equal(_bits(got), _bits(want[i])), i
        listed = s.open(world.emb, [5.0, 0.25], [5.4, 0.3])
        with pytest.raises(ValueError):
            s.f0_stats(listed)
    with _session(world, dev, hop, f0="given") as s:
        with pytest.raises(ValueError):
            s.open(world.emb, Dc.RunningF0Stats(), TRG)
        assert s._slots == [None] and s.open(world.emb, [5.0, 0.25], [5.4, 0.3]) == 0
    # the C entry point, through the wrapper: nothing is enqueued
    cap = 16
    audio, exc = torch.zeros((1, cap * hop), device=dev), torch.zeros((1, cap * hop), device=dev)
    f0r, f0s = torch.full((1, cap), 7.0, device=dev), torch.full((1, cap), 7.0, device=dev)
    phase = torch.zeros((1, 2), dtype=torch.float64, device=dev)
    rec = torch.full((1, 2, 4), 3.0, dtype=torch.float64, device=dev)
    ok = (5.0, 0.2, 10.0, 1.0, 5.4, 0.3)
    base = dict(record=rec, streams=[0], first_frame=[0], n=[4], seen=[16], ended=[0], parity=[0], seed=[0], stats=[None], running=[ok])
    fixed = dict(cap=cap, max_frames=8, sample_rate=24000.0, f0_floor=70.0, f0_ceil=340.0, threshold=0.15, sine_amp=0.1, noise_amp=0.0)
    for kw in (dict(record=None), dict(running=[(5.0, 0.0, 10.0, 1.0, 5.4, 0.3)]), dict(running=[(5.0, 0.2, 0.0, 1.0, 5.4, 0.3)]),
               dict(running=[(5.0, 0.2, 10.0, 1.5, 5.4, 0.3)]), dict(running=[(5.0, 0.2, 10.0, 0.0, 5.4, 0.3)]),
               dict(running=[(float("inf"), 0.2, 10.0, 1.0, 5.4, 0.3)]), dict(stats=[(5.0, 0.2, 5.4, 0.3)]), dict(n=[9])):
        with pytest.raises(ValueError):
            E.stream_f0_running(audio, f0r, f0s, exc, phase, **dict(base, **kw), **fixed)
    torch.cuda.synchronize()
    assert not exc.cpu().numpy().any() and not phase.cpu().numpy().any()
    assert (rec.cpu().numpy() == 3.0).all() and (f0r.cpu().numpy() == 7.0).all() and (f0s.cpu().numpy() == 7.0).all()
    E.stream_f0_running(audio, f0r, f0s, exc, phase, **base, **fixed)      # (silence: four unvoiced frames from a fresh state)
    torch.cuda.synchronize()
    assert np.array_equal(f0r.cpu().numpy()[0], [0.0] * 4 + [7.0] * 12) and np.array_equal(f0s.cpu().numpy()[0], [0.0] * 4 + [7.0] * 12)
    assert np.array_equal(rec.cpu().numpy()[0], [[3.0] * 4, [0.0] * 4]) and not exc.cpu().numpy().any()
