"""GPU tests (-m gpu) of the live-stream decode: the push and assemble kernels (csrc/fastsvc_stream.hip) bit for bit
against a numpy ring model and SignalGenerator, and StreamSession against the float64 oracle of the WHOLE utterance (no
speaker: the same function), against every window run alone (with a speaker: per-window InstanceNorm statistics), across
push schedules and slot reuse, in bfloat16 storage, and its refusals."""
import numpy as np
import pytest
import torch

import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd import synth as S

pytestmark = pytest.mark.gpu

# tests/test_decode_windowed_gpu.py's constants, with their meanings
TIGHT = 1e-4                # x max(1, |ref|max): the suite's float32 bound against the oracle
BATCHING = 2e-5             # x max(1, |ref|max): the batching invariance the harness states (tests/test_parity_gpu.py)
BF16_MEAN, BF16_MAX = 3e-2, 0.13        # tests/test_config_matrix_gpu.py: x rms / x max(1, |ref|max) of the reference
SIZES = (1, 3, 4, 45, 0, 7, 48)         # chunk sizes the kernel tests cycle through


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    A.load_library()
    return torch.device("cuda:0")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _module(cfg, sd, dev, storage="float32"):
    g = A.FastSVCGenerator(in_channels=cfg.in_channels, mid_channels=list(cfg.mid_channels),
                           upsampling_scales=list(cfg.upsampling_scales), out_channels=cfg.out_channels,
                           spk_emb_size=cfg.spk_emb_size, use_spk_emb=cfg.use_spk_emb)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    g.remove_weight_norm()
    g.activation_storage = storage
    return g.eval().to(dev)


def _sg(hop, noise=0.0):
    return A.SignalGenerator(sample_rate=24000, hop_size=hop, sine_amp=0.1, noise_amp=noise, signal_types=["sine"])


def _f0(F, seed):
    """F0 in {0} u [50, 1000] Hz as float32: voiced and unvoiced stretches of random lengths."""
    rng = np.random.default_rng(seed)
    f0 = rng.uniform(50.0, 1000.0, F).astype(np.float32)
    f0[0], f0[-1] = 50.0, 1000.0
    i = 0
    while i < F:
        n = int(rng.integers(1, 40))
        if rng.random() < 0.35:
            f0[i: i + n] = 0.0
        i += n
    return f0


class _Rings:
    """The device state of n streams, as StreamSession holds it, full of NaN."""

    def __init__(self, dev, n, cap, C, hop):
        nan = float("nan")
        self.n, self.cap, self.C, self.hop, self.dev = n, cap, C, hop, dev
        self.ppg = torch.full((n, cap, C), nan, dtype=torch.float32, device=dev)
        self.lft = torch.full((n, cap * hop), nan, dtype=torch.float32, device=dev)
        self.exc = torch.full((n, cap * hop), nan, dtype=torch.float32, device=dev)
        self.phase = torch.full((n, 2), nan, dtype=torch.float64, device=dev)
        self.pos, self.par = [0] * n, [0] * n

    def push(self, chunks, max_push, noise=0.0, seeds=None, base=0):
        """chunks: {stream: (ppg (k, C), f0 (k,), lft (k hop,))}, packed back to back from element `base`."""
        from svcc23_fastsvc_amd.engine import stream_push
        up, offs = [np.zeros(base, np.float32)], []
        for s, (ppg, f0, lft) in chunks.items():
            offs.append(sum(u.size for u in up))
            up += [ppg.reshape(-1), f0, lft]
        streams = list(chunks)
        ks = [chunks[s][1].size for s in streams]
        stream_push(torch.from_numpy(np.concatenate(up + [np.zeros(1, np.float32)])).to(self.dev), streams, ks, offs,
                    [self.pos[s] for s in streams], [self.pos[s] == 0 for s in streams], [self.par[s] for s in streams],
                    [0 if seeds is None else seeds[s] for s in streams], self.ppg, self.lft, self.exc, self.phase, max_push,
                    24000.0, 0.1, noise)
        for s, k in zip(streams, ks):
            self.pos[s] += k
            self.par[s] ^= 1 if k else 0

    def excitation(self, s, lo, hi):
        """Samples of frames [lo, hi) of stream s, out of the ring."""
        idx = torch.arange(lo, hi, device=self.dev) % self.cap
        return self.exc[s].view(self.cap, self.hop)[idx].reshape(-1).cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ push
@pytest.mark.parametrize("C,hop", [(144, 160), (100, 60)])
def test_push_equals_a_numpy_ring_model(dev, C, hop):
    """Two streams (and a third that is never pushed) in rings of 64 frames full of NaN; chunks of 1, 3, 4, 45, 0, 7, 48
    frames, another phase of the cycle per stream, one slice 16-byte aligned in the upload buffer and the other not,
    until both rings have wrapped three times.  After EVERY push the three rings equal a numpy model bit for bit - the
    excitation ring against SignalGenerator's on the whole f0 - and what was never written is still NaN."""
    cap, F = 64, 64 * 3 + 50
    total = F + 2 * sum(SIZES)                          # (the stream that is ahead stays within a cycle of the other)
    rng = np.random.default_rng(C)
    sg = _sg(hop)
    feats = []
    for s in range(2):
        f0 = _f0(total, 10 * C + s)
        exc = sg(torch.from_numpy(f0).to(dev).view(1, 1, -1)).cpu().numpy().reshape(-1)
        feats.append((rng.standard_normal((total, C)).astype(np.float32), f0,
                      rng.standard_normal(total * hop).astype(np.float32), exc))
    r = _Rings(dev, 3, cap, C, hop)
    want = [np.full((3, cap, w), np.nan, np.float32) for w in (C, hop, hop)]
    step = 0
    while min(r.pos[:2]) < F:
        chunks = {}
        for s in (1, 0):
            k, a = SIZES[(step + 3 * s) % len(SIZES)], r.pos[s]
            ppg, f0, lft, exc = feats[s]
            chunks[s] = (ppg[a: a + k], f0[a: a + k], lft[a * hop: (a + k) * hop])
            idx = np.arange(a, a + k) % cap
            want[0][s, idx] = ppg[a: a + k]
            want[1][s, idx] = lft[a * hop: (a + k) * hop].reshape(k, hop)
            want[2][s, idx] = exc[a * hop: (a + k) * hop].reshape(k, hop)
        r.push(chunks, 48, base=step % 2)               # (every other push: no slice is 16-byte aligned)
        for name, got, w in zip(("ppg", "lft", "excitation"), (r.ppg, r.lft, r.exc), want):
            assert np.array_equal(_bits(got.cpu().numpy().reshape(w.shape)), _bits(w)), (name, step, r.pos)
        step += 1
    assert 3 * cap <= min(r.pos[:2]) and max(r.pos[:2]) <= total and r.pos[2] == 0
    assert np.isnan(r.phase[2].cpu().numpy()).all() and np.isfinite(r.phase[:2].cpu().numpy()).all()


def test_push_refuses_what_it_cannot_run(dev):
    from svcc23_fastsvc_amd.engine import stream_push
    r = _Rings(dev, 2, 16, 4, 4)
    up = torch.zeros(8 * 9, device=dev)
    ok = dict(streams=[0, 1], n=[8, 0], up_off=[0, 0], pos=[0, 0], first=[1, 1], parity=[0, 0], seed=[0, 0])

    def call(max_push=8, **kw):
        stream_push(up, **dict(ok, **kw), ppg_ring=r.ppg, lft_ring=r.lft, exc_ring=r.exc, phase=r.phase, max_push=max_push,
                    sample_rate=24000.0, sine_amp=0.1, noise_amp=0.0)
    for key, val in (("n", [9, 0]), ("n", [-1, 0]), ("up_off", [1, 0]), ("up_off", [-1, 0]), ("streams", [0, 2]),
                     ("streams", [0, 0]), ("pos", [-1, 0])):
        with pytest.raises(ValueError):
            call(**{key: val})
    with pytest.raises(ValueError):                      # (a chunk may wrap once: max_push <= cap)
        call(max_push=17)
    assert np.isnan(r.ppg.cpu().numpy()).all() and np.isnan(r.phase.cpu().numpy()).all()       # nothing changed
    call()
    assert not r.ppg[0, :8].cpu().numpy().any() and np.isnan(r.ppg[0, 8:].cpu().numpy()).all()


def test_push_of_more_streams_than_one_launch_takes(dev):
    """70 streams (two launches), C = 5 and hop = 6 (no 16-byte path at all), 1 - 7 frames each into rings of 8 frames,
    twice, so that the second chunk wraps: the rings against the numpy model, bit for bit."""
    from svcc23_fastsvc_amd.engine import stream_launch_count
    n, cap, C, hop = 70, 8, 5, 6
    assert stream_launch_count(n) == 2
    rng = np.random.default_rng(70)
    r = _Rings(dev, n, cap, C, hop)
    want = [np.full((n, cap, w), np.nan, np.float32) for w in (C, hop)]
    for _ in range(2):
        chunks = {}
        for s in range(n):
            k, a = 1 + (s + r.pos[s]) % 7, r.pos[s]
            ppg, lft = rng.standard_normal((k, C)).astype(np.float32), rng.standard_normal(k * hop).astype(np.float32)
            chunks[s] = (ppg, np.full(k, 100.0 + s, np.float32), lft)
            want[0][s, np.arange(a, a + k) % cap] = ppg
            want[1][s, np.arange(a, a + k) % cap] = lft.reshape(k, hop)
        r.push(chunks, 7)
        assert np.array_equal(_bits(r.ppg.cpu().numpy()), _bits(want[0]))
        assert np.array_equal(_bits(r.lft.cpu().numpy().reshape(n, cap, hop)), _bits(want[1]))
    assert max(r.pos) > cap and np.isfinite(r.phase.cpu().numpy()).all()
    exc = r.exc.cpu().numpy().reshape(n, cap, hop)
    assert all(np.isfinite(exc[s, np.arange(r.pos[s] - min(r.pos[s], cap), r.pos[s]) % cap]).all() for s in range(n))


# ------------------------------------------------------------------------------------------------------ excitation
def _streamed(dev, f0, chunks, slot=0, noise=0.0, seed=0, hop=160):
    """The excitation of f0 pushed in these chunks into `slot` of three, collected out of the ring after every push."""
    r = _Rings(dev, 3, 64, 4, hop)
    out, a = [], 0
    for k in chunks:
        r.push({slot: (np.zeros((k, 4), np.float32), f0[a: a + k], np.zeros(k * hop, np.float32))}, 48, noise,
               seeds={slot: seed})
        out.append(r.excitation(slot, a, a + k))
        a += k
    assert a == f0.size
    return np.concatenate(out)


def _chunks(F, phase):
    out, left, i = [], F, phase
    while left:
        out.append(min(SIZES[i % len(SIZES)], left))
        left -= out[-1]
        i += 1
    return out


def test_streamed_excitation_is_the_whole_utterance_one(dev):
    """300 frames of f0 in {0} u [50, 1000] Hz.  Noise off: streamed in irregular chunks, frame by frame and in
    chunks of 48 it is SignalGenerator's excitation of the whole f0, bit for bit.  Noise 0.003: two chunkings with one
    seed give the same bits, two slots with one seed give the same bits, another seed gives other bits, and the
    unvoiced stretches are not silent."""
    F, hop = 300, 160
    f0 = _f0(F, 5)
    whole = _sg(hop)(torch.from_numpy(f0).to(dev).view(1, 1, -1)).cpu().numpy().reshape(-1)
    for chunks in (_chunks(F, 0), _chunks(F, 3), [1] * F, [48] * 6 + [12]):
        got = _streamed(dev, f0, chunks)
        assert np.array_equal(_bits(got), _bits(whole)), chunks[:8]
    a = _streamed(dev, f0, _chunks(F, 0), noise=0.003, seed=7)
    b = _streamed(dev, f0, _chunks(F, 2), noise=0.003, seed=7)
    c = _streamed(dev, f0, _chunks(F, 0), slot=2, noise=0.003, seed=7)
    d = _streamed(dev, f0, _chunks(F, 0), noise=0.003, seed=8)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))
    assert not np.array_equal(a, d) and not np.array_equal(a, whole)
    unvoiced = np.repeat(f0 == 0, hop)
    assert unvoiced.any() and len(np.unique(a[unvoiced])) > unvoiced.sum() // 2
    assert np.abs(a - whole).max() < 0.003 * 8           # (the same sine under the noise)


# -------------------------------------------------------------------------------------------------------- assemble
@pytest.mark.parametrize("C,hop", [(144, 160), (100, 60)])
def test_assemble_equals_numpy_slices_of_the_rings(dev, C, hop):
    """Rows of 1, 3, 4, 45 and 60 frames from two streams whose rings of 64 frames have wrapped (positions 100 and
    171), at first frames of every residue mod 4 - rows that straddle the wrap among them - and 70 rows, so two launches;
    outputs full of NaN: window_assemble's three outputs, bit for bit, the tails exactly zero.  Rows outside the retained
    frames raise ValueError."""
    from svcc23_fastsvc_amd.engine import stream_assemble, stream_launch_count
    rng = np.random.default_rng(hop)
    cap, width, pos = 64, 60, [100, 171, 0]
    hist = [(rng.standard_normal((p, C)).astype(np.float32), rng.standard_normal((p, hop)).astype(np.float32),
             rng.standard_normal((p, hop)).astype(np.float32)) for p in pos]
    rings = [np.full((3, cap, w), np.nan, np.float32) for w in (C, hop, hop)]
    for s, p in enumerate(pos):
        for f in range(max(0, p - cap), p):
            for q in range(3):
                rings[q][s, f % cap] = hist[s][q][f]
    d_ppg, d_lft, d_exc = (torch.from_numpy(a).to(dev) for a in rings)
    d_lft, d_exc = d_lft.view(3, cap * hop), d_exc.view(3, cap * hop)
    R = 70
    assert stream_launch_count(R) == 2 and stream_launch_count(64) == 1 and stream_launch_count(0) == 0
    lens = [(1, 3, 4, 45, 60)[r % 5] for r in range(R)]
    streams = [r % 2 for r in range(R)]
    firsts = []
    for r in range(R):
        lo, hi = pos[streams[r]] - cap, pos[streams[r]] - lens[r]
        firsts.append((lo, hi)[r % 3] if r % 3 < 2 else int(rng.integers(lo, hi + 1)))
    wraps = sum(1 for r in range(R) if firsts[r] % cap + lens[r] > cap)
    assert wraps >= 10 and {f % 4 for f in firsts} == {0, 1, 2, 3}
    want = [np.zeros((R, C, width), np.float32), np.zeros((R, 1, width * hop), np.float32), np.zeros((R, 1, width * hop), np.float32)]
    for r in range(R):
        s, a, n = streams[r], firsts[r], lens[r]
        want[0][r, :, :n] = hist[s][0][a: a + n].T
        want[1][r, 0, :n * hop] = hist[s][1][a: a + n].reshape(-1)
        want[2][r, 0, :n * hop] = hist[s][2][a: a + n].reshape(-1)
    outs = [torch.full(w.shape, float("nan"), dtype=torch.float32, device=dev) for w in want]
    got = stream_assemble(d_ppg, d_lft, d_exc, pos, streams, firsts, lens, width, out=outs)
    for g, o, w in zip(got, outs, want):
        assert g is o and np.array_equal(_bits(g.cpu().numpy()), _bits(w))
    for s, first, n in ((0, 35, 4), (0, 97, 4), (1, 106, 1), (1, 171, 1), (2, 0, 1), (0, -1, 1), (3, 0, 1), (0, 40, 61), (0, 36, 64 + 1)):
        with pytest.raises(ValueError):
            stream_assemble(d_ppg, d_lft, d_exc, pos, [s], [first], [n], width)
    stream_assemble(d_ppg, d_lft, d_exc, pos, [0, 1, 2], [36, 107, 0], [60, 60, 0], width)          # (the edges are fine)


# -------------------------------------------------------------------------------------------------------- sessions
FRAMES = [160, 52, 9]
CORE, FADE = 32, 8
# per stream: the frames of every push; a stream's last push carries its end
SCHEDULE = [[48, 20, 0, 45, 3, 44], [7, 45], [4, 1, 0, 4]]


class _World:
    pass


@pytest.fixture(scope="module")
def world(dev):
    """The recipe generator (weights seed 611), three utterances of 160, 52 and 9 frames (hash generator; the first two
    are tests/test_decode_windowed_gpu.py's), their excitation (noise off: SignalGenerator on the whole f0, which the
    streamed excitation must equal), the float64 oracle of each WHOLE utterance without a speaker, and what a
    speakerless float32 session returns for SCHEDULE - computed once, shared, left unchanged."""
    from oracle import fastsvc_oracle as O
    w = _World()
    cfg = w.cfg = S.FULL_CONFIG
    w.sd = S.synth_state_dict(cfg, 611)
    w.wf = S.fold_weight_norm(w.sd)
    w.batches = [S.synth_batch(cfg, 1, F, 612 + i) for i, F in enumerate(FRAMES)]
    w.feats = [dict(f0=b.f0[0].T.copy(), ppg=b.ppg[0].T.copy(), lft=b.lft[0].T.copy()) for b in w.batches]
    w.emb = w.batches[0].spk_emb[0]
    w.models = {}

    def model(storage):
        if storage not in w.models:
            w.models[storage] = _module(cfg, w.sd, dev, storage)
        return w.models[storage]
    w.model = model
    w.sg = _sg(cfg.hop)
    w.R = Dc.receptive_field_frames(cfg)
    w.exc = [w.sg(torch.from_numpy(b.f0).to(dev)).cpu().numpy().reshape(-1) for b in w.batches]
    w.oracle = [O.forward_dedup(w.wf, cfg.upsampling_scales, b.ppg, e.reshape(1, 1, -1), b.lft, None,
                                dtype=torch.float64).numpy()[0, 0] for b, e in zip(w.batches, w.exc)]
    w.nospk = _play(w, dev, "float32", SCHEDULE, pcm16=False, trace=True)
    return w


def _chunk(feat, a, k, hop):
    return dict(ppg=feat["ppg"][a: a + k], f0=feat["f0"][a: a + k], lft=feat["lft"][a * hop: (a + k) * hop])


def _play(w, dev, storage, schedule, emb=None, trace=False, which=(0, 1, 2), **kw):
    """Run the streams `which` side by side through one session, push i of every stream in one call -> per stream the
    list of pieces, plus the session's counters (and the trace)."""
    hop = w.cfg.hop
    res = _World()
    with Dc.StreamSession(w.model(storage), w.sg, dev, n_streams=len(which), core=CORE, fade=FADE, max_push=48, **kw) as s:
        if trace:
            s._stream_trace = {}
        ids = [s.open(emb) for _ in which]
        res.pieces, res.forwards = [[] for _ in which], []
        at = [0] * len(which)
        for i in range(max(len(schedule[u]) for u in which)):
            chunks, end = {}, []
            for j, u in enumerate(which):
                if i < len(schedule[u]):
                    chunks[ids[j]] = _chunk(w.feats[u], at[j], schedule[u][i], hop)
                    at[j] += schedule[u][i]
                    if i == len(schedule[u]) - 1:
                        end.append(ids[j])
            before = s.forwards
            out = s.push(chunks, end)
            assert sorted(out) == sorted(chunks)
            res.forwards.append(s.forwards - before)
            for j in range(len(which)):
                if ids[j] in out:
                    res.pieces[j].append(out[ids[j]])
        assert [at[j] for j in range(len(which))] == [FRAMES[u] for u in which]
        res.latency = (s.latency_frames, s.latency_frames_max, s.context, s.cap)
        if trace:
            res.exc = [torch.cat(s._stream_trace["excitation"][i]).cpu().numpy() for i in ids]
            res.rows = [(rows, t.cpu().numpy()) for rows, t in s._stream_trace["forwards"]]
    res.y = [np.concatenate(p) for p in res.pieces]
    return res


def _rel(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / max(1.0, float(np.abs(ref).max()))


def _return_frame(t, F, core, context, fade):
    """The frame whose push returns the samples of frame t (StreamSession's latency rule), the end at frame F - 1."""
    k = t // core
    r = (k + 1) * core + context - 1
    if t % core >= core - fade // 2:
        r = (k + 2) * core + context - 1
    return min(r, F - 1)


def _piece_sizes(u, hop):
    """Samples every push of SCHEDULE[u] returns, by the latency rule."""
    back = np.array([_return_frame(t, FRAMES[u], CORE, 36, FADE) for t in range(FRAMES[u])])
    return [int(((back >= h - k) & (back < h)).sum()) * hop for k, h in zip(SCHEDULE[u], np.cumsum(SCHEDULE[u]))]


def test_speakerless_streams_are_the_whole_utterance(dev, world):
    """Three streams of 160, 52 and 9 frames in three slots at once, irregular pushes of at most 48 frames, core 32, the
    default context (36), fade 8, float32 samples: against the float64 oracle of each WHOLE utterance on the traced
    excitation within TIGHT - and that excitation is SignalGenerator's of the whole f0, bit for bit.  Every piece has the
    length the latency rule predicts; a push that completes no window returns empty arrays and runs no forward.  With
    context 16 the same call is NOT within TIGHT (the oracle alone puts a 16-frame context 1.7e-1 of the range away)."""
    w, hop = world, world.cfg.hop
    res = w.nospk
    assert res.latency == (CORE + 36, 2 * CORE + 36, 36, 32 + 72 + 48) and w.R <= 36
    for u, F in enumerate(FRAMES):
        assert np.array_equal(_bits(res.exc[u]), _bits(w.exc[u])), u
        y, ref = res.y[u], w.oracle[u]
        assert y.dtype == np.float32 and y.shape == ref.shape == (F * hop,)
        err = _rel(y, ref)
        print(f"STREAM nospk stream {u}: {err:.3e} x max(1, |ref|max = {np.abs(ref).max():.3g})")
        assert err <= TIGHT, (u, err)
        assert [p.size for p in res.pieces[u]] == _piece_sizes(u, hop), u
    # the rows of every forward are the streams' window plans, in push order
    rows = [r for chunk, _ in res.rows for r in chunk]
    for j in range(3):
        assert [(0,) + r[1:] for r in rows if r[0] == j] == Dc.window_plan([FRAMES[j]], CORE, 36)
    # a push runs one forward exactly when a window of some stream completes in it: pushes 1, 3 and 5
    sizes = [_piece_sizes(u, hop) for u in range(3)]
    assert res.forwards == [int(any(i < len(sz) and sz[i] for sz in sizes)) for i in range(6)] == [0, 1, 0, 1, 0, 1]
    short = _play(w, dev, "float32", SCHEDULE, pcm16=False, context=16)
    errs = [_rel(y, ref) for y, ref in zip(short.y, w.oracle)]
    print("STREAM nospk context 16:", " ".join(f"{e:.3e}" for e in errs))
    assert max(errs) > TIGHT


def test_streams_with_a_speaker_are_every_window_run_alone(dev, world):
    """With an embedding InstanceNorm normalises per window: a stream's samples are stitch_windows of every window row
    run alone (one forward of one row each) on the traced excitation, within the batching invariance; and the default
    PCM-16 result is within one step of to_pcm16 of the float32 one."""
    w = world
    hop = w.cfg.hop
    m = w.model("float32")
    res = _play(w, dev, "float32", SCHEDULE, emb=w.emb, pcm16=False, trace=True)
    emb = torch.from_numpy(w.emb[None]).to(dev)
    for u, F in enumerate(FRAMES):
        rows = Dc.window_plan([F], CORE, 36)
        b, alone = w.batches[u], []
        with torch.no_grad():
            for _, a, e, _, _ in rows:
                ins = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in
                       (b.ppg[:, :, a:e], res.exc[u][a * hop: e * hop].reshape(1, 1, -1), b.lft[:, :, a * hop: e * hop])]
                alone.append(m(*ins, emb).cpu().numpy()[0, 0])
        want = Dc.stitch_windows(alone, rows, hop, FADE)[0]
        err = _rel(res.y[u], want)
        print(f"STREAM spk stream {u}: {err:.3e} to the windows run alone")
        assert err <= BATCHING, (u, err)
    pcm = _play(w, dev, "float32", SCHEDULE, emb=w.emb)
    for p, y in zip(pcm.y, res.y):
        assert p.dtype == np.int16 and p.shape == y.shape
        assert np.abs(p.astype(np.int32) - Dc.to_pcm16(y).astype(np.int32)).max() <= 1


def test_schedules_agree_and_a_reused_slot_is_fresh(dev, world):
    """The 160-frame stream, with a speaker: frame by frame, in pushes of 48, as 33 frames and then 48s, and as 33, 48,
    18, 48, 13 (two windows become ready in one push in mid-stream, and run as neighbours of one forward), and with
    max_batch 2, which splits the windows a push completes over two forwards: the results agree within the batching
    invariance.
    Then, in ONE session with one slot: the 52-frame stream, its end, and the 160-frame stream opened in the same slot
    give what a fresh session gives - no phase, ring contents or fade slots are left over."""
    w, hop = world, world.cfg.hop
    scheds = {"by frame": [1] * 160, "48s": [48, 48, 48, 16], "33 + 48s": [33, 48, 48, 31], "two at once": [33, 48, 18, 48, 13]}
    ys = {}
    for name, sc in scheds.items():
        res = _play(w, dev, "float32", [sc, [], []], emb=w.emb, pcm16=False, which=(0,))
        ys[name] = res.y[0]
        assert sum(res.forwards) <= 5 and res.y[0].shape == (160 * hop,)
        if name == "33 + 48s":
            assert res.forwards == [0, 1, 1, 1]          # (81 frames: window 0; 129: window 1; the end: windows 2, 3 and 4)
        if name == "two at once":
            assert res.forwards == [0, 1, 0, 1, 1]       # (81: window 0; 147: windows 1 and 2 in one forward; the end: 3 and 4)
    # the same pushes with forwards of at most 2 rows: the end's three windows are split 2 + 1, and the first of those
    # forwards reads one fade slot of the stream and stages into the other
    res = _play(w, dev, "float32", [scheds["33 + 48s"], [], []], emb=w.emb, pcm16=False, which=(0,), max_batch=2)
    assert res.forwards == [0, 1, 1, 2]
    ys["forwards of 2 rows"] = res.y[0]
    for name in ("48s", "33 + 48s", "two at once", "forwards of 2 rows"):
        err = _rel(ys[name], ys["by frame"].astype(np.float64))
        print(f"STREAM schedule {name} against frame by frame: {err:.3e}")
        assert err <= BATCHING, (name, err)
    with Dc.StreamSession(w.model("float32"), w.sg, dev, n_streams=1, core=CORE, fade=FADE, max_push=48, pcm16=False) as s:
        a = s.open(w.emb)
        with pytest.raises(ValueError):
            s.open(w.emb)                                # (all slots busy)
        s.push({a: _chunk(w.feats[1], 0, 45, hop)})
        s.push({a: _chunk(w.feats[1], 45, 7, hop)}, end=[a])
        b = s.open(w.emb)
        assert b != a and s._ids[b] == 0
        out, at = [], 0
        for k in scheds["48s"]:
            out.append(s.push({b: _chunk(w.feats[0], at, k, hop)}, end=[b] if at + k == 160 else ())[b])
            at += k
    err = _rel(np.concatenate(out), ys["48s"].astype(np.float64))
    print(f"STREAM reused slot against a fresh session: {err:.3e}")
    assert err <= BATCHING, err


def test_bfloat16_storage_against_the_oracle(dev, world):
    """The speakerless case in bfloat16 storage against the whole-utterance oracle: tests/test_config_matrix_gpu.py's
    bfloat16 bounds, as in the windowed test."""
    w = world
    res = _play(w, dev, "bfloat16", SCHEDULE, pcm16=False)
    for u, (y, ref) in enumerate(zip(res.y, w.oracle)):
        err = np.abs(y.astype(np.float64) - ref)
        rms, mag = float(np.sqrt(np.mean(ref ** 2))), max(1.0, float(np.abs(ref).max()))
        print(f"STREAM bfloat16 stream {u}: mean/rms {err.mean() / rms:.3e} max/mag {err.max() / mag:.3e}")
        assert np.isfinite(y).all()
        assert float(err.mean()) <= BF16_MEAN * rms, (u, float(err.mean()), rms)
        assert float(err.max()) <= BF16_MAX * mag, (u, float(err.max()), mag)


def test_refusals_leave_the_session_usable(dev, world):
    """Every ValueError of open and push - two of them before each valid push of the 160-frame stream - and the valid
    pushes still return what an undisturbed session returns for the same pushes, bit for bit (the same rows in the same
    batches; the forward is bit-reproducible)."""
    w, hop = world, world.cfg.hop
    feat = w.feats[0]
    sc = [48, 20, 0, 45, 3, 44]
    want = _play(w, dev, "float32", [sc, [], []], pcm16=False, which=(0,)).pieces[0]
    good = _chunk(feat, 0, 4, hop)
    with Dc.StreamSession(w.model("float32"), w.sg, dev, n_streams=3, core=CORE, fade=FADE, max_push=48, pcm16=False) as s:
        gone = s.open()
        assert s.end([gone])[gone].size == 0             # (a stream that ends without a frame)
        s.open(), s.open()                               # (two streams that stay open and idle: ours is in slot 2)
        a = s.open()
        assert s._ids[a] == 2
        with pytest.raises(ValueError):
            s.open()                                     # all slots busy
        bad = [
            ({a: dict(good, ppg=good["ppg"][:, :-1])}, ()),                              # wrong channel count
            ({a: dict(good, ppg=good["ppg"].reshape(-1))}, ()),                          # ppg not 2-D
            ({a: dict(good, f0=good["f0"][:3])}, ()),                                    # f0 of another length
            ({a: dict(good, lft=good["lft"][:-1])}, ()),                                 # lft is not n * hop
            ({a: _chunk(feat, 0, 49, hop)}, ()),                                         # n > max_push
            ({a: good, 99: good}, ()),                                                   # an unknown id
            ({a: good, gone: good}, ()),                                                 # an ended id
            ({a: good}, (gone,)),                                                        # an ended id in end
            ({a: dict(ppg=good["ppg"], f0=good["f0"])}, ()),                             # a chunk without lft
        ]
        at, forwards = 0, s.forwards
        for i, k in enumerate(sc):
            for chunks, end in (bad[i % len(bad)], bad[(i + 6) % len(bad)]):
                with pytest.raises(ValueError):
                    s.push(chunks, end)
            assert s.forwards == forwards
            got = s.push({a: _chunk(feat, at, k, hop)}, end=[a] if i == len(sc) - 1 else ())[a]
            at += k
            forwards = s.forwards
            assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want[i])), i
        with pytest.raises(ValueError):
            s.push({a: good})                            # it has ended
    with pytest.raises(ValueError):
        Dc.StreamSession(w.model("float32"), w.sg, dev, core=30)
    with pytest.raises(ValueError):
        Dc.StreamSession(w.model("float32"), w.sg, dev, core=32, context=0, fade=8)
    with pytest.raises(ValueError):
        Dc.StreamSession(w.model("float32"), w.sg, dev, max_push=2000)
    with Dc.StreamSession(w.model("float32"), w.sg, dev, n_streams=2) as s:
        s.open(w.emb)
        with pytest.raises(ValueError):
            s.open()                                     # every open stream has an embedding, or none does
        with pytest.raises(ValueError):
            s.open(w.emb[:-1])
        with pytest.raises(ValueError):
            s.open(w.emb, src_f0_stats=[5.0, 1.0])
        assert s.max_push == 32 and s.latency_frames == 68
