"""GPU tests (-m gpu) of running InstanceNorm statistics for live streams: the running-sums kernels
(csrc/fastsvc_normgroup.hip) against math.fsum with the carry, its two parity entries and the pass-through rule bit for
bit; and StreamSession(norm="running") against the float64 running reference (tests/running_norm_ref.py) in the three
storages, across schedules that cut a stream's windows into forwards differently, slot reuse, refused pushes, and the cases
in which it must be norm="window" byte for byte."""
import math

import numpy as np
import pytest
import torch

import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd import synth as S
# the suite's constants and the stream tests' world: sessions of FRAMES = 160, 52 and 9 frames under SCHEDULE
from test_decode_stream_gpu import BF16_MAX, BF16_MEAN, CORE, FADE, FRAMES, SCHEDULE, TIGHT, _bits, _chunk, _module, _play, _sg, _World
from test_decode_window_norm_gpu import F16_DIV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    A.load_library()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------ the kernels
# One batch of 14 rows in 9 of 11 carry slots (3 and 8 stay untouched).  Per row: slot, frames, core [lo, hi), prior, reset.
ROWS = [
    (0, 112, 7, 39, 71, 0),       # alone in its slot: odd own_lo, a look-ahead of 73 frames, a carry
    (1, 45, 13, 45, 50, 0),       # two rows: odd own_lo and an EMPTY look-ahead ...
    (1, 112, 33, 34, 82, 0),      # ... then a one-frame core
    (2, 112, 0, 32, 0, 1),        # three rows: window 0 of a stream (pass-through; the carry is NaN and must not be read) ...
    (2, 112, 4, 36, 32, 0),       # ... its window 1 in the same batch, which starts from zero too ...
    (2, 45, 1, 45, 64, 0),        # ... and a third
    (4, 45, 3, 20, 3, 1),         # reset with own_lo > 0: not a pass-through row
    (5, 1, 0, 1, 7, 0),           # a one-frame row: N / L = 8
    (6, 3, 1, 2, 4, 0),           # the middle frame of three, one frame of look-ahead
    (7, 4, 1, 4, 1, 1),           # reset, three of four frames
    (9, 4, 0, 4, 0, 1),           # pass-through without a look-ahead
    (10, 112, 111, 112, 500, 0),  # three rows: the last frame of a long row ...
    (10, 3, 0, 3, 501, 0),        # ... a whole short row that is NOT reset ...
    (10, 112, 1, 112, 504, 0),    # ... and nearly a whole long one
]
N_SLOTS = 11
PARITY = [0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0]       # per slot
PATTERN = -1234.5


def _arrays(rows):
    return ([r[0] for r in rows], [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows], [r[5] for r in rows],
            [PARITY[r[0]] for r in rows])


def _fresh_slots(rows):
    """Slots whose first row of `rows` starts a stream."""
    first = {}
    for r in rows:
        first.setdefault(r[0], r[5])
    return {s for s, reset in first.items() if reset}


def _carry_in(C, dev, rows):
    """(N_SLOTS, 2, C, 2): the current entry of every slot random (NaN where a stream starts), the other one PATTERN."""
    gen = torch.Generator(device="cpu").manual_seed(7 * C)
    cur = torch.randn((N_SLOTS, C, 2), generator=gen, dtype=torch.float64) * torch.tensor([50.0, 400.0], dtype=torch.float64)
    cur[..., 1] = cur[..., 1].abs()
    for s in _fresh_slots(rows):
        cur[s] = float("nan")
    carry = torch.full((N_SLOTS, 2, C, 2), PATTERN, dtype=torch.float64)
    for s in range(N_SLOTS):
        carry[s, PARITY[s]] = cur[s]
    return carry.to(dev)


@pytest.mark.parametrize("storage", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("C,len_mul", [(24, 2), (24, 160), (192, 2), (192, 160)])
def test_running_stats_against_fsum(dev, storage, C, len_mul):
    """fastsvc_norm_running_stats on the stored values against math.fsum.  Per entry |got - want| <= n 2^-53 sum |terms|
    scale, test_group_stats_against_numpy_float64's bound, with n counting the carry as a term: the forward bound of a
    float64 sum of n terms in any order (the smallest case here, the one-frame row at two columns a frame, has n = 3 and
    scales by 1/8 exactly).  Every column in front of own_lo and beyond the row's length is NaN, as is the carry of the
    slots in which a stream starts: one read shows.  The new carry lands in entry parity ^ 1 within the same bound, entry
    parity keeps its bits, untouched slots keep both, pass-through rows keep the pattern in their statistics, two calls
    give identical bits - and the batch cut in two calls chained through the carry gives the bits of the one call."""
    from svcc23_fastsvc_amd.engine import norm_running_stats
    dtype = dict(float32=torch.float32, bfloat16=torch.bfloat16, float16=torch.float16)[storage]
    B, ld = len(ROWS), 112 * len_mul
    lens = [r[1] for r in ROWS]
    gen = torch.Generator(device=dev).manual_seed(1000 * C + len_mul)
    u = (torch.randn((B, C, ld), generator=gen, device=dev) * 2.0 + 0.75).to(dtype)
    live = torch.zeros((B, ld), dtype=torch.bool)
    for b, (_, n, lo, _, _, _) in enumerate(ROWS):
        live[b, lo * len_mul: n * len_mul] = True
    u.masked_fill_(~live.to(dev)[:, None, :], float("nan"))
    carry0 = _carry_in(C, dev, ROWS)
    outs = []
    for _ in range(2):
        st = torch.full((B, C, 2), PATTERN, dtype=torch.float64, device=dev)
        carry = carry0.clone()
        norm_running_stats(u, lens, len_mul, _arrays(ROWS), carry, st)
        outs.append((st.cpu().numpy(), carry.cpu().numpy()))
    got, carry = outs[0]
    assert np.array_equal(got.view(np.uint64), outs[1][0].view(np.uint64))
    assert np.array_equal(carry.view(np.uint64), outs[1][1].view(np.uint64))
    c0 = carry0.cpu().numpy()
    used = sorted({r[0] for r in ROWS})
    for s in range(N_SLOTS):
        assert np.array_equal(carry[s, PARITY[s]].view(np.uint64), c0[s, PARITY[s]].view(np.uint64)), s      # never written
        if s not in used:
            assert (carry[s, PARITY[s] ^ 1] == PATTERN).all(), s
    passthrough = [b for b, r in enumerate(ROWS) if r[5] and r[2] == 0]
    assert passthrough == [3, 10] and (got[passthrough] == PATTERN).all()
    # the exact sums; at 160 columns a frame on a subset of the channels (the channel only moves the row's base address)
    chans = list(range(C)) if len_mul == 2 else sorted(set(range(0, C, 8)) | {1, C - 1})
    eps = 2.0 ** -53
    x = u[:, chans].to(torch.float64).cpu().numpy()                                     # (2-byte elements convert exactly)
    fresh = _fresh_slots(ROWS)
    worst = 0.0

    def check(value, terms, L, N, what):
        nonlocal worst
        assert np.isfinite(terms).all(), what
        want = math.fsum(terms) * float(L) / float(N)
        bound = len(terms) * eps * float(np.abs(terms).sum()) * (float(L) / float(N))
        err = abs(value - want)
        worst = max(worst, err / bound)
        assert err <= bound, (what, value, want, bound)

    for k, c in enumerate(chans):
        cores = {s: [] for s in used}            # per slot: the carry and the cores so far, as terms of sum u / sum u^2
        for s in used:
            cores[s] = [[], []] if s in fresh else [[c0[s, PARITY[s], c, 0]], [c0[s, PARITY[s], c, 1]]]
        for b, (s, n, lo, hi, prior, reset) in enumerate(ROWS):
            core, look = x[b, k, lo * len_mul: hi * len_mul], x[b, k, hi * len_mul: n * len_mul]
            cores[s][0].extend(core)
            cores[s][1].extend(core * core)
            if b in passthrough:
                continue
            L, N = n * len_mul, (prior + n - lo) * len_mul
            for j, extra in enumerate((look, look * look)):
                check(got[b, c, j], np.array(cores[s][j] + list(extra)), L, N, (b, c, j))
        for s in used:
            for j in range(2):
                check(carry[s, PARITY[s] ^ 1, c, j], np.array(cores[s][j]), 1, 1, ("carry", s, c, j))
    print(f"NORMRUNNING stats {storage} C {C} len_mul {len_mul}: worst error {worst:.3f} of the bound")
    # the same windows in two calls: every slot's first row, then the rest with those slots' parity flipped
    first_rows = [b for b, r in enumerate(ROWS) if b == 0 or ROWS[b - 1][0] != r[0]]
    rest = [b for b in range(B) if b not in first_rows]
    st = torch.full((B, C, 2), PATTERN, dtype=torch.float64, device=dev)
    chained = carry0.clone()
    for part, flip in ((first_rows, False), (rest, True)):
        rows = [ROWS[b] for b in part]
        arrays = list(_arrays(rows))
        if flip:
            arrays[4] = [0] * len(rows)                          # (nobody starts a stream in the second call)
            arrays[5] = [p ^ 1 for p in arrays[5]]
        sub = torch.full((len(part), C, 2), PATTERN, dtype=torch.float64, device=dev)
        norm_running_stats(u[part].contiguous(), [lens[b] for b in part], len_mul, tuple(arrays), chained, sub)
        st[part] = sub
    assert np.array_equal(st.cpu().numpy().view(np.uint64), got.view(np.uint64))
    chained = chained.cpu().numpy()
    for s in used:                                               # (slots with one row end in the other entry, the rest came back)
        twice = any(ROWS[b][0] == s for b in rest)
        assert np.array_equal(chained[s, PARITY[s] ^ (0 if twice else 1)].view(np.uint64),
                              carry[s, PARITY[s] ^ 1].view(np.uint64)), s


def test_running_stats_rejects_bad_arguments(dev):
    from svcc23_fastsvc_amd.engine import norm_running_stats
    u = torch.zeros((2, 3, 8), device=dev)
    st = torch.zeros((2, 3, 2), dtype=torch.float64, device=dev)
    carry = torch.zeros((2, 2, 3, 2), dtype=torch.float64, device=dev)
    ok = ([0, 1], [0, 1], [2, 4], [0, 5], [1, 0], [0, 1])
    norm_running_stats(u, [4, 4], 2, ok, carry, st)
    for i, row in ((0, [0, 2]), (0, [1, 0]), (2, [2, 5]), (3, [0, 0]), (5, [0, 2])):
        with pytest.raises(ValueError):
            norm_running_stats(u, [4, 4], 2, ok[:i] + (row,) + ok[i + 1:], carry, st)
    with pytest.raises(ValueError):
        norm_running_stats(u, [4, 4], 3, ok, carry, st)             # the pitch is no multiple of len_mul
    with pytest.raises(ValueError):
        norm_running_stats(u, [4, 4], 2, ok, carry[:, :1], st)      # one entry a slot
    with pytest.raises(ValueError):
        norm_running_stats(u, [4, 4], 2, ok, carry.to(torch.float32), st)


# ------------------------------------------------------------------------------------------------------ the streams
# three streams side by side, forwards of at most two rows: push 1 completes window 0 of stream 0 and BOTH windows of
# stream 1, whose flush is cut across two forwards; push 3 runs windows 1 and 2 of stream 0 in one forward
SCHEDULE2 = [[33, 48, 18, 48, 13], [48, 4], [9]]


@pytest.fixture(scope="module")
def world(dev):
    """tests/test_decode_stream_gpu.py's world - the recipe generator (weights seed 611), streams of 160, 52 and 9 frames
    (batch seeds 612..614), noise off - with the embedding; what a float32 norm="running" session returns for SCHEDULE; and
    the float64 running reference of each stream on the excitation that session traced.  Computed once, shared, left
    unchanged."""
    from running_norm_ref import stream_reference
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
    assert Dc.receptive_field_frames(cfg) <= 36
    w.run = _play(w, dev, "float32", SCHEDULE, emb=w.emb, pcm16=False, trace=True, norm="running")
    w.ref = [stream_reference(w.wf, cfg.upsampling_scales, b.ppg, e.reshape(1, 1, -1), b.lft, w.emb, CORE, 36, FADE)[0]
             for b, e in zip(w.batches, w.run.exc)]
    return w


def _rel(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / max(1.0, float(np.abs(ref).max()))


def test_running_streams_are_the_running_reference(dev, world):
    """Streams of 160, 52 and 9 frames with an embedding under SCHEDULE, float32 storage: within TIGHT of the float64
    running reference on the traced excitation - which norm="window" is not, for the stream that has late windows."""
    w = world
    for u, (y, ref) in enumerate(zip(w.run.y, w.ref)):
        assert y.dtype == np.float32 and y.shape == ref.shape == (FRAMES[u] * w.cfg.hop,)
        err = _rel(y, ref)
        print(f"STREAM-NORM running stream {u}: {err:.3e} x max(1, |ref|max = {np.abs(ref).max():.3g})")
        assert err <= TIGHT, (u, err)
    per_window = _play(w, dev, "float32", SCHEDULE, emb=w.emb, pcm16=False)
    err = _rel(per_window.y[0], w.ref[0])
    print(f"STREAM-NORM window stream 0 against the running reference: {err:.3e}")
    assert err > TIGHT


@pytest.mark.parametrize("storage", ["bfloat16", "float16"])
def test_two_byte_storages_against_the_running_reference(dev, world, storage):
    """The same streams in bfloat16 and float16 storage: tests/test_config_matrix_gpu.py's bfloat16 bounds, an eighth of
    them in float16."""
    w = world
    div = F16_DIV if storage == "float16" else 1.0
    res = _play(w, dev, storage, SCHEDULE, emb=w.emb, pcm16=False, norm="running")
    for u, (y, ref) in enumerate(zip(res.y, w.ref)):
        err = np.abs(y.astype(np.float64) - ref)
        rms, mag = float(np.sqrt(np.mean(ref ** 2))), max(1.0, float(np.abs(ref).max()))
        print(f"STREAM-NORM {storage} stream {u}: mean/rms {err.mean() / rms:.3e} max/mag {err.max() / mag:.3e}")
        assert np.isfinite(y).all()
        assert float(err.mean()) <= BF16_MEAN / div * rms, (u, float(err.mean()), rms)
        assert float(err.max()) <= BF16_MAX / div * mag, (u, float(err.max()), mag)


def test_another_schedule_gives_the_same_streams(dev, world):
    """SCHEDULE2 with max_push 48 > core and forwards of at most two rows: two windows of a stream share a forward, a
    stream's flush is cut across forwards (its window 0 resets the carry in one, its window 1 reads it in the next).
    Within 2 TIGHT of SCHEDULE's result: both are within TIGHT of one reference."""
    w = world
    res = _play(w, dev, "float32", SCHEDULE2, emb=w.emb, pcm16=False, trace=True, norm="running", max_batch=2)
    assert res.forwards == [1, 2, 0, 1, 1]
    assert [[(r[0], r[3] // CORE) for r in chunk] for chunk, _ in res.rows] == \
        [[(2, 0)], [(0, 0), (1, 0)], [(1, 1)], [(0, 1), (0, 2)], [(0, 3), (0, 4)]]                   # (stream, window)
    for u, (y, first, ref) in enumerate(zip(res.y, w.run.y, w.ref)):
        err = float(np.abs(y.astype(np.float64) - first).max()) / max(1.0, float(np.abs(ref).max()))
        print(f"STREAM-NORM schedule 2 stream {u}: {err:.3e} to the first schedule, {_rel(y, ref):.3e} to the reference")
        assert err <= 2 * TIGHT, (u, err)


def test_a_stream_of_one_window_is_the_window_mode_bit_for_bit(dev, world):
    """The 9-frame stream ends inside window 0, a pass-through row: norm="window"'s bytes, float32 and PCM-16."""
    w = world
    for pcm16 in (False, True):
        a = _play(w, dev, "float32", SCHEDULE, emb=w.emb, pcm16=pcm16, which=(2,), norm="running")
        b = _play(w, dev, "float32", SCHEDULE, emb=w.emb, pcm16=pcm16, which=(2,))
        assert a.y[0].dtype == b.y[0].dtype and a.y[0].size == 9 * w.cfg.hop
        assert np.array_equal(_bits(a.y[0]), _bits(b.y[0])), pcm16


def test_a_reused_slot_is_fresh(dev, world):
    """One session with one slot: the 52-frame stream, its end, then the 160-frame stream in the same slot gives, bit for
    bit, what that stream gives in a new session - the first stream's carry is not read."""
    w, hop = world, world.cfg.hop
    sc = [48, 48, 48, 16]
    want = _play(w, dev, "float32", [sc, [], []], emb=w.emb, pcm16=False, which=(0,), norm="running").y[0]
    with Dc.StreamSession(w.model("float32"), w.sg, dev, n_streams=1, core=CORE, fade=FADE, max_push=48, pcm16=False,
                          norm="running") as s:
        a = s.open(w.emb)
        s.push({a: _chunk(w.feats[1], 0, 45, hop)})
        s.push({a: _chunk(w.feats[1], 45, 7, hop)}, end=[a])
        b = s.open(w.emb)
        assert b != a and s._ids[b] == 0
        out, at = [], 0
        for k in sc:
            out.append(s.push({b: _chunk(w.feats[0], at, k, hop)}, end=[b] if at + k == 160 else ())[b])
            at += k
    assert np.array_equal(_bits(np.concatenate(out)), _bits(want))


def test_without_an_embedding_nothing_is_carried(dev, world):
    """norm="running" with open(trg_emb=None): norm="window"'s bits (which are the speakerless whole-utterance result)."""
    w = world
    a = _play(w, dev, "float32", SCHEDULE, pcm16=False, norm="running")
    b = _play(w, dev, "float32", SCHEDULE, pcm16=False)
    for u in range(3):
        assert np.array_equal(_bits(a.y[u]), _bits(b.y[u])), u


def test_a_refused_push_leaves_carry_and_parity_alone(dev, world):
    """Two refused pushes before every valid one of the 160-frame stream: the carry keeps its bits and the slot its parity
    across each refusal, and the stream still is the running reference within TIGHT."""
    w, hop = world, world.cfg.hop
    feat = w.feats[0]
    good = _chunk(feat, 0, 4, hop)
    with Dc.StreamSession(w.model("float32"), w.sg, dev, n_streams=2, core=CORE, fade=FADE, max_push=48, pcm16=False,
                          norm="running") as s:
        s.open(w.emb)                                    # (an idle stream in slot 0: ours is in slot 1)
        a = s.open(w.emb)
        bad = [({a: dict(good, ppg=good["ppg"][:, :-1])}, ()), ({a: _chunk(feat, 0, 49, hop)}, ()), ({a: good, 99: good}, ()),
               ({a: dict(good, lft=good["lft"][:-1])}, ()), ({a: good}, (99,))]
        out, at = [], 0
        for i, k in enumerate(SCHEDULE[0]):
            carry = s._carry.clone().view(torch.int64)
            parity = [st.norm_parity for st in s._slots]
            for chunks, end in (bad[i % len(bad)], bad[(i + 2) % len(bad)]):
                with pytest.raises(ValueError):
                    s.push(chunks, end)
            assert torch.equal(s._carry.view(torch.int64), carry) and [st.norm_parity for st in s._slots] == parity
            out.append(s.push({a: _chunk(feat, at, k, hop)}, end=[a] if i == len(SCHEDULE[0]) - 1 else ())[a])
            at += k
        assert parity[0] == 0                            # (the idle stream never ran)
    err = _rel(np.concatenate(out), w.ref[0])
    print(f"STREAM-NORM after refused pushes: {err:.3e}")
    assert err <= TIGHT, err


def test_running_needs_a_model_that_takes_an_embedding(dev, world):
    w, cfg = world, world.cfg
    g = A.FastSVCGenerator(in_channels=cfg.in_channels, mid_channels=list(cfg.mid_channels),
                           upsampling_scales=list(cfg.upsampling_scales), out_channels=cfg.out_channels,
                           spk_emb_size=cfg.spk_emb_size, use_spk_emb=False).eval().to(dev)
    with pytest.raises(ValueError, match="takes a speaker embedding"):
        Dc.StreamSession(g, w.sg, dev, norm="running")
    with Dc.StreamSession(g, w.sg, dev, norm="window") as s:
        assert s.norm == "window" and s._carry is None
    with pytest.raises(ValueError, match="norm must be"):
        Dc.StreamSession(w.model("float32"), w.sg, dev, norm="utterance")
    m = w.model("float32")
    b = S.synth_batch(cfg, 2, 8, 620)
    ins = [torch.from_numpy(v).to(dev) for v in (b.ppg, b.sine, b.lft, b.spk_emb)]
    running = ([0, 1], [0, 0], [8, 8], [0, 0], [1, 1], [0, 0])
    carry = torch.empty((2, m.plan.norm_carry_bytes() // 8), dtype=torch.float64, device=dev)
    with torch.no_grad():
        with pytest.raises(ValueError, match="exclude each other"):
            m(*ins, norm_running=running, norm_carry=carry, norm_groups=([0, 1], [0, 0], [8, 8]))
        with pytest.raises(ValueError, match="norm_carry"):
            m(*ins, norm_running=running)
        with pytest.raises(ValueError, match="slot"):
            m(*ins, norm_running=([0, 2],) + running[1:], norm_carry=carry)
        # every row a window 0: the plain forward's bits, and the carry holds the rows' own sums
        want = m(*ins).cpu().numpy()
        got = m(*ins, norm_running=running, norm_carry=carry).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    assert np.isfinite(carry.view(2, 2, -1)[:, 1].cpu().numpy()).all()
