"""GPU tests (-m gpu) of the forgetting horizon of running InstanceNorm statistics: the decayed pool
(csrc/fastsvc_normgroup.hip, fastsvc_norm_running_stats_decay) against exact weighted sums with the carry, its two parity
entries and the pass-through rule bit for bit; StreamSession(norm="running", horizon=H) against the float64 reference with
the same horizon (tests/running_horizon_ref.py) in the three storages, across schedules, slot reuse and refused pushes; the
staging-scale raise after a change of level at the shortest horizon; and horizon=None, which must be the mode without one
byte for byte."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd import synth as S
# the suite's constants and the stream tests' world: sessions of FRAMES = 160, 52 and 9 frames under SCHEDULE
from test_decode_stream_gpu import BF16_MAX, BF16_MEAN, CORE, FADE, FRAMES, SCHEDULE, TIGHT, _bits, _chunk, _module, _play, _sg, _World
from test_decode_stream_norm_gpu import N_SLOTS, PARITY, PATTERN, ROWS, SCHEDULE2, _arrays, _carry_in, _fresh_slots
from test_decode_window_norm_gpu import F16_DIV

pytestmark = pytest.mark.gpu

HORIZON = 64.0
CONTEXT = 36


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    A.load_library()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------ the kernels
# per row of ROWS (14 rows in 9 of 11 slots): what the slot's sum is multiplied by in front of the row's core - 1, two
# exact fractions and the decay of a core of 32 frames at horizon 64 - and the frames it is normalised over, which only
# have to be at least the row's own (len - own_lo): prior + len - own_lo, today's count, stretched or shrunk a little
DECAYS = [math.exp(-32 / 64), 0.5, 0.75, 1.0, math.exp(-32 / 64), 0.75, 0.5, 0.75, 1.0, math.exp(-32 / 64), 0.5,
          0.75, math.exp(-32 / 64), 0.5]
WEIGHTS = [float(r[4] + r[1] - r[2]) * f for r, f in zip(ROWS, [1.0, 0.8125, 1.0, 1.0, 0.931, 1.37, 1.0, 0.6, 1.25, 1.0,
                                                               1.0, 0.3, 2.0, 0.77])]


def _exact_sum(terms):
    """The exact sum of floats as a Fraction: math.fsum rounds the exact sum once, and its own residual is a float."""
    terms = np.asarray(terms, dtype=np.float64).tolist()
    hi = math.fsum(terms)
    return Fraction(hi) + Fraction(math.fsum(terms + [-hi]))


@pytest.mark.parametrize("storage", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("C,len_mul", [(24, 2), (192, 160)])
def test_decayed_stats_against_exact_weighted_sums(dev, storage, C, len_mul):
    """fastsvc_norm_running_stats_decay on the stored values.  A term - an element, its square, or the carry - that enters
    the fold in front of the cores of the rows q1 < q2 < .. <= b has the weight decay[q1] decay[q2] .. (as real numbers);
    the wanted sum is taken exactly (math.fsum per range, with its residual, weighted in rational arithmetic).  Per entry
    |got - want| <= (n + d) 2^-53 sum |w_i t_i| L / N with n terms and d multiplications in the row's fold: the forward
    bound of a float64 sum of n terms in any order (tests/test_decode_stream_norm_gpu.py), plus one rounding per multiply,
    each of which touches only what has been summed so far.  Every column in front of own_lo and beyond the row's length is
    NaN, as is the carry of the slots in which a stream starts.  The new carry lands in entry parity ^ 1 within the same
    bound, entry parity keeps its bits, untouched slots keep both, pass-through rows keep the pattern, two calls give
    identical bits, the batch cut in two calls chained through the carry gives the bits of the one call - and with every
    decay 1 and today's integer weights the bits are fastsvc_norm_running_stats'."""
    from svcc23_fastsvc_amd.engine import norm_running_stats
    dtype = dict(float32=torch.float32, bfloat16=torch.bfloat16, float16=torch.float16)[storage]
    B, ld = len(ROWS), 112 * len_mul
    assert len(DECAYS) == len(WEIGHTS) == B and all(w >= r[1] - r[2] for w, r in zip(WEIGHTS, ROWS))
    lens = [r[1] for r in ROWS]
    gen = torch.Generator(device=dev).manual_seed(1000 * C + len_mul + 1)
    u = (torch.randn((B, C, ld), generator=gen, device=dev) * 2.0 + 0.75).to(dtype)
    live = torch.zeros((B, ld), dtype=torch.bool)
    for b, (_, n, lo, _, _, _) in enumerate(ROWS):
        live[b, lo * len_mul: n * len_mul] = True
    u.masked_fill_(~live.to(dev)[:, None, :], float("nan"))
    carry0 = _carry_in(C, dev, ROWS)
    forget = (DECAYS, WEIGHTS, [w * 1.5 for w in WEIGHTS])
    outs = []
    for _ in range(2):
        st = torch.full((B, C, 2), PATTERN, dtype=torch.float64, device=dev)
        carry = carry0.clone()
        norm_running_stats(u, lens, len_mul, _arrays(ROWS), carry, st, decay=forget)
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
    chans = list(range(C)) if len_mul == 2 else sorted(set(range(0, C, 16)) | {1, C - 1})
    eps = 2.0 ** -53
    x = u[:, chans].to(torch.float64).cpu().numpy()                                     # (2-byte elements convert exactly)
    fresh = _fresh_slots(ROWS)
    worst = 0.0

    def check(value, ranges, scale, d, what):
        """ranges: [(weight as a Fraction, the terms)] -> value against sum w t * scale, scale = L / N as a Fraction."""
        nonlocal worst
        assert all(np.isfinite(t).all() for _, t in ranges), what
        want = sum((w * _exact_sum(t) for w, t in ranges), Fraction(0)) * scale
        n = sum(len(t) for _, t in ranges)
        bound = (n + d) * eps * sum(float(w) * float(np.abs(t).sum()) for w, t in ranges) * float(scale)
        err = float(abs(Fraction(float(value)) - want))
        worst = max(worst, err / bound)
        assert err <= bound, (what, value, float(want), bound)

    for k, c in enumerate(chans):
        for j in range(2):                       # sum u, sum u^2
            # per slot: the ranges so far with their weights - the carry first - and the multiplications so far
            folds = {s: ([] if s in fresh else [[Fraction(1), np.array([c0[s, PARITY[s], c, j]])]]) for s in used}
            mults = {s: 0 for s in used}
            for b, (s, n, lo, hi, prior, reset) in enumerate(ROWS):
                core, look = x[b, k, lo * len_mul: hi * len_mul], x[b, k, hi * len_mul: n * len_mul]
                for r in folds[s]:
                    r[0] *= Fraction(DECAYS[b])
                mults[s] += 1
                folds[s].append([Fraction(1), core * core if j else core])
                if b in passthrough:
                    continue
                scale = Fraction(n * len_mul) / Fraction(WEIGHTS[b] * float(len_mul))       # (N is the rounded double)
                check(got[b, c, j], folds[s] + [[Fraction(1), look * look if j else look]], scale, mults[s], (b, c, j))
            for s in used:
                check(carry[s, PARITY[s] ^ 1, c, j], folds[s], Fraction(1), mults[s], ("carry", s, c, j))
    print(f"NORMHORIZON stats {storage} C {C} len_mul {len_mul}: worst error {worst:.3f} of the bound")
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
        norm_running_stats(u[part].contiguous(), [lens[b] for b in part], len_mul, tuple(arrays), chained, sub,
                           decay=tuple([a[b] for b in part] for a in forget))
        st[part] = sub
    assert np.array_equal(st.cpu().numpy().view(np.uint64), got.view(np.uint64))
    chained = chained.cpu().numpy()
    for s in used:                                               # (slots with one row end in the other entry, the rest came back)
        twice = any(ROWS[b][0] == s for b in rest)
        assert np.array_equal(chained[s, PARITY[s] ^ (0 if twice else 1)].view(np.uint64),
                              carry[s, PARITY[s] ^ 1].view(np.uint64)), s
    # nothing forgotten: the kernel without a horizon, bit for bit
    plain_w = [float(r[4] + r[1] - r[2]) for r in ROWS]
    res = []
    for decay in (None, ([1.0] * B, plain_w, plain_w)):
        st = torch.full((B, C, 2), PATTERN, dtype=torch.float64, device=dev)
        carry = carry0.clone()
        norm_running_stats(u, lens, len_mul, _arrays(ROWS), carry, st, decay=decay)
        res.append((st.cpu().numpy(), carry.cpu().numpy()))
    assert np.array_equal(res[0][0].view(np.uint64), res[1][0].view(np.uint64))
    assert np.array_equal(res[0][1].view(np.uint64), res[1][1].view(np.uint64))
    assert not np.array_equal(res[0][0].view(np.uint64), got.view(np.uint64))


def test_decayed_stats_reject_bad_arguments(dev):
    from svcc23_fastsvc_amd.engine import norm_running_stats
    u = torch.zeros((2, 3, 8), device=dev)
    st = torch.zeros((2, 3, 2), dtype=torch.float64, device=dev)
    carry = torch.zeros((2, 2, 3, 2), dtype=torch.float64, device=dev)
    rows = ([0, 1], [0, 1], [2, 4], [0, 5], [1, 0], [0, 1])
    ok = ([1.0, 0.5], [4.0, 3.0], [4.0, 6.0])
    norm_running_stats(u, [4, 4], 2, rows, carry, st, decay=ok)
    for i, row in ((0, [1.0, 0.0]), (0, [1.5, 0.5]), (1, [3.9, 3.0]), (1, [4.0, float("nan")]), (2, [3.0, 6.0]), (2, [4.0])):
        with pytest.raises(ValueError):
            norm_running_stats(u, [4, 4], 2, rows, carry, st, decay=ok[:i] + (row,) + ok[i + 1:])
    with pytest.raises(ValueError):
        norm_running_stats(u, [4, 4], 2, rows, carry, st, decay=ok[:2])


# ------------------------------------------------------------------------------------------------------ the streams
@pytest.fixture(scope="module")
def world(dev):
    """tests/test_decode_stream_norm_gpu.py's world - the recipe generator (weights seed 611), streams of 160, 52 and 9
    frames (batch seeds 612..614), noise off, with the embedding; what a float32 norm="running" session with horizon 64
    returns for SCHEDULE; and the float64 reference with that horizon on the excitation the session traced.  Computed once,
    shared, left unchanged."""
    from running_horizon_ref import stream_reference
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
    assert Dc.receptive_field_frames(cfg) <= CONTEXT
    w.run = _play(w, dev, "float32", SCHEDULE, emb=w.emb, pcm16=False, trace=True, norm="running", horizon=HORIZON)
    w.ref = [stream_reference(w.wf, cfg.upsampling_scales, b.ppg, e.reshape(1, 1, -1), b.lft, w.emb, CORE, CONTEXT, FADE,
                              "running", HORIZON)[0] for b, e in zip(w.batches, w.run.exc)]
    return w


def _rel(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / max(1.0, float(np.abs(ref).max()))


def test_horizon_streams_are_the_horizon_reference(dev, world):
    """Streams of 160, 52 and 9 frames with an embedding under SCHEDULE, float32 storage, horizon 64: within TIGHT of the
    float64 reference with the same horizon on the traced excitation - which the session without a horizon is not, for
    the stream that has late windows."""
    w = world
    for u, (y, ref) in enumerate(zip(w.run.y, w.ref)):
        assert y.dtype == np.float32 and y.shape == ref.shape == (FRAMES[u] * w.cfg.hop,)
        err = _rel(y, ref)
        print(f"STREAM-HORIZON 64 stream {u}: {err:.3e} x max(1, |ref|max = {np.abs(ref).max():.3g})")
        assert err <= TIGHT, (u, err)
    never = _play(w, dev, "float32", SCHEDULE, emb=w.emb, pcm16=False, norm="running")
    err = _rel(never.y[0], w.ref[0])
    print(f"STREAM-HORIZON no horizon, stream 0 against the horizon reference: {err:.3e}")
    assert err > TIGHT


@pytest.mark.parametrize("storage", ["bfloat16", "float16"])
def test_two_byte_storages_against_the_horizon_reference(dev, world, storage):
    """The same streams in bfloat16 and float16 storage: tests/test_config_matrix_gpu.py's bfloat16 bounds, an eighth of
    them in float16."""
    w = world
    div = F16_DIV if storage == "float16" else 1.0
    res = _play(w, dev, storage, SCHEDULE, emb=w.emb, pcm16=False, norm="running", horizon=HORIZON)
    for u, (y, ref) in enumerate(zip(res.y, w.ref)):
        err = np.abs(y.astype(np.float64) - ref)
        rms, mag = float(np.sqrt(np.mean(ref ** 2))), max(1.0, float(np.abs(ref).max()))
        print(f"STREAM-HORIZON {storage} stream {u}: mean/rms {err.mean() / rms:.3e} max/mag {err.max() / mag:.3e}")
        assert np.isfinite(y).all()
        assert float(err.mean()) <= BF16_MEAN / div * rms, (u, float(err.mean()), rms)
        assert float(err.max()) <= BF16_MAX / div * mag, (u, float(err.max()), mag)


def test_another_schedule_gives_the_same_streams(dev, world):
    """SCHEDULE2 with max_push 48 > core and forwards of at most two rows: two windows of a stream share a forward (the
    second is multiplied onto the first's sums inside the launch), a stream's flush is cut across forwards.  Within 2 TIGHT
    of SCHEDULE's result: both are within TIGHT of one reference."""
    w = world
    res = _play(w, dev, "float32", SCHEDULE2, emb=w.emb, pcm16=False, trace=True, norm="running", max_batch=2, horizon=HORIZON)
    assert res.forwards == [1, 2, 0, 1, 1]
    for u, (y, first, ref) in enumerate(zip(res.y, w.run.y, w.ref)):
        err = float(np.abs(y.astype(np.float64) - first).max()) / max(1.0, float(np.abs(ref).max()))
        print(f"STREAM-HORIZON schedule 2 stream {u}: {err:.3e} to the first schedule, {_rel(y, ref):.3e} to the reference")
        assert err <= 2 * TIGHT, (u, err)


def test_a_stream_of_one_window_is_the_window_mode_bit_for_bit(dev, world):
    """The 9-frame stream ends inside window 0, a pass-through row: norm="window"'s bytes, float32 and PCM-16."""
    w = world
    for pcm16 in (False, True):
        a = _play(w, dev, "float32", SCHEDULE, emb=w.emb, pcm16=pcm16, which=(2,), norm="running", horizon=HORIZON)
        b = _play(w, dev, "float32", SCHEDULE, emb=w.emb, pcm16=pcm16, which=(2,))
        assert a.y[0].dtype == b.y[0].dtype and a.y[0].size == 9 * w.cfg.hop
        assert np.array_equal(_bits(a.y[0]), _bits(b.y[0])), pcm16


def _frames_after(core_his, core=CORE, H=HORIZON):
    """w after the cores that end at core_his, by the recurrence."""
    w, lo = 0.0, 0
    for hi in core_his:
        w = float(hi - lo) if lo == 0 else math.exp(-(hi - lo) / H) * w + (hi - lo)
        lo = hi
    return w


def test_a_reused_slot_is_fresh(dev, world):
    """One session with one slot: the 52-frame stream, its end, then the 160-frame stream in the same slot gives, bit for
    bit, what that stream gives in a new session - neither the first stream's carry nor its frame count is read:
    norm_frames restarts at 0 and follows the recurrence."""
    w, hop = world, world.cfg.hop
    sc = [48, 48, 48, 16]
    want = _play(w, dev, "float32", [sc, [], []], emb=w.emb, pcm16=False, which=(0,), norm="running", horizon=HORIZON).y[0]
    with Dc.StreamSession(w.model("float32"), w.sg, dev, n_streams=1, core=CORE, fade=FADE, max_push=48, pcm16=False,
                          norm="running", horizon=HORIZON) as s:
        a = s.open(w.emb)
        assert s.norm_frames(a) == 0.0
        s.push({a: _chunk(w.feats[1], 0, 45, hop)})
        assert s.norm_frames(a) == 0.0                   # (window 0 needs 68 frames)
        s.push({a: _chunk(w.feats[1], 45, 7, hop)}, end=[a])
        with pytest.raises(ValueError, match="not open"):
            s.norm_frames(a)
        b = s.open(w.emb)
        assert b != a and s._ids[b] == 0 and s.norm_frames(b) == 0.0
        out, at, frames = [], 0, []
        for k in sc:
            last = at + k == 160
            if not last:
                out.append(s.push({b: _chunk(w.feats[0], at, k, hop)})[b])
                frames.append(s.norm_frames(b))
            else:
                out.append(s.push({b: _chunk(w.feats[0], at, k, hop)}, end=[b])[b])
            at += k
        # 48, 96 and 144 frames seen: no window; window 0 (68 frames); windows 0 and 1 (100) and 2 (132)
        assert frames == [0.0, _frames_after([32]), _frames_after([32, 64, 96])]
    assert np.array_equal(_bits(np.concatenate(out)), _bits(want))


def test_without_an_embedding_nothing_is_carried(dev, world):
    """norm="running" with a horizon and open(trg_emb=None): norm="window"'s bits, and no frames are counted."""
    w, hop = world, world.cfg.hop
    a = _play(w, dev, "float32", SCHEDULE, pcm16=False, norm="running", horizon=HORIZON)
    b = _play(w, dev, "float32", SCHEDULE, pcm16=False)
    for u in range(3):
        assert np.array_equal(_bits(a.y[u]), _bits(b.y[u])), u
    with Dc.StreamSession(w.model("float32"), w.sg, dev, core=CORE, fade=FADE, max_push=48, norm="running", horizon=HORIZON) as s:
        i = s.open(None)
        s.push({i: _chunk(w.feats[0], 0, 48, hop)})
        s.push({i: _chunk(w.feats[0], 48, 48, hop)})
        assert s.forwards == 1 and s.norm_frames(i) == 0.0


def test_a_refused_push_leaves_frames_carry_and_parity_alone(dev, world):
    """Two refused pushes before every valid one of the 160-frame stream: the carry keeps its bits, the slot its parity
    and its frame count across each refusal, and the stream still is the horizon reference within TIGHT."""
    w, hop = world, world.cfg.hop
    feat = w.feats[0]
    good = _chunk(feat, 0, 4, hop)
    with Dc.StreamSession(w.model("float32"), w.sg, dev, n_streams=2, core=CORE, fade=FADE, max_push=48, pcm16=False,
                          norm="running", horizon=HORIZON) as s:
        s.open(w.emb)                                    # (an idle stream in slot 0: ours is in slot 1)
        a = s.open(w.emb)
        bad = [({a: dict(good, ppg=good["ppg"][:, :-1])}, ()), ({a: _chunk(feat, 0, 49, hop)}, ()), ({a: good, 99: good}, ()),
               ({a: dict(good, lft=good["lft"][:-1])}, ()), ({a: good}, (99,))]
        out, at, seen_w = [], 0, []
        for i, k in enumerate(SCHEDULE[0]):
            carry = s._carry.clone().view(torch.int64)
            state = [(st.norm_parity, st.norm_w) for st in s._slots]
            for chunks, end in (bad[i % len(bad)], bad[(i + 2) % len(bad)]):
                with pytest.raises(ValueError):
                    s.push(chunks, end)
            assert torch.equal(s._carry.view(torch.int64), carry) and [(st.norm_parity, st.norm_w) for st in s._slots] == state
            seen_w.append(state[1][1])
            out.append(s.push({a: _chunk(feat, at, k, hop)}, end=[a] if i == len(SCHEDULE[0]) - 1 else ())[a])
            at += k
        assert state[0] == (0, 0.0)                      # (the idle stream never ran)
        assert seen_w[0] == 0.0 and seen_w[-1] == _frames_after([32, 64]) and sorted(seen_w) == seen_w
    err = _rel(np.concatenate(out), w.ref[0])
    print(f"STREAM-HORIZON after refused pushes: {err:.3e}")
    assert err <= TIGHT, err


def test_horizon_arguments(dev, world):
    w, cfg = world, world.cfg
    m = w.model("float32")
    for kw, what in ((dict(norm="window", horizon=64), "needs norm"), (dict(horizon=64), "needs norm"),
                     (dict(norm="running", horizon=CORE - 1), "shorter than the core"),
                     (dict(norm="running", horizon=0), "positive"), (dict(norm="running", horizon=-64.0), "positive"),
                     (dict(norm="running", horizon=float("inf")), "finite"), (dict(norm="running", horizon=float("nan")), "finite")):
        with pytest.raises(ValueError, match=what):
            Dc.StreamSession(m, w.sg, dev, core=CORE, **kw)
    with Dc.StreamSession(m, w.sg, dev, core=CORE, norm="running", horizon=CORE) as s:
        assert s.horizon == float(CORE)
    with Dc.StreamSession(m, w.sg, dev, core=CORE) as s:
        with pytest.raises(ValueError, match="norm_frames needs"):
            s.norm_frames(0)
    b = S.synth_batch(cfg, 2, 8, 620)
    ins = [torch.from_numpy(v).to(dev) for v in (b.ppg, b.sine, b.lft, b.spk_emb)]
    running = ([0, 1], [0, 0], [8, 8], [0, 0], [1, 1], [0, 0])
    forget = ([1.0, 1.0], [8.0, 8.0], [8.0, 8.0])
    carry = torch.empty((2, m.plan.norm_carry_bytes() // 8), dtype=torch.float64, device=dev)
    with torch.no_grad():
        with pytest.raises(ValueError, match="norm_decay goes with norm_running"):
            m(*ins, norm_decay=forget)
        with pytest.raises(ValueError, match="row 1: decay"):
            m(*ins, norm_running=running, norm_carry=carry, norm_decay=([1.0, 0.0],) + forget[1:])
        with pytest.raises(ValueError, match="row 0: weight"):
            m(*ins, norm_running=running, norm_carry=carry, norm_decay=(forget[0], [7.5, 8.0], forget[2]))
        # every row a window 0: the plain forward's bits, and the carry holds the rows' own sums
        want = m(*ins).cpu().numpy()
        got = m(*ins, norm_running=running, norm_carry=carry, norm_decay=forget).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    assert np.isfinite(carry.view(2, 2, -1)[:, 1].cpu().numpy()).all()
    m.train()
    try:
        with pytest.raises(NotImplementedError):
            m(*ins, norm_running=running, norm_carry=carry, norm_decay=forget)
    finally:
        m.eval()


# ------------------------------------------------------------------------------------------------------ the raise
def _push_sizes(s, sid, feat, sizes, hop, before_push=None):
    """The stream in pushes of these sizes, the last one carrying its end -> its samples."""
    out, at = [], 0
    for i, k in enumerate(sizes):
        if before_push is not None:
            before_push(at)
        out.append(s.push({sid: _chunk(feat, at, k, hop)}, end=[sid] if i == len(sizes) - 1 else ())[sid])
        at += k
    return np.concatenate(out)


def test_level_jump_at_the_shortest_horizon_in_float32(dev, world):
    """tests/test_decode_stream_horizon.py's stream: 320 frames whose ppg, lft and excitation amplitude are four times
    larger from frame 160 on, float32 storage, horizon 32 = core.  A column of the left context lies up to two cores back and
    weighs e^-2 there: the normalised row is bounded by sqrt(weight / e^-2), 2.7 times what the weighted population alone
    would suggest, and right behind the jump the quiet context is what the loud statistics do NOT cover - the staging scale
    has to come from bound[], or the split-binary16 staging saturates.  Within TIGHT of the float64 reference with the same
    horizon on the traced excitation; the reference is finite and every core behind the jump reaches a quarter of its
    range, so TIGHT x range speaks about those windows."""
    from running_horizon_ref import stream_reference
    from test_decode_stream_horizon import GAIN, JUMP, TOTAL, level_jump_stream
    w, cfg = world, world.cfg
    hop = cfg.hop
    b, ppg, _, lft = level_jump_stream(cfg)
    feat = dict(f0=b.f0[0].T.copy(), ppg=ppg[0].T.copy(), lft=lft[0].T.copy())
    sg = _sg(hop)
    amp = float(sg.sine_amp)

    def louder(at):                                      # (the push reads the amplitude: pushes of 32 frames, 160 = 5 x 32)
        sg.sine_amp = amp * (GAIN if at >= JUMP else 1.0)
    with Dc.StreamSession(w.model("float32"), sg, dev, core=CORE, fade=FADE, pcm16=False, norm="running", horizon=float(CORE)) as s:
        s._stream_trace = {}
        a = s.open(w.emb)
        y = _push_sizes(s, a, feat, [32] * (TOTAL // 32), hop, louder)
        exc = torch.cat(s._stream_trace["excitation"][a]).cpu().numpy()
    assert s.context == CONTEXT and np.abs(exc[JUMP * hop:]).max() > 3.0 * np.abs(exc[:JUMP * hop]).max()
    ref, rows = stream_reference(w.wf, cfg.upsampling_scales, ppg, exc.reshape(1, 1, -1), lft, w.emb, CORE, CONTEXT, FADE,
                                 "running", float(CORE))
    assert np.isfinite(ref).all() and len(rows) == 10
    peaks = [float(np.abs(ref[lo * hop: hi * hop]).max()) for _, _, _, lo, hi in rows]
    print("STREAM-HORIZON level jump, reference |.|max per core: " + " ".join(f"{p:.3g}" for p in peaks))
    assert min(peaks[JUMP // CORE:]) >= 0.25 * max(peaks), peaks
    err = _rel(y, ref)
    print(f"STREAM-HORIZON level jump, horizon 32, float32: {err:.3e} x max(1, |ref|max = {max(peaks):.3g})")
    assert np.isfinite(y).all() and err <= TIGHT, err


# ------------------------------------------------------------------------------------------------------ no horizon
def test_no_horizon_is_the_running_mode_byte_for_byte(dev, world):
    """The 160-frame stream: horizon=None is the session without the argument - and both are the bytes of the DECAYED entry
    point fed decay 1, weight = bound = in_hi (a session whose horizon is set to infinity behind the constructor's back:
    exp(-c / inf) is exactly 1), so the new pool kernel and the old one agree through whole forwards, raise included."""
    w, hop = world, world.cfg.hop
    old = _play(w, dev, "float32", SCHEDULE, emb=w.emb, pcm16=False, which=(0,), norm="running").y[0]
    new = _play(w, dev, "float32", SCHEDULE, emb=w.emb, pcm16=False, which=(0,), norm="running", horizon=None).y[0]
    assert np.array_equal(_bits(old), _bits(new))
    with Dc.StreamSession(w.model("float32"), w.sg, dev, core=CORE, fade=FADE, max_push=48, pcm16=False, norm="running") as s:
        s.horizon = math.inf
        a = s.open(w.emb)
        y = _push_sizes(s, a, w.feats[0], SCHEDULE[0], hop)              # (the same forwards: batching is not bitwise)
    assert np.array_equal(_bits(y), _bits(old))
