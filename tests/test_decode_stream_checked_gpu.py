"""GPU tests (-m gpu) of checked live streams: the per-window check kernel (csrc/fastsvc_stream_check.hip) against
decode.output_report on arbitrary unaligned spans bit for bit, its carry word, its argument checks; and
decode.StreamSession(checked=True) against unchecked sessions in the storages involved - bit for bit wherever a window
was not replaced, within the suite's bfloat16 bound where float16 and bfloat16 windows meet.

The session premise (test_premise_...): stream A's ppg and lft are scaled by 2^12 on frames [96, 110).  With core 32 and
the default context of 36 frames window k reads frames [32 k - 36, 32 k + 68), so windows 1 - 4 read scaled frames and
windows 0, 5 and 6 do not (frames [100, 110) would spare window 1, which reads up to frame 99)."""
import ctypes

import numpy as np
import pytest
import torch

import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd import synth as S
from test_decode_stream_gpu import BF16_MAX

pytestmark = pytest.mark.gpu

FILL = 0x7F7F7F7F
SPECIALS = [np.nan, np.inf, -np.inf, 1.0, -1.0, 1.0001, -1.0001]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    A.load_library()
    return torch.device("cuda:0")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def _want_report(y, lo, hi, carry_word=None):
    """decode.output_report of every row's span as the (B, 4) int32 table the device writes."""
    nf, cl, mx = Dc.output_report([y[b, lo[b]: hi[b]] for b in range(len(lo))])
    word = np.zeros_like(nf) if carry_word is None else np.asarray(carry_word, np.int32)
    return np.stack([nf, cl, mx.view(np.int32), word], axis=1)


# ---------------------------------------------------------------------------------------------------------- the kernel
WIDTH = 4104
SPANS = [(0, 0), (0, 1), (3, 3), (1, 8), (5, 4104), (7, 2055), (4, 4100), (0, 4104), (2049, 2050), (4103, 4104)]


@pytest.fixture(scope="module")
def rows(dev):
    """Hash-generator samples in [-1.2, 1.2]; special values at lo - 1, lo, hi - 1 and hi of every span; on the device once
    4 bytes off a 16-byte boundary and once aligned."""
    B = len(SPANS)
    y = (S.hash_uniform(79, 5, B * WIDTH) * 2.4 - 1.2).astype(np.float32).reshape(B, WIDTH)
    j = 0
    for b, (lo, hi) in enumerate(SPANS):
        for k in sorted({lo - 1, lo, hi - 1, hi}):
            if 0 <= k < WIDTH:
                y[b, k] = SPECIALS[j % len(SPECIALS)]
                j += 1
    buf = torch.zeros(B * WIDTH + 1, dtype=torch.float32, device=dev)
    off = buf[1:].view(B, WIDTH)
    off.copy_(torch.from_numpy(y))
    aligned = off.clone()
    assert off.data_ptr() % 16 == 4 and off.is_contiguous() and aligned.data_ptr() % 16 == 0
    return y, off, aligned


def test_reports_equal_the_host_reference_on_the_span_bit_for_bit(dev, rows):
    y, off, aligned = rows
    lo, hi = [s[0] for s in SPANS], [s[1] for s in SPANS]
    want = _want_report(y, lo, hi)
    assert want[:, 0].sum() > 0 and want[:, 1].sum() > 100 and (want[:, 0] == 0).any()      # (the set exercises every field)
    whole = _want_report(y, [0] * len(SPANS), [WIDTH] * len(SPANS))
    assert (whole[:, 0] > want[:, 0]).any()                    # (a special value just outside a span: one read shows)
    for yd in (off, aligned):
        got = A.stream_check(yd, lo, hi)
        assert got.shape == (len(SPANS), 4) and got.dtype == torch.int32 and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want), yd.data_ptr() % 16
        assert np.array_equal(A.stream_check(yd[:, None, :], lo, hi, slots=[0] * len(SPANS), entries=[-1] * len(SPANS)).cpu().numpy(), want)
    # the whole row: fastsvc_output_check's table
    assert np.array_equal(A.stream_check(off, [0] * len(SPANS), [WIDTH] * len(SPANS)).cpu().numpy(),
                          A.output_check(off, [WIDTH] * len(SPANS)).cpu().numpy())


@pytest.mark.parametrize("entry_doubles", [1, 2, 255, 1152])
def test_the_carry_word_counts_the_entry_that_was_written_and_nothing_else(dev, entry_doubles):
    """Records of 5 slots, 3 doubles of padding behind the two entries.  Everything is NaN - the other entry, the other
    slots, the padding, the doubles on both sides of a scanned entry - except the scanned entries, which are finite but
    for what is planted at their first and last double."""
    ed, n_slots = entry_doubles, 5
    K = 2 * ed + 3
    carry = np.full((n_slots, K), np.nan)
    rng = np.random.default_rng(ed)
    # per row: slot, entry, what is planted at the first / last double
    plan = [(0, 0, None, None), (1, 1, np.nan, None), (2, 0, None, np.inf), (3, 1, -np.inf, np.nan), (4, -1, None, None),
            (1, 1, np.nan, None)]
    want = []
    for slot, entry, first, last in plan:
        if entry < 0:
            want.append(0)
            continue
        e = carry[slot, entry * ed: (entry + 1) * ed]
        e[:] = rng.standard_normal(ed) * 1e300                 # (finite, the largest exponents included)
        planted = set()
        if first is not None:
            e[0] = first
            planted.add(0)
        if last is not None:
            e[ed - 1] = last
            planted.add(ed - 1)
        want.append(len(planted))
    assert np.isnan(carry[4]).all() and max(want) == (2 if ed > 1 else 1)
    y = np.linspace(-0.5, 0.5, len(plan) * 24, dtype=np.float32).reshape(len(plan), 24)
    lo, hi = [1] * len(plan), [23] * len(plan)
    yd, cd = torch.from_numpy(y).to(dev), torch.from_numpy(carry).to(dev)
    got = A.stream_check(yd, lo, hi, carry=cd, slots=[p[0] for p in plan], entries=[p[1] for p in plan], entry_doubles=ed)
    assert np.array_equal(got.cpu().numpy(), _want_report(y, lo, hi, want))
    # entry -1 everywhere: no carry is read, a null carry is fine
    none = A.stream_check(yd, lo, hi, carry=None, slots=[0] * len(plan), entries=[-1] * len(plan), entry_doubles=ed)
    assert np.array_equal(none.cpu().numpy(), _want_report(y, lo, hi))
    # a record of exactly two entries: the last double of entry 1 is the last of the buffer
    tight = np.ascontiguousarray(carry[:, : 2 * ed])
    tight[4] = 1.0
    tight[4, 2 * ed - 1] = np.inf
    got = A.stream_check(yd[:1], lo[:1], hi[:1], carry=torch.from_numpy(tight).to(dev), slots=[4], entries=[1], entry_doubles=ed)
    assert np.array_equal(got.cpu().numpy(), _want_report(y[:1], lo[:1], hi[:1], [1]))


def test_rows_past_64_report_from_a_second_launch(dev):
    B, width = 65, 80
    lo = [b % 7 for b in range(B)]
    hi = [5 + b % 65 for b in range(B)]
    hi = [max(h, l) for l, h in zip(lo, hi)]
    y = (S.hash_uniform(80, 5, B * width) * 2.4 - 1.2).astype(np.float32).reshape(B, width)
    for b in (0, 63, 64):
        y[b, (lo[b] + hi[b]) // 2] = np.nan
    want = _want_report(y, lo, hi)
    assert list(np.nonzero(want[:, 0])[0]) == [0, 63, 64]
    table = torch.full((B + 1, 4), FILL, dtype=torch.int32, device=dev)        # entry 65: a guard
    A.stream_check(torch.from_numpy(y).to(dev), lo, hi, out=table[:B])
    got = table.cpu().numpy()
    assert np.array_equal(got[:B], want)
    assert np.all(got[B] == FILL)                              # nothing past entry 64 is written


def test_every_call_overwrites_the_report(dev, rows):
    y, off, aligned = rows
    lo, hi = [s[0] for s in SPANS], [s[1] for s in SPANS]
    want = _want_report(y, lo, hi)
    report = torch.full((len(SPANS), 4), FILL, dtype=torch.int32, device=dev)
    assert A.stream_check(off, lo, hi, out=report) is report
    first = report.cpu().numpy().copy()
    A.stream_check(off, lo, hi, out=report)
    assert np.array_equal(first, want) and np.array_equal(report.cpu().numpy(), want)


def test_bad_arguments_are_invalid_and_write_nothing(dev):
    lib = A.load_library()
    B, width, ed = 2, 16, 4
    y = torch.ones(B, width, device=dev) * 3
    carry = torch.zeros((3, 2 * ed), dtype=torch.float64, device=dev)
    report = torch.full((B, 4), FILL, dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    Y, REP, CARRY = vp(y.data_ptr()), vp(report.data_ptr()), vp(carry.data_ptr())

    def call(lo=(0, 0), hi=(16, 16), slot=(0, 2), entry=(0, 1), yp=Y, rep=REP, cp=CARRY, carry_bytes=2 * ed * 8, doubles=ed,
             n_slots=3, w=width):
        return lib.fastsvc_stream_check(yp, B, w, (i32 * B)(*lo), (i32 * B)(*hi), cp, carry_bytes, doubles, n_slots,
                                        None if slot is None else (i32 * B)(*slot), None if entry is None else (i32 * B)(*entry),
                                        rep, stream)

    INVALID = -1                                               # FASTSVC_E_INVALID
    assert call(yp=None) == INVALID                            # a null y
    assert call(rep=None) == INVALID                           # a null report
    assert call(lo=(0, 9), hi=(16, 8)) == INVALID              # lo > hi
    assert call(hi=(16, 17)) == INVALID                        # hi > width
    assert call(lo=(-1, 0)) == INVALID                         # negative values
    assert call(lo=(0, -4), hi=(16, -2)) == INVALID
    assert call(slot=(0, -1)) == INVALID
    assert call(carry_bytes=-64) == INVALID
    assert call(doubles=-4) == INVALID
    assert call(w=-16) == INVALID
    assert call(entry=(0, 2)) == INVALID                       # an entry outside {-1, 0, 1}
    assert call(entry=(-2, 1)) == INVALID
    assert call(cp=None) == INVALID                            # an entry >= 0 with a null carry
    assert call(entry=(-1, 0), cp=None) == INVALID
    assert call(carry_bytes=2 * ed * 8 - 8) == INVALID         # carry_bytes < 2 * entry_doubles * 8
    assert call(doubles=ed + 1) == INVALID
    assert call(slot=(0, 3)) == INVALID                        # a slot outside the carry
    assert b"fastsvc_stream_check" in lib.fastsvc_last_error()
    torch.cuda.synchronize(dev)
    assert np.all(report.cpu().numpy() == FILL)
    assert call() == 0                                         # (the same call with good arguments does write)
    assert call(entry=(-1, -1), cp=None, carry_bytes=0, doubles=0, n_slots=0) == 0           # (no carry at all is fine)
    assert call(slot=None, entry=None, cp=None, carry_bytes=0, doubles=0, n_slots=0) == 0
    torch.cuda.synchronize(dev)
    assert np.array_equal(report.cpu().numpy(), _want_report(y.cpu().numpy(), [0, 0], [16, 16]))
    with pytest.raises(ValueError):                            # and through the binding
        A.stream_check(y, [0, 0], [16, 17])
    with pytest.raises(ValueError):
        A.stream_check(y, [0, 0], [16, 16], out=torch.empty((B, 3), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        A.stream_check(y, [0, 0], [16, 16], carry=carry, slots=[0, 1], entries=[0, 2], entry_doubles=ed)
    with pytest.raises(ValueError):
        A.stream_check(y, [0, 0], [16, 16], carry=carry, slots=[0, 1])


# --------------------------------------------------------------------------------------------------------- the session
CORE, FADE, MAX_PUSH = 32, 8, 48
FRAMES = dict(A=224, B=52, C=9)
LOUD = (96, 110)                   # stream A's frames whose ppg and lft are scaled out of float16 storage's range
SCALE = 2.0 ** 12
# the frames of every push; a stream's last push carries its end.  A: window 0 runs in push 1, window 1 in push 2 - beside
# both windows of B, which ends there - windows 2 and 3 together in push 3, window 4 in push 4, windows 5 and 6 at the end
SCHEDULE = dict(A=[40, 30, 48, 46, 33, 27], B=[20, 0, 32], C=[4, 5])
FLAGGED_WINDOW, FLAGGED_RUNNING = [1, 2, 3, 4], [1, 2, 3, 4, 5, 6]
NORMS = [dict(norm="window"), dict(norm="running"), dict(norm="running", horizon=64)]
NORM_IDS = ["window", "running", "horizon64"]


class _World:
    pass


def _module(cfg, sd, dev, storage):
    g = A.FastSVCGenerator(in_channels=cfg.in_channels, mid_channels=list(cfg.mid_channels),
                           upsampling_scales=list(cfg.upsampling_scales), out_channels=cfg.out_channels,
                           spk_emb_size=cfg.spk_emb_size, use_spk_emb=cfg.use_spk_emb)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    g.remove_weight_norm()
    g.activation_storage = storage
    return g.eval().to(dev)


def _features(cfg):
    rng = np.random.default_rng(31)
    feats = {}
    for name, f in FRAMES.items():
        f0 = np.where(rng.random(f) < 0.3, 0.0, rng.uniform(80, 400, f))
        feats[name] = dict(f0=f0, ppg=rng.standard_normal((f, cfg.in_channels)).astype(np.float32),
                           lft=rng.uniform(-9, 1, f * cfg.hop).astype(np.float32))
    plain = dict(feats["A"])
    loud = dict(f0=plain["f0"], ppg=plain["ppg"].copy(), lft=plain["lft"].copy())
    loud["ppg"][LOUD[0]: LOUD[1]] *= np.float32(SCALE)
    loud["lft"][LOUD[0] * cfg.hop: LOUD[1] * cfg.hop] *= np.float32(SCALE)
    feats["A"], feats["A_plain"] = loud, plain
    emb = rng.standard_normal(cfg.spk_emb_size).astype(np.float32)
    return feats, emb


def _play(w, dev, storage, which, trace=False, after_push=None, **kw):
    """The streams `which` side by side through one session, push i of every stream in one call -> per stream its
    samples, the forwards of every push, a checked session's reports per (stream, window), its last totals and the trace."""
    hop = w.cfg.hop
    res = _World()
    model = w.models[storage]
    kw.setdefault("max_batch", 32)
    with Dc.StreamSession(model, w.sg, dev, n_streams=len(which), core=CORE, fade=FADE, max_push=MAX_PUSH, pcm16=False, **kw) as s:
        if trace:
            s._stream_trace = {}
        ids = {u: s.open(w.emb) for u in which}
        name = {i: u for u, i in ids.items()}
        pieces, at = {u: [] for u in which}, {u: 0 for u in which}
        res.forwards, res.reports, res.totals = [], {}, {}
        for i in range(max(len(SCHEDULE[u[0]]) for u in which)):
            chunks, end = {}, []
            for u in which:
                sched, f = SCHEDULE[u[0]], w.feats[u]
                if i < len(sched):
                    a, k = at[u], sched[i]
                    chunks[ids[u]] = dict(ppg=f["ppg"][a: a + k], f0=f["f0"][a: a + k], lft=f["lft"][a * hop: (a + k) * hop])
                    at[u] += k
                    if i == len(sched) - 1:
                        end.append(ids[u])
            before = s.forwards
            out = s.push(chunks, end)
            res.forwards.append(s.forwards - before)
            assert model.activation_storage == storage         # (back in its first storage after every push)
            for sid, y in out.items():
                assert y.dtype == np.float32
                pieces[name[sid]].append(y)
            if s.checked:
                rep = s.last_report
                assert sorted(k for k in rep if k != "totals") == sorted(chunks)
                assert sorted(rep.get("totals", {})) == sorted(end)
                for sid in chunks:
                    for d in rep[sid]:
                        assert (name[sid], d["window"]) not in res.reports
                        res.reports[(name[sid], d["window"])] = d
                for sid in end:
                    res.totals[name[sid]] = rep["totals"][sid]
            if after_push is not None:
                after_push(s, i)
        assert all(at[u] == FRAMES[u[0]] for u in which)
        if trace:
            res.trace_y = [(rows, y.cpu().numpy()) for rows, y in s._stream_trace.get("y", [])]
            res.names = name
    res.y = {u: np.concatenate(pieces[u]) for u in which}
    for u in which:
        assert res.y[u].size == FRAMES[u[0]] * hop
    return res


@pytest.fixture(scope="module")
def world(dev):
    """Models in the two storages (weights seed 12), the streams, and what UNCHECKED sessions return for them - computed
    once, shared by the session tests and left unchanged."""
    w = _World()
    cfg = w.cfg = S.FULL_CONFIG
    sd = S.synth_state_dict(cfg, 12)
    w.models = {st: _module(cfg, sd, dev, st) for st in ("float16", "bfloat16")}
    w.sg = A.SignalGenerator(sample_rate=24000, hop_size=cfg.hop, sine_amp=0.1, noise_amp=0.0, signal_types=["sine"])
    w.feats, w.emb = _features(cfg)
    w.f16 = [_play(w, dev, "float16", ("A", "B", "C"), **kw) for kw in NORMS]
    w.f16_plain = [_play(w, dev, "float16", ("A_plain", "B", "C"), **kw) for kw in NORMS]
    w.bf16 = [_play(w, dev, "bfloat16", ("A", "B", "C"), **kw) for kw in NORMS]
    w.bf16_alone = _play(w, dev, "bfloat16", ("A",), norm="window")
    return w


def _window_is_bad(y, k, hop):
    """Whether window k owns a non-finite sample outside the fade zones it shares with its neighbours."""
    h = FADE // 2
    lo = k * CORE + (h if k else 0)
    hi = min((k + 1) * CORE - h, y.size // hop) if (k + 1) * CORE * hop < y.size else y.size // hop
    return not np.isfinite(y[lo * hop: hi * hop]).all()


def test_premise_float16_overflows_where_stated_and_bfloat16_nowhere(dev, world):
    hop = world.cfg.hop
    n_win = -(-FRAMES["A"] // CORE)
    assert n_win == 7
    for k in range(n_win):                                     # (which windows read a scaled frame)
        reads = max(0, k * CORE - 36) < LOUD[1] and LOUD[0] < min(FRAMES["A"], (k + 1) * CORE + 36)
        assert reads == (k in FLAGGED_WINDOW), k
    for kw, res, bres in zip(NORMS, world.f16, world.bf16):
        bad = [k for k in range(n_win) if _window_is_bad(res.y["A"], k, hop)]
        whole = [k for k in range(n_win) if not np.isfinite(res.y["A"][(k * CORE + 4) * hop: ((k + 1) * CORE - 4) * hop]).any()]
        print(f"PREMISE float16 {kw}: non-finite windows of A {bad}, wholly non-finite {whole}")
        assert bad == (FLAGGED_WINDOW if kw["norm"] == "window" else FLAGGED_RUNNING), kw
        assert np.isfinite(res.y["B"]).all() and np.isfinite(res.y["C"]).all()
        assert all(np.isfinite(v).all() for v in bres.y.values()), kw
    assert np.isfinite(world.bf16_alone.y["A"]).all()
    for res in world.f16_plain:
        assert all(np.isfinite(v).all() for v in res.y.values())


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _within_bf16(got, ref, scale_ref):
    return float(np.abs(got.astype(np.float64) - ref).max()) <= BF16_MAX * max(1.0, float(np.abs(scale_ref).max()))


@pytest.mark.parametrize("kw,j", list(zip(NORMS, range(3))), ids=NORM_IDS)
def test_nothing_to_do_is_the_unchecked_session(dev, world, kw, j):
    ref = world.f16_plain[j]
    got = _play(world, dev, "float16", ("A_plain", "B", "C"), checked=True, **kw)
    assert got.forwards == ref.forwards
    for u in ref.y:
        assert _same(got.y[u], ref.y[u]), u
    assert len(got.reports) == 7 + 2 + 1
    for key, d in got.reports.items():
        assert d["storage"] == "float16" and d["tried"] == [] and d["nonfinite"] == 0 and d["carry_nonfinite"] == 0, key
        assert d["max_abs"] > 0
    assert got.totals["A_plain"] == dict(windows=7, fell_back=0, nonfinite=0, clipped=got.totals["A_plain"]["clipped"],
                                         max_abs=max(d["max_abs"] for (u, _), d in got.reports.items() if u == "A_plain"),
                                         storages={"float16": 7})


def _check_reports_against_trace(got, hop):
    """Every report's numbers are decode.output_report's of the span of the traced y the samples came from."""
    seen = 0
    for rows, y in got.trace_y:
        srows = [Dc.StreamRow(0, lo // CORE, in_lo, in_hi, lo, hi, hi == FRAMES[got.names[sid][0]]) for sid, in_lo, in_hi, lo, hi in rows]
        los, his = Dc.stream_check_spans(srows, hop, FADE * hop // 2)
        nf, cl, mx = Dc.output_report([y[r, 0, los[r]: his[r]] for r in range(len(rows))])
        for r, (sid, _, _, lo, _) in enumerate(rows):
            d = got.reports[(got.names[sid], lo // CORE)]
            assert (d["nonfinite"], d["clipped"]) == (int(nf[r]), int(cl[r])), (sid, lo)
            assert np.float32(d["max_abs"]).view(np.uint32) == mx[r].view(np.uint32), (sid, lo)
            seen += 1
    assert seen == len(got.reports)


def _flagged_forwards(got, flagged):
    return sum(1 for rows, _ in got.trace_y if any(got.names[sid] == "A" and lo // CORE in flagged for sid, _, _, lo, _ in rows))


def test_window_norm_replaces_exactly_the_flagged_windows(dev, world):
    hop = world.cfg.hop
    ref16, refb = world.f16[0], world.bf16_alone
    got = _play(world, dev, "float16", ("A", "B", "C"), checked=True, trace=True, norm="window")
    assert all(np.isfinite(v).all() for v in got.y.values())
    assert _same(got.y["B"], ref16.y["B"]) and _same(got.y["C"], ref16.y["C"])
    # A: float16 bits | zone around frame 32 | bfloat16 bits | zone around frame 160 | float16 bits
    h = FADE // 2
    cuts = [0, (CORE - h) * hop, (CORE + h) * hop, (5 * CORE - h) * hop, (5 * CORE + h) * hop, FRAMES["A"] * hop]
    y, y16, yb = got.y["A"], ref16.y["A"], refb.y["A"]
    for seg, ref in ((0, y16), (2, yb), (4, y16)):
        a, b = cuts[seg], cuts[seg + 1]
        assert np.isfinite(ref[a:b]).all() and _same(y[a:b], ref[a:b]), seg
    for seg in (1, 3):
        a, b = cuts[seg], cuts[seg + 1]
        assert not np.isfinite(y16[a:b]).all()                 # (the unchecked float16 session blends a NaN in)
        assert _within_bf16(y[a:b], yb[a:b], yb), seg
    for (u, k), d in got.reports.items():
        fell = u == "A" and k in FLAGGED_WINDOW
        assert (d["storage"], d["tried"]) == (("bfloat16", ["float16"]) if fell else ("float16", [])), (u, k)
        assert d["nonfinite"] == 0 and d["carry_nonfinite"] == 0
    assert sorted(got.reports) == sorted([("A", k) for k in range(7)] + [("B", 0), ("B", 1), ("C", 0)])
    _check_reports_against_trace(got, hop)
    extra = _flagged_forwards(got, FLAGGED_WINDOW)
    assert extra == 3 and sum(got.forwards) == sum(ref16.forwards) + extra
    assert got.totals["A"]["fell_back"] == 4 and got.totals["A"]["storages"] == {"float16": 3, "bfloat16": 4}
    assert got.totals["B"]["fell_back"] == 0 and got.totals["B"]["storages"] == {"float16": 2}       # (a whole stream did not)


@pytest.mark.parametrize("j", [1, 2], ids=NORM_IDS[1:])
def test_running_norm_keeps_the_carry_finite_and_returns_to_float16(dev, world, j):
    hop, kw = world.cfg.hop, NORMS[j]
    ref16, refb = world.f16[j], world.bf16[j]
    pushes = []

    def carry_is_finite(s, i):
        torch.cuda.synchronize(dev)
        for st in s._slots:
            if st is not None and st.done > 0:
                entry = s._carry[st.slot].view(2, -1)[st.norm_parity].cpu().numpy()
                assert np.isfinite(entry).all(), (i, st.id)
                pushes.append(i)

    got = _play(world, dev, "float16", ("A", "B", "C"), checked=True, trace=True, after_push=carry_is_finite, **kw)
    assert pushes == [1, 2, 3, 4]                              # (A, open with windows behind it; B and C run theirs as they end)
    assert all(np.isfinite(v).all() for v in got.y.values())
    assert _same(got.y["B"], ref16.y["B"]) and _same(got.y["C"], ref16.y["C"])
    for (u, k), d in got.reports.items():
        fell = u == "A" and k in FLAGGED_WINDOW
        assert (d["storage"], d["tried"]) == (("bfloat16", ["float16"]) if fell else ("float16", [])), (u, k)
        assert d["nonfinite"] == 0 and d["carry_nonfinite"] == 0
    assert len(got.reports) == 10
    # windows 5 and 6 ran in float16 on a carry the bfloat16 windows left: the bfloat16 session's samples, to the suite's bound
    a = (5 * CORE + FADE // 2) * hop
    assert not np.isfinite(ref16.y["A"][a:]).all()             # (what the unchecked float16 stream returns there: the hazard)
    assert _within_bf16(got.y["A"][a:], refb.y["A"][a:], refb.y["A"])
    assert _within_bf16(got.y["A"], refb.y["A"], refb.y["A"])
    assert _same(got.y["A"][: (CORE - FADE // 2) * hop], ref16.y["A"][: (CORE - FADE // 2) * hop])       # (window 0: float16's bits)
    _check_reports_against_trace(got, hop)
    extra = _flagged_forwards(got, FLAGGED_WINDOW)
    assert extra == 3 and sum(got.forwards) == sum(ref16.forwards) + extra
    assert got.totals["A"]["storages"] == {"float16": 3, "bfloat16": 4} and got.totals["C"]["fell_back"] == 0


@pytest.mark.parametrize("j", [0, 1], ids=NORM_IDS[:2])
def test_without_fallbacks_the_session_only_reports(dev, world, j):
    kw, ref = NORMS[j], world.f16[j]
    got = _play(world, dev, "float16", ("A", "B", "C"), checked=True, fallback=(), **kw)
    assert got.forwards == ref.forwards
    for u in ref.y:
        assert _same(got.y[u], ref.y[u]), u
    flagged = FLAGGED_WINDOW if j == 0 else FLAGGED_RUNNING
    for (u, k), d in got.reports.items():
        assert d["storage"] == "float16" and d["tried"] == []
        if u == "A" and k in flagged:
            assert d["nonfinite"] > 0, k
            assert (d["carry_nonfinite"] > 0) == (j == 1), (k, d)
        else:
            assert d["nonfinite"] == 0 and d["carry_nonfinite"] == 0, (u, k)
    assert got.totals["A"]["fell_back"] == 0 and got.totals["A"]["nonfinite"] == sum(got.reports[("A", k)]["nonfinite"] for k in flagged)


@pytest.mark.parametrize("j", [0, 1], ids=NORM_IDS[:2])
def test_forwards_of_two_rows_flag_and_replace_the_same_windows(dev, world, j):
    kw = NORMS[j]
    wide = _play(world, dev, "float16", ("A", "B", "C"), checked=True, **kw)
    got = _play(world, dev, "float16", ("A", "B", "C"), checked=True, trace=True, max_batch=2, **kw)
    assert max(got.forwards) >= 2                              # (a push of several forwards: A 1 | B 0, then B 1)
    assert any(len({sid for sid, *_ in a[0]} & {sid for sid, *_ in b[0]}) for a, b in zip(got.trace_y, got.trace_y[1:]))
    assert sorted(got.reports) == sorted(wide.reports)
    for key, d in got.reports.items():
        assert (d["storage"], d["tried"]) == (wide.reports[key]["storage"], wide.reports[key]["tried"]), key
        assert d["nonfinite"] == 0
    assert [k for (u, k), d in sorted(got.reports.items()) if d["tried"]] == FLAGGED_WINDOW
    assert any(not d["tried"] for (u, k), d in got.reports.items() if u == "A") and not got.totals["B"]["fell_back"]
    for u in wide.y:
        assert np.isfinite(got.y[u]).all() and _within_bf16(got.y[u], wide.y[u], wide.y[u]), u


def test_slot_reuse_refused_pushes_and_totals(dev, world):
    hop, f = world.cfg.hop, world.feats["A"]
    model = world.models["float16"]

    def chunk(a, k):
        return dict(ppg=f["ppg"][a: a + k], f0=f["f0"][a: a + k], lft=f["lft"][a * hop: (a + k) * hop])

    def run(refuse):
        """Frames [64, 136) of A as a stream of its own (the scaled frames sit in both its windows), then a second one."""
        with Dc.StreamSession(model, world.sg, dev, n_streams=1, core=CORE, fade=FADE, max_push=MAX_PUSH, pcm16=False,
                              norm="running", checked=True) as s:
            a = s.open(world.emb)
            assert s.totals(a) == dict(windows=0, fell_back=0, nonfinite=0, clipped=0, max_abs=0.0, storages={})
            out = [s.push({a: chunk(64, 40)})[a]]
            assert out[0].size == 0 and s.last_report == {a: []}             # (no window ran: an empty list)
            out.append(s.push({a: chunk(104, 30)})[a])
            assert [d["window"] for d in s.last_report[a]] == [0] and s.totals(a)["windows"] == 1
            if refuse:
                torch.cuda.synchronize(dev)
                carry, report, before = s._carry.clone(), s.last_report, s.forwards
                bad = chunk(134, 2)
                bad["ppg"] = bad["ppg"][:, :-1]
                with pytest.raises(ValueError):
                    s.push({a: bad}, end=[a])
                with pytest.raises(ValueError):
                    s.push({a: chunk(134, 2), 99: chunk(0, 1)})
                torch.cuda.synchronize(dev)
                assert s.last_report is report and s.forwards == before and s.totals(a)["windows"] == 1
                assert np.array_equal(_bits(s._carry.cpu().numpy()), _bits(carry.cpu().numpy()))
            out.append(s.push({a: chunk(134, 2)}, end=[a])[a])
            assert model.activation_storage == "float16"
            totals = s.last_report["totals"][a]
            assert [d["window"] for d in s.last_report[a]] == [1, 2]
            with pytest.raises(ValueError):
                s.totals(a)                                    # (the stream has ended: its totals are in the report)
            b = s.open(world.emb)                              # the slot again
            assert s.totals(b)["windows"] == 0 and s.totals(b)["storages"] == {}
            tail = s.push({b: chunk(0, 20)}, end=[b])[b]
            assert s.last_report["totals"][b] == dict(s.last_report["totals"][b], windows=1, fell_back=0, storages={"float16": 1})
            assert [d["storage"] for d in s.last_report[b]] == ["float16"]
        return np.concatenate(out), tail, totals

    y, tail, totals = run(False)
    y2, tail2, totals2 = run(True)
    assert np.isfinite(y).all() and y.size == 72 * hop and np.isfinite(tail).all()
    assert _same(y, y2) and _same(tail, tail2) and totals == totals2
    assert totals["windows"] == 3 and totals["fell_back"] >= 2 and totals["nonfinite"] == 0
    assert totals["storages"].get("bfloat16", 0) == totals["fell_back"]
    with pytest.raises(ValueError, match="checked=True"):
        with Dc.StreamSession(model, world.sg, dev, n_streams=1, core=CORE, fade=FADE, max_push=MAX_PUSH) as s:
            assert s.last_report is None
            s.totals(s.open(world.emb))
