"""GPU tests (-m gpu) of the checked decode path: the checked PCM-16 packing and the output check
(csrc/fastsvc_decodeio.hip) against the unchecked packing byte for byte and against decode.output_report bit for bit, and
decode.DecodeSession(checked=True) against unchecked sessions in the storages involved, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd import synth as S

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A
SPECIALS = [np.nan, np.inf, -np.inf, 1.0, -1.0, 1.0001, -1.0001]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    A.load_library()
    return torch.device("cuda:0")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_bits(x), _bits(y))
                                    for x, y in zip(a, b))


def _pcm(v):
    """to_pcm16 with the device's NaN -> 0 (the host's conversion of a NaN is implementation-defined)."""
    return Dc.to_pcm16(np.where(np.isnan(v), np.float32(0), v))


def _want_report(y, lens):
    """decode.output_report as the (B, 4) int32 table the device writes (max_abs as its bit pattern, reserved 0)."""
    nf, cl, mx = Dc.output_report(y, lens)
    return np.stack([nf, cl, mx.view(np.int32), np.zeros_like(nf)], axis=1)


# ---------------------------------------------------------------------------------------------- the two kernels
WIDTH = 4104
LENS = [0, 1, 7, 8, 9, 2047, 2048, 2049, 4097, 4104]


@pytest.fixture(scope="module")
def rows(dev):
    """The rows of tests 1 - 3: hash-generator samples in [-1.2, 1.2]; every row's first and last valid sample and the
    sample just past len are special values; y is a view 4 bytes into a larger buffer (never 16-byte aligned); the rows are
    packed back to back from element 3 of dst, where no row of these lengths starts on a 16-byte boundary (asserted by the
    byte test)."""
    B = len(LENS)
    y = (S.hash_uniform(77, 5, B * WIDTH) * 2.4 - 1.2).astype(np.float32).reshape(B, WIDTH)
    j = 0
    for b, n in enumerate(LENS):
        for k in sorted({0, n - 1, n}):
            if 0 <= k < WIDTH:
                y[b, k] = SPECIALS[j % len(SPECIALS)]
                j += 1
    offsets, pos = [], 3
    for n in LENS:
        offsets.append(pos)
        pos += n
    total = pos + 13
    buf = torch.zeros(B * WIDTH + 1, dtype=torch.float32, device=dev)
    yd = buf[1:].view(B, WIDTH)
    yd.copy_(torch.from_numpy(y))
    assert yd.data_ptr() % 16 == 4 and yd.is_contiguous()
    assert np.isnan(y[0, 0]) and LENS[0] == 0                  # (a special value just past a len of 0)
    return y, yd, offsets, total


def _dst(dev, total):
    return torch.full((total,), GUARD, dtype=torch.int16, device=dev)


def test_checked_pack_writes_the_bytes_of_the_unchecked_pack(dev, rows):
    y, yd, offsets, total = rows
    d0, d1 = _dst(dev, total), _dst(dev, total)
    for d in (d0, d1):                                         # no row on a 16-byte boundary
        assert all((d.data_ptr() + 2 * o) % 16 for o, n in zip(offsets, LENS) if n)
    plain = A.pcm16_pack(yd, LENS, offsets, out=d0)
    report = torch.empty((len(LENS), 4), dtype=torch.int32, device=dev)
    checked = A.pcm16_pack(yd, LENS, offsets, out=d1, report=report)
    assert plain is d0 and checked is d1
    plain, checked = plain.cpu().numpy(), checked.cpu().numpy()
    assert plain.tobytes() == checked.tobytes()                # raw bytes, the guard pattern around the rows included
    touched = np.zeros(total, bool)
    for b, (n, o) in enumerate(zip(LENS, offsets)):
        assert np.array_equal(checked[o: o + n], _pcm(y[b, :n])), b
        touched[o: o + n] = True
    assert np.all(checked[~touched] == GUARD)


def test_reports_equal_the_host_reference_bit_for_bit(dev, rows):
    y, yd, offsets, total = rows
    want = _want_report(y, LENS)
    assert want[:, 0].sum() > 0 and want[:, 1].sum() > 100 and (want[:, 0] == 0).any()      # (the set exercises every field)
    report = torch.empty((len(LENS), 4), dtype=torch.int32, device=dev)
    A.pcm16_pack(yd, LENS, offsets, out=_dst(dev, total), report=report)
    assert np.array_equal(report.cpu().numpy(), want)
    got = A.output_check(yd, LENS)
    assert got.shape == (len(LENS), 4) and got.dtype == torch.int32 and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)
    nf, cl, mx = A.report_arrays(got)
    hn, hc, hm = Dc.output_report(y, LENS)
    assert np.array_equal(nf, hn) and np.array_equal(cl, hc) and np.array_equal(mx.view(np.uint32), hm.view(np.uint32))
    # a 16-byte aligned source takes the other load path: the same report
    aligned = yd.clone()
    assert aligned.data_ptr() % 16 == 0
    assert np.array_equal(A.output_check(aligned, LENS).cpu().numpy(), want)


def test_clipping_is_decided_exactly_at_the_edges_of_the_int16_range(dev):
    """The floats around the two ties (32767.5 / 32767 and -32768.5 / 32767, seven on each side of each), +-1, the powers
    of two next to them, the largest finite floats: one sample per row, so that every decision shows in its own count."""
    f32 = np.float32
    vals = [1.0, -1.0, 1 + 2.0 ** -14, 1 + 2.0 ** -15, -1 - 2.0 ** -15, -1 - 2.0 ** -14, 3.4e38, -3.4e38, 0.0, -0.0, 1e-45]
    for tie in (f32(32767.5) / f32(32767.0), f32(-32768.5) / f32(32767.0)):
        lo = hi = tie
        vals.append(tie)
        for _ in range(7):
            lo, hi = np.nextafter(lo, f32(0)), np.nextafter(hi, f32(np.sign(tie) * 2))
            vals += [lo, hi]
    y = np.zeros((len(vals), 9), f32)
    y[:, 4] = np.array(vals, f32)
    lens = [9] * len(vals)
    want = _want_report(y, lens)
    assert 14 <= want[:, 1].sum() <= len(vals) - 14                               # (both sides of both edges are there)
    yd = torch.from_numpy(y).to(dev)
    assert np.array_equal(A.output_check(yd, lens).cpu().numpy(), want)
    report = torch.empty((len(vals), 4), dtype=torch.int32, device=dev)
    pcm = A.pcm16_pack(yd, lens, report=report).cpu().numpy()
    assert np.array_equal(report.cpu().numpy(), want)
    assert np.array_equal(pcm, Dc.to_pcm16(y))


def test_every_call_overwrites_the_report(dev, rows):
    y, yd, offsets, total = rows
    want = _want_report(y, LENS)
    for run in (lambda r: A.pcm16_pack(yd, LENS, offsets, out=_dst(dev, total), report=r),
                lambda r: A.output_check(yd, LENS, out=r)):
        report = torch.full((len(LENS), 4), 0x7F7F7F7F, dtype=torch.int32, device=dev)
        run(report)
        first = report.cpu().numpy().copy()
        run(report)
        assert np.array_equal(first, want) and np.array_equal(report.cpu().numpy(), want)


def test_rows_past_64_report_from_a_second_launch(dev):
    B, width = 65, 80
    lens = [5 + b % 65 for b in range(B)]
    assert min(lens) == 5 and max(lens) == 69
    y = (S.hash_uniform(78, 5, B * width) * 2.4 - 1.2).astype(np.float32).reshape(B, width)
    for b in (0, 63, 64):
        y[b, lens[b] // 2] = np.nan
    want = _want_report(y, lens)
    assert list(np.nonzero(want[:, 0])[0]) == [0, 63, 64]
    yd = torch.from_numpy(y).to(dev)
    for pack in (True, False):
        table = torch.full((B + 1, 4), 0x7F7F7F7F, dtype=torch.int32, device=dev)    # entry 65: a guard
        if pack:
            pcm = A.pcm16_pack(yd, lens, report=table[:B]).cpu().numpy()
            assert np.array_equal(pcm, np.concatenate([_pcm(y[b, :n]) for b, n in enumerate(lens)]))
        else:
            A.output_check(yd, lens, out=table[:B])
        got = table.cpu().numpy()
        assert np.array_equal(got[:B], want), pack
        assert np.all(got[B] == 0x7F7F7F7F), pack              # nothing past entry 64 is written


def test_bad_arguments_are_invalid_and_write_nothing(dev):
    lib = A.load_library()
    B, width = 2, 16
    y = torch.ones(B, width, device=dev) * 3
    dst = _dst(dev, 40)
    report = torch.full((B, 4), 0x7F7F7F7F, dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    vp = ctypes.c_void_p

    def pack(lens, offsets, dst_elems, rep):
        return lib.fastsvc_pcm16_pack_checked(vp(y.data_ptr()), (ctypes.c_int32 * B)(*lens), (ctypes.c_int64 * B)(*offsets),
                                              vp(dst.data_ptr()), dst_elems, rep, B, width, stream)

    def check(lens, rep):
        return lib.fastsvc_output_check(vp(y.data_ptr()), (ctypes.c_int32 * B)(*lens), rep, B, width, stream)

    INVALID = -1                                               # FASTSVC_E_INVALID
    rep = vp(report.data_ptr())
    assert pack([16, 16], [0, 16], 40, None) == INVALID        # a null report
    assert check([16, 16], None) == INVALID
    assert pack([16, 17], [0, 16], 40, rep) == INVALID         # a len greater than the width
    assert check([16, 17], rep) == INVALID
    assert pack([16, -1], [0, 16], 40, rep) == INVALID
    assert pack([16, 16], [0, 25], 40, rep) == INVALID         # a row leaving dst_elems
    assert pack([16, 16], [-1, 16], 40, rep) == INVALID
    torch.cuda.synchronize(dev)
    assert np.all(dst.cpu().numpy() == GUARD) and np.all(report.cpu().numpy() == 0x7F7F7F7F)
    assert pack([16, 16], [0, 24], 40, rep) == 0               # (the same call with good arguments does write)
    torch.cuda.synchronize(dev)
    assert np.array_equal(report.cpu().numpy(), _want_report(y.cpu().numpy(), [16, 16]))
    with pytest.raises(ValueError):                            # and through the binding
        A.pcm16_pack(y, [16, 17], report=torch.empty((B, 4), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        A.pcm16_pack(y, [16, 16], report=torch.empty((B, 3), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        A.output_check(y, [16, 17])


# ---------------------------------------------------------------------------------------------- the session
FRAMES = [9, 12, 12, 20, 33]
LOUD = [1, 4]                      # the utterances whose ppg and lft are scaled out of float16 storage's range
SCALE = 2.0 ** 12
MAX_BATCH = 2
TRG = [5.2, 1.0]


def _module(cfg, sd, dev, storage):
    g = A.FastSVCGenerator(in_channels=cfg.in_channels, mid_channels=list(cfg.mid_channels),
                           upsampling_scales=list(cfg.upsampling_scales), out_channels=cfg.out_channels,
                           spk_emb_size=cfg.spk_emb_size, use_spk_emb=cfg.use_spk_emb)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    g.remove_weight_norm()
    g.activation_storage = storage
    return g.eval().to(dev)


def _features(cfg, scale):
    rng = np.random.default_rng(31)
    feats = []
    for i, f in enumerate(FRAMES):
        f0 = np.where(rng.random((f, 1)) < 0.3, 0.0, rng.uniform(80, 400, (f, 1)))
        k = np.float32(scale if i in LOUD else 1.0)
        feats.append(dict(f0=f0, ppg=rng.standard_normal((f, cfg.in_channels)).astype(np.float32) * k,
                          lft=rng.uniform(-9, 1, (f * cfg.hop, 1)).astype(np.float32) * k))
    emb = rng.standard_normal(cfg.spk_emb_size).astype(np.float32)
    return feats, emb


class _World:
    pass


@pytest.fixture(scope="module")
def world(dev):
    """Models in the two storages, the scaled and the plain utterances, and what UNCHECKED sessions return for them -
    computed once, shared by the session tests and left unchanged."""
    w = _World()
    cfg = w.cfg = S.FULL_CONFIG
    sd = S.synth_state_dict(cfg, 12)
    w.models = {st: _module(cfg, sd, dev, st) for st in ("float16", "bfloat16")}
    w.sg = A.SignalGenerator(sample_rate=24000, hop_size=cfg.hop, sine_amp=0.1, noise_amp=0.0, signal_types=["sine"])
    w.src = [[5.0, 1.0]] * len(FRAMES)
    w.loud, w.emb = _features(cfg, SCALE)
    w.plain, _ = _features(cfg, 1.0)
    w.ref = {}
    for name, feats in (("loud", w.loud), ("plain", w.plain)):
        for st in (("float16", "bfloat16") if name == "loud" else ("float16",)):
            with Dc.DecodeSession(w.models[st], feats, w.sg, dev, w.src, max_batch=MAX_BATCH) as s:
                w.batches = s.batches
                w.ref[name, st, False] = s.convert(w.emb, TRG, pcm16=False)
                w.ref[name, st, True] = s.convert(w.emb, TRG)
                w.uploaded = s.uploaded_bytes["convert"][-1]
    return w


def _session(w, dev, feats, **kw):
    return Dc.DecodeSession(w.models["float16"], feats, w.sg, dev, w.src, max_batch=MAX_BATCH, checked=True, **kw)


def test_premise_float16_overflows_on_exactly_the_scaled_utterances(world):
    """What the session tests rest on, with unchecked sessions: scaled by SCALE, utterances LOUD - and only they - come
    out of float16 storage non-finite, and every utterance comes out of bfloat16 storage finite."""
    w = world
    bad16 = [i for i, y in enumerate(w.ref["loud", "float16", False]) if not np.isfinite(y).all()]
    badbf = [i for i, y in enumerate(w.ref["loud", "bfloat16", False]) if not np.isfinite(y).all()]
    print("non-finite utterances: float16", bad16, "bfloat16", badbf)
    assert bad16 == LOUD and badbf == []
    assert all(np.isfinite(y).all() for y in w.ref["plain", "float16", False])
    # (and one batch holds a scaled and a plain utterance side by side: its plain row must stay float16's)
    assert any(any(i in LOUD for i in chunk) and any(i not in LOUD for i in chunk) for chunk in w.batches)


@pytest.mark.parametrize("pcm16", [True, False])
def test_checked_session_replaces_exactly_the_flagged_rows(dev, world, pcm16):
    w = world
    f16, bf = w.ref["loud", "float16", pcm16], w.ref["loud", "bfloat16", pcm16]
    with _session(w, dev, w.loud) as s:
        got = s.convert(w.emb, TRG, pcm16=pcm16)
        report, forwards = s.last_report, s.forwards
        assert w.models["float16"].activation_storage == "float16"
        again = s.convert(w.emb, TRG, pcm16=pcm16)
        assert s.last_report == report and s.forwards == forwards
    assert _same(got, again)                                                       # a second convert: the same bytes
    for i in range(len(FRAMES)):
        want = bf if i in LOUD else f16
        assert _same([got[i]], [want[i]]), i                                       # contracts B / A
        r = report[i]
        assert r["storage"] == ("bfloat16" if i in LOUD else "float16") and r["tried"] == (["float16"] if i in LOUD else []), i
        # contract C: the report is output_report of the float32 waveform of the returned rows
        nf, cl, mx = Dc.output_report([w.ref["loud", r["storage"], False][i]])
        assert (r["nonfinite"], r["clipped"]) == (int(nf[0]), int(cl[0])), i
        assert np.float32(r["max_abs"]).view(np.uint32) == mx.view(np.uint32)[0], i
        assert r["nonfinite"] == 0
    rerun = sum(1 for chunk in s.batches if any(i in LOUD for i in chunk))
    assert s.batches == w.batches and 0 < rerun < len(s.batches)
    assert forwards == len(s.batches) + rerun


def test_checked_session_with_nothing_to_do_is_the_unchecked_one(dev, world):
    w = world
    with _session(w, dev, w.plain) as s:
        pcm = s.convert(w.emb, TRG)
        assert s.forwards == len(s.batches)
        assert s.uploaded_bytes["convert"] == [w.uploaded]
        assert all(r["nonfinite"] == 0 and r["storage"] == "float16" and r["tried"] == [] for r in s.last_report)
        ys = s.convert(w.emb, TRG, pcm16=False)
        assert s.forwards == len(s.batches) and s.uploaded_bytes["convert"] == [w.uploaded] * 2
        nf, cl, mx = Dc.output_report(ys)
        for i, r in enumerate(s.last_report):
            assert (r["nonfinite"], r["clipped"], np.float32(r["max_abs"])) == (0, int(cl[i]), mx[i]), i
    assert _same(pcm, w.ref["plain", "float16", True]) and _same(ys, w.ref["plain", "float16", False])


def test_exhausted_fallback_returns_the_last_result_and_says_so(dev, world):
    w = world
    with _session(w, dev, w.loud, fallback=()) as s:
        for pcm16 in (True, False):
            got = s.convert(w.emb, TRG, pcm16=pcm16)
            assert _same(got, w.ref["loud", "float16", pcm16])
            assert s.forwards == len(s.batches)
            for i, r in enumerate(s.last_report):
                assert (r["nonfinite"] > 0) == (i in LOUD) and r["storage"] == "float16" and r["tried"] == [], i
    with _session(w, dev, w.loud, fallback=(), strict=True) as s:
        with pytest.raises(A.FastSVCError, match=r"\[1, 4\]"):
            s.convert(w.emb, TRG)
        assert [i for i, r in enumerate(s.last_report) if r["nonfinite"]] == LOUD
    assert w.models["float16"].activation_storage == "float16"
