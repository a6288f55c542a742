"""GPU tests (-m gpu) of the resident decode path: the time-major batch assembly and the PCM-16 packing kernels
(csrc/fastsvc_decodeio.hip) bit for bit against numpy, and decode.DecodeSession bit for bit against the existing
decode_utterances + to_pcm16."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd import synth as S

pytestmark = pytest.mark.gpu

TOL = 1e-3          # the bar test_batched_decode_equals_the_reference_decode_loop holds against the live reference's loop


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    A.load_library()
    return torch.device("cuda:0")


def _module(cfg, sd, dev, storage="float32"):
    g = A.FastSVCGenerator(in_channels=cfg.in_channels, mid_channels=list(cfg.mid_channels),
                           upsampling_scales=list(cfg.upsampling_scales), out_channels=cfg.out_channels,
                           spk_emb_size=cfg.spk_emb_size, use_spk_emb=cfg.use_spk_emb)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    g.remove_weight_norm()
    g.activation_storage = storage
    return g.eval().to(dev)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


@pytest.mark.parametrize("B", [1, 64, 65, 130])
@pytest.mark.parametrize("C", [144, 100, 48, 3, 1])
def test_gather_time_major_equals_numpy_transpose(dev, C, B):
    """(x.T, zero-padded), bit-equal: lengths 0, 1, 7 and the full width among random ones, a destination full of NaN,
    source blocks on 16-byte boundaries (the 16-byte read path where C % 4 == 0) and at offsets that are not multiples
    of 4 elements (the element-wise path), widths that are and are not multiples of 4."""
    rng = np.random.default_rng(1000 * C + B)
    for width, aligned in ((128, True), (128, False), (77, False), (77, True), (7, False)):
        lens = [int(v) for v in rng.integers(0, width + 1, B)]
        for j, v in enumerate((width, 0, 1, 7)):
            if j < B:
                lens[(j * 5) % B] = min(v, width)
        if B == 1:
            lens = [width]
        offsets, pos = [], 1 if not aligned else 0
        for b in range(B):
            if aligned:
                pos = (pos + 3) // 4 * 4
            elif pos % 4 == 0:
                pos += 1 + b % 3                             # never a multiple of 4 elements
            offsets.append(pos)
            pos += lens[b] * C
        host = rng.standard_normal(pos + 5).astype(np.float32)
        want = np.zeros((B, C, width), np.float32)
        for b in range(B):
            want[b, :, :lens[b]] = host[offsets[b]: offsets[b] + lens[b] * C].reshape(lens[b], C).T
        packed = torch.from_numpy(host).to(dev)
        out = torch.full((B, C, width), float("nan"), dtype=torch.float32, device=dev)
        got = A.gather_time_major(packed, offsets, lens, C, width, out=out)
        assert got is out
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (C, B, width, aligned)
        if not aligned:
            assert all(o % 4 for o in offsets)
    if B == 1:                                               # the lengths the parametrised batches cannot hold at B = 1
        for n in (0, 1, 7):
            host = rng.standard_normal(3 + n * C).astype(np.float32)
            want = np.zeros((1, C, 16), np.float32)
            want[0, :, :n] = host[3:].reshape(n, C).T
            got = A.gather_time_major(torch.from_numpy(host).to(dev), [3], [n], C, 16,
                                      out=torch.full((1, C, 16), float("nan"), device=dev))
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (C, n)


def test_gather_time_major_rejects_blocks_outside_the_buffer(dev):
    packed = torch.zeros(40, device=dev)
    with pytest.raises(ValueError):
        A.gather_time_major(packed, [0, 30], [5, 5], 4, 8)          # second block ends at 50 > 40
    with pytest.raises(ValueError):
        A.gather_time_major(packed, [0], [9], 4, 8)                 # longer than the width
    with pytest.raises(ValueError):
        A.gather_time_major(packed, [-4], [2], 4, 8)


_NEXT = np.nextafter
_SPECIAL = np.array(
    [0.5, -0.5, 1.5, -1.5, 1.0, -1.0,
     _NEXT(np.float32(1), np.float32(2)), _NEXT(np.float32(1), np.float32(0)),
     _NEXT(np.float32(-1), np.float32(-2)), _NEXT(np.float32(-1), np.float32(0)),
     np.float32(32768.0) / np.float32(32767.0), -np.float32(32768.0) / np.float32(32767.0),
     1e30, -1e30, -0.0, 0.0, 1e-40, -1e-40, 1.4e-45, 1.5 / 32767.0, 2.5 / 32767.0, -2.5 / 32767.0, 1e-5], dtype=np.float32)


def _pack_and_check(dev, y, lens, offsets, total):
    guard = np.int16(0x5A5A)
    out = torch.full((total,), int(guard), dtype=torch.int16, device=dev)
    got = A.pcm16_pack(torch.from_numpy(y).to(dev), lens, offsets, out=out)
    assert got is out
    got = got.cpu().numpy()
    touched = np.zeros(total, bool)
    for b, (n, o) in enumerate(zip(lens, offsets)):
        assert np.array_equal(got[o: o + n], Dc.to_pcm16(y[b, :n])), (b, n, o)
        touched[o: o + n] = True
    assert np.all(got[~touched] == guard)                   # nothing outside the rows was written
    return got


def test_pcm16_pack_equals_to_pcm16(dev):
    """Bit-equal to the host's float64 rint / clip: 10^6 N(0, 0.7^2) samples, the exact ties, the edges of the range,
    row lengths 1 .. 240000 at aligned and at odd destination offsets, with a guard pattern around every row."""
    rng = np.random.default_rng(7)
    # 10^6 samples (four rows back to back, default offsets and output)
    y = rng.normal(0.0, 0.7, (4, 250000)).astype(np.float32)
    got = A.pcm16_pack(torch.from_numpy(y).to(dev), [250000] * 4).cpu().numpy()
    assert got.dtype == np.int16 and got.shape == (10 ** 6,)
    assert np.array_equal(got, Dc.to_pcm16(y))
    assert (np.abs(y) > 1).sum() > 1000                      # (the set does saturate)
    # the ties and edges by value
    want = {0.5: 16384, -0.5: -16384, 1.5: 32767, -1.5: -32768, 1.0: 32767, -1.0: -32767, 1e30: 32767, -1e30: -32768}
    sp = A.pcm16_pack(torch.from_numpy(_SPECIAL[None]).to(dev), [len(_SPECIAL)]).cpu().numpy()
    assert np.array_equal(sp, Dc.to_pcm16(_SPECIAL))
    for v, p in want.items():
        assert sp[list(_SPECIAL).index(np.float32(v))] == p, v
    # row lengths, aligned and odd offsets, guard pattern; every row starts with the special values (as far as it is long)
    lens = [1, 7, 8, 9, 161, 240000]
    width = 240000
    y = rng.normal(0.0, 0.7, (len(lens), width)).astype(np.float32)
    y[:, :len(_SPECIAL)] = _SPECIAL
    y[1, :7] = _SPECIAL[:7][::-1]
    for shift in (0, 8, 1, 3, 4, 5, 7):                      # destination start relative to a 16-byte boundary, in samples
        offsets, pos = [], 16
        for n in lens:
            pos = (pos + 7) // 8 * 8 + shift + 8             # at least 8 guard samples before every row
            offsets.append(pos)
            pos += n
        _pack_and_check(dev, y, lens, offsets, pos + 24)
    # rows back to back at odd lengths: every start lands somewhere else relative to 16 bytes; more than 64 rows
    B = 130
    lens = [int(v) for v in rng.integers(0, 40, B)]
    y = rng.normal(0.0, 0.7, (B, 39)).astype(np.float32)
    offsets = [int(v) for v in np.concatenate([[0], np.cumsum(lens)[:-1]])]
    _pack_and_check(dev, y, lens, offsets, sum(lens))
    _pack_and_check(dev, y, lens, [o + 3 for o in offsets], sum(lens) + 11)
    # a (B, 1, width) waveform batch, as the generator returns it
    got = A.pcm16_pack(torch.from_numpy(y[:, None, :]).to(dev), lens).cpu().numpy()
    assert np.array_equal(got, np.concatenate([Dc.to_pcm16(y[b, :n]) for b, n in enumerate(lens)]))


def test_pcm16_pack_infinities_saturate_and_nan_is_zero(dev):
    y = np.array([[np.inf, -np.inf, np.nan, -np.nan, 0.25, np.nan, np.inf, -np.inf, np.nan, 1.0, -1.0]], dtype=np.float32)
    for shift in (0, 1):                                     # the 16-byte store path and the element path
        out = torch.zeros(y.shape[1] + shift, dtype=torch.int16, device=dev)
        got = A.pcm16_pack(torch.from_numpy(y).to(dev), [y.shape[1]], [shift], out=out).cpu().numpy()[shift:]
        assert list(got) == [32767, -32768, 0, 0, 8192, 0, 32767, -32768, 0, 32767, -32767]


def test_pcm16_pack_rejects_rows_outside_the_buffer(dev):
    y = torch.zeros(2, 8, device=dev)
    with pytest.raises(ValueError):
        A.pcm16_pack(y, [8, 8], [0, 8], out=torch.zeros(15, dtype=torch.int16, device=dev))
    with pytest.raises(ValueError):
        A.pcm16_pack(y, [8, 9])


def _invariance_set(cfg):
    """The 11 utterances of test_pipelined_decode_is_batching_invariant (same seeds)."""
    frames = [31, 7, 25, 26, 18, 40, 12, 33, 9, 21, 38]
    rng = np.random.default_rng(11)
    feats = []
    for f in frames:
        f0 = np.where(rng.random((f, 1)) < 0.3, 0.0, rng.uniform(80, 400, (f, 1)))
        feats.append(dict(f0=f0, ppg=rng.standard_normal((f, cfg.in_channels)).astype(np.float32),
                          lft=rng.uniform(-9, 1, (f * cfg.hop, 1)).astype(np.float32)))
    emb = rng.standard_normal(cfg.spk_emb_size).astype(np.float32)
    return frames, feats, emb


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
def test_session_equals_decode_utterances_bit_for_bit(dev, storage):
    cfg = S.FULL_CONFIG
    frames, feats, emb = _invariance_set(cfg)
    m = _module(cfg, S.synth_state_dict(cfg, 12), dev, storage)
    sg = A.SignalGenerator(sample_rate=24000, hop_size=cfg.hop, sine_amp=0.1, noise_amp=0.0, signal_types=["sine"])
    src = [[5.0, 1.0]] * len(feats)
    for max_batch, tol in ((2, 0.125), (3, 0.9), (16, 0.9)):
        kw = dict(trg_emb=emb, src_f0_stats=src, trg_f0_stats=[5.2, 1.0], max_batch=max_batch, pad_tolerance=tol)
        ref = Dc.decode_utterances(m, feats, sg, dev, **kw)
        again = Dc.decode_utterances(m, feats, sg, dev, **kw)
        assert _same(ref, again), "decode_utterances does not reproduce itself (DESIGN section 7)"
        with Dc.DecodeSession(m, feats, sg, dev, src, max_batch=max_batch, pad_tolerance=tol) as s:
            assert s.batches == list(Dc.bucket_ragged(range(len(feats)), frames, max_batch, tol))
            ys = s.convert(emb, [5.2, 1.0], pcm16=False)
            assert all(y.dtype == np.float32 and y.shape == (f * cfg.hop,) for y, f in zip(ys, frames))
            assert _same(ys, ref), (storage, max_batch)
            pcm = s.convert(emb, [5.2, 1.0])
            assert all(p.dtype == np.int16 for p in pcm)
            assert _same(pcm, [Dc.to_pcm16(y) for y in ref]), (storage, max_batch)


def test_session_converts_many_speakers_from_one_upload(dev):
    cfg = S.FULL_CONFIG
    frames, feats, emb_a = _invariance_set(cfg)
    emb_b = np.random.default_rng(5).standard_normal(cfg.spk_emb_size).astype(np.float32)
    stats_a, stats_b = [5.2, 1.0], [4.7, 1.0]
    m = _module(cfg, S.synth_state_dict(cfg, 12), dev)
    sg = A.SignalGenerator(sample_rate=24000, hop_size=cfg.hop, sine_amp=0.1, noise_amp=0.0, signal_types=["sine"])
    src = [[5.0, 1.0]] * len(feats)
    mb, tol = 3, 0.9
    ref_a = Dc.decode_utterances(m, feats, sg, dev, emb_a, src, stats_a, mb, tol)
    ref_b = Dc.decode_utterances(m, feats, sg, dev, emb_b, src, stats_b, mb, tol)
    assert not _same(ref_a, ref_b)
    with Dc.DecodeSession(m, feats, sg, dev, src, max_batch=mb, pad_tolerance=tol) as s:
        a1 = s.convert(emb_a, stats_a)
        b1 = s.convert(emb_b, stats_b)
        a2 = s.convert(emb_a, stats_a)
        bf = s.convert(emb_b, stats_b, pcm16=False)
        assert _same(a1, [Dc.to_pcm16(y) for y in ref_a])
        assert _same(b1, [Dc.to_pcm16(y) for y in ref_b])
        assert _same(a2, a1)                                 # A, B, A: A's result twice
        assert _same(bf, ref_b)
        # the features went up once, unpadded: ppg + lft of every utterance, nothing else
        assert s.uploaded_bytes["init"] == 4 * sum(frames) * (cfg.in_channels + cfg.hop)
        # every convert uploads F0-sized data only: the padded f0 of every batch, the embedding, and at most 32 bytes
        # of descriptors per utterance (here none: the descriptors travel in kernel arguments)
        padded_f0 = 4 * sum(len(chunk) * frames[chunk[0]] for chunk in s.batches)
        bound = padded_f0 + 4 * cfg.spk_emb_size + 32 * len(feats)
        assert len(s.uploaded_bytes["convert"]) == 4
        for n in s.uploaded_bytes["convert"]:
            assert 0 < n <= bound, (n, bound)
        assert padded_f0 < 0.01 * s.uploaded_bytes["init"]
    with pytest.raises(RuntimeError):
        s.convert(emb_a, stats_a)


def test_session_without_speaker_or_shift_and_past_the_launch_limit(dev):
    """No embedding and no F0 shift (the defaults), and a batch of more than 64 utterances (two launches of each new
    kernel inside the session)."""
    cfg = S.FULL_CONFIG
    rng = np.random.default_rng(21)
    frames = [int(v) for v in rng.integers(6, 9, 70)]
    feats = []
    for f in frames:
        f0 = np.where(rng.random((f, 1)) < 0.3, 0.0, rng.uniform(80, 400, (f, 1)))
        feats.append(dict(f0=f0, ppg=rng.standard_normal((f, cfg.in_channels)).astype(np.float32),
                          lft=rng.uniform(-9, 1, (f * cfg.hop, 1)).astype(np.float32)))
    m = _module(cfg, S.synth_state_dict(cfg, 12), dev)
    sg = A.SignalGenerator(sample_rate=24000, hop_size=cfg.hop, sine_amp=0.1, noise_amp=0.0, signal_types=["sine"])
    ref = Dc.decode_utterances(m, feats, sg, dev, max_batch=128, pad_tolerance=0.9)
    with Dc.DecodeSession(m, feats, sg, dev, max_batch=128, pad_tolerance=0.9) as s:
        assert len(s.batches) == 1 and len(s.batches[0]) == 70
        assert _same(s.convert(pcm16=False), ref)
        assert _same(s.convert(), [Dc.to_pcm16(y) for y in ref])


def test_session_on_the_reference_decode_chain(dev):
    """tests/golden/decode_chain.npz (the live reference's one-utterance-at-a-time loop) through a session."""
    g = load_golden("decode_chain.npz")
    cfg = S.FULL_CONFIG
    seed_w = int(g["meta"][0])
    frames = [int(v) for v in g["frames"]]
    batches = [S.synth_batch(cfg, 1, F, 400 + i) for i, F in enumerate(frames)]
    feats = [dict(f0=b.f0[0].T.copy(), ppg=b.ppg[0].T.copy(), lft=b.lft[0].T.copy()) for b in batches]
    m = _module(cfg, S.synth_state_dict(cfg, seed_w), dev)
    sg = A.SignalGenerator(sample_rate=24000, hop_size=cfg.hop, sine_amp=0.1, noise_amp=0.0, signal_types=["sine"])
    with Dc.DecodeSession(m, feats, sg, dev, [g["srcstats"]] * 3, max_batch=8, pad_tolerance=0.9) as s:
        ys = s.convert(batches[0].spk_emb, g["trgstats"], pcm16=False)
        pcm = s.convert(batches[0].spk_emb, g["trgstats"])
    for i, y in enumerate(ys):
        want = g[f"y.{i}"]
        assert y.shape == want.shape
        assert float(np.abs(y - want).max()) <= TOL, i
        assert pcm[i].dtype == np.int16 and np.array_equal(pcm[i], Dc.to_pcm16(y))
