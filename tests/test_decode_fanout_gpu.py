"""GPU tests (-m gpu) of the speaker fan-out of the resident decode path: the batch assembly kernel
(csrc/fastsvc_fanout.hip) against numpy, and decode.DecodeSession.convert_many against a hand-made oracle bit for bit,
against sequential converts, in its upload accounting and in a checked session."""
import numpy as np
import pytest
import torch

import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd import synth as S
import range_cases as RC

pytestmark = pytest.mark.gpu


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
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_bits(x), _bits(y))
                                    for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- the kernel
def _store(rng, frames, C, hop, aligned):
    """Packed ppg / lft / f0 buffers with the blocks on 16-byte boundaries (aligned) or never on one; utterance 1 has one
    frame, utterance 2 is all unvoiced."""
    offs = {"ppg": [], "lft": [], "f0": []}
    pos = {"ppg": 0, "lft": 0, "f0": 0} if aligned else {"ppg": 1, "lft": 3, "f0": 2}
    for u, n in enumerate(frames):
        for key, count in (("ppg", n * C), ("lft", n * hop), ("f0", n)):
            if aligned:
                pos[key] = (pos[key] + 3) // 4 * 4
            elif pos[key] % 4 == 0:
                pos[key] += 1 + u % 3                          # never a multiple of 4 elements
            offs[key].append(pos[key])
            pos[key] += count
    ppg = rng.standard_normal(pos["ppg"] + 5).astype(np.float32)
    lft = rng.uniform(-9, 1, pos["lft"] + 5).astype(np.float32)
    f0 = np.where(rng.random(pos["f0"] + 5) < 0.3, 0.0, rng.uniform(60, 900, pos["f0"] + 5)).astype(np.float32)
    f0[offs["f0"][2]: offs["f0"][2] + frames[2]] = 0.0
    f0[offs["f0"][0]] = 123.25                                 # (utterance 0 and the 1-frame utterance start voiced)
    f0[offs["f0"][1]] = 440.0
    return ppg, lft, f0, offs


def _stats(rng, n, unit_std):
    std = np.ones(n) if unit_std else rng.uniform(0.1, 0.6, n)
    return np.stack([rng.uniform(4.5, 6.0, n), std], axis=1)


@pytest.mark.parametrize("R", [1, 64, 65, 130])
@pytest.mark.parametrize("C,hop,E", [(144, 160, 512), (3, 5, 7)])
@pytest.mark.parametrize("n_spk", [1, 3])
def test_fanout_assemble_equals_numpy(dev, R, C, hop, E, n_spk):
    """Rows across the 64-row launch boundary; ppg, lft, emb and every padded element bit-exact in destinations full of
    NaN; f0 exactly 0 where unvoiced or padded and, where voiced, within 1 float32 ulp of F0Statistics.convert assigned
    to float32 - both sides round a double whose error is a few double ulps to float32, so the results differ by at
    most one step (a bound from the formats, not from this kernel's output); with no statistics f0 is bit-exact."""
    rng = np.random.default_rng(10000 * R + 100 * C + n_spk)
    for width, aligned, unit_std in ((77, True, True), (77, False, False), (130, False, True), (7, True, False)):
        frames = [width, 1, min(9, width), min(33, width), min(64, width), min(65, width), max(width - 1, 1)]
        U = len(frames)
        ppg, lft, f0, offs = _store(rng, frames, C, hop, aligned)
        src, trg = _stats(rng, U, unit_std), _stats(rng, n_spk, unit_std)
        table = rng.standard_normal((n_spk, E)).astype(np.float32)
        utt = [r % U for r in range(R)] if R > 1 else [0]
        spk = [(r * 5 + r // U) % n_spk for r in range(R)]
        want_ppg = np.zeros((R, C, width), np.float32)
        want_lft = np.zeros((R, 1, width * hop), np.float32)
        want_raw = np.zeros((R, 1, width), np.float32)
        want_f0 = np.zeros((R, 1, width), np.float32)
        for r, (u, s) in enumerate(zip(utt, spk)):
            n = frames[u]
            want_ppg[r, :, :n] = ppg[offs["ppg"][u]: offs["ppg"][u] + n * C].reshape(n, C).T
            want_lft[r, 0, : n * hop] = lft[offs["lft"][u]: offs["lft"][u] + n * hop]
            f = f0[offs["f0"][u]: offs["f0"][u] + n]
            want_raw[r, 0, :n] = f
            want_f0[r, 0, :n] = Dc.F0Statistics().convert(f.astype(np.float64), src[u], trg[s])
        d = {k: torch.from_numpy(v).to(dev) for k, v in (("ppg", ppg), ("lft", lft), ("f0", f0), ("emb", table))}
        d_src, d_trg = torch.from_numpy(src).to(dev), torch.from_numpy(trg).to(dev)
        if not aligned:
            assert all(o % 4 for key in offs for o in offs[key])
        shapes = [(R, C, width), (R, 1, width * hop), (R, 1, width), (R, E)]
        for shifted in (False, True):
            out = [torch.full(shp, float("nan"), dtype=torch.float32, device=dev) for shp in shapes]
            got = A.fanout_assemble(d["ppg"], d["lft"], d["f0"], offs["ppg"], offs["lft"], offs["f0"], frames, utt, spk,
                                    C, hop, width, src_stats=d_src if shifted else None, spk_stats=d_trg,
                                    spk_emb=d["emb"], out=out)
            assert all(g is o for g, o in zip(got, out))
            g_ppg, g_lft, g_f0, g_emb = (t.cpu().numpy() for t in got)
            tag = (R, C, hop, E, n_spk, width, aligned, shifted)
            assert np.array_equal(_bits(g_ppg), _bits(want_ppg)), tag
            assert np.array_equal(_bits(g_lft), _bits(want_lft)), tag
            assert np.array_equal(_bits(g_emb), _bits(table[spk])), tag
            if not shifted:                                    # (one table missing: a copy)
                assert np.array_equal(_bits(g_f0), _bits(want_raw)), tag
                continue
            voiced = want_raw > 0
            assert voiced.any() and (~voiced).any()
            assert np.all(_bits(g_f0)[~voiced] == 0), tag      # unvoiced and padded: exactly +0
            steps = np.abs(_bits(g_f0)[voiced].astype(np.int64) - _bits(want_f0)[voiced].astype(np.int64))
            print(f"fanout f0 {tag}: {int(voiced.sum())} voiced frames, largest distance {int(steps.max())} ulp, "
                  f"{int((steps > 0).sum())} differ")
            assert steps.max() <= 1, tag
        # without an embedding table nothing is returned for it, and the other three do not change
        got = A.fanout_assemble(d["ppg"], d["lft"], d["f0"], offs["ppg"], offs["lft"], offs["f0"], frames, utt, spk,
                                C, hop, width, src_stats=d_src, spk_stats=d_trg)
        assert got[3] is None and np.array_equal(_bits(got[0].cpu().numpy()), _bits(want_ppg))
        assert np.array_equal(_bits(got[2].cpu().numpy()), _bits(g_f0))


def test_fanout_assemble_rejects_bad_rows_and_writes_nothing(dev):
    C, hop, width, E = 4, 2, 8, 3
    frames = [5, 8]
    ppg, lft, f0 = (torch.zeros(n, device=dev) for n in (13 * C, 13 * hop, 13))
    emb = torch.ones(2, E, device=dev)
    shapes = [(2, C, width), (2, 1, width * hop), (2, 1, width), (2, E)]
    out = [torch.full(shp, 7.0, device=dev) for shp in shapes]

    def call(ppg_off=(0, 5 * C), lft_off=(0, 5 * hop), f0_off=(0, 5), n_frames=frames, utt=(0, 1), spk=(0, 1), w=width):
        return A.fanout_assemble(ppg, lft, f0, list(ppg_off), list(lft_off), list(f0_off), list(n_frames), list(utt),
                                 list(spk), C, hop, w, spk_emb=emb, out=out)

    bad = {"a ppg block outside its buffer": dict(ppg_off=(0, 6 * C)),            # ends at 14 C > 13 C
           "an lft block outside its buffer": dict(lft_off=(0, 6 * hop)),
           "an f0 block outside its buffer": dict(f0_off=(0, 6)),
           "a negative offset": dict(f0_off=(-1, 5)),
           "utt out of range": dict(utt=(0, 2)),
           "utt negative": dict(utt=(-1, 1)),
           "spk out of range": dict(spk=(0, 2)),
           "frames > width": dict(n_frames=(5, 9), ppg_off=(0, 0), lft_off=(0, 0), f0_off=(0, 0))}
    for what, kw in bad.items():
        with pytest.raises(ValueError, match=r"fastsvc_fanout_assemble: row 1|fastsvc_fanout_assemble: row 0"):
            call(**kw)
        torch.cuda.synchronize(dev)
        assert all(bool((t == 7.0).all()) for t in out), what
    lib = A.load_library()
    assert lib.fastsvc_fanout_launch_count(130) == 3
    got = call()                                               # (the same call with good arguments does write)
    torch.cuda.synchronize(dev)
    assert not any(bool((t == 7.0).any()) for t in got)


# ---------------------------------------------------------------------------------------------- the session
FRAMES = [9, 12, 12, 20, 33]
N_SPK = 3
MAX_BATCH, TOL = 4, 0.9
SRC = [[5.0, 1.0], [4.8, 1.0], [5.1, 0.4], [5.0, 1.0], [5.3, 0.5]]
TRG = [[5.2, 1.0], [4.7, 1.0], [5.5, 0.3]]


class _World:
    pass


def _features(cfg, frames, seed=31):
    rng = np.random.default_rng(seed)
    feats = []
    for f in frames:
        f0 = np.where(rng.random((f, 1)) < 0.3, 0.0, rng.uniform(80, 400, (f, 1)))
        feats.append(dict(f0=f0, ppg=rng.standard_normal((f, cfg.in_channels)).astype(np.float32),
                          lft=rng.uniform(-9, 1, (f * cfg.hop, 1)).astype(np.float32)))
    embs = [rng.standard_normal(cfg.spk_emb_size).astype(np.float32) for _ in range(N_SPK)]
    return feats, embs


def _sg(cfg, noise_amp, seed=5):
    return A.SignalGenerator(sample_rate=24000, hop_size=cfg.hop, sine_amp=0.1, noise_amp=noise_amp,
                             signal_types=["sine"], seed=seed)


@pytest.fixture(scope="module")
def world(dev):
    w = _World()
    cfg = w.cfg = S.FULL_CONFIG
    sd = S.synth_state_dict(cfg, 12)
    w.models = {st: _module(cfg, sd, dev, st) for st in ("float32", "bfloat16")}
    w.feats, w.embs = _features(cfg, FRAMES)
    return w


@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
@pytest.mark.parametrize("shift", [True, False])
def test_convert_many_equals_a_hand_made_pass_bit_for_bit(dev, world, storage, shift):
    """What convert_many promises, spelled out with the package's own pieces: for every batch of fanout_batches, in
    order, fanout_assemble -> SignalGenerator (a fresh one of the same seed: the noise is seeded per call) -> the model
    -> pcm16_pack; every returned array equal."""
    w, cfg = world, world.cfg
    m, hop, C = w.models[storage], cfg.hop, cfg.in_channels
    speakers = [(w.embs[s], TRG[s] if shift else None) for s in range(N_SPK)]
    with Dc.DecodeSession(m, w.feats, _sg(cfg, 0.003), dev, SRC, max_batch=MAX_BATCH, pad_tolerance=TOL) as s:
        got_pcm = s.convert_many(speakers)
    with Dc.DecodeSession(m, w.feats, _sg(cfg, 0.003), dev, SRC, max_batch=MAX_BATCH, pad_tolerance=TOL) as s:
        got_f32 = s.convert_many(speakers, pcm16=False)
    # the oracle's own store: the utterances back to back in their given order (any layout serves the kernel)
    ppg = np.concatenate([u["ppg"].reshape(-1) for u in w.feats]).astype(np.float32)
    lft = np.concatenate([u["lft"].reshape(-1)[: f * hop] for u, f in zip(w.feats, FRAMES)]).astype(np.float32)
    f0 = np.concatenate([u["f0"].reshape(-1) for u in w.feats]).astype(np.float32)
    f0_off = [int(v) for v in np.concatenate([[0], np.cumsum(FRAMES)[:-1]])]
    d_ppg, d_lft, d_f0 = (torch.from_numpy(a).to(dev) for a in (ppg, lft, f0))
    d_src = torch.from_numpy(np.asarray(SRC, np.float64)).to(dev)
    d_trg = torch.from_numpy(np.asarray(TRG, np.float64)).to(dev)
    d_emb = torch.from_numpy(np.stack(w.embs)).to(dev)
    batches = Dc.fanout_batches(FRAMES, N_SPK, MAX_BATCH, TOL)
    assert len(batches) >= 4 and any(len({u for u, _ in chunk}) > 1 for chunk in batches)
    for pcm16, got in ((True, got_pcm), (False, got_f32)):
        sg = _sg(cfg, 0.003)
        seen = set()
        for chunk in batches:
            utt, spk = [u for u, _ in chunk], [sp for _, sp in chunk]
            lens, width = [FRAMES[u] for u in utt], FRAMES[utt[0]]
            b_ppg, b_lft, b_f0, b_emb = A.fanout_assemble(
                d_ppg, d_lft, d_f0, [o * C for o in f0_off], [o * hop for o in f0_off], f0_off, FRAMES, utt, spk, C, hop,
                width, src_stats=d_src if shift else None, spk_stats=d_trg if shift else None, spk_emb=d_emb)
            with torch.no_grad():
                y = m(b_ppg, sg(b_f0), b_lft, b_emb, lengths=lens).to(torch.float32)
            if pcm16:
                rows = A.pcm16_pack(y, [n * hop for n in lens]).cpu().numpy()
                rows = np.split(rows, np.cumsum([n * hop for n in lens])[:-1])
            else:
                rows = [y[j].reshape(-1)[: n * hop].cpu().numpy() for j, n in enumerate(lens)]
            for (u, sp), row in zip(chunk, rows):
                assert _same([got[sp][u]], [row]), (storage, shift, pcm16, u, sp)
                seen.add((u, sp))
        assert len(seen) == len(FRAMES) * N_SPK
    assert all(p.dtype == np.int16 for row in got_pcm for p in row)
    assert all(y.dtype == np.float32 and y.shape == (f * hop,) for row in got_f32 for y, f in zip(row, FRAMES))


def test_one_speaker_without_a_shift_is_convert_bit_for_bit(dev, world):
    """Identical batches, the same excitation calls in the same order (fresh generators of equal seed, noise on)."""
    w, cfg = world, world.cfg
    for storage in ("float32", "bfloat16"):
        m = w.models[storage]
        with Dc.DecodeSession(m, w.feats, _sg(cfg, 0.003), dev, SRC, max_batch=MAX_BATCH, pad_tolerance=TOL) as s:
            want = s.convert(w.embs[1])
        with Dc.DecodeSession(m, w.feats, _sg(cfg, 0.003), dev, SRC, max_batch=MAX_BATCH, pad_tolerance=TOL) as s:
            got = s.convert_many([(w.embs[1], None)])
            assert Dc.fanout_batches(FRAMES, 1, MAX_BATCH, TOL) == [[(i, 0) for i in chunk] for chunk in s.batches]
        assert len(got) == 1 and got[0][0].dtype == np.int16 and _same(got[0], want), storage
        assert any(np.abs(p).max() > 0 for p in want)


def test_fanout_agrees_with_sequential_converts_within_the_batching_invariance(dev, world):
    """Other batches, so not bit-equal: the bound is the harness's batching invariance of float32 storage
    (tests/test_parity_gpu.py: 2e-5 x max(1, |ref| max))."""
    w, cfg = world, world.cfg
    m = w.models["float32"]
    with Dc.DecodeSession(m, w.feats, _sg(cfg, 0.0), dev, SRC, max_batch=MAX_BATCH, pad_tolerance=TOL) as s:
        want = [s.convert(e, pcm16=False) for e in w.embs]
        got = s.convert_many([(e, None) for e in w.embs], pcm16=False)
    worst = 0.0
    for sp in range(N_SPK):
        for u in range(len(FRAMES)):
            ref = want[sp][u]
            err = float(np.abs(got[sp][u] - ref).max()) / max(1.0, float(np.abs(ref).max()))
            worst = max(worst, err)
            assert got[sp][u].shape == ref.shape and err <= 2e-5, (u, sp, err)
    print(f"fan-out against sequential converts, float32 storage: largest scaled difference {worst:.3e}")
    assert not _same(want[0], want[1])                         # (the speakers do differ)


def test_uploads_are_counted_once_and_per_call(dev, world):
    w, cfg = world, world.cfg
    m = w.models["float32"]
    speakers = [(w.embs[s], TRG[s]) for s in range(N_SPK)]
    with Dc.DecodeSession(m, w.feats, _sg(cfg, 0.0), dev, SRC, max_batch=MAX_BATCH, pad_tolerance=TOL) as plain:
        plain.convert(w.embs[0], TRG[0])
        plain.convert(w.embs[1], TRG[1])
        assert set(plain.uploaded_bytes) == {"init", "convert"}
    with Dc.DecodeSession(m, w.feats, _sg(cfg, 0.0), dev, SRC, max_batch=MAX_BATCH, pad_tolerance=TOL) as s:
        s.convert(w.embs[0], TRG[0])
        s.convert_many(speakers)
        s.convert_many(speakers[:2])
        s.convert(w.embs[1], TRG[1])
        up = s.uploaded_bytes
        assert up["fanout_init"] == 4 * sum(FRAMES) + 16 * len(FRAMES)          # packed f0 + the source statistics, once
        E = cfg.spk_emb_size
        assert up["convert_many"] == [N_SPK * (4 * E + 16), 2 * (4 * E + 16)]   # the speaker tables only
        assert up["init"] == plain.uploaded_bytes["init"] and up["convert"] == plain.uploaded_bytes["convert"]
    # no source statistics: no table, no statistics per call, and no shift
    with Dc.DecodeSession(m, w.feats, _sg(cfg, 0.0), dev, None, max_batch=MAX_BATCH, pad_tolerance=TOL) as s:
        c = s.convert_many(speakers[:1])
        assert s.uploaded_bytes["fanout_init"] == 4 * sum(FRAMES) and s.uploaded_bytes["convert_many"] == [4 * cfg.spk_emb_size]
        assert _same(c[0], s.convert(w.embs[0], TRG[0]))
        with pytest.raises(ValueError):
            s.convert_many([(w.embs[0], None), (None, None)])


# ---------------------------------------------------------------------------------------------- a checked session
RANGE_CASE = "inputs*2^8"          # tests/range_cases.py: outside float16 storage's range contract


def test_checked_fanout_replaces_exactly_the_flagged_rows(dev):
    """The two utterances of the range case next to the two of `base` (the same weights, inputs in range), two speakers,
    float16 storage with fallback bfloat16: the rows an unchecked float16 pass returns non-finite - and only they - come
    back from bfloat16, every other row with the unchecked float16 bits; the model ends in float16."""
    cfg = S.FULL_CONFIG
    sd, loud, _ = RC.build_case(cfg, RANGE_CASE)
    _, plain, _ = RC.build_case(cfg, "base")
    feats = [dict(f0=b.f0[i].T.copy(), ppg=b.ppg[i].T.copy(), lft=b.lft[i].T.copy()) for b in (loud, plain) for i in range(RC.B)]
    speakers = [(plain.spk_emb[i], None) for i in range(RC.B)]
    m = _module(cfg, sd, dev, "float16")
    sg = _sg(cfg, 0.0)
    kw = dict(max_batch=3, pad_tolerance=0.125)

    def unchecked(storage, pcm16):
        m.use_activation_storage(storage)
        try:
            with Dc.DecodeSession(m, feats, sg, dev, **kw) as s:
                return s.convert_many(speakers, pcm16=pcm16)
        finally:
            m.use_activation_storage("float16")

    f16 = {p: unchecked("float16", p) for p in (True, False)}
    bf = {p: unchecked("bfloat16", p) for p in (True, False)}
    pairs = [(u, sp) for u in range(len(feats)) for sp in range(len(speakers))]
    flagged = [(u, sp) for u, sp in pairs if not np.isfinite(f16[False][sp][u]).all()]
    print("non-finite (utterance, speaker) rows in float16 storage:", flagged)
    assert flagged and len(flagged) < len(pairs), "the premise: some rows leave float16's range, not all"
    assert all(np.isfinite(bf[False][sp][u]).all() for u, sp in pairs)
    batches = Dc.fanout_batches([RC.F] * len(feats), len(speakers), 3, 0.125)
    rerun = [chunk for chunk in batches if any(pair in flagged for pair in chunk)]
    assert any(any(pair not in flagged for pair in chunk) for chunk in rerun)      # (a re-run batch holds an unflagged row)
    for pcm16 in (True, False):
        with Dc.DecodeSession(m, feats, sg, dev, checked=True, fallback=("bfloat16",), **kw) as s:
            got = s.convert_many(speakers, pcm16=pcm16)
            report, forwards = s.last_report, s.forwards
        assert m.activation_storage == "float16"
        assert forwards == len(batches) + len(rerun)
        assert len(report) == len(speakers) and all(len(r) == len(feats) for r in report)
        for u, sp in pairs:
            r = report[sp][u]
            hit = (u, sp) in flagged
            assert r["storage"] == ("bfloat16" if hit else "float16") and r["tried"] == (["float16"] if hit else []), (u, sp)
            assert _same([got[sp][u]], [(bf if hit else f16)[pcm16][sp][u]]), (u, sp, pcm16)
            nf, cl, mx = Dc.output_report([(bf if hit else f16)[False][sp][u]])
            assert (r["nonfinite"], r["clipped"]) == (0, int(cl[0])) and np.float32(r["max_abs"]) == mx[0], (u, sp)
    # no fallback left: the last result comes back, and strict names the pairs
    with Dc.DecodeSession(m, feats, sg, dev, checked=True, fallback=(), strict=True, **kw) as s:
        with pytest.raises(A.FastSVCError, match="utterance, speaker"):
            s.convert_many(speakers)
        assert [(u, sp) for u, sp in pairs if s.last_report[sp][u]["nonfinite"]] == flagged
    assert m.activation_storage == "float16"
