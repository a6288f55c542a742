"""GPU tests (-m gpu) of the windowed decode: the assembly and stitch kernels (csrc/fastsvc_window.hip) bit for bit
against numpy slices and decode.stitch_windows + to_pcm16, and DecodeSession.convert_windowed against the float64
oracle of the WHOLE utterance (no speaker: the same function), against every window run alone (with a speaker: per-window
InstanceNorm statistics), against convert (one window), in the 2-byte storages, checked with a fallback, and on an
utterance longer than one forward takes."""
import numpy as np
import pytest
import torch

import range_cases as RC
import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd import synth as S

pytestmark = pytest.mark.gpu

TIGHT = 1e-4                # x max(1, |ref|max): the suite's float32 bound against the oracle
BATCHING = 2e-5             # x max(1, |ref|max): the batching invariance the harness states (tests/test_parity_gpu.py)
BF16_MEAN, BF16_MAX = 3e-2, 0.13        # tests/test_config_matrix_gpu.py: x rms / x max(1, |ref|max) of the reference
F16_DIV = 8.0               # binary16's ulp is 1/8 of bfloat16's (tests/test_storage_f16_gpu.py)
GUARD = 0x5A5A


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


def _sg(cfg, noise=0.0):
    return A.SignalGenerator(sample_rate=24000, hop_size=cfg.hop, sine_amp=0.1, noise_amp=noise, signal_types=["sine"])


# ------------------------------------------------------------------------------------------------------- assemble
@pytest.mark.parametrize("C,hop", [(144, 160), (100, 60)])
def test_assemble_equals_numpy_slices(dev, C, hop):
    """70 rows (two launches) of 1, 3, 4, 45 and 112 frames cut at offsets that are not multiples of 4 elements (and,
    for C = 144, at 16-byte aligned ones too: the 16-byte read path), destinations full of NaN: the ppg slice transposed,
    the lft and excitation slices copied, everything past a row's length exactly zero - bit for bit."""
    rng = np.random.default_rng(C)
    from svcc23_fastsvc_amd.engine import window_assemble, window_launch_count
    R, width = 70, 112
    assert window_launch_count(R) == 2
    lens = [(1, 3, 4, 45, 112)[r % 5] for r in range(R)]
    F = 400
    ppg = rng.standard_normal(1 + F * C).astype(np.float32)
    lft = rng.standard_normal(3 + F * hop).astype(np.float32)
    sine = rng.standard_normal(3 + F * hop).astype(np.float32)
    for aligned in (False, True):
        base_p, base_s = (0, 0) if aligned else (1, 3)
        starts = [int(v) for v in rng.integers(0, F - width, R)]
        if aligned:
            starts = [s // 4 * 4 for s in starts]
        ppg_off = [base_p + s * C for s in starts]
        sig_off = [base_s + s * hop for s in starts]
        if not aligned:
            assert all(o % 4 for o in ppg_off) or C % 4
            assert any(o % 4 for o in sig_off)
        want_p = np.zeros((R, C, width), np.float32)
        want_l = np.zeros((R, 1, width * hop), np.float32)
        want_s = np.zeros((R, 1, width * hop), np.float32)
        for r, n in enumerate(lens):
            want_p[r, :, :n] = ppg[ppg_off[r]: ppg_off[r] + n * C].reshape(n, C).T
            want_l[r, 0, :n * hop] = lft[sig_off[r]: sig_off[r] + n * hop]
            want_s[r, 0, :n * hop] = sine[sig_off[r]: sig_off[r] + n * hop]
        outs = [torch.full(w.shape, float("nan"), dtype=torch.float32, device=dev) for w in (want_p, want_l, want_s)]
        got = window_assemble(torch.from_numpy(ppg).to(dev), torch.from_numpy(lft).to(dev), torch.from_numpy(sine).to(dev),
                              ppg_off, sig_off, lens, C, hop, width, out=outs)
        for g, o, w in zip(got, outs, (want_p, want_l, want_s)):
            assert g is o
            assert np.array_equal(_bits(g.cpu().numpy()), _bits(w)), (C, aligned)


def test_assemble_rejects_slices_outside_the_buffers(dev):
    from svcc23_fastsvc_amd.engine import window_assemble
    ppg, sig = torch.zeros(40, device=dev), torch.zeros(80, device=dev)
    for ppg_off, sig_off, lens in (([24], [0], [5]), ([0], [64], [5]), ([0], [0], [9]), ([-4], [0], [2]), ([0], [-1], [2])):
        with pytest.raises(ValueError):
            window_assemble(ppg, sig, sig, ppg_off, sig_off, lens, 4, 4, 8)
    with pytest.raises(ValueError):
        window_assemble(ppg, sig, torch.zeros(81, device=dev), [0], [0], [2], 4, 4, 8)


# --------------------------------------------------------------------------------------------------------- stitch
def _pcm(v):
    """to_pcm16 with the device's NaN -> 0 (the host's conversion of a NaN is implementation-defined)."""
    return Dc.to_pcm16(np.where(np.isnan(v), 0.0, v))


def _special_rows(rng, rows, hop, half):
    """Window waveforms in [-1.3, 1.3] (so some samples saturate), with NaN, +-inf and values around the clipping edges
    sprinkled over them - inside the fade zones too, where inf - inf makes a NaN of two finite-free samples."""
    specials = np.array([np.nan, np.inf, -np.inf, 1.0, -1.0, 1.0001, -1.0001, 32768.0 / 32767.0, 0.5, 1.5 / 32767.0], np.float32)
    ys = []
    for r in rows:
        n = (r[2] - r[1]) * hop
        y = rng.uniform(-1.3, 1.3, n).astype(np.float32)
        idx = rng.integers(0, n, 12)
        y[idx] = specials[rng.integers(0, len(specials), 12)]
        for edge in ((r[3] - r[1]) * hop, (r[4] - r[1]) * hop):          # a few inside the zones around the core's edges
            for d in (-half // 2, 0, half // 2 - 1):
                k = edge + d
                if half and 0 <= k < n:
                    y[k] = specials[rng.integers(0, 3)]
        ys.append(y)
    return ys


@pytest.mark.parametrize("hop", [160, 60])
@pytest.mark.parametrize("fade", [0, 2, 8])
def test_stitch_equals_the_numpy_reference(dev, hop, fade):
    """Utterances of 100, 33, 8 and 70 frames in windows of 16 + 2 x 8 (the last windows of 4, 1 and 6 frames; 33's is
    shorter than half a fade zone), their rows spread over batches of 3 (neighbours in different batches, in both
    orders), of 64 (all neighbours in one batch) and of 3 in reverse order; the row padding full of NaN.  PCM-16, float32
    and the per-utterance report, bit for bit: into per-batch buffers with a guard pattern, and into one packed buffer at
    destination offsets that are not multiples of 8."""
    from svcc23_fastsvc_amd.engine import window_stitch
    rng = np.random.default_rng(1000 * hop + fade)
    frames, core, context = [100, 33, 8, 70], 16, 8
    rows = Dc.window_plan(frames, core, context)
    half = fade * hop // 2
    ys = _special_rows(rng, rows, hop, half)
    want = Dc.stitch_windows(ys, rows, hop, fade)
    want_f = [w.astype(np.float32) for w in want]
    want_p = [_pcm(w) for w in want]
    nf, cl, mx = Dc.output_report(want_f)
    want_rep = np.stack([nf, cl, mx.view(np.int32), np.zeros_like(nf)], axis=1)
    assert nf.sum() > 0 and cl.sum() > 0
    base, pos = [], 3                                    # the packed buffer: utterance u at base[u], never 16-byte aligned
    for f in frames:
        base.append(pos)
        pos += f * hop + 5
    for max_batch, order, packed in ((3, 1, False), (64, 1, False), (3, -1, False), (3, 1, True)):
        batches = Dc.window_batches(rows, max_batch, 0.125)[::order]
        layout, stage_elems = Dc.stitch_layout(rows, batches, hop, fade)
        if max_batch == 3 and fade:
            modes = {m for lay in layout for m in lay["left_mode"] + lay["right_mode"]}
            assert {1, 2} <= modes                       # (neighbours in different batches)
        stage = torch.full((max(stage_elems, 1),), float("nan"), dtype=torch.float32, device=dev)
        rep = torch.zeros((len(frames), 4), dtype=torch.int32, device=dev)
        got_p = [np.full(f * hop, 12345, np.int16) for f in frames]
        got_f = [np.full(f * hop, 7.0, np.float32) for f in frames]
        big_p = torch.full((pos,), GUARD, dtype=torch.int16, device=dev)
        big_f = torch.full((pos,), 3.0, dtype=torch.float32, device=dev)
        for chunk, lay in zip(batches, layout):
            B, W = len(chunk), lay["width"]
            y = np.full((B, W), np.nan, np.float32)
            for j, r in enumerate(chunk):
                y[j, :len(ys[r])] = ys[r]
            yd = torch.from_numpy(y).to(dev)
            if packed:
                offs = [base[u] + lo for u, lo, _ in lay["runs"]]
                window_stitch(yd, lay["n_samples"], lay["core_lo"], lay["core_hi"], lay["half"], lay["left_mode"],
                              lay["right_mode"], lay["left_src"], lay["right_src"], offs, stage=stage, out_pcm=big_p,
                              out_float=big_f, utt=lay["utt"], report=rep)
                continue
            out_p = torch.full((lay["total"] + 8,), GUARD, dtype=torch.int16, device=dev)
            out_f = torch.full((lay["total"] + 8,), 3.0, dtype=torch.float32, device=dev)
            window_stitch(yd[:, None, :], lay["n_samples"], lay["core_lo"], lay["core_hi"], lay["half"], lay["left_mode"],
                          lay["right_mode"], lay["left_src"], lay["right_src"], lay["dst_off"], stage=stage, out_pcm=out_p,
                          out_float=out_f, utt=lay["utt"], report=rep)
            hp, hf = out_p.cpu().numpy(), out_f.cpu().numpy()
            touched = np.zeros(hp.size, bool)
            for (u, lo, hi), off in zip(lay["runs"], lay["dst_off"]):
                got_p[u][lo:hi] = hp[off: off + hi - lo]
                got_f[u][lo:hi] = hf[off: off + hi - lo]
                touched[off: off + hi - lo] = True
            assert np.all(hp[~touched] == GUARD) and np.all(hf[~touched] == 3.0)     # nothing outside the runs was written
        if packed:
            hp, hf = big_p.cpu().numpy(), big_f.cpu().numpy()
            touched = np.zeros(pos, bool)
            for u, f in enumerate(frames):
                got_p[u], got_f[u] = hp[base[u]: base[u] + f * hop], hf[base[u]: base[u] + f * hop]
                touched[base[u]: base[u] + f * hop] = True
            assert np.all(hp[~touched] == GUARD) and np.all(hf[~touched] == 3.0)
        for u in range(len(frames)):
            assert np.array_equal(got_p[u], want_p[u]), (u, max_batch, order, packed)
            assert np.array_equal(got_f[u], want_f[u], equal_nan=True), (u, max_batch, order, packed)
            finite = np.isfinite(want_f[u])
            assert np.array_equal(_bits(got_f[u][finite]), _bits(want_f[u][finite])), u
        assert np.array_equal(rep.cpu().numpy(), want_rep), (max_batch, order, packed)


def test_stitch_rejects_what_it_cannot_run(dev):
    from svcc23_fastsvc_amd.engine import window_stitch
    y = torch.zeros(2, 64, device=dev)
    out = torch.zeros(128, dtype=torch.int16, device=dev)
    stage = torch.zeros(16, device=dev)
    ok = dict(n_samples=[64, 64], core_lo=[0, 16], core_hi=[48, 64], half=8, left_mode=[0, 4], right_mode=[3, 0],
              left_src=[0, 0], right_src=[64 + 8, 0], dst_off=[0, 56])
    window_stitch(y, **ok, stage=stage, out_pcm=out)
    for key, val in (("core_hi", [65, 64]), ("core_lo", [0, 4]), ("right_src", [128 - 8, 0]), ("dst_off", [0, 100]),
                     ("left_mode", [0, 7]), ("right_mode", [1, 0]), ("n_samples", [65, 64])):
        bad = dict(ok)
        bad[key] = val
        if key == "right_mode":
            bad["right_src"] = [8, 0]                    # a staged zone of 16 samples at slot 8 of a 16-sample buffer
        with pytest.raises(ValueError):
            window_stitch(y, **bad, stage=stage, out_pcm=out)
    with pytest.raises(ValueError):
        window_stitch(y, **ok, stage=stage)              # no destination
    with pytest.raises(ValueError):
        window_stitch(y, **dict(ok, half=0), stage=stage, out_pcm=out)       # zones without a fade


# ------------------------------------------------------------------------------------------------------ sessions
FRAMES = [160, 52]
CORE, FADE = 32, 8


class _World:
    pass


@pytest.fixture(scope="module")
def world(dev):
    """The recipe generator (weights seed 611), two utterances of 160 and 52 frames (hash generator), the excitation a
    session makes for them (noise off: the same in every call), and the float64 oracle of each WHOLE utterance on that
    excitation, without and with the speaker embedding - computed once, shared, left unchanged."""
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
    w.sg = _sg(cfg)
    w.R = Dc.receptive_field_frames(cfg)
    with Dc.DecodeSession(w.model("float32"), w.feats, w.sg, dev) as s:
        s._window_trace = {}
        w.y_nospk = s.convert_windowed(core=CORE, fade=FADE, pcm16=False)
        w.exc = [e.cpu().numpy() for e in s._window_trace["excitation"]]
        w.trace_batches = [(rows, t.cpu().numpy()) for rows, t in s._window_trace["batches"]]
    w.oracle = {}
    for spk in (False, True):
        w.oracle[spk] = [O.forward_dedup(w.wf, cfg.upsampling_scales, b.ppg, e.reshape(1, 1, -1), b.lft,
                                         w.emb[None] if spk else None, dtype=torch.float64).numpy()[0, 0]
                         for b, e in zip(w.batches, w.exc)]
    return w


def _rel(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / max(1.0, float(np.abs(ref).max()))


def test_speakerless_windows_are_the_whole_utterance(dev, world):
    """No speaker embedding: core 32, the default context (the receptive field, 33, rounded up to 36), fade 8 - against
    the float64 oracle of each WHOLE utterance within TIGHT; with context 16 the same call is NOT (the oracle alone puts
    a window with 16 frames of context 1.7e-1 of the range away)."""
    w = world
    assert w.R <= 36
    for i, (y, ref) in enumerate(zip(w.y_nospk, w.oracle[False])):
        assert y.dtype == np.float32 and y.shape == ref.shape == (FRAMES[i] * w.cfg.hop,)
        err = _rel(y, ref)
        print(f"WINDOWED nospk utterance {i}: {err:.3e} x max(1, |ref|max = {np.abs(ref).max():.3g})")
        assert err <= TIGHT, (i, err)
    with Dc.DecodeSession(w.model("float32"), w.feats, w.sg, dev) as s:
        short = s.convert_windowed(core=CORE, context=16, fade=FADE, pcm16=False)
        pcm = s.convert_windowed(core=CORE, fade=FADE)
    errs = [_rel(y, ref) for y, ref in zip(short, w.oracle[False])]
    print("WINDOWED nospk context 16:", " ".join(f"{e:.3e}" for e in errs))
    assert max(errs) > TIGHT
    # the PCM-16 result is to_pcm16 of the stitched float64 values: within one step of the float32 result's
    for p, y in zip(pcm, w.y_nospk):
        assert p.dtype == np.int16 and np.abs(p.astype(np.int32) - Dc.to_pcm16(y).astype(np.int32)).max() <= 1


def test_windows_with_a_speaker_are_every_window_run_alone(dev, world):
    """With an embedding InstanceNorm normalises per window: the result is stitch_windows of every window row run alone
    (one forward of one row each), within the batching invariance.  The difference to the whole-utterance oracle is
    printed, not asserted: per-window statistics are a different function."""
    w = world
    cfg, hop = w.cfg, w.cfg.hop
    m = w.model("float32")
    with Dc.DecodeSession(m, w.feats, w.sg, dev, max_batch=3) as s:
        got = s.convert_windowed(w.emb, core=CORE, fade=FADE, pcm16=False)
        assert s.forwards == len(Dc.window_batches(Dc.window_plan(FRAMES, CORE, 36), 3, 0.125))
    rows = Dc.window_plan(FRAMES, CORE, 36)
    emb = torch.from_numpy(w.emb[None]).to(dev)
    alone = []
    with torch.no_grad():
        for u, a, e, _, _ in rows:
            b = w.batches[u]
            ins = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in
                   (b.ppg[:, :, a:e], w.exc[u][a * hop: e * hop].reshape(1, 1, -1), b.lft[:, :, a * hop: e * hop])]
            alone.append(m(*ins, emb).cpu().numpy()[0, 0])
    want = Dc.stitch_windows(alone, rows, hop, FADE)
    for i in range(len(FRAMES)):
        err = _rel(got[i], want[i])
        print(f"WINDOWED spk utterance {i}: {err:.3e} to the windows run alone; "
              f"{_rel(got[i], w.oracle[True][i]):.3e} to the whole-utterance oracle (|ref|max {np.abs(w.oracle[True][i]).max():.3g})")
        assert err <= BATCHING, (i, err)


def test_excitation_is_continuous_across_windows(dev, world):
    """With noise: the core slices of the assembled excitation rows, concatenated, are bit for bit the excitation the
    same call made for each whole utterance; and so is every row as a whole (context included)."""
    w = world
    hop = w.cfg.hop
    with Dc.DecodeSession(w.model("float32"), w.feats, _sg(w.cfg, noise=0.003), dev, [[5.0, 1.0]] * 2, max_batch=3) as s:
        s._window_trace = {}
        s.convert_windowed(w.emb, [5.2, 1.0], core=CORE, fade=FADE)
        exc = [e.cpu().numpy() for e in s._window_trace["excitation"]]
        seen = [np.full(f * hop, np.nan, np.float32) for f in FRAMES]
        for rows, sine in s._window_trace["batches"]:
            sine = sine.cpu().numpy()
            for j, (u, a, e, lo, hi) in enumerate(rows):
                assert np.array_equal(_bits(sine[j, 0, :(e - a) * hop]), _bits(exc[u][a * hop: e * hop]))
                assert not sine[j, 0, (e - a) * hop:].any()
                seen[u][lo * hop: hi * hop] = sine[j, 0, (lo - a) * hop: (hi - a) * hop]
    for u in range(len(FRAMES)):
        assert np.array_equal(_bits(seen[u]), _bits(exc[u])), u
        assert len(np.unique(exc[u])) > exc[u].size // 2                 # (noise: the unvoiced stretches are not silent)
    # (noise off: the excitation does not depend on the call)
    assert not np.array_equal(exc[0], w.exc[0])


def test_one_window_is_convert(dev, world):
    """An utterance of at most `core` frames is one row, the whole utterance: convert's bytes, PCM-16 and float32."""
    w = world
    with Dc.DecodeSession(w.model("float32"), w.feats[1:], w.sg, dev, [[5.0, 1.0]]) as s:
        for pcm16 in (True, False):
            want = s.convert(w.emb, [5.2, 1.0], pcm16=pcm16)
            got = s.convert_windowed(w.emb, [5.2, 1.0], core=64, pcm16=pcm16)
            assert len(got) == 1 and got[0].dtype == want[0].dtype and np.array_equal(_bits(got[0]), _bits(want[0])), pcm16
        assert s.uploaded_bytes["convert"] and len(s.uploaded_bytes["convert_windowed"]) == 2


@pytest.mark.parametrize("storage", ["bfloat16", "float16"])
def test_two_byte_storages_against_the_oracle(dev, world, storage):
    """The shapes of the speakerless test in bfloat16 and float16 storage against the whole-utterance oracle:
    tests/test_config_matrix_gpu.py's bfloat16 bounds, an eighth of them in float16."""
    w = world
    div = F16_DIV if storage == "float16" else 1.0
    with Dc.DecodeSession(w.model(storage), w.feats, w.sg, dev) as s:
        got = s.convert_windowed(core=CORE, fade=FADE, pcm16=False)
    for i, (y, ref) in enumerate(zip(got, w.oracle[False])):
        err = np.abs(y.astype(np.float64) - ref)
        rms, mag = float(np.sqrt(np.mean(ref ** 2))), max(1.0, float(np.abs(ref).max()))
        print(f"WINDOWED {storage} utterance {i}: mean/rms {err.mean() / rms:.3e} max/mag {err.max() / mag:.3e}")
        assert np.isfinite(y).all()
        assert float(err.mean()) <= BF16_MEAN / div * rms, (i, float(err.mean()), rms)
        assert float(err.max()) <= BF16_MAX / div * mag, (i, float(err.max()), mag)


def test_checked_session_runs_a_flagged_utterance_again_in_the_fallback(dev):
    """range_cases' `g_up*2^8` (the up blocks' gains x 256: between two InstanceNorms the activations pass 65504) leaves
    float16 storage non-finite and bfloat16 storage finite.  A checked float16 session with fallback bfloat16 returns,
    for the flagged utterances, what an unchecked bfloat16 session computes - every window of them - and says so."""
    cfg = S.FULL_CONFIG
    sd, b, spk = RC.build_case(cfg, "g_up*2^8")
    assert spk
    feats = [dict(f0=b.f0[i].T.copy(), ppg=b.ppg[i].T.copy(), lft=b.lft[i].T.copy()) for i in range(RC.B)]
    emb = b.spk_emb[0]
    sg = _sg(cfg)
    kw = dict(core=16, context=8, fade=8)
    ref = {}
    for st in ("float16", "bfloat16"):
        with Dc.DecodeSession(_module(cfg, sd, dev, st), feats, sg, dev, max_batch=4) as s:
            ref[st, False] = s.convert_windowed(emb, pcm16=False, **kw)
            ref[st, True] = s.convert_windowed(emb, **kw)
    bad = [i for i, y in enumerate(ref["float16", False]) if not np.isfinite(y).all()]
    print("WINDOWED checked: non-finite in float16", bad)
    assert bad == list(range(RC.B)) and all(np.isfinite(y).all() for y in ref["bfloat16", False])
    m = _module(cfg, sd, dev, "float16")
    n_batches = len(Dc.window_batches(Dc.window_plan([RC.F] * RC.B, 16, 8), 4, 0.125))
    with Dc.DecodeSession(m, feats, sg, dev, max_batch=4, checked=True) as s:
        for pcm16 in (True, False):
            got = s.convert_windowed(emb, pcm16=pcm16, **kw)
            assert m.activation_storage == "float16" and s.forwards == 2 * n_batches
            for i in range(RC.B):
                assert np.array_equal(_bits(got[i]), _bits(ref["bfloat16", pcm16][i])), (i, pcm16)
                r = s.last_report[i]
                assert r["storage"] == "bfloat16" and r["tried"] == ["float16"] and r["nonfinite"] == 0, r
                nf, cl, mx = Dc.output_report([ref["bfloat16", False][i]])
                assert r["clipped"] == int(cl[0]) and np.float32(r["max_abs"]).view(np.uint32) == mx.view(np.uint32)[0], r
    with Dc.DecodeSession(m, feats, sg, dev, max_batch=4, checked=True, fallback=()) as s:
        got = s.convert_windowed(emb, pcm16=False, **kw)
        assert s.forwards == n_batches
        for i in range(RC.B):
            nf, _, _ = Dc.output_report([ref["float16", False][i]])
            assert s.last_report[i]["nonfinite"] == int(nf[0]) > 0 and s.last_report[i]["storage"] == "float16"


def test_an_utterance_longer_than_one_forward_takes(dev):
    """72 000 frames = 11.52 M samples, past the forward's 11 184 811: convert refuses without running anything,
    convert_windowed(core=400) returns every sample, finite, and its peak device memory stays within 1.5 x (what convert
    needs for a 32 x 480-frame batch + the long session's resident features)."""
    cfg = S.FULL_CONFIG
    hop, C = cfg.hop, cfg.in_channels
    m = _module(cfg, S.synth_state_dict(cfg, 611), dev)
    sg = _sg(cfg)
    emb = S.synth_batch(cfg, 1, 4, 3).spk_emb[0]
    block = S.synth_batch(cfg, 1, 480, 614)              # hashed features, tiled to the long utterance
    small = [dict(f0=block.f0[0].T.copy(), ppg=block.ppg[0].T.copy(), lft=block.lft[0].T.copy())] * 32
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    with Dc.DecodeSession(m, small, sg, dev) as s:
        assert len(s.batches) == 1
        s.convert(emb)
    peak_small = torch.cuda.max_memory_allocated(dev) - base
    F = 72000
    assert F > S.max_forward_frames(cfg) and F * hop == 11520000
    reps = F // 480
    long = [dict(f0=S.synth_f0(1, F, 615)[0].T.copy(), ppg=np.tile(block.ppg[0].T, (reps, 1)),
                 lft=np.tile(block.lft[0].T, (reps, 1)))]
    resident = 4 * F * (C + hop)
    del s
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    with Dc.DecodeSession(m, long, sg, dev) as s:        # (the constructor takes any length)
        assert s.uploaded_bytes["init"] == resident
        with pytest.raises(A.FastSVCError, match="too long.*convert_windowed"):
            s.convert(emb)
        assert s.forwards == 0
        ys = s.convert_windowed(emb, core=400, pcm16=False)
        forwards = s.forwards
    peak_long = torch.cuda.max_memory_allocated(dev) - base
    print(f"WINDOWED long: {forwards} forwards, peak {peak_long / 2 ** 20:.0f} MiB; convert of 32 x 480 frames "
          f"{peak_small / 2 ** 20:.0f} MiB + resident {resident / 2 ** 20:.0f} MiB")
    assert len(ys) == 1 and ys[0].shape == (11520000,) and ys[0].dtype == np.float32
    assert np.isfinite(ys[0]).all() and float(np.abs(ys[0]).max()) > 0
    assert peak_long <= 1.5 * (peak_small + resident), (peak_long, peak_small, resident)
