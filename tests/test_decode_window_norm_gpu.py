"""GPU tests (-m gpu) of windowed decode with whole-utterance InstanceNorm statistics: the grouped-sums kernels
(csrc/fastsvc_normgroup.hip) against numpy float64, the pass-through rule bit for bit, and
DecodeSession.convert_windowed(norm="utterance") against the float64 oracle of the WHOLE utterance WITH the speaker
embedding - the regime in which per-window statistics (norm="window") are a different function."""
import numpy as np
import pytest
import torch

import range_cases as RC
import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd import synth as S

pytestmark = pytest.mark.gpu

# (the constants of tests/test_decode_windowed_gpu.py)
TIGHT = 1e-4                # x max(1, |ref|max): the suite's float32 bound against the oracle
BF16_MEAN, BF16_MAX = 3e-2, 0.13        # x rms / x max(1, |ref|max) of the reference
F16_DIV = 8.0               # binary16's ulp is 1/8 of bfloat16's

FRAMES = [160, 52]
CORE, FADE = 32, 8


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


def _sg(cfg):
    return A.SignalGenerator(sample_rate=24000, hop_size=cfg.hop, sine_amp=0.1, noise_amp=0.0, signal_types=["sine"])


def _rel(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / max(1.0, float(np.abs(ref).max()))


# ------------------------------------------------------------------------------------------------------ the kernels
R70 = 70
LENS70 = [(1, 3, 4, 45, 112)[r % 5] for r in range(R70)]


def _groups70():
    """70 rows of 1, 3, 4, 45 and 112 frames: a group of 5 rows that are not adjacent, a pair, singletons that own part
    of their frames (odd own_lo among them, one-frame ranges), and singletons that own everything (pass-through)."""
    group = list(range(R70))
    lo = [0] * R70
    hi = list(LENS70)
    for r in (9, 23, 38, 44, 69):                         # the group of 5: lengths 112, 45, 45, 112, 112
        group[r] = 9
    group[14] = 13                                       # the pair: 45 and 112 frames
    for r in (9, 13):
        lo[r], hi[r] = 0, 32
    lo[23], hi[23] = 7, 39
    lo[38], hi[38] = 13, 45                              # odd own_lo, up to the row's end
    lo[44], hi[44] = 33, 34                              # one frame
    lo[69], hi[69] = 1, 112
    lo[14], hi[14] = 41, 112
    for r in range(3, R70, 5):                           # 45-frame rows not yet used: partial singletons, odd starts
        if group[r] == r and r not in (13,):
            lo[r], hi[r] = 1 + 2 * (r % 7), 45 - (r % 3)
    lo[1], hi[1] = 1, 2                                  # a 3-frame row owning its middle frame
    lo[6], hi[6] = 2, 3                                  # ... and its last
    lo[2], hi[2] = 1, 4                                  # a 4-frame row owning 3 frames
    lo[19], hi[19] = 111, 112                            # the last frame of a long row
    passthrough = [r for r in range(R70) if group[r] == r and group.count(r) == 1 and lo[r] == 0 and hi[r] == LENS70[r]]
    assert len(passthrough) >= 20 and 0 in passthrough and 4 in passthrough
    return group, lo, hi, passthrough


@pytest.mark.parametrize("storage", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("C,len_mul", [(24, 2), (24, 160), (192, 2), (192, 160)])
def test_group_stats_against_numpy_float64(dev, storage, C, len_mul):
    """fastsvc_norm_group_stats on the stored values against float64 numpy.  Per entry |got - want| <= n 2^-53 sum |terms|
    with n the number of terms of the pooled sum: the textbook forward bound of a float64 sum of n terms in any order.
    The sum takes n - 1 roundings and `* len / N` two more; for the smallest groups here (n = 2, 4) the division is by
    a power of two and exact, so the bound covers them, and from n = 6 on the worst case of n + 1 roundings all at half
    an ulp in one direction is out of reach (measured: at most 0.46 of the bound).  `want` is the exact sum (math.fsum)
    scaled in float64.  Padding
    and unowned columns are NaN: a single one read shows in a sum.  Two calls give identical bits; pass-through rows keep
    the pattern their slots were filled with."""
    import math
    from svcc23_fastsvc_amd.engine import norm_group_stats
    dtype = dict(float32=torch.float32, bfloat16=torch.bfloat16, float16=torch.float16)[storage]
    group, lo, hi, passthrough = _groups70()
    ld = 112 * len_mul
    gen = torch.Generator(device=dev).manual_seed(1000 * C + len_mul)
    u = (torch.randn((R70, C, ld), generator=gen, device=dev) * 2.0 + 0.75).to(dtype)      # the stored values ...
    own = torch.zeros((R70, ld), dtype=torch.bool)
    for r in range(R70):
        own[r, lo[r] * len_mul: hi[r] * len_mul] = True
    u.masked_fill_(~own.to(dev)[:, None, :], float("nan"))                                  # ... NaN wherever nothing is owned
    pattern = -1234.5
    outs = []
    for _ in range(2):
        st = torch.full((R70, C, 2), pattern, dtype=torch.float64, device=dev)
        norm_group_stats(u, LENS70, len_mul, (group, lo, hi), st)
        outs.append(st.cpu().numpy())
    got = outs[0]
    assert np.array_equal(got.view(np.uint64), outs[1].view(np.uint64))
    assert (got[passthrough] == pattern).all()
    # the exact sums (math.fsum) of every group once; at 160 columns a frame on a subset of the channels (the channel only
    # moves the row's base address, by a multiple of 16 bytes here)
    chans = list(range(C)) if len_mul == 2 else sorted(set(range(0, C, 8)) | {1, C - 1})
    eps = 2.0 ** -53
    exact = {}
    for g in sorted(set(group) - set(passthrough)):
        members = [r for r in range(R70) if group[r] == g]
        x = torch.cat([u[r, chans, lo[r] * len_mul: hi[r] * len_mul] for r in members], dim=1).to(torch.float64).cpu().numpy()
        assert np.isfinite(x).all()                      # (2-byte elements convert exactly)
        exact[g] = (x.shape[1], [(math.fsum(t), float(np.abs(t).sum())) for t in x], [(math.fsum(t * t), float((t * t).sum())) for t in x])
    worst = 0.0
    for b in range(R70):
        if b in passthrough:
            continue
        N, e1, e2 = exact[group[b]]
        assert N == sum((hi[r] - lo[r]) * len_mul for r in range(R70) if group[r] == group[b])
        scale = float(LENS70[b] * len_mul) / float(N)
        for k, c in enumerate(chans):
            for j, (s, sabs) in enumerate((e1[k], e2[k])):
                want = s * float(LENS70[b] * len_mul) / float(N)
                bound = N * eps * sabs * scale
                err = abs(got[b, c, j] - want)
                worst = max(worst, err / bound)
                assert err <= bound, (b, c, j, got[b, c, j], want, bound)
    print(f"NORMGROUP stats {storage} C {C} len_mul {len_mul}: worst error {worst:.3f} of the bound")


def test_group_stats_rejects_bad_arguments(dev):
    from svcc23_fastsvc_amd.engine import norm_group_stats
    u = torch.zeros((2, 3, 8), device=dev)
    st = torch.zeros((2, 3, 2), dtype=torch.float64, device=dev)
    ok = ([0, 0], [0, 2], [2, 4])
    norm_group_stats(u, [4, 4], 2, ok, st)
    for groups in (([0, 0], [0, 2], [2, 5]), ([1, 0], [0, 2], [2, 4]), ([0, 0], [2, 2], [2, 4])):
        with pytest.raises(ValueError):
            norm_group_stats(u, [4, 4], 2, groups, st)
    with pytest.raises(ValueError):
        norm_group_stats(u, [4, 4], 3, ok, st)           # the pitch is no multiple of len_mul
    with pytest.raises(ValueError):
        norm_group_stats(u, [4, 4], 2, ok, st.to(torch.float32))


# ------------------------------------------------------------------------------------------------------ the forward
class _World:
    pass


@pytest.fixture(scope="module")
def world(dev):
    """The world of tests/test_decode_windowed_gpu.py: the recipe generator (weights seed 611), utterances of 160 and 52
    frames (batch seeds 612, 613), noise off, and the float64 oracle of each WHOLE utterance WITH the embedding on the
    excitation a session makes - computed once, shared, left unchanged."""
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
    assert Dc.receptive_field_frames(cfg) <= 36
    w.exc = _excitation(w, w.feats, dev)

    def oracle(batches, exc):
        return [O.forward_dedup(w.wf, cfg.upsampling_scales, b.ppg, e.reshape(1, 1, -1), b.lft, w.emb[None],
                                dtype=torch.float64).numpy()[0, 0] for b, e in zip(batches, exc)]
    w.oracle_of = oracle
    w.oracle = oracle(w.batches, w.exc)
    return w


def _excitation(w, feats, dev):
    with Dc.DecodeSession(w.model("float32"), feats, w.sg, dev) as s:
        s._window_trace = {}
        s.convert_windowed(core=64, fade=FADE, pcm16=False)
        return [e.cpu().numpy() for e in s._window_trace["excitation"]]


@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
def test_singleton_groups_are_the_plain_forward_bit_for_bit(dev, world, storage):
    """A ragged batch of 5 rows of 48, 48, 40, 20 and 4 frames with an embedding: norm_groups all singleton and whole-row
    is the pass-through case for every row - the bits of norm_groups=None."""
    w = world
    cfg, hop = w.cfg, w.cfg.hop
    lens = [48, 48, 40, 20, 4]
    b = S.synth_batch(cfg, 5, 48, 620)
    m = w.model(storage)
    ins = [torch.from_numpy(v).to(dev) for v in (b.ppg, b.sine, b.lft, b.spk_emb)]
    with torch.no_grad():
        want = m(*ins, lengths=lens).cpu().numpy()
        got = m(*ins, lengths=lens, norm_groups=(list(range(5)), [0] * 5, lens)).cpu().numpy()
        # (without an embedding the groups are ignored altogether)
        want0 = m(*ins[:3], lengths=lens).cpu().numpy()
        got0 = m(*ins[:3], lengths=lens, norm_groups=([0, 0, 0, 3, 3], [0, 8, 0, 0, 0], [8, 48, 40, 20, 4])).cpu().numpy()
    assert np.isfinite(want).all() and float(np.abs(want).max()) > 0
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(got0), _bits(want0))
    for i, n in enumerate(lens):
        assert not got[i, 0, n * hop:].any()


def test_utterance_statistics_make_windows_the_whole_utterance(dev, world):
    """The point of norm="utterance": with the embedding, core 32 and the default context, 7 window rows in one batch
    (max_batch 8, two groups) and in two (max_batch 5) are within TIGHT of the float64 oracle of each WHOLE utterance and
    within 2 TIGHT of convert (both are within TIGHT of that oracle); norm="window" is not within TIGHT."""
    w = world
    m = w.model("float32")
    with Dc.DecodeSession(m, w.feats, w.sg, dev) as s:
        whole = s.convert(w.emb, pcm16=False)
    res = {}
    for max_batch, n_forwards in ((8, 1), (5, 2)):
        with Dc.DecodeSession(m, w.feats, w.sg, dev, max_batch=max_batch) as s:
            res[max_batch] = s.convert_windowed(w.emb, core=CORE, fade=FADE, norm="utterance", pcm16=False)
            assert s.forwards == n_forwards
    with Dc.DecodeSession(m, w.feats, w.sg, dev, max_batch=8) as s:
        per_window = s.convert_windowed(w.emb, core=CORE, fade=FADE, norm="window", pcm16=False)
    worst_window = 0.0
    for i, ref in enumerate(w.oracle):
        for max_batch in (8, 5):
            y = res[max_batch][i]
            assert y.dtype == np.float32 and y.shape == ref.shape
            e_or, e_cv = _rel(y, ref), _rel(y, whole[i].astype(np.float64))
            print(f"WINDOW-NORM utterance {i} max_batch {max_batch}: {e_or:.3e} to the whole-utterance oracle, {e_cv:.3e} to "
                  f"convert (convert itself {_rel(whole[i], ref):.3e}; |ref|max {np.abs(ref).max():.3g})")
            assert e_or <= TIGHT, (i, max_batch, e_or)
            assert float(np.abs(y.astype(np.float64) - whole[i]).max()) <= 2 * TIGHT * max(1.0, float(np.abs(ref).max())), (i, max_batch)
        e_w = _rel(per_window[i], ref)
        print(f"WINDOW-NORM utterance {i} norm=window: {e_w:.3e} to the whole-utterance oracle")
        worst_window = max(worst_window, e_w)
    assert worst_window > TIGHT


def test_too_many_windows_are_refused_before_any_forward(dev, world):
    w = world
    with Dc.DecodeSession(w.model("float32"), w.feats, w.sg, dev, max_batch=4) as s:
        with pytest.raises(ValueError, match="utterance 0 has 5 windows but max_batch is 4"):
            s.convert_windowed(w.emb, core=CORE, fade=FADE, norm="utterance")
        assert s.forwards == 0
        with pytest.raises(ValueError, match="norm must be"):
            s.convert_windowed(w.emb, core=CORE, fade=FADE, norm="batch")


@pytest.mark.parametrize("storage", ["bfloat16", "float16"])
def test_two_byte_storages_against_the_oracle(dev, world, storage):
    """The shapes of the float32 test in bfloat16 and float16 storage, with the embedding, against the whole-utterance
    oracle: tests/test_config_matrix_gpu.py's bfloat16 bounds, an eighth of them in float16."""
    w = world
    div = F16_DIV if storage == "float16" else 1.0
    with Dc.DecodeSession(w.model(storage), w.feats, w.sg, dev, max_batch=8) as s:
        got = s.convert_windowed(w.emb, core=CORE, fade=FADE, norm="utterance", pcm16=False)
    for i, (y, ref) in enumerate(zip(got, w.oracle)):
        err = np.abs(y.astype(np.float64) - ref)
        rms, mag = float(np.sqrt(np.mean(ref ** 2))), max(1.0, float(np.abs(ref).max()))
        print(f"WINDOW-NORM {storage} utterance {i}: mean/rms {err.mean() / rms:.3e} max/mag {err.max() / mag:.3e}")
        assert np.isfinite(y).all()
        assert float(err.mean()) <= BF16_MEAN / div * rms, (i, float(err.mean()), rms)
        assert float(err.max()) <= BF16_MAX / div * mag, (i, float(err.max()), mag)


def test_one_loud_window_among_quiet_ones(dev, world):
    """The operand bound of float32 storage: 160 frames whose ppg, lft and f0 are scaled by 1e-3 everywhere except frames
    64..96 - one loud window among five.  With the utterance's statistics the loud window's normalised values exceed
    sqrt(its own length), the bound the split-binary16 staging scale is derived from without the adjustment
    (DESIGN.md 4.9).  Finite and within TIGHT of its whole-utterance oracle.

    Measured: 3.5e-6.  This input does NOT discriminate: an A/B build with the adjustment compiled out
    (-DFASTSVC_EXP_NG_NORAISE) gives the same 3.5e-6.  The staging scale leaves a factor 2 - 4 between the bound and
    binary16's ceiling, and five windows move the bound only by sqrt(160 / 104) = 1.24.  An input that needs the
    adjustment must put nearly all of a channel's energy into a few columns of one window of an utterance of more than
    16 x 104 frames (> 52 windows in one batch); that sharper input has not been constructed, the adjustment stays."""
    w = world
    b = S.synth_batch(w.cfg, 1, 160, 612)
    hop = w.cfg.hop
    gain = np.full(160, 1e-3, np.float32)
    gain[64:96] = 1.0
    b.ppg[0] *= gain[None, :]
    b.lft[0] *= np.repeat(gain, hop)[None, :]
    b.f0[0] *= gain[None, :]
    feats = [dict(f0=b.f0[0].T.copy(), ppg=b.ppg[0].T.copy(), lft=b.lft[0].T.copy())]
    exc = _excitation(w, feats, dev)
    ref = w.oracle_of([b], exc)[0]
    with Dc.DecodeSession(w.model("float32"), feats, w.sg, dev, max_batch=8) as s:
        got = s.convert_windowed(w.emb, core=CORE, fade=FADE, norm="utterance", pcm16=False)[0]
        assert s.forwards == 1
    assert np.isfinite(got).all()
    err = _rel(got, ref)
    print(f"WINDOW-NORM loud window: {err:.3e} to the whole-utterance oracle (|ref|max {np.abs(ref).max():.3g})")
    assert err <= TIGHT, err


def test_one_window_utterances_are_convert(dev, world):
    """An utterance of one window is a pass-through row: convert's bytes, PCM-16 and float32."""
    w = world
    with Dc.DecodeSession(w.model("float32"), w.feats[1:], w.sg, dev, [[5.0, 1.0]]) as s:
        for pcm16 in (True, False):
            want = s.convert(w.emb, [5.2, 1.0], pcm16=pcm16)
            got = s.convert_windowed(w.emb, [5.2, 1.0], core=64, norm="utterance", pcm16=pcm16)
            assert len(got) == 1 and got[0].dtype == want[0].dtype and np.array_equal(_bits(got[0]), _bits(want[0])), pcm16


def test_checked_session_falls_back_with_whole_groups(dev):
    """The case of test_checked_session_runs_a_flagged_utterance_again_in_the_fallback (range_cases' `g_up*2^8`, core 16,
    context 8) with norm="utterance": a checked float16 session with fallback bfloat16 returns, for the flagged
    utterances, what an unchecked bfloat16 norm="utterance" session computes, bit for bit, and says so."""
    cfg = S.FULL_CONFIG
    sd, b, spk = RC.build_case(cfg, "g_up*2^8")
    assert spk
    feats = [dict(f0=b.f0[i].T.copy(), ppg=b.ppg[i].T.copy(), lft=b.lft[i].T.copy()) for i in range(RC.B)]
    emb = b.spk_emb[0]
    sg = _sg(cfg)
    kw = dict(core=16, context=8, fade=8, norm="utterance")
    ref = {}
    for st in ("float16", "bfloat16"):
        with Dc.DecodeSession(_module(cfg, sd, dev, st), feats, sg, dev, max_batch=8) as s:
            ref[st] = s.convert_windowed(emb, pcm16=False, **kw)
    bad = [i for i, y in enumerate(ref["float16"]) if not np.isfinite(y).all()]
    print("WINDOW-NORM checked: non-finite in float16", bad)
    assert bad and all(np.isfinite(y).all() for y in ref["bfloat16"])
    m = _module(cfg, sd, dev, "float16")
    with Dc.DecodeSession(m, feats, sg, dev, max_batch=8, checked=True) as s:
        got = s.convert_windowed(emb, pcm16=False, **kw)
        assert m.activation_storage == "float16" and s.forwards == 2
        for i in bad:
            assert np.array_equal(_bits(got[i]), _bits(ref["bfloat16"][i])), i
            r = s.last_report[i]
            assert r["storage"] == "bfloat16" and r["tried"] == ["float16"] and r["nonfinite"] == 0, r
        for i in set(range(RC.B)) - set(bad):
            assert s.last_report[i]["storage"] == "float16" and np.array_equal(_bits(got[i]), _bits(ref["float16"][i]))
