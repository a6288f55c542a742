"""float16 (IEEE binary16) activation storage on the GPU (-m gpu): `Plan(cfg, storage="float16")`.

Every assertion compares the HIP float16 forward with the float64 oracle; the ratio assertions also run the HIP
bfloat16 forward on the same inputs in the same test.  binary16 has 11 significand bits against bfloat16's 8, so its
rounding is 8x finer; the CPU model of tests/test_storage_f16.py predicts 5.2x .. 13.6x smaller mean errors, the
tests ask for 3x on the mean and 2x on the maximum (one sample).

Absolute bounds (x max(1, |ref|max)): twice the largest value observed on the MI355X over the cases of
test_default_generator_vs_oracle_and_bfloat16 - see F16_MEAN / F16_MAX below.
"""
import numpy as np
import pytest
import torch

import config_matrix as CM
import range_cases as RC
import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import synth as S

pytestmark = pytest.mark.gpu

MEAN_RATIO = 1.0 / 3.0      # float16 mean error <= a third of bfloat16's
MAX_RATIO = 1.0 / 2.0       # float16 max error <= half of bfloat16's
# Observed on the MI355X over test_default_generator_vs_oracle_and_bfloat16 (8 x 600 with / without speaker, 1 x 600),
# relative to max(1, |ref|max): mean-abs 2.13e-4 / 1.97e-4 / 2.17e-4, max-abs 3.13e-3 / 3.46e-3 / 2.54e-3 (bfloat16 on
# the same inputs: mean 1.7e-3 / 1.5e-3 / 1.7e-3, max 2.2e-2 / 2.6e-2 / 2.1e-2).  Bounds = 2 x the largest.
F16_MEAN = 4.4e-4
F16_MAX = 7.0e-3
# x the tap's own maximum.  The CPU model's worst tap is 3.6e-3 of its maximum, x 2 = 2^-7 = 7.8e-3; observed worst on the
# MI355X: 2.63e-3 (up.3.out, with speaker; 2.61e-3 without) -> tightened to 2 x that.
TAP_TOL = 5.3e-3
# PCM-16 steps between the float16 decode and the golden waveform: observed 368 (bfloat16 storage: 2114) -> 2 x
PCM_STEPS = 736


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    A.load_library()
    return torch.device("cuda:0")


def _t(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _oracle():
    from oracle import fastsvc_oracle as O
    return O


def _errs(y, ref):
    e = np.abs(np.asarray(y, np.float64) - np.asarray(ref, np.float64))
    return float(e.mean()), float(e.max())


def _check_pair(y16, ybf, ref, what, absolute=True):
    """the two ratios (and the absolute bounds) of a float16 result against the bfloat16 result of the same inputs"""
    assert np.isfinite(y16).all(), what
    m16, x16 = _errs(y16, ref)
    mbf, xbf = _errs(ybf, ref)
    mag = max(1.0, float(np.abs(ref).max()))
    print(f"F16ERR {what}: f16 mean {m16:.3e} max {x16:.3e} | bf16 mean {mbf:.3e} max {xbf:.3e} | ratio mean "
          f"{mbf / max(m16, 1e-30):.2f} max {xbf / max(x16, 1e-30):.2f} | mag {mag:.3g} rel mean {m16 / mag:.3e} max {x16 / mag:.3e}")
    assert m16 <= MEAN_RATIO * mbf, (what, m16, mbf)
    assert x16 <= MAX_RATIO * xbf, (what, x16, xbf)
    if absolute:
        assert m16 <= F16_MEAN * mag, (what, m16, mag)
        assert x16 <= F16_MAX * mag, (what, x16, mag)


# ---- 1: the yaml generator at cfg2 -----------------------------------------------------------------------------------

def test_default_generator_vs_oracle_and_bfloat16(dev):
    """8 x 600 frames with and without a speaker embedding, and one utterance alone."""
    O = _oracle()
    cfg = S.FULL_CONFIG
    sd = S.synth_state_dict(cfg, 201)
    wf = S.fold_weight_norm(sd)
    B, F = 8, 600
    b = S.synth_batch(cfg, B, F, 202)
    p16 = A.Plan(cfg, storage="float16", compact_workspace=True)
    pbf = A.Plan(cfg, storage="bfloat16", compact_workspace=True)
    blob = p16.pack(sd).to(dev)
    for spk in (True, False):
        emb = b.spk_emb if spk else None
        ins = [_t(dev, a) for a in (b.ppg, b.sine, b.lft, emb)]
        y16 = p16.forward(blob, *ins).cpu().numpy()
        ybf = pbf.forward(blob, *ins).cpu().numpy()
        ref = O.forward_dedup(wf, cfg.upsampling_scales, b.ppg, b.sine, b.lft, emb, dtype=torch.float64).numpy()
        _check_pair(y16, ybf, ref, f"cfg2/{'spk' if spk else 'nospk'}")
    one = [_t(dev, a[:1]) for a in (b.ppg, b.sine, b.lft, b.spk_emb)]
    y16 = p16.forward(blob, *one).cpu().numpy()
    ybf = pbf.forward(blob, *one).cpu().numpy()
    ref = O.forward_dedup(wf, cfg.upsampling_scales, b.ppg[:1], b.sine[:1], b.lft[:1], b.spk_emb[:1], dtype=torch.float64).numpy()
    _check_pair(y16, ybf, ref, "cfg2/one utterance")


# ---- 2: the configuration matrix -------------------------------------------------------------------------------------

B_FULL, F_FULL = 2, 24
LENS, F_PAD = [28, 25, 22, 23, 7, 1], 28          # n mod 4 in {0, 1, 2, 3} and a single frame
SEED_X_FULL, SEED_X_RAGGED = 621, 622
MATRIX = [(n, spk) for n in CM.NAMES for spk in CM.speaker_modes(n)]
MATRIX_IDS = [f"{n}-{'spk' if spk else 'nospk'}" for n, spk in MATRIX]
_W, _P = {}, {}


def _weights(name):
    if name not in _W:
        sd = S.synth_state_dict(CM.config(name), CM.SEED_W)
        _W[name] = (sd, S.fold_weight_norm(sd))
    return _W[name]


def _plan(name, storage, dev):
    if (name, storage) not in _P:
        plan = A.Plan(CM.config(name), storage=storage)
        _P[(name, storage)] = (plan, plan.pack(_weights(name)[0]).to(dev))
    return _P[(name, storage)]


@pytest.mark.parametrize("name,spk", MATRIX, ids=MATRIX_IDS)
def test_config_matrix_full_batch(dev, name, spk):
    O = _oracle()
    cfg = CM.config(name)
    b = S.synth_batch(cfg, B_FULL, F_FULL, SEED_X_FULL)
    ins = [_t(dev, a) for a in (b.ppg, b.sine, b.lft)] + [_t(dev, b.spk_emb) if spk else None]
    ys = {st: _plan(name, st, dev)[0].forward(_plan(name, st, dev)[1], *ins).cpu().numpy() for st in ("float16", "bfloat16")}
    ref = O.forward_dedup(_weights(name)[1], cfg.upsampling_scales, b.ppg, b.sine, b.lft, b.spk_emb if spk else None,
                          dtype=torch.float64).numpy()
    assert ys["float16"].shape == ref.shape
    _check_pair(ys["float16"], ys["bfloat16"], ref, f"{name}/{spk}/full", absolute=False)


@pytest.mark.parametrize("name,spk", MATRIX, ids=MATRIX_IDS)
def test_config_matrix_ragged_batch_with_poisoned_padding(dev, name, spk):
    """Padded F = 28, lengths 28 / 25 / 22 / 23 / 7 / 1, garbage in the inputs' padding, the workspace filled with
    float32 1000.0 and with bytes 0xFF: the valid samples of the whole batch against every utterance's oracle run alone
    (the two ratios over all of them together), the output's padding exactly zero."""
    O = _oracle()
    cfg = CM.config(name)
    hop = cfg.hop
    b = S.synth_batch(cfg, len(LENS), F_PAD, SEED_X_RAGGED)
    ppg, sine, lft = b.ppg.copy(), b.sine.copy(), b.lft.copy()
    for i, n in enumerate(LENS):
        ppg[i, :, n:] = 1e3; sine[i, :, n * hop:] = -1e3; lft[i, :, n * hop:] = 1e3
    ins = [_t(dev, a) for a in (ppg, sine, lft)] + [_t(dev, b.spk_emb) if spk else None]
    refs = [O.forward_dedup(_weights(name)[1], cfg.upsampling_scales, b.ppg[j:j + 1, :, :n], b.sine[j:j + 1, :, :n * hop],
                            b.lft[j:j + 1, :, :n * hop], b.spk_emb[j:j + 1] if spk else None, dtype=torch.float64).numpy()
            for j, n in enumerate(LENS)]
    ref = np.concatenate([r.reshape(-1) for r in refs])
    for fill in ("1000", "0xFF"):
        ys = {}
        for st in ("float16", "bfloat16"):
            plan, blob = _plan(name, st, dev)
            ws = torch.empty(plan.workspace_bytes(len(LENS), F_PAD) // 4 * 4 + 4, dtype=torch.uint8, device=dev)
            if fill == "0xFF":
                ws.fill_(0xFF)
            else:
                ws[: ws.numel() // 4 * 4].view(torch.float32).fill_(float(fill))
            y = plan.forward(blob, *ins, lengths=LENS, workspace=ws).cpu().numpy()
            assert np.isfinite(y).all(), (st, fill)
            for j, n in enumerate(LENS):
                assert not y[j, :, n * hop:].any(), (st, fill, j)
            ys[st] = np.concatenate([y[j, :, :n * hop].reshape(-1) for j, n in enumerate(LENS)])
        _check_pair(ys["float16"], ys["bfloat16"], ref, f"{name}/{spk}/ragged/{fill}", absolute=False)


# ---- 3: taps ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spk", [True, False], ids=["spk", "nospk"])
def test_workspace_taps_vs_oracle(dev, spk):
    """down_lft.k, down_sine.k, ss.k, up.k.xmid, up.k.out of the yaml generator at 2 x 40 frames (weights and inputs of
    range_cases `base`): each within 2^-7 of the oracle tap's own maximum.  A forward that ran bfloat16 kernels on
    binary16 data (or the reverse) fails here by orders of magnitude."""
    O = _oracle()
    cfg = S.FULL_CONFIG
    sd, b, _ = RC.build_case(cfg, "base")
    B, F = RC.B, RC.F
    plan = A.Plan(cfg, storage="float16")
    plan.keep_last_block_output(B, F)
    blob = plan.pack(sd).to(dev)
    ws = torch.zeros(plan.workspace_bytes(B, F), dtype=torch.uint8, device=dev)
    emb = b.spk_emb if spk else None
    y = plan.forward(blob, *[_t(dev, a) for a in (b.ppg, b.sine, b.lft, emb)], workspace=ws)
    torch.cuda.synchronize()
    ref, taps = O.forward_dedup(S.fold_weight_norm(sd), cfg.upsampling_scales, b.ppg, b.sine, b.lft, emb,
                                dtype=torch.float64, return_taps=True)
    worst = 0.0
    n = cfg.n_stages
    for k in range(n):
        got = {}
        h = plan.tap(f"down_h.{k}", B, F, ws)
        assert h.dtype == torch.float16
        h = h.double().cpu()
        got[f"down_lft.{k}"], got[f"down_sine.{k}"] = h[:B], h[B:2 * B]
        ss = plan.tap(f"ss.{k}", B, F, ws).double().cpu()
        want_ss = torch.cat([taps[f"scale.{k}"], taps[f"shift.{k}"]], dim=1)
        for name in (f"up.{k}.xmid", f"up.{k}.out"):
            got[name] = plan.tap(name, B, F, ws).double().cpu()
        pairs = [(nm, g, taps[nm]) for nm, g in got.items()] + [(f"ss.{k}", ss, want_ss)]
        for nm, g, want in pairs:
            assert tuple(g.shape) == tuple(want.shape), (nm, g.shape, want.shape)
            mag = float(want.abs().max())
            rel = float((g - want).abs().max()) / mag
            worst = max(worst, rel)
            print(f"F16TAP {'spk' if spk else 'nospk'} {nm}: {rel:.3e} of its maximum {mag:.3g}")
            assert rel <= TAP_TOL, (nm, rel, mag)
    print(f"F16TAP worst {worst:.3e}")
    assert torch.isfinite(y).all()


# ---- 4: routes agree with each other ---------------------------------------------------------------------------------
# Bit-identical where the bfloat16 tests demand it.  Where two routes round the same tensors but sum in another order in
# front of a rounding, each test states where its bound comes from (no bound is taken from what the code gives).

def test_routes_pipeline_and_phase_kernels_are_bit_identical(dev):
    """Conditioning stages 0 / 1 as layer pipelines (launch-table algorithm 5) and as phase kernels (4) at 8 x 600 frames:
    same products in the same order - identical bits, as the bfloat16 test demands."""
    cfg = S.FULL_CONFIG
    sd = S.synth_state_dict(cfg, 61)
    B, F = 8, 600
    T = F * cfg.hop

    def plan_for(algo):
        pl = A.Plan(cfg, storage="float16", compact_workspace=True)
        pl.load_tuned({f"cond.0|{B}|{T}|h": [1, 1, 1, 1, algo], f"cond.1|{B}|{T // 5}|h": [1, 1, 1, 1, algo]})
        return pl

    pipe, phase = plan_for(5), plan_for(4)
    blob = pipe.pack(sd).to(dev)
    ins = list(S.device_batch(cfg, B, F, 4321, dev))
    wp = torch.full((pipe.workspace_bytes(B, F),), 0xFF, dtype=torch.uint8, device=dev)
    wq = torch.full((phase.workspace_bytes(B, F),), 0xFF, dtype=torch.uint8, device=dev)
    rp, rq = [], []
    yp = pipe.forward(blob, *ins, workspace=wp, profile=rp)
    yq = phase.forward(blob, *ins, workspace=wq, profile=rq)
    torch.cuda.synchronize()
    kp = {r["layer"]: r["kernel"] for r in rp}
    kq = {r["layer"]: r["kernel"] for r in rq}
    assert kp["cond.0"] == "cond_stage0_pipe<h1>" and kp["cond.1"] == "cond_stage1_pipe<h1>", kp
    assert kq["cond.0"] == "cond_stage0<h1>" and kq["cond.1"] == "cond_stage1<h1>", kq
    for t in ("ss.0", "down_hd.1", "ss.1", "down_hd.2"):
        assert torch.equal(pipe.tap(t, B, F, wp), phase.tap(t, B, F, wq)), t
    assert torch.equal(yp, yq)
    assert torch.isfinite(yp).all()


# The bfloat16 tests' bounds for two routes that round the same tensors but sum in another order in front of a rounding
# (tests/test_parity_gpu.py) are differences of roundings, so they scale with the format's ulp: binary16's is 1/8 of
# bfloat16's.  Same shapes and seeds as those tests, their bounds / 8.
ULP = 1.0 / 8.0


def test_routes_residual_conv_folded_into_d3(dev):
    """`up.<i>.d3x` against the separate residual launches (test_residual_conv_folded_into_d3's bfloat16 arm): waveform
    mean 1e-2 / 8, max 0.2 / 8; the xmid / u2 / out taps of the two plans within 4e-2 / 8 of each other and 6e-2 / 8 of
    the oracle (x max(1, |tap|max)); a ragged batch against every utterance alone.  Both routes meet the two ratios."""
    O = _oracle()
    cfg = S.FULL_CONFIG
    sd = S.synth_state_dict(cfg, 91)
    B, F = 3, 52
    b = S.synth_batch(cfg, B, F, 92)
    ins = [_t(dev, a) for a in (b.ppg, b.sine, b.lft, b.spk_emb)]
    fused, sep = A.Plan(cfg, storage="float16"), A.Plan(cfg, storage="float16")
    for pl in (fused, sep):
        pl.keep_last_block_output(B, F)
    sep.keep_residual_convs_separate(B, F)
    blob = fused.pack(sd).to(dev)
    ref, taps = O.forward_dedup(S.fold_weight_norm(sd), cfg.upsampling_scales, b.ppg, b.sine, b.lft, b.spk_emb,
                                dtype=torch.float64, return_taps=True)
    ws_f = torch.zeros(fused.workspace_bytes(B, F), dtype=torch.uint8, device=dev)
    ws_s = torch.zeros(sep.workspace_bytes(B, F), dtype=torch.uint8, device=dev)
    recs, recs_s = [], []
    y_f = fused.forward(blob, *ins, workspace=ws_f, profile=recs)
    y_s = sep.forward(blob, *ins, workspace=ws_s, profile=recs_s)
    torch.cuda.synchronize()
    layers = {r["layer"]: r["kernel"] for r in recs}
    for i, s in enumerate(cfg.upsampling_scales):
        assert layers[f"up.{i}.d3x"].split(",")[4:7] == ["0", "4", str(s)], layers
        assert layers[f"up.{i}.d3x"].endswith("h1>"), layers[f"up.{i}.d3x"]
        assert f"up.{i}.res_stretch" not in layers and f"up.{i}.d3" not in layers
        assert f"up.{i}.res_stretch" in {r["layer"] for r in recs_s} and f"up.{i}.d3x" not in {r["layer"] for r in recs_s}
    ybf = A.Plan(cfg, storage="bfloat16").forward(blob, *ins).cpu().numpy()
    _check_pair(y_f.cpu().numpy(), ybf, ref.numpy(), "route/d3x", absolute=False)
    _check_pair(y_s.cpu().numpy(), ybf, ref.numpy(), "route/separate residual", absolute=False)
    d = (y_f - y_s).abs()
    print(f"F16ROUTE d3x vs separate: mean {float(d.mean()):.3e} max {float(d.max()):.3e}")
    assert float(d.mean()) <= 1e-2 * ULP and float(d.max()) <= 0.2 * ULP
    for i in range(cfg.n_stages):
        for name in ("xmid", "u2", "out"):
            got, want = fused.tap(f"up.{i}.{name}", B, F, ws_f).double().cpu(), taps[f"up.{i}.{name}"]
            other = sep.tap(f"up.{i}.{name}", B, F, ws_s).double().cpu()
            mag = max(1.0, float(want.abs().max()))
            e_o, e_r = float((got - want).abs().max()) / mag, float((got - other).abs().max()) / mag
            print(f"F16ROUTE up.{i}.{name}: d3x vs oracle {e_o:.3e}, vs separate {e_r:.3e} (x max(1, |tap|max))")
            assert e_o <= 6e-2 * ULP, (i, name, e_o)
            assert e_r <= 4e-2 * ULP, (i, name, e_r)
    lengths = [52, 28, 12]
    y_r = fused.forward(blob, *ins, lengths=lengths)
    for j, n in enumerate(lengths):
        alone = fused.forward(blob, ins[0][j:j + 1, :, :n].contiguous(), ins[1][j:j + 1, :, :n * cfg.hop].contiguous(),
                              ins[2][j:j + 1, :, :n * cfg.hop].contiguous(), ins[3][j:j + 1])
        dj = (y_r[j:j + 1, :, :n * cfg.hop] - alone).abs()
        assert float(dj.max()) <= 0.2 * ULP and float(dj.mean()) <= 1e-2 * ULP, (j, n, float(dj.max()), float(dj.mean()))
        if n < F:
            assert float(y_r[j, :, n * cfg.hop:].abs().max()) == 0.0


def test_routes_conv_last_on_the_last_block(dev):
    """conv_last in the last block's epilogue against its own launch (test_conv_last_rides_on_the_last_block: 0.1 in
    bfloat16 storage -> 0.1 / 8), full and ragged; the padding stays zero."""
    cfg = S.FULL_CONFIG
    sd = S.synth_state_dict(cfg, 95)
    B, F = 2, 52
    b = S.synth_batch(cfg, B, F, 96)
    ins = [_t(dev, a) for a in (b.ppg, b.sine, b.lft, b.spk_emb)]
    ys = []
    for keep in (False, True):
        plan = A.Plan(cfg, load_shipped_table=False, storage="float16")
        if keep:
            plan.keep_last_block_output(B, F)
        blob = plan.pack(sd).to(dev)
        recs = []
        y = plan.forward(blob, *ins, profile=recs).cpu()
        yr = plan.forward(blob, *ins, lengths=[52, 20]).cpu()
        assert ("conv_last" in {r["layer"] for r in recs}) == keep
        assert float(yr[1, :, 20 * cfg.hop:].abs().max()) == 0.0
        ys.append((y, yr))
    print(f"F16ROUTE conv_last fused vs own launch: max {float((ys[0][0] - ys[1][0]).abs().max()):.3e}, "
          f"ragged {float((ys[0][1] - ys[1][1]).abs().max()):.3e}")
    assert float((ys[0][0] - ys[1][0]).abs().max()) <= 0.1 * ULP
    assert float((ys[0][1] - ys[1][1]).abs().max()) <= 0.1 * ULP


def test_routes_whole_stage_conditioning_launches(dev):
    """The compact-workspace plan (conditioning stages 0 / 1 as ONE launch each, what the module runs) against the
    separate launches of the default layout (test_bfloat16_activation_storage_mode: mean 1e-2 -> 1e-2 / 8)."""
    cfg = S.FULL_CONFIG
    sd = S.synth_state_dict(cfg, 81)
    B, F = 2, 48
    b = S.synth_batch(cfg, B, F, 82)
    ins = [_t(dev, a) for a in (b.ppg, b.sine, b.lft, b.spk_emb)]
    sep, whole = A.Plan(cfg, storage="float16"), A.Plan(cfg, storage="float16", compact_workspace=True)
    blob = sep.pack(sd).to(dev)
    rs, rw = [], []
    y_s = sep.forward(blob, *ins, profile=rs)
    y_w = whole.forward(blob, *ins, profile=rw)
    assert "cond.0" in {r["layer"] for r in rw} and "cond.0" not in {r["layer"] for r in rs}
    d = (y_s - y_w).abs()
    print(f"F16ROUTE whole-stage vs separate conditioning launches: mean {float(d.mean()):.3e} max {float(d.max()):.3e}")
    assert float(d.mean()) <= 1e-2 * ULP


def test_routes_fused_pairs_match_the_separate_launches(dev):
    """A down stage's c2 -> c3 pair, stage 0's c1 -> c2 -> c3 and the FiLM conv -> heads pair as ONE launch each (kernel
    modes 6 / 7, the binary16 `hxc` fragment sets) against the separate launches, which algorithm 0 under the fused keys
    ("|h") selects: test_fused_conditioning_stages_match_the_separate_launches in float16 storage, its bfloat16 bound
    (0.25) / 8 on the waveform against the oracle, fused against separate (full and ragged) and every ragged utterance
    against itself alone."""
    O = _oracle()
    cfg = S.FULL_CONFIG
    sd = S.synth_state_dict(cfg, 91)
    B, F = 3, 44
    lengths = [44, 29, 8]
    b = S.synth_batch(cfg, B, F, 92)
    ins = [_t(dev, a) for a in (b.ppg, b.sine, b.lft, b.spk_emb)]
    hop = cfg.hop
    n = cfg.n_stages
    Ts, T = [], F * hop
    for k in range(n):
        T //= ([1] + list(reversed(cfg.upsampling_scales[1:])))[k]
        Ts.append(T)
    unfused = {f"down.{k}.c23|{B}|{Ts[k]}|h": [3, 1, 4, 1, 0] for k in range(n)}
    unfused.update({f"film.{k}.chain|{B}|{Ts[k]}|h": [3, 1, 4, 1, 0] for k in range(n)})
    unfused[f"down.0.c123|{B}|{Ts[0]}|h"] = [3, 1, 4, 1, 0]
    outs = {}
    for name, table in (("fused", {}), ("separate", unfused)):
        plan = A.Plan(cfg, load_shipped_table=False, storage="float16")
        plan.load_tuned(table)
        blob = plan.pack(sd).to(dev)
        recs = []
        y = plan.forward(blob, *ins, profile=recs)
        yr = plan.forward(blob, *ins, lengths=lengths)
        modes = sorted({int(r["kernel"].split(",")[4]) for r in recs if r["kernel"].startswith("conv_hx")})
        layers = {r["layer"] for r in recs}
        assert all(r["kernel"].endswith("h1>") for r in recs if r["kernel"].startswith("conv_hx")), recs
        assert ("film.0.chain" in layers) == (name == "fused") and ("film.0.heads" in layers) == (name != "fused")
        outs[name] = (y.cpu(), yr.cpu(), modes, len(recs))
    assert 6 in outs["fused"][2] and 7 in outs["fused"][2]
    assert 6 not in outs["separate"][2] and 7 not in outs["separate"][2]
    assert outs["fused"][3] < outs["separate"][3]
    ref = O.forward_dedup(S.fold_weight_norm(sd), cfg.upsampling_scales, b.ppg, b.sine, b.lft, b.spk_emb)
    close = 0.25 * ULP
    for name in outs:
        assert float((outs[name][0] - ref).abs().max()) <= close, name
    d0, d1 = (outs["fused"][0] - outs["separate"][0]).abs(), (outs["fused"][1] - outs["separate"][1]).abs()
    print(f"F16ROUTE fused pairs vs separate: max {float(d0.max()):.3e} mean {float(d0.mean()):.3e}, ragged max {float(d1.max()):.3e}")
    assert float(d0.max()) <= close and float(d1.max()) <= close
    plan = A.Plan(cfg, load_shipped_table=False, storage="float16")
    blob = plan.pack(sd).to(dev)
    for i, L in enumerate(lengths):
        one = plan.forward(blob, *[t[i:i + 1, ..., :L * (hop if t.shape[-1] == F * hop else 1)].contiguous() for t in ins[:3]],
                           ins[3][i:i + 1]).cpu()
        assert float((outs["fused"][1][i:i + 1, ..., :L * hop] - one).abs().max()) <= close, i


def _wide_table(B, F, tpw=2):
    """launch-table entries (float16 storage) that put every eligible layer on conv_wx (algorithm 6); the table of
    tests/test_wide_gpu.py under the "|h" keys"""
    t = {}
    for layer, T in [
        ("film.2.heads", 8 * F), ("down.3.c2_d2", 2 * F), ("down.3.c3_d4", 2 * F), ("film.3.conv", 2 * F), ("film.3.heads", 2 * F),
        ("up.0.conv_first", F), ("up.0.d9", 2 * F), ("up.0.d27", 2 * F),
    ]:
        t[f"{layer}|{B}|{T}|h"] = [6, 4, 2, tpw, 6]
    for k in (2, 3):
        t[f"down.{k}.c23|{B}|{(8 if k == 2 else 2) * F}|h"] = [1, 1, 4, 1, 0]      # c2 / c3 as separate launches
    return t


WIDE_LAYERS = {"film.2.heads", "down.3.c2_d2", "down.3.c3_d4", "film.3.conv", "film.3.heads", "up.0.conv_first", "up.0.d9", "up.0.d27"}


@pytest.mark.parametrize("B,F,lens", [(2, 96, None), (3, 140, None), (3, 100, [100, 64, 36])])
def test_routes_wide_layer_kernel_equals_the_wave_specialised_kernels(dev, B, F, lens):
    """conv_wx (launch-table algorithm 6) on the wide layers against conv_hx: tests/test_wide_gpu.py's test in float16
    storage, the same three batches (the ragged one exercises conv_wx's row ends and the fall-back to conv_hx's tail
    instances).  Same products in the same order, so the conditioning tensors are bit-identical; behind an InstanceNorm
    (float64 atomics, order-dependent last bit) a staged value's rounding flips here and there.  A flip is one binary16
    ulp, an eighth of a bfloat16 one, so the largest difference of a block output gets that test's bound / 8 (2^-9 of
    the maximum); a finer format flips more often by as much as each flip is smaller, so the mean difference, the sums
    and the waveform (flips propagated through the later blocks) keep the bounds that test states."""
    cfg = S.FULL_CONFIG
    sd = S.synth_state_dict(cfg, 91)
    b = S.synth_batch(cfg, B, F, 92)
    ins = [_t(dev, a) for a in (b.ppg, b.sine, b.lft, b.spk_emb)]
    ref = A.Plan(cfg, storage="float16", load_shipped_table=False)
    ref.load_tuned({k: v for k, v in _wide_table(B, F).items() if ".c23|" in k})
    blob = ref.pack(sd).to(dev)
    ws_r = torch.zeros(ref.workspace_bytes(B, F), dtype=torch.uint8, device=dev)
    recs_r = []
    y_r = ref.forward(blob, *ins, workspace=ws_r, profile=recs_r, lengths=lens)
    assert not any(r["kernel"].startswith("conv_wx<") for r in recs_r)
    wide = A.Plan(cfg, storage="float16", load_shipped_table=False)
    wide.load_tuned(_wide_table(B, F))
    ws_w = torch.empty(wide.workspace_bytes(B, F), dtype=torch.uint8, device=dev)
    ws_w.fill_(0xFF)
    recs_w = []
    y_w = wide.forward(blob, *ins, workspace=ws_w, profile=recs_w, lengths=lens)
    on_wx = {r["layer"]: r["kernel"] for r in recs_w if r["kernel"].startswith("conv_wx<")}
    expect = WIDE_LAYERS if lens is None else {l for l in WIDE_LAYERS if l.startswith("film.2.")}
    assert set(on_wx) == expect, sorted(expect ^ set(on_wx))
    assert all(k.endswith("h1>") for k in on_wx.values()), on_wx

    def valid(t):
        if lens is None:
            return t
        rate = t.shape[-1] // F
        assert t.shape[0] // B in (1, 2)
        return torch.cat([t[j, :, : lens[j % B] * rate].reshape(-1) for j in range(t.shape[0])])

    for tap in ("down_c2.2", "down_h.2", "film_u.2", "ss.2", "down_c2.3", "down_h.3", "film_u.3", "ss.3"):
        a, c = valid(ref.tap(tap, B, F, ws_r)), valid(wide.tap(tap, B, F, ws_w))
        assert a.dtype == torch.float16 and torch.equal(a, c), (tap, float((a.float() - c.float()).abs().max()))
    for tap in ("up.0.out", "up.1.out"):
        a, c = valid(ref.tap(tap, B, F, ws_r)).float(), valid(wide.tap(tap, B, F, ws_w)).float()
        print(f"F16ROUTE conv_wx vs conv_hx {B}x{F} {tap}: max {float((a - c).abs().max()) / float(a.abs().max()):.3e} of its "
              f"maximum, mean {float((a - c).abs().mean()) / float(a.abs().mean()):.3e} of its mean")
        assert float((a - c).abs().max()) <= 2.0 ** -9 * float(a.abs().max()), tap
        assert float((a - c).abs().mean()) <= 2e-3 * float(a.abs().mean()), tap
    for i in (0, 1):
        a, c = ref.tap(f"up.{i}.stats", B, F, ws_r), wide.tap(f"up.{i}.stats", B, F, ws_w)      # (3B, C, 2): sum, sum of squares
        n = (2 if i == 0 else 8) * F
        scale = (a[..., 1] * n).sqrt() + 1.0                                                      # >= sum |u|
        assert float(((a[..., 0] - c[..., 0]).abs() / scale).max()) <= 2e-3, i
        assert float(((a[..., 1] - c[..., 1]).abs() / (a[..., 1] + 1.0)).max()) <= 2e-3, i
    ya, yc = (y_r, y_w) if lens is None else (torch.cat([y_r[j, :, : lens[j] * cfg.hop].reshape(-1) for j in range(B)]),
                                              torch.cat([y_w[j, :, : lens[j] * cfg.hop].reshape(-1) for j in range(B)]))
    print(f"F16ROUTE conv_wx vs conv_hx {B}x{F} waveform: max {float((ya - yc).abs().max()):.3e}")
    assert float((ya - yc).abs().max()) <= 2e-2 * max(1.0, float(ya.abs().max()))


# ---- 5: the range contract -------------------------------------------------------------------------------------------

def test_range_contract(dev):
    """tests/range_cases.py: a case qualifies when every tap the oracle returns stays at or below 2^14 in magnitude.
    Qualifying cases meet the two ratios.  The others are outside the contract: the call returns (FASTSVC_OK: forward
    raises otherwise), and a following float16 forward of `base` on the same workspace gives the bits it gave before."""
    O = _oracle()
    cfg = S.FULL_CONFIG
    B, F = RC.B, RC.F
    p16 = A.Plan(cfg, storage="float16")
    pbf = A.Plan(cfg, storage="bfloat16")
    ws = torch.zeros(p16.workspace_bytes(B, F), dtype=torch.uint8, device=dev)
    sd0, b0, _ = RC.build_case(cfg, "base")
    blob0 = p16.pack(sd0).to(dev)
    ins0 = [_t(dev, a) for a in (b0.ppg, b0.sine, b0.lft, b0.spk_emb)]
    y_base = p16.forward(blob0, *ins0, workspace=ws).clone()
    qualified, outside = [], []
    for name in RC.CASES:
        sd, b, spk = RC.build_case(cfg, name)
        emb = b.spk_emb if spk else None
        ref, taps = O.forward_dedup(S.fold_weight_norm(sd), cfg.upsampling_scales, b.ppg, b.sine, b.lft, emb,
                                    dtype=torch.float64, return_taps=True)
        top = max(float(t.abs().max()) for t in taps.values())
        blob = p16.pack(sd).to(dev)
        ins = [_t(dev, a) for a in (b.ppg, b.sine, b.lft, emb)]
        y16 = p16.forward(blob, *ins, workspace=ws).cpu().numpy()
        if top <= 2.0 ** 14:
            qualified.append(name)
            ybf = pbf.forward(blob, *ins).cpu().numpy()
            _check_pair(y16, ybf, ref.numpy(), f"range/{name} (largest tap {top:.3g})", absolute=False)
        else:
            outside.append(name)
            print(f"F16RANGE outside the contract: {name} (largest tap {top:.3g}), finite output: {bool(np.isfinite(y16).all())}")
            again = p16.forward(blob0, *ins0, workspace=ws)
            assert torch.equal(again, y_base), name
    print("F16RANGE qualified:", qualified)
    print("F16RANGE outside:", outside)
    assert len(qualified) >= 14 and len(qualified) + len(outside) == len(RC.CASES) == 23


# ---- 6: determinism --------------------------------------------------------------------------------------------------

def test_determinism_at_cfg3_and_batch_permutation(dev):
    """Two forwards of 64 x 1500 frames give identical bits; a permuted batch gives the permuted result within the
    jitter bound of the bfloat16 / float32 test (2e-5: the float64 InstanceNorm sums are accumulated atomically)."""
    cfg = S.FULL_CONFIG
    plan = A.Plan(cfg, storage="float16", compact_workspace=True)
    blob = plan.pack(S.synth_state_dict(cfg, 201)).to(dev)
    ins = list(S.device_batch(cfg, 64, 1500, 7, dev))
    ws = torch.empty(plan.workspace_bytes(64, 1500), dtype=torch.uint8, device=dev)
    y1 = plan.forward(blob, *ins, workspace=ws).clone()
    y2 = plan.forward(blob, *ins, workspace=ws).clone()
    assert torch.isfinite(y1).all()
    assert torch.equal(y1, y2)
    del ws, y1, y2, ins
    b = S.synth_batch(cfg, 3, 600, 10)
    small = [_t(dev, a) for a in (b.ppg, b.sine, b.lft, b.spk_emb)]
    perm = torch.tensor([2, 0, 1], device=dev)
    ya = plan.forward(blob, *small)
    yp = plan.forward(blob, *[t[perm].contiguous() for t in small])
    assert float((ya[perm] - yp).abs().max()) <= 2e-5


# ---- 7: decode -------------------------------------------------------------------------------------------------------

def test_decode_utterances_in_float16_storage(dev):
    """decode_utterances with activation_storage = "float16" on the inputs of tests/golden/decode_chain.npz: the PCM-16
    waveform within PCM_STEPS of the golden one."""
    from conftest import load_golden
    from svcc23_fastsvc_amd import decode as D
    g = load_golden("decode_chain.npz")
    cfg = S.FULL_CONFIG
    frames = [int(v) for v in g["frames"]]
    batches = [S.synth_batch(cfg, 1, F, 400 + i) for i, F in enumerate(frames)]
    feats = [dict(f0=b.f0[0].T.copy(), ppg=b.ppg[0].T.copy(), lft=b.lft[0].T.copy()) for b in batches]
    sd = S.synth_state_dict(cfg, int(g["meta"][0]))
    worst = {}
    for storage in ("float16", "bfloat16"):
        m = A.FastSVCGenerator(in_channels=cfg.in_channels, mid_channels=list(cfg.mid_channels),
                               upsampling_scales=list(cfg.upsampling_scales), out_channels=cfg.out_channels,
                               spk_emb_size=cfg.spk_emb_size, use_spk_emb=cfg.use_spk_emb)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        m.remove_weight_norm()
        m.activation_storage = storage
        m = m.eval().to(dev)
        sg = A.SignalGenerator(sample_rate=24000, hop_size=cfg.hop, sine_amp=0.1, noise_amp=0.0, signal_types=["sine"])
        ys = D.decode_utterances(m, feats, sg, dev, trg_emb=batches[0].spk_emb, src_f0_stats=[g["srcstats"]] * 3,
                                 trg_f0_stats=g["trgstats"], max_batch=8, pad_tolerance=0.9)
        worst[storage] = 0
        for i, y in enumerate(ys):
            pcm, want = D.to_pcm16(y).astype(np.int64), D.to_pcm16(g[f"y.{i}"]).astype(np.int64)
            assert pcm.shape == want.shape == (frames[i] * cfg.hop,)
            worst[storage] = max(worst[storage], int(np.abs(pcm - want).max()))
    print(f"F16DECODE worst PCM-16 difference: float16 {worst['float16']} steps, bfloat16 {worst['bfloat16']} steps")
    assert worst["float16"] <= PCM_STEPS, worst
