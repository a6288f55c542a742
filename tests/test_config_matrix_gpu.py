"""Parity matrix over generator configurations (tests/config_matrix.py) x activation storage x speaker mode (-m gpu).

The kernels pick their route from the channel count, the stretch factor S, the row rate of each tensor relative to the
frame rate, the storage dtype, whether a speaker embedding is given and the launch table.  Every case here runs the
HIP forward against the float64 oracle (pinned to the live reference at these configurations by
tests/test_oracle_golden.py::test_oracle_against_live_reference_on_the_config_matrix) and asserts the route each up
block's residual conv took, so that a route gate which disagrees with its kernel fails here.

Bounds: float32 storage holds the suite's TIGHT * max(1, |ref|max).  bfloat16 storage holds the bound
tools/stress_parity.py states (mean-abs <= 3e-2 x rms of the reference; 5e-2 for a 1-frame utterance) and a max-abs
bound of BF16_MAX x max(1, |ref|max).  Observed on the MI355X over every bfloat16 case here: mean-abs up to 2.6e-2 x rms
(3.1e-2 for the 1-frame utterance), max-abs up to 6.1e-2 x max(1, |ref|max) (s2_second, 13 frames through the padding
route) - BF16_MAX is twice that."""
import numpy as np
import pytest
import torch

import config_matrix as CM
import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import synth as S

pytestmark = pytest.mark.gpu

TIGHT = 1e-4
BF16_MEAN = 3e-2            # x rms of the reference (tools/stress_parity.py)
BF16_MEAN_1F = 5e-2         # ... a 1-frame utterance
BF16_MAX = 0.13             # x max(1, |ref|max)
B_FULL, F_FULL = 2, 24
LENS, F_PAD = [28, 25, 22, 23, 7, 1], 28          # n mod 4 in {0, 1, 2, 3} and a single frame
SEED_X_FULL, SEED_X_RAGGED = 621, 622

CASES = [(n, st, spk) for n in CM.NAMES for st in ("float32", "bfloat16") for spk in CM.speaker_modes(n)]
CASE_IDS = [f"{n}-{st}-{'spk' if spk else 'nospk'}" for n, st, spk in CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    A.load_library()
    return torch.device("cuda:0")


def _t(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_WEIGHTS, _PLANS, _ORACLE = {}, {}, {}


def _weights(name):
    if name not in _WEIGHTS:
        sd = S.synth_state_dict(CM.config(name), CM.SEED_W)
        _WEIGHTS[name] = (sd, S.fold_weight_norm(sd))
    return _WEIGHTS[name]


def _plan(name, storage, dev):
    if (name, storage) not in _PLANS:
        plan = A.Plan(CM.config(name), storage=storage)
        _PLANS[(name, storage)] = (plan, plan.pack(_weights(name)[0]).to(dev))
    return _PLANS[(name, storage)]


def _batch(name, ragged):
    cfg = CM.config(name)
    return S.synth_batch(cfg, len(LENS), F_PAD, SEED_X_RAGGED) if ragged else S.synth_batch(cfg, B_FULL, F_FULL, SEED_X_FULL)


def _oracle(name, spk, ragged):
    """float64 oracle: the full batch, or every utterance of the ragged batch alone at its own length (with taps)"""
    key = (name, spk, tuple(LENS) if ragged else None)
    if key not in _ORACLE:
        from oracle import fastsvc_oracle as O
        cfg = CM.config(name)
        wf = _weights(name)[1]
        b = _batch(name, ragged)
        run = lambda sl, n: O.forward_dedup(wf, cfg.upsampling_scales, b.ppg[sl, :, :n], b.sine[sl, :, :n * cfg.hop],
                                            b.lft[sl, :, :n * cfg.hop], b.spk_emb[sl] if spk else None,
                                            dtype=torch.float64, return_taps=True)
        if ragged:
            _ORACLE[key] = [run(slice(j, j + 1), n) for j, n in enumerate(LENS)]
        else:
            _ORACLE[key] = run(slice(0, B_FULL), F_FULL)
    return _ORACLE[key]


def _check_output(got, ref, storage, one_frame=False, what=""):
    """got, ref: float64 numpy arrays of the same shape"""
    err = np.abs(got - ref)
    mag = max(1.0, float(np.abs(ref).max()))
    if storage == "float32":
        assert float(err.max()) <= TIGHT * mag, (what, float(err.max()), mag)
    else:
        rms = float(np.sqrt(np.mean(ref ** 2)))
        bound = (BF16_MEAN_1F if one_frame else BF16_MEAN) * rms
        print(f"ERR {what} mean/rms {float(err.mean()) / rms:.3e} max/mag {float(err.max()) / mag:.3e}")
        assert float(err.mean()) <= bound, (what, float(err.mean()), rms)
        assert float(err.max()) <= BF16_MAX * mag, (what, float(err.max()), mag)


def _mw(c):                 # channel tile per output channel count (fastsvc_plan.cpp choose_mw): 16 * MW channels
    return 3 if c % 48 == 0 else 1 if c <= 16 else 2 if c <= 32 else 3


def _x2_instance(mw, nch32, s):     # conv_hx_x2_ok: the fused residual instances
    return (nch32 == 1 and s == 5) if mw == 2 else (s in (2, 4)) if mw == 3 else False


def fused_residual(cfg, i, storage, spk, ragged):
    """Whether up block i runs its stretched residual conv inside the d = 3 launch (`up.<i>.d3x`), from the gates of
    run_d3x: float32 storage without a speaker keeps the block on the exact float32 kernels; the instance must exist
    for (channel tile, K chunks, S); a ragged batch needs the d = 3 conv's rows a multiple of 4 frames' worth, and the
    bfloat16 S = 2 instances (4-column requests of the residual operand) need the operand's rows so as well."""
    s, C = cfg.upsampling_scales[i], cfg.mid_channels[i]
    rate = int(np.prod(cfg.upsampling_scales[: i + 1]))         # output columns per frame
    if storage == "float32" and not spk:
        return False
    if not _x2_instance(_mw(C), (C + 31) // 32, s):
        return False
    if ragged and rate % 4:
        return False
    if storage == "bfloat16" and s == 2 and ragged and (rate // s) % 4:
        return False
    return True


def _check_routes(recs, cfg, storage, spk, ragged, name):
    layers = {r["layer"]: r["kernel"] for r in recs}
    route = []
    for i, s in enumerate(cfg.upsampling_scales):
        if fused_residual(cfg, i, storage, spk, ragged):
            # conv_hx<MW,NW,WM,WN,mode 0,FiLM-affine epilogue 4,stretch factor,..>
            assert layers.get(f"up.{i}.d3x", "").split(",")[4:7] == ["0", "4", str(s)], (i, layers.get(f"up.{i}.d3x"))
            assert f"up.{i}.res_stretch" not in layers and f"up.{i}.d3" not in layers, i
            route.append(f"up.{i}:d3x")
        else:
            assert f"up.{i}.d3x" not in layers, (i, layers[f"up.{i}.d3x"])
            assert f"up.{i}.res_stretch" in layers and f"up.{i}.d3" in layers, i
            route.append(f"up.{i}:sep")
    if cfg.out_channels != 1:
        assert layers.get("conv_last") == "pointwise_out"        # (conv_last rides on the last block for one output only)
    print(f"ROUTE {name} {storage} {'spk' if spk else 'nospk'} {'ragged' if ragged else 'full'} " + " ".join(route))


@pytest.mark.parametrize("name,storage,spk", CASES, ids=CASE_IDS)
def test_full_batch_vs_oracle(dev, name, storage, spk):
    """B = 2, F = 24: the waveform against the float64 oracle; the residual conv's route per up block."""
    cfg = CM.config(name)
    plan, blob = _plan(name, storage, dev)
    b = _batch(name, False)
    recs = []
    y = plan.forward(blob, _t(dev, b.ppg), _t(dev, b.sine), _t(dev, b.lft), _t(dev, b.spk_emb) if spk else None,
                     profile=recs).cpu().double().numpy()
    ref = _oracle(name, spk, False)[0].numpy()
    assert y.shape == ref.shape == (B_FULL, cfg.out_channels, F_FULL * cfg.hop)
    _check_output(y, ref, storage, what=f"{name}/{storage}/{spk}/full")
    _check_routes(recs, cfg, storage, spk, False, name)


@pytest.mark.parametrize("name,storage,spk", CASES, ids=CASE_IDS)
def test_ragged_batch_with_poisoned_padding_vs_every_utterance_alone(dev, name, storage, spk):
    """Padded F = 28, lengths 28 / 25 / 22 / 23 / 7 / 1, garbage in the inputs' padding and a workspace filled with
    float32 1000.0, bytes 0xFF (NaN patterns) and float32 1e30 in turn: every utterance equals the oracle run alone at
    its own length, the output's padding is exactly zero.  The last 4 valid columns of every block's xmid (= the d = 3
    conv + the stretched residual conv, where a row end of the residual operand falls) against the oracle's taps.  The
    residual conv's route per up block (the first forward is profiled)."""
    cfg = CM.config(name)
    hop = cfg.hop
    plan, blob = _plan(name, storage, dev)
    b = _batch(name, True)
    B = len(LENS)
    ppg, sine, lft = b.ppg.copy(), b.sine.copy(), b.lft.copy()
    for i, n in enumerate(LENS):
        ppg[i, :, n:] = 1e3; sine[i, :, n * hop:] = -1e3; lft[i, :, n * hop:] = 1e3
    ins = [_t(dev, a) for a in (ppg, sine, lft)] + [_t(dev, b.spk_emb) if spk else None]
    alone = _oracle(name, spk, True)
    ws = torch.empty(plan.workspace_bytes(B, F_PAD) // 4 * 4 + 4, dtype=torch.uint8, device=dev)
    for fill in ("1000", "0xFF", "1e30"):
        if fill == "0xFF":
            ws.fill_(0xFF)
        else:
            ws[: ws.numel() // 4 * 4].view(torch.float32).fill_(float(fill))
        recs = [] if fill == "1000" else None
        y = plan.forward(blob, *ins, lengths=LENS, workspace=ws, profile=recs).cpu().double().numpy()
        assert np.isfinite(y).all(), fill
        for j, n in enumerate(LENS):
            T = n * hop
            _check_output(y[j:j + 1, :, :T], alone[j][0].numpy(), storage, one_frame=(n == 1),
                          what=f"{name}/{storage}/{spk}/ragged/{fill}/n={n}")
            assert not y[j, :, T:].any(), (fill, j)
        for i in range(cfg.n_stages):
            tap = plan.tap(f"up.{i}.xmid", B, F_PAD, ws).cpu().double().numpy()
            rate = tap.shape[-1] // F_PAD
            for j, n in enumerate(LENS):
                want = alone[j][1][f"up.{i}.xmid"].numpy()[0]
                assert want.shape[-1] == n * rate
                lo = max(0, n * rate - 4)
                got = tap[j, :, lo:n * rate]
                mag = max(1.0, float(np.abs(want).max()))
                err = float(np.abs(got - want[:, lo:]).max()) if np.isfinite(got).all() else float("inf")
                tol = TIGHT * mag if storage == "float32" else 6e-2 * mag
                assert err <= tol, (fill, f"up.{i}.xmid", j, n, err, mag)
        if recs is not None:
            _check_routes(recs, cfg, storage, spk, True, name)


def test_odd_frame_count_through_the_padding_route_in_bfloat16(dev):
    """bfloat16 storage pads a frame count that is not a multiple of 4 and runs the batch as a ragged one (engine.py):
    a single utterance of 13 frames, every configuration, with and without a speaker where it has one."""
    from oracle import fastsvc_oracle as O
    for name in CM.NAMES:
        cfg = CM.config(name)
        plan, blob = _plan(name, "bfloat16", dev)
        b = S.synth_batch(cfg, 1, 13, 623)
        for spk in CM.speaker_modes(name):
            y = plan.forward(blob, _t(dev, b.ppg), _t(dev, b.sine), _t(dev, b.lft), _t(dev, b.spk_emb) if spk else None)
            y = y.cpu().double().numpy()
            ref = O.forward_dedup(_weights(name)[1], cfg.upsampling_scales, b.ppg, b.sine, b.lft, b.spk_emb if spk else None,
                                  dtype=torch.float64).numpy()
            assert y.shape == ref.shape == (1, cfg.out_channels, 13 * cfg.hop)
            _check_output(y, ref, "bfloat16", what=f"{name}/bfloat16/{spk}/F=13")


# ---- the wide-layer kernel (conv_wx, launch-table algorithm 6) falls back where it has no instance -------------------
# Instances: (prologue, epilogue) in {none, LeakyReLU, InstanceNorm + LeakyReLU} x {plain, residual} and (InstanceNorm,
# FiLM affine); C_in a multiple of 8.  Without a speaker embedding no layer has the norm prologue, so a FiLM-affine
# epilogue (kernel field 5 = 4) must never be on conv_wx.

def _wx_epilogues(recs):
    return {r["layer"]: r["kernel"].split(",")[4] for r in recs if r["kernel"].startswith("conv_wx<")}


@pytest.mark.parametrize("B,F", [(2, 48), (64, 1500)])
def test_default_config_bfloat16_without_speaker_on_the_shipped_table(dev, B, F):
    """The shipped launch table holds algorithm-6 entries (up.0.d9 among them, at cfg3's 64 x 1500 frames), which also
    serve other batch shapes nearest to them.  Without a speaker the d = 9 conv's FiLM-affine epilogue has no conv_wx
    instance (no InstanceNorm prologue): the route must keep it on conv_hx instead of failing the forward, and still
    put the layers that have an instance on conv_wx.  At 2 x 48 the nearest entries of every layer are conv_hx ones;
    at 64 x 1500 the table's own entries apply.  Utterance 0 against the float64 oracle at the bfloat16 bounds."""
    from oracle import fastsvc_oracle as O
    cfg = S.FULL_CONFIG
    sd = S.synth_state_dict(cfg, 631)
    ppg, sine, lft, _ = S.device_batch(cfg, B, F, 632, dev)
    plan = A.Plan(cfg, storage="bfloat16")
    assert plan.tuned_shapes()["up.0.d9|64|3000|b"][4] == 6
    blob = plan.pack(sd).to(dev)
    recs = []
    y = plan.forward(blob, ppg, sine, lft, None, profile=recs)[:1].cpu().double().numpy()
    ref = O.forward_dedup(S.fold_weight_norm(sd), cfg.upsampling_scales, ppg[:1].cpu().numpy(), sine[:1].cpu().numpy(),
                          lft[:1].cpu().numpy(), None, dtype=torch.float64).numpy()
    _check_output(y, ref, "bfloat16", what=f"default/bfloat16/nospk/table/{B}x{F}")
    wx = _wx_epilogues(recs)
    print(f"WX default nospk {B}x{F}", sorted(wx.items()))
    assert "4" not in wx.values(), wx
    assert not {f"up.{i}.d9" for i in range(cfg.n_stages)} & set(wx), wx
    if B == 64:
        assert "up.0.d27" in wx, wx                    # (its residual epilogue has the instance: the table's choice holds)


def test_every_eligible_layer_on_the_wide_kernel_odd_widths(dev):
    """`odd_widths` (C_in = 100, no speaker) with a launch table that puts every direct conv of the forward on
    algorithm 6: the forward succeeds and matches the oracle; up.0.conv_first (C_in & 7) and the d = 9 convs (FiLM-affine
    epilogue without the norm prologue) stay on conv_hx, up.0.d27 (192 channels, residual epilogue) runs on conv_wx."""
    from oracle import fastsvc_oracle as O
    name = "odd_widths"
    cfg = CM.config(name)
    B, F = 2, 48
    b = S.synth_batch(cfg, B, F, 633)
    ins = [_t(dev, a) for a in (b.ppg, b.sine, b.lft)] + [None]
    base = A.Plan(cfg, storage="bfloat16", load_shipped_table=False)
    blob = base.pack(_weights(name)[0]).to(dev)
    recs = []
    base.forward(blob, *ins, profile=recs)
    direct = {r["layer"] for r in recs if r["kernel"].startswith("conv_hx<") and r["kernel"].split(",")[4] == "0"
              and not r["layer"].endswith(".d3x")}
    assert {"up.0.conv_first", "up.0.d9", "up.0.d27"} <= direct, sorted(direct)
    rates = {F * int(np.prod(cfg.upsampling_scales[:k])) for k in range(cfg.n_stages + 1)}
    wide = A.Plan(cfg, storage="bfloat16", load_shipped_table=False)
    wide.load_tuned({f"{layer}|{B}|{T}|b": [6, 4, 2, 2, 6] for layer in direct for T in rates})
    recs = []
    y = wide.forward(blob, *ins, profile=recs).cpu().double().numpy()
    ref = O.forward_dedup(_weights(name)[1], cfg.upsampling_scales, b.ppg, b.sine, b.lft, None, dtype=torch.float64).numpy()
    _check_output(y, ref, "bfloat16", what="odd_widths/bfloat16/nospk/wide")
    wx = _wx_epilogues(recs)
    print("WX odd_widths", sorted(wx.items()))
    kernels = {r["layer"]: r["kernel"] for r in recs}
    assert kernels["up.0.conv_first"].startswith("conv_hx<"), kernels["up.0.conv_first"]
    for i in range(cfg.n_stages):
        assert kernels[f"up.{i}.d9"].startswith("conv_hx<"), (i, kernels[f"up.{i}.d9"])
    # the rest of the layers with 48-channel groups in multiples of 4 (192 / 384 output channels) run on conv_wx
    assert set(wx) == {"down.3.c2_d2", "down.3.c3_d4", "film.3.conv", "film.3.heads", "up.0.d27"}, wx
