"""The stretched residual operand of the fused d = 3 launches (`up.<i>.d3x`, csrc/fastsvc_hx.hip, ConvParams::x2) at the
stretch factors 4 and 5 in 2-byte storage: fetched by 16-byte requests into a raw LDS tile and gathered from there
(F_X2_GATHER, launch-table algorithm 8) against the eight element loads per item (algorithm 7), one layer at a time,
and against the oracle.

Reference layers: conv_block1 / the stretched residual conv of `FastSVCUpsampleNet` (harana/models/fastsvc.py:94-100).

Only the place a staging thread's eight elements come from differs: the stretched window, the products, their order and
the epilogue are the same, so the layer's outputs must be bit-identical and its InstanceNorm sums equal up to the order
of the float64 atomics.  Also here: the S = 2 instances' row-end gate (conv_hx_x2_rows_ok) on a config whose x2 block is
not the first."""
import numpy as np
import pytest
import torch

import config_matrix as CM
import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import synth as S

pytestmark = pytest.mark.gpu

SUFFIX = {"bfloat16": "|b", "float16": "|h"}
TAG = {"bfloat16": "x1", "float16": "h1"}
ELEMENT, GATHER = 7, 8         # launch-table algorithms of an up.<i>.d3x entry that pin the second operand's path
# layer -> (output columns per frame, launch shape NW / WM / WN, kernel, block index)
LAYERS = {
    "up.1.d3x": (8, (4, 2, 2), "conv_hx<3,4,2,2,0,4,4,%s>", 1),     # S = 4, C = 96: three K chunks, 2 x 2 waves
    "up.2.d3x": (32, (2, 1, 4), "conv_hx<3,2,1,4,0,4,4,%s>", 2),    # S = 4, C = 48: two chunks, two workgroups per CU
    "up.3.d3x": (160, (2, 1, 4), "conv_hx<2,2,1,4,0,4,5,%s>", 3),   # S = 5, C = 24: one chunk; 128-column tiles start at every phase
}
# (B, F, lengths, tiles per workgroup): 13 frames end rows inside a 16-byte piece of the operand (26 / 104 / 416 input
# columns), 9 frames leave whole tiles behind the row end, tpw 2; 8 x 152 with tpw 1: more workgroups than 2 x CUs
SHAPES = [(2, 16, [13, 13], 2), (2, 16, [13, 9], 2), (8, 152, None, 1)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    A.load_library()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def weights():
    return S.synth_state_dict(S.FULL_CONFIG, 95)


def _table(storage, B, F, tpw, algo):
    return {f"{layer}|{B}|{rate * F}{SUFFIX[storage]}": [*shape, tpw, algo[layer]] for layer, (rate, shape, _, _) in LAYERS.items()}


_CACHE = {}        # plans that ran, packed weights and inputs: every forward of the module runs once


def _run(dev, weights, storage, B, F, lens, tpw, algo):
    """forward with the three d3x entries at algo[layer]; the profile record must name the instance of each and the path
    its second operand took"""
    key = (storage, B, F, tuple(lens or ()), tpw, tuple(sorted(algo.items())))
    if key in _CACHE:
        return _CACHE[key]
    cfg = S.FULL_CONFIG
    plan = A.Plan(cfg, storage=storage, load_shipped_table=False)
    plan.load_tuned(_table(storage, B, F, tpw, algo))
    if ("blob", storage) not in _CACHE:
        _CACHE[("blob", storage)] = plan.pack(weights).to(dev)
    if ("ins", B, F) not in _CACHE:
        b = S.synth_batch(cfg, B, F, 96)
        _CACHE[("ins", B, F)] = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (b.ppg, b.sine, b.lft, b.spk_emb)]
    ws = torch.empty(plan.workspace_bytes(B, F), dtype=torch.uint8, device=dev)
    ws.fill_(0xFF)
    recs = []
    y = plan.forward(_CACHE[("blob", storage)], *_CACHE[("ins", B, F)], workspace=ws, profile=recs, lengths=lens)
    by_layer = {r["layer"]: r for r in recs}
    for layer, (_, _, kernel, _) in LAYERS.items():
        want = "gather" if algo[layer] == GATHER else "element"
        assert by_layer[layer]["kernel"] == kernel % TAG[storage], (layer, by_layer[layer]["kernel"])
        assert by_layer[layer]["x2_path"] == want, (layer, by_layer[layer]["x2_path"], want)
    _CACHE[key] = (plan, ws, y)
    return _CACHE[key]


def _own_columns(t, B, F, lens):
    """each utterance's own columns (behind them lies nobody's data)"""
    if lens is None:
        return t.reshape(-1)
    rate = t.shape[-1] // F
    return torch.cat([t[j, :, : lens[j % B] * rate].reshape(-1) for j in range(t.shape[0])])


def _assert_same_layer(pa, ws_a, pb, ws_b, B, F, lens, k, rate):
    for tap in (f"up.{k}.xmid", f"up.{k}.u2"):
        a, c = _own_columns(pa.tap(tap, B, F, ws_a), B, F, lens), _own_columns(pb.tap(tap, B, F, ws_b), B, F, lens)
        assert a.numel() > 0 and torch.equal(a, c), (tap, float((a.float() - c.float()).abs().max()))
    a, c = pa.tap(f"up.{k}.stats", B, F, ws_a), pb.tap(f"up.{k}.stats", B, F, ws_b)   # (3B, C, 2): sum, sum of squares
    n = torch.tensor([rate * (F if lens is None else lens[j % B]) for j in range(a.shape[0])], dtype=torch.float64, device=a.device)[:, None]
    d1 = float(((a[..., 0] - c[..., 0]).abs() / ((c[..., 1] * n).sqrt() + 1.0)).max())            # (denominator >= sum |u|)
    d2 = float(((a[..., 1] - c[..., 1]).abs() / (c[..., 1] + 1.0)).max())
    print(f"X2G up.{k} {B}x{F} {lens}: sums differ by {d1:.3e} / {d2:.3e} (relative)")
    assert float(c[..., 1].min()) > 0.0                                                           # (the sums were written at all)
    assert d1 <= 1e-9 and d2 <= 1e-9


@pytest.mark.parametrize("storage", ["bfloat16", "float16"])
@pytest.mark.parametrize("B,F,lens,tpw", SHAPES)
@pytest.mark.parametrize("layer", sorted(LAYERS))
def test_gathered_operand_equals_element_loads(dev, weights, storage, B, F, lens, tpw, layer):
    base = {l: ELEMENT for l in LAYERS}
    pb, ws_b, _ = _run(dev, weights, storage, B, F, lens, tpw, base)                        # every d3x on element loads
    pa, ws_a, _ = _run(dev, weights, storage, B, F, lens, tpw, {**base, layer: GATHER})     # ONE entry differs
    rate, _, _, k = LAYERS[layer]
    _assert_same_layer(pa, ws_a, pb, ws_b, B, F, lens, k, rate)


@pytest.mark.parametrize("storage", ["bfloat16", "float16"])
def test_unaligned_operand_rows_keep_the_element_loads(dev, storage):
    """2-byte storage takes frame counts that are multiples of 4, so with the yaml scales every operand row is a multiple of
    8 columns long.  `three_stage` (scales 4, 4, 5): up.0's operand runs at the frame rate - F = 12 columns per row, its
    16-byte pieces would not be aligned: the entry that asks for the raw tile gets element loads (the record says so) and
    the same bits; at F = 16 the same entry gets the raw tile."""
    cfg = CM.config("three_stage")
    sd = S.synth_state_dict(cfg, CM.SEED_W)
    B = 2
    blob = None
    for F, want in ((12, "element"), (16, "gather")):
        b = S.synth_batch(cfg, B, F, 97)
        ins = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (b.ppg, b.sine, b.lft, b.spk_emb)]
        runs = {}
        for algo in (ELEMENT, GATHER):
            plan = A.Plan(cfg, storage=storage, load_shipped_table=False)
            plan.load_tuned({f"up.0.d3x|{B}|{4 * F}{SUFFIX[storage]}": [4, 2, 2, 1, algo]})
            blob = plan.pack(sd).to(dev) if blob is None else blob
            ws = torch.empty(plan.workspace_bytes(B, F), dtype=torch.uint8, device=dev)
            ws.fill_(0xFF)
            recs = []
            plan.forward(blob, *ins, workspace=ws, profile=recs)
            rec = {r["layer"]: r for r in recs}["up.0.d3x"]
            assert rec["kernel"] == "conv_hx<3,4,2,2,0,4,4,%s>" % TAG[storage], rec
            assert rec["x2_path"] == ("element" if algo == ELEMENT else want), (F, algo, rec)
            runs[algo] = (plan, ws)
        _assert_same_layer(*runs[GATHER], *runs[ELEMENT], B, F, None, 0, 4)


@pytest.mark.parametrize("storage", ["bfloat16", "float16"])
def test_gathered_forward_vs_oracle(dev, weights, storage):
    """forward with the raw tile forced on in all three layers against the float64-exact oracle, at the tolerance of the
    2-byte storage modes (tests/test_hx_two_per_cu_gpu.py::test_two_per_cu_forward_vs_oracle)"""
    B, F = 2, 200
    _, _, y = _run(dev, weights, storage, B, F, None, 2, {l: GATHER for l in LAYERS})
    from oracle import fastsvc_oracle as O
    cfg = S.FULL_CONFIG
    b = S.synth_batch(cfg, B, F, 96)
    if "ref" not in _CACHE:
        _CACHE["ref"] = O.forward_dedup(S.fold_weight_norm(weights), cfg.upsampling_scales, b.ppg, b.sine, b.lft, b.spk_emb).double().numpy()
    err = np.abs(y.cpu().double().numpy() - _CACHE["ref"])
    print(f"X2G {storage} forward vs oracle: mean {err.mean():.3e} max {err.max():.3e}")
    assert err.mean() <= 2e-2 and err.max() <= 0.25, (err.mean(), err.max())


def test_s2_operand_rows_that_end_inside_a_group_of_four_columns():
    """The S = 2 instances request 4 columns of the residual operand at once and test the row end once per group, so they
    are gated on rows a multiple of 4 long (conv_hx_x2_rows_ok).  `s2_second` (scales 2, 2, 4, 5: the x2 block is up.1,
    its operand runs at twice the frame rate), ragged odd lengths, bfloat16: every block's xmid against the oracle's taps
    of each utterance alone, at the bound tests/test_config_matrix_gpu.py holds that tap to (6e-2 x max(1, |ref|max));
    the last column of every utterance - where a column past the row end would land - on its own."""
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    A.load_library()
    dev = torch.device("cuda:0")
    from oracle import fastsvc_oracle as O
    cfg = CM.config("s2_second")
    lens, F = [7, 5, 3], 8         # (2-byte storage: the padded frame count is a multiple of 4)
    B = len(lens)
    sd = S.synth_state_dict(cfg, CM.SEED_W)
    wf = S.fold_weight_norm(sd)
    b = S.synth_batch(cfg, B, F, 623)
    plan = A.Plan(cfg, storage="bfloat16")
    blob = plan.pack(sd).to(dev)
    ws = torch.empty(plan.workspace_bytes(B, F), dtype=torch.uint8, device=dev)
    ws.fill_(0xFF)
    ins = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (b.ppg, b.sine, b.lft, b.spk_emb)]
    plan.forward(blob, *ins, lengths=lens, workspace=ws)
    for j, n in enumerate(lens):
        _, taps = O.forward_dedup(wf, cfg.upsampling_scales, b.ppg[j:j + 1, :, :n], b.sine[j:j + 1, :, :n * cfg.hop],
                                  b.lft[j:j + 1, :, :n * cfg.hop], b.spk_emb[j:j + 1], dtype=torch.float64, return_taps=True)
        for i in range(cfg.n_stages):
            tap = plan.tap(f"up.{i}.xmid", B, F, ws).cpu().double().numpy()
            rate = tap.shape[-1] // F
            want = taps[f"up.{i}.xmid"].numpy()[0]
            assert want.shape[-1] == n * rate
            got = tap[j, :, : n * rate]
            mag = max(1.0, float(np.abs(want).max()))
            assert np.isfinite(got).all(), (i, j)
            err, last = float(np.abs(got - want).max()), float(np.abs(got[:, -1] - want[:, -1]).max())
            print(f"X2ROWS up.{i}.xmid utterance {j} ({n} frames): max err {err:.3e}, last column {last:.3e}, bound {6e-2 * mag:.3e}")
            assert last <= 6e-2 * mag, (i, j, n, last, mag)
            assert err <= 6e-2 * mag, (i, j, n, err, mag)
