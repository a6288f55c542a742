"""The conv_hx instances budgeted for two workgroups per CU (csrc/fastsvc_hx.hip, hx_two_cu: the C = 48 FiLM-affine convs
up.2.d3x and up.2.d9 on the tile MW 3 x NW 2) against instances of the same kernel that kept their budget (NW 3), one
layer at a time, and against the oracle.

Reference layers: conv_block1 / conv_block2 of `FastSVCUpsampleNet` (harana/models/fastsvc.py:94-112).

The re-budgeted instances hold the weight ring back over a tile's epilogue and keep the lanes' InstanceNorm sums in LDS
between tiles: same products, same order of accumulation, same element-wise epilogue - the layer's own outputs must be
bit-identical whatever the tile shape; its InstanceNorm sums are joined over other tiles (128 instead of 192 columns)
and agree to float64 rounding of float32 partial sums."""
import numpy as np
import pytest
import torch

import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import synth as S

pytestmark = pytest.mark.gpu

RATE = 32                      # columns per frame at up.2's output rate (2 x 4 x 4)
SUFFIX = {"bfloat16": "|b", "float16": "|h"}
TAG = {"bfloat16": "x1", "float16": "h1"}
# layer -> (kernel of the re-budgeted instance, kernel of the untouched one, output taps, index of its sums in up.2.stats)
LAYERS = {
    "up.2.d3x": ("conv_hx<3,2,1,4,0,4,4,%s>", "conv_hx<3,3,1,4,0,4,4,%s>", ("up.2.xmid", "up.2.u2"), 1),
    "up.2.d9": ("conv_hx<3,2,1,4,0,4,1,%s>", "conv_hx<3,3,1,4,0,4,1,%s>", ("up.2.u3",), 2),
}
# (B, F, lengths, tiles per workgroup): F = 16 with 13 frames = 416 columns - three full 128-column tiles and a
# 32-column tail, two K chunks, tpw 2: a workgroup walks two tiles and another takes the tail; its ragged twin; and
# 8 x 152 with one tile per workgroup = 304 workgroups per launch - a CU holds two, the staggered start runs
SHAPES = [(2, 16, [13, 13], 2), (2, 16, [13, 9], 2), (8, 152, None, 1)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    A.load_library()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def weights():
    return S.synth_state_dict(S.FULL_CONFIG, 95)


def _table(storage, B, F, tpw, nw):
    """launch-table entries of both layers: nw[layer] = 2 (re-budgeted instance) or 3 (untouched)"""
    return {f"{layer}|{B}|{RATE * F}{SUFFIX[storage]}": [nw[layer], 1, 4, tpw, 3] for layer in LAYERS}


_CACHE = {}        # plans that ran, packed weights and inputs: every forward of the module runs once


def _run(dev, weights, storage, B, F, lens, tpw, nw):
    cache = _CACHE
    key = (storage, B, F, tuple(lens or ()), tpw, tuple(sorted(nw.items())))
    if key in cache:
        return cache[key]
    cfg = S.FULL_CONFIG
    plan = A.Plan(cfg, storage=storage, load_shipped_table=False)
    plan.load_tuned(_table(storage, B, F, tpw, nw))
    if ("blob", storage) not in cache:
        cache[("blob", storage)] = plan.pack(weights).to(dev)
    if ("ins", B, F) not in cache:
        b = S.synth_batch(cfg, B, F, 96)
        cache[("ins", B, F)] = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (b.ppg, b.sine, b.lft, b.spk_emb)]
    ws = torch.empty(plan.workspace_bytes(B, F), dtype=torch.uint8, device=dev)
    ws.fill_(0xFF)
    recs = []
    y = plan.forward(cache[("blob", storage)], *cache[("ins", B, F)], workspace=ws, profile=recs, lengths=lens)
    kernels = {r["layer"]: r["kernel"] for r in recs}
    for layer, (two, one, _, _) in LAYERS.items():                 # each plan really launched the instance it was meant to
        assert kernels[layer] == (two if nw[layer] == 2 else one) % TAG[storage], (layer, kernels[layer])
    cache[key] = (plan, ws, y)
    return cache[key]


def _own_columns(t, B, F, lens):
    """each utterance's own columns (behind them lies nobody's data)"""
    if lens is None:
        return t.reshape(-1)
    rate = t.shape[-1] // F
    return torch.cat([t[j, :, : lens[j % B] * rate].reshape(-1) for j in range(t.shape[0])])


@pytest.mark.parametrize("storage", ["bfloat16", "float16"])
@pytest.mark.parametrize("B,F,lens,tpw", SHAPES)
@pytest.mark.parametrize("layer", sorted(LAYERS))
def test_two_per_cu_instance_equals_the_untouched_instance(dev, weights, storage, B, F, lens, tpw, layer):
    base = {l: 3 for l in LAYERS}
    pb, ws_b, _ = _run(dev, weights, storage, B, F, lens, tpw, base)               # plan B: both layers on NW 3
    pa, ws_a, _ = _run(dev, weights, storage, B, F, lens, tpw, {**base, layer: 2})  # plan A: ONE entry differs
    _, _, taps, si = LAYERS[layer]
    for tap in taps:
        a, c = _own_columns(pa.tap(tap, B, F, ws_a), B, F, lens), _own_columns(pb.tap(tap, B, F, ws_b), B, F, lens)
        assert a.numel() > 0 and torch.equal(a, c), (tap, float((a.float() - c.float()).abs().max()))
    a, c = pa.tap("up.2.stats", B, F, ws_a), pb.tap("up.2.stats", B, F, ws_b)      # (3B, C, 2): sum, sum of squares
    # (the layers in front ran the same instances: their sums differ by the order of the float64 atomics at most)
    assert float(((a[: si * B] - c[: si * B]).abs() / (c[: si * B].abs() + 1.0)).max()) <= 1e-9
    a, c = a[si * B: (si + 1) * B], c[si * B: (si + 1) * B]
    n = torch.tensor([RATE * (F if lens is None else lens[j]) for j in range(B)], dtype=torch.float64, device=a.device)[:, None]
    scale = (c[..., 1] * n).sqrt() + 1.0                                           # >= sum |u|
    d1 = float(((a[..., 0] - c[..., 0]).abs() / scale).max())
    d2 = float(((a[..., 1] - c[..., 1]).abs() / (c[..., 1] + 1.0)).max())
    print(f"TWOCU {storage} {layer} {B}x{F} {lens}: sums differ by {d1:.3e} / {d2:.3e} (relative)")
    assert float(c[..., 1].min()) > 0.0                                            # (the sums were written at all)
    assert d1 <= 2e-3 and d2 <= 2e-3


@pytest.mark.parametrize("storage", ["bfloat16", "float16"])
def test_two_per_cu_forward_vs_oracle(dev, weights, storage):
    """forward with both re-budgeted instances forced on against the float64-exact oracle, at the tolerance of the 2-byte
    storage modes (tests/test_wide_gpu.py::test_wide_layer_kernel_forward_vs_oracle)"""
    B, F = 2, 200
    _, _, y = _run(dev, weights, storage, B, F, None, 2, {l: 2 for l in LAYERS})
    err = np.abs(y.cpu().double().numpy() - _oracle(weights, B, F))
    print(f"TWOCU {storage} forward vs oracle: mean {err.mean():.3e} max {err.max():.3e}")
    assert err.mean() <= 2e-2 and err.max() <= 0.25, (err.mean(), err.max())


def _oracle(weights, B, F, cache={}):
    if (B, F) not in cache:
        from oracle import fastsvc_oracle as O
        cfg = S.FULL_CONFIG
        b = S.synth_batch(cfg, B, F, 96)
        cache[(B, F)] = O.forward_dedup(S.fold_weight_norm(weights), cfg.upsampling_scales, b.ppg, b.sine, b.lft, b.spk_emb).double().numpy()
    return cache[(B, F)]


@pytest.mark.parametrize("storage", ["bfloat16", "float16"])
def test_two_per_cu_instances_repeat_bit_for_bit(dev, weights, storage):
    """8 x 152, one tile per workgroup: two workgroups share a CU and start staggered - whichever of them runs ahead, the
    layers' outputs must not depend on it"""
    B, F = 8, 152
    plan, ws, _ = _run(dev, weights, storage, B, F, None, 1, {l: 2 for l in LAYERS})
    blob, ins = _CACHE[("blob", storage)], _CACHE[("ins", B, F)]
    taps = [t for _, _, ts, _ in LAYERS.values() for t in ts]
    first = {t: plan.tap(t, B, F, ws).clone() for t in taps}
    for _ in range(2):
        plan.forward(blob, *ins, workspace=ws)
        torch.cuda.synchronize()
        for t in taps:
            assert torch.equal(plan.tap(t, B, F, ws), first[t]), t
