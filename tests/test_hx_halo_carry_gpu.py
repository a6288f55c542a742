"""conv_hx's halo carry (csrc/fastsvc_hx.hip, hx_carry) against the same launch at one tile per workgroup, and the oracle.

Reference layers: conv_block2 / conv_block3 of `FastSVCUpsampleNet` (harana/models/fastsvc.py:103-111): the d = 9 and d = 27
convs of the last two up blocks - C = 48 (two K chunks: the shared window rows are copied in place) and C = 24 (one chunk:
copied across the two window buffers).

From its second tile on a workgroup stages only the 128 fresh rows of a window and copies the 2 halo_al rows it shares
with the previous tile out of LDS.  With tpw = 1 every tile is a first tile and nothing is carried: that launch is the
reference.  Carried rows are bit-copies of what re-staging would write, so every output of the layer must be bit-identical
whatever tpw is; the d = 9 layers' InstanceNorm sums are float64 sums of the same float32 per-tile partials in another
order and agree to float64 rounding.  The workspace is pre-filled with 0xFF: a window row that was neither carried nor
staged shows."""
import numpy as np
import pytest
import torch

import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import synth as S

pytestmark = pytest.mark.gpu

RATE = {2: 32, 3: 160}         # columns per frame behind up block 2 / 3
SUFFIX = {"bfloat16": "|b", "float16": "|h"}
TAG = {"bfloat16": "x1", "float16": "h1"}
# layer -> (block, kernel instance, output taps - None: the waveform, conv_last rides on up.3.d27 -, index of its sums in up.<k>.stats)
LAYERS = {
    "up.2.d9": (2, "conv_hx<3,2,1,4,0,4,1,%s>", ("up.2.u3",), 2),
    "up.2.d27": (2, "conv_hx<3,2,1,4,0,2,1,%s>", ("up.2.out",), None),
    "up.3.d9": (3, "conv_hx<2,2,1,4,0,4,1,%s>", ("up.3.u3",), 2),
    "up.3.d27": (3, "conv_hx<2,2,1,4,0,2,1,%s>", (None,), None),
}
# name -> (B, padded F, frame counts, tiles per workgroup of the carrying launches).  Tiles are 128 columns; 2 halo_al is 32
# (d = 9) or 64 (d = 27) rows.
#   tail:   up.2 13 frames = 416 columns = 3 tiles + 32, up.3 5 frames = 800 = 6 tiles + 32: tpw 2 - a second workgroup that
#           stages its own left halo; 3 - an odd unit count and the phantom unit; 24 - one workgroup walks the whole row
#   inside: rows that end inside the carried zone or right at a tile edge, T mod 128 <= 2 halo_al: up.2 9 frames = 288 =
#           2 x 128 + 32; up.3 3 frames = 480 = 3 x 128 + 96, 4 frames = 640 = 5 x 128, 1 frame = 160 = 128 + 32 - the carried
#           rows hold the conv's zero padding
#   short:  1 frame at up.2 = 32 columns: the window is mostly padding and tpw exceeds the tile count
#   many:   8 x 304 frames, tpw 2: 304 workgroups per launch at up.2, 1520 at up.3 - two share a CU, the staggered start runs
SHAPES = {
    "tail2": (2, 16, [13, 13], (2, 3, 24)),
    "inside2": (2, 16, [13, 9], (2, 3, 24)),
    "tail3": (2, 8, [5, 5], (2, 3, 24)),
    "inside3": (2, 8, [5, 3], (2, 3, 24)),
    "edge3": (2, 8, [4, 1], (2, 3, 24)),
    "short": (2, 4, [1, 1], (3,)),
    "many": (8, 304, None, (2,)),
}
CASES = [(name, tpw) for name, (_, _, _, tpws) in SHAPES.items() for tpw in tpws]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    A.load_library()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def weights():
    return S.synth_state_dict(S.FULL_CONFIG, 95)


def _table(storage, B, F, tpw):
    """launch-table entries of the four layers: the 128-column tile (NW 2 x WN 4) at `tpw` tiles per workgroup"""
    return {f"{layer}|{B}|{RATE[blk] * F}{SUFFIX[storage]}": [2, 1, 4, tpw, 3] for layer, (blk, _, _, _) in LAYERS.items()}


_CACHE = {}        # plans that ran, packed weights, inputs and oracle results: every forward of the module runs once


def _run(dev, weights, storage, shape, tpw):
    cache = _CACHE
    key = (storage, shape, tpw)
    if key in cache:
        return cache[key]
    B, F, lens, _ = SHAPES[shape]
    cfg = S.FULL_CONFIG
    plan = A.Plan(cfg, storage=storage, load_shipped_table=False)
    plan.load_tuned(_table(storage, B, F, tpw))
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
    for layer, (_, kernel, _, _) in LAYERS.items():                # the plan really launched the instance it was meant to
        assert kernels[layer] == kernel % TAG[storage], (layer, kernels[layer])
    assert plan.tuned_shapes()[f"up.3.d27|{B}|{RATE[3] * F}{SUFFIX[storage]}"][3] == tpw
    cache[key] = (plan, ws, y)
    return cache[key]


def _own_columns(t, B, F, lens):
    """each utterance's own columns (behind them lies nobody's data)"""
    if lens is None:
        return t.reshape(-1)
    rate = t.shape[-1] // F
    return torch.cat([t[j, :, : lens[j % B] * rate].reshape(-1) for j in range(t.shape[0])])


@pytest.mark.parametrize("storage", ["bfloat16", "float16"])
@pytest.mark.parametrize("shape,tpw", CASES)
@pytest.mark.parametrize("layer", sorted(LAYERS))
def test_carried_windows_equal_restaged_windows(dev, weights, storage, shape, tpw, layer):
    B, F, lens, _ = SHAPES[shape]
    pr, ws_r, y_r = _run(dev, weights, storage, shape, 1)          # every tile a first tile: nothing is carried
    pc, ws_c, y_c = _run(dev, weights, storage, shape, tpw)
    blk, _, taps, si = LAYERS[layer]
    for tap in taps:
        a = _own_columns(y_c if tap is None else pc.tap(tap, B, F, ws_c), B, F, lens)
        c = _own_columns(y_r if tap is None else pr.tap(tap, B, F, ws_r), B, F, lens)
        assert a.numel() > 0 and torch.equal(a, c), (tap, float((a.float() - c.float()).abs().max()))
    if tap is None and lens is not None:                           # the waveform's padding is zero
        for j, n in enumerate(lens):
            assert float(y_c[j, :, n * RATE[3]:].abs().max() if n < F else 0.0) == 0.0
    if si is None:
        return
    a, c = pc.tap(f"up.{blk}.stats", B, F, ws_c), pr.tap(f"up.{blk}.stats", B, F, ws_r)      # (3B, C, 2): sum, sum of squares
    a, c = a[si * B: (si + 1) * B], c[si * B: (si + 1) * B]
    n = torch.tensor([RATE[blk] * (F if lens is None else lens[j]) for j in range(B)], dtype=torch.float64, device=a.device)[:, None]
    scale = (c[..., 1] * n).sqrt() + 1.0                           # >= sum |u| (Cauchy-Schwarz)
    d1 = float(((a[..., 0] - c[..., 0]).abs() / scale).max())
    d2 = float(((a[..., 1] - c[..., 1]).abs() / (c[..., 1] + 1.0)).max())
    print(f"CARRY {storage} {layer} {shape} tpw {tpw}: sums differ by {d1:.3e} / {d2:.3e} (relative)")
    assert float(c[..., 1].min()) > 0.0                            # (the sums were written at all)
    # the same float32 per-tile partials, added in float64 in another order: fewer than 2^20 additions of 2^-53 relative
    # error each, against the sum of magnitudes - 2^-33 = 1.2e-10; bound 1e-9
    assert d1 <= 1e-9 and d2 <= 1e-9


def _oracle(weights, shape, cache={}):
    """the waveform of every utterance at its own length, float64"""
    if shape not in cache:
        from oracle import fastsvc_oracle as O
        B, F, lens, _ = SHAPES[shape]
        cfg = S.FULL_CONFIG
        b = S.synth_batch(cfg, B, F, 96)
        wf = S.fold_weight_norm(weights)
        if lens is None:
            cache[shape] = [O.forward_dedup(wf, cfg.upsampling_scales, b.ppg, b.sine, b.lft, b.spk_emb).double().numpy()]
        else:
            cache[shape] = [O.forward_dedup(wf, cfg.upsampling_scales, b.ppg[j:j + 1, :, :n], b.sine[j:j + 1, :, : n * cfg.hop],
                                            b.lft[j:j + 1, :, : n * cfg.hop], b.spk_emb[j:j + 1]).double().numpy()
                            for j, n in enumerate(lens)]
    return cache[shape]


@pytest.mark.parametrize("storage", ["bfloat16", "float16"])
@pytest.mark.parametrize("shape,tpw", CASES)
def test_carrying_forward_vs_oracle(dev, weights, storage, shape, tpw):
    """against the float64-exact oracle at the tolerance of the 2-byte storage modes
    (tests/test_wide_gpu.py::test_wide_layer_kernel_forward_vs_oracle)"""
    B, F, lens, _ = SHAPES[shape]
    _, _, y = _run(dev, weights, storage, shape, tpw)
    y = y.cpu().double().numpy()
    refs = _oracle(weights, shape)
    if lens is None:
        err = np.abs(y - refs[0])
    else:
        err = np.concatenate([np.abs(y[j:j + 1, :, : n * RATE[3]] - refs[j]).reshape(-1) for j, n in enumerate(lens)])
    print(f"CARRY {storage} {shape} tpw {tpw} forward vs oracle: mean {err.mean():.3e} max {err.max():.3e}")
    assert err.mean() <= 2e-2 and err.max() <= 0.25, (err.mean(), err.max())


@pytest.mark.parametrize("storage", ["bfloat16", "float16"])
def test_carrying_launches_repeat_bit_for_bit(dev, weights, storage):
    """8 x 304 at two tiles per workgroup: two workgroups share a CU and start staggered - whichever of them runs ahead, the
    layers' outputs must not depend on it"""
    B, F, _, _ = SHAPES["many"]
    plan, ws, y = _run(dev, weights, storage, "many", 2)
    blob, ins = _CACHE[("blob", storage)], _CACHE[("ins", B, F)]
    taps = [t for _, _, ts, _ in LAYERS.values() for t in ts if t is not None]
    first = {t: plan.tap(t, B, F, ws).clone() for t in taps}
    y0 = y.clone()
    for _ in range(2):
        y1 = plan.forward(blob, *ins, workspace=ws)
        torch.cuda.synchronize()
        assert torch.equal(y1, y0)
        for t in taps:
            assert torch.equal(plan.tap(t, B, F, ws), first[t]), t
