"""Device-side weight packer against the host packer, on the GPU (-m gpu): `Plan.pack_device` must write the bytes
`Plan.pack` writes.  Equality of the blobs viewed as uint8, no tolerance; the expected side of every comparison is the host
packer (pinned in tests/test_pack_device.py and behind every golden test), never the code under test.
"""
import numpy as np
import pytest
import torch

import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import synth as S
from svcc23_fastsvc_amd import training as TR
import config_matrix as CM
import range_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    A.load_library()
    return torch.device("cuda:0")


def _to_dev(sd, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for k, v in sd.items()}


def _garbage(n, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev, generator=g)


def _compare(plan, sd, dev, what):
    """host blob vs device blob of one state dict; `out` pre-filled with 0xFF, the scratch with garbage"""
    want = plan.pack(sd).view(torch.uint8)
    out = torch.full((plan.blob_bytes // 4,), float("nan"), dtype=torch.float32, device=dev)
    out.view(torch.uint8).fill_(0xFF)
    scratch = _garbage(plan.pack_device_scratch_bytes, dev, 7)
    got = plan.pack_device(_to_dev(sd, dev), out=out, scratch=scratch)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    got8 = got.view(torch.uint8).cpu()
    if not torch.equal(got8, want):
        bad = torch.nonzero(got8 != want).flatten()
        w = (bad[:8] // 4).tolist()
        pytest.fail(f"{what}: {bad.numel()} of {want.numel()} bytes differ; first float offsets {w}, "
                    f"host {want.view(torch.float32)[w].tolist()} device {got8.view(torch.float32)[w].tolist()}")
    return got


CONFIGS = {"tiny": (lambda: S.TINY_CONFIG, 77), "full": (lambda: S.FULL_CONFIG, 201)}
CONFIGS.update({name: ((lambda n=name: CM.config(n)), CM.SEED_W) for name in CM.NAMES})


@pytest.mark.parametrize("layout", ["weight_norm", "folded"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_device_blob_is_the_host_blob(dev, name, layout):
    cfg, seed = CONFIGS[name][0](), CONFIGS[name][1]
    sd = S.synth_state_dict(cfg, seed, weight_norm=True)
    if layout == "folded":
        sd = S.fold_weight_norm(sd)
        assert not any(k.endswith(".weight_g") for k in sd)
    _compare(A.Plan(cfg), sd, dev, f"{name}/{layout}")


def test_the_two_key_layouts_are_different_blobs():
    """numpy's fold is not the packer's: the comparison above is per layout for a reason"""
    cfg = S.FULL_CONFIG
    plan = A.Plan(cfg)
    sd = S.synth_state_dict(cfg, 201, weight_norm=True)
    a, b = plan.pack(sd).view(torch.uint8), plan.pack(S.fold_weight_norm(sd)).view(torch.uint8)
    assert int((a != b).sum()) > 1_000_000


RANGE_NAMES = [n for n in RC.CASES if n.startswith(("g_all", "g_up", "g_cond", "g_spread", "nospk_film_scale", "nospk_g_up"))]


@pytest.mark.parametrize("name", RANGE_NAMES)
def test_exponents_across_their_range(dev, name):
    cfg = S.FULL_CONFIG
    base = S.synth_state_dict(cfg, RC.SEED_W)
    sd, _, _ = RC.build_case(cfg, name)
    assert any(not np.array_equal(sd[k], base[k]) for k in sd), name       # the case does change the weights
    _compare(A.Plan(cfg), sd, dev, name)


def _hand_made(kind):
    cfg = S.FULL_CONFIG
    sd = dict(S.synth_state_dict(cfg, 201, weight_norm=True))
    layer = "upsampling_nets.1.conv_block1.1"             # 96 -> 96, k = 3: every format but the decimating pair
    g, v = sd[layer + ".weight_g"].copy(), sd[layer + ".weight_v"].copy()
    row = v[5].astype(np.float64)
    norm = float(np.sqrt((row ** 2).sum()))
    if kind == "zero_channel":
        g.reshape(-1)[5] = 0.0
        for k in ("film_lft.1.conv_scale", "downsampling_sine.2.downsample_block.4"):
            gg = sd[k + ".weight_g"].copy()
            gg.reshape(-1)[3] = 0.0
            sd[k + ".weight_g"] = gg
    elif kind == "weight_70000":
        # folded weight = v * g / ||v||: make the largest entry of the row 70000 (an infinity in the binary16 set)
        g.reshape(-1)[5] = np.float32(70000.0 * norm / np.abs(row).max())
    elif kind == "weight_1e-9":
        g.reshape(-1)[5] = np.float32(1e-9 * norm / np.abs(row).max())
    elif kind == "v_row_1e-20":
        v[5] = (v[5] * np.float32(1e-20 / np.abs(row).max())).astype(np.float32)
        assert 0 < float(np.abs(v[5]).max()) ** 2 < 1.2e-38                 # the squares are float32 denormals
    elif kind == "nan_weight":
        v[5].reshape(-1)[7] = np.float32("nan")
    sd[layer + ".weight_g"], sd[layer + ".weight_v"] = g, v
    return cfg, sd


@pytest.mark.parametrize("layout", ["weight_norm", "folded"])
@pytest.mark.parametrize("kind", ["zero_channel", "weight_70000", "weight_1e-9", "v_row_1e-20", "nan_weight"])
def test_hand_made_values(dev, kind, layout):
    """Values the host packer defines a result for (an infinity in the binary16 set, binary16 zeros and subnormals, float32
    denormals in the fold's sum of squares, a NaN): nothing is run with them but the two packers."""
    cfg, sd = _hand_made(kind)
    if layout == "folded":
        with np.errstate(all="ignore"):
            sd = S.fold_weight_norm(sd)
    _compare(A.Plan(cfg), sd, dev, f"{kind}/{layout}")


@pytest.mark.parametrize("storage", ["float32", "bfloat16", "float16"])
def test_forward_from_either_blob_is_the_same_bits(dev, storage):
    cfg = S.FULL_CONFIG
    plan = A.Plan(cfg, storage=storage)
    sd = S.synth_state_dict(cfg, 201)
    b = S.device_batch(cfg, 2, 40, 77, dev)
    host_blob = plan.pack(sd).to(dev)
    dev_blob = plan.pack_device(_to_dev(sd, dev))
    y_host = plan.forward(host_blob, *b).clone()
    y_dev = plan.forward(dev_blob, *b).clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y_host).all())
    assert torch.equal(y_host.view(torch.int32), y_dev.view(torch.int32))


def test_repack_in_place_after_a_parameter_update(dev):
    """The case a training loop lives on: same buffer, new values, forwards before and after on the same stream."""
    cfg = S.FULL_CONFIG
    plan = A.Plan(cfg)
    params = _to_dev(S.synth_state_dict(cfg, 201), dev)
    b = S.device_batch(cfg, 2, 40, 77, dev)
    blob = plan.pack_device(params)
    y0 = plan.forward(blob, *b).clone()
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    for k, p in params.items():                             # an in-place "optimizer step"
        p.add_(torch.randn(p.shape, device=dev, generator=g) * 1e-3 * p.abs().mean())
    again = plan.pack_device(params, out=blob)
    assert again.data_ptr() == blob.data_ptr()
    y1 = plan.forward(blob, *b).clone()
    torch.cuda.synchronize()
    fresh = plan.pack({k: v.cpu().numpy() for k, v in params.items()})
    assert torch.equal(blob.view(torch.uint8).cpu(), fresh.view(torch.uint8))
    y_want = plan.forward(fresh.to(dev), *b)
    torch.cuda.synchronize()
    assert torch.equal(y1.view(torch.int32), y_want.view(torch.int32))
    assert not torch.equal(y0, y1)


def test_two_packs_give_the_same_bytes(dev):
    cfg = S.FULL_CONFIG
    plan = A.Plan(cfg)
    params = _to_dev(S.synth_state_dict(cfg, 201), dev)
    a = plan.pack_device(params, scratch=_garbage(plan.pack_device_scratch_bytes, dev, 1))
    b = plan.pack_device(params, scratch=_garbage(plan.pack_device_scratch_bytes, dev, 2))
    torch.cuda.synchronize()
    assert a.data_ptr() != b.data_ptr()
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_pack_device_takes_non_contiguous_tensors_and_refuses_the_rest(dev):
    cfg = S.TINY_CONFIG
    plan = A.Plan(cfg)
    sd = S.synth_state_dict(cfg, 77)
    params = _to_dev(sd, dev)
    key = next(k for k, v in params.items() if k.endswith(".weight_v") and v.dim() == 3 and v.shape[2] == 3)
    wide = torch.zeros(params[key].shape[:2] + (6,), device=dev)
    wide[..., ::2] = params[key]
    strided = dict(params)
    strided[key] = wide[..., ::2]
    assert not strided[key].is_contiguous()
    got = plan.pack_device(strided)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.uint8).cpu(), plan.pack(sd).view(torch.uint8))
    with pytest.raises(A.FastSVCError):
        plan.pack_device({**params, key: params[key].cpu()})
    with pytest.raises(A.FastSVCError):
        plan.pack_device({**params, key: params[key].double()})
    with pytest.raises(KeyError):
        plan.pack_device({k: v for k, v in params.items() if k != key})
    with pytest.raises(ValueError):
        plan.pack_device(params, out=torch.empty(plan.blob_bytes // 4 - 1, device=dev))


def _train_three_steps(dev, pack_on_device):
    """the recipe-size construction of tests/test_training.py::test_recipe_size_train_step_matches_the_reference_step"""
    from conftest import load_golden
    g = load_golden("train_recipe.npz")
    cfg = S.FULL_CONFIG
    seed_w, seed_x, seed_d, seed_t, B, F = (int(v) for v in g["meta"])
    T = F * cfg.hop
    torch.manual_seed(0)
    gen = A.FastSVCGenerator(in_channels=cfg.in_channels, mid_channels=list(cfg.mid_channels),
                             upsampling_scales=list(cfg.upsampling_scales), out_channels=1,
                             spk_emb_size=cfg.spk_emb_size, use_spk_emb=True)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in S.synth_state_dict(cfg, seed_w).items()})
    gen = gen.to(dev).train()
    disc = TR.MelGANMultiScaleDiscriminator(**TR.RECIPE["discriminator_params"])
    S.fill_module_from_hash(disc, seed_d)
    disc = disc.to(dev).train()
    step = TR.TrainStep(gen, disc, dict(discriminator_train_start_steps=0, pack_on_device=pack_on_device), steps=1)
    assert gen.pack_on_device is pack_on_device
    b = S.synth_batch(cfg, B, F, seed_x)
    x = tuple(torch.from_numpy(a).to(dev) for a in (b.ppg, b.sine, b.lft, b.spk_emb))
    target = torch.from_numpy((0.3 * S.hash_normalish(seed_t, S.stream_id("train.target"), B * T)).reshape(B, 1, T).astype(np.float32)).to(dev)
    gen.packed_weights(dev)                                 # the plan exists: wrap its host packer and count
    calls = {"pack": 0, "pack_prefetch": 0, "pack_device": 0}
    plan = gen.plan
    for name in calls:
        def wrapped(*a, _f=getattr(plan, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        setattr(plan, name, wrapped)
    logs = [step.step((x, target)) for _ in range(3)]
    torch.cuda.synchronize()
    state = {"g": {k: v.detach().cpu().clone() for k, v in gen.state_dict().items()},
             "d": {k: v.detach().cpu().clone() for k, v in disc.state_dict().items()}}
    return logs, state, calls


def test_train_step_is_bit_identical_with_the_device_packer(dev):
    """Same seeds, three steps, host route against device route: every loss and every parameter bit for bit.
    The comparison needs a step that reproduces ITSELF: with MIOpen's default algorithm choice the last convolution of
    each MelGAN scale does not (two runs of the host route differ from each other from the first adversarial loss on -
    measured on an MI355X), so the convolutions are pinned to MIOpen's deterministic algorithms for both runs."""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        logs_h, state_h, calls_h = _train_three_steps(dev, False)
        logs_d, state_d, calls_d = _train_three_steps(dev, True)
    finally:
        torch.backends.cudnn.deterministic = was
    assert calls_h["pack"] > 0 and calls_h["pack_device"] == 0          # the switch does select the route
    assert calls_d["pack"] == 0 and calls_d["pack_prefetch"] == 0 and calls_d["pack_device"] > 0, calls_d
    for it, (lh, ld) in enumerate(zip(logs_h, logs_d)):
        assert set(lh) == set(ld) and "discriminator_loss" in lh
        for k in lh:
            assert np.float64(lh[k]).tobytes() == np.float64(ld[k]).tobytes(), (it, k, lh[k], ld[k])
    for tag in ("g", "d"):
        for k, v in state_h[tag].items():
            assert torch.equal(v.view(torch.int32) if v.dtype == torch.float32 else v,
                               state_d[tag][k].view(torch.int32) if v.dtype == torch.float32 else state_d[tag][k]), (tag, k)
