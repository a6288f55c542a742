"""CPU-side tests of the drop-in boundary: the C-ABI library loads and exports every symbol the
header declares, the host-only plan/pack entry points behave, and the nn.Module mirrors the
reference surface (constructor, state_dict keys, weight-norm handling, error behaviour).
No compute kernels are launched here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import synth as S
from svcc23_fastsvc_amd.engine import ABI_SYMBOLS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built():
    from svcc23_fastsvc_amd.build import build
    build()


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "fastsvc_hip.h")).read()
    declared = set(re.findall(r"\b(fastsvc_[a-z0-9_]+)\s*\(", header))
    assert declared == set(ABI_SYMBOLS), declared ^ set(ABI_SYMBOLS)
    lib = ctypes.CDLL(A.library_path())
    for sym in declared:
        assert hasattr(lib, sym), sym
    assert lib.fastsvc_abi_version() == 1


def test_plan_sizes_and_flops():
    plan = A.Plan(S.FULL_CONFIG)
    assert plan.blob_bytes % 256 == 0 and plan.blob_bytes >= 2_744_353 * 4
    # de-duplicated dataflow, 1x1 convs after the decimation: ~193 kFLOP per output sample
    assert 185e3 < plan.flops_per_sample < 203e3
    assert plan.workspace_bytes(2, 10) < plan.workspace_bytes(4, 10) < plan.workspace_bytes(4, 20)
    assert plan.launch_count(True) == plan.launch_count(False) + 1


def test_compact_layout_leaves_out_what_the_whole_stage_launches_keep_in_lds():
    """Compact plans run conditioning stages 0 and 1 as one launch each (csrc/fastsvc_cond.hip): h_k, r_k, c1 / c2 and
    film_u of those stages never reach memory, so the layout holds zero-sized placeholders for them (the names stay valid
    taps) - except in the exact-float32 mode of very short inputs (F <= 4), which runs the separate launches."""
    full = A.Plan(S.FULL_CONFIG)
    for storage in ("float32", "bfloat16"):
        plan = A.Plan(S.FULL_CONFIG, storage=storage, compact_workspace=True)
        B, F = 64, 1500
        for name in ("down_h.0", "down_h.1", "down_r.1", "down_c1.0", "down_c2.1", "film_u.0", "film_u.1"):
            assert plan.tap_info(name, B, F)[1] == 0, name
            assert full.tap_info(name, B, F)[1] > 0, name
        for name in ("down_hd.1", "down_hd.2", "ss.0", "ss.1", "down_h.2", "down_r.2", "film_u.2", "down_h.3"):
            assert plan.tap_info(name, B, F)[1] == full.tap_info(name, B, F)[1] > 0, name
        # cfg3 (64 x 10 s): 18.7 GB float32 / 9.4 GB bfloat16, below 45 % of the one-buffer-per-tensor float32 layout
        frac = plan.workspace_bytes(B, F) / full.workspace_bytes(B, F)
        assert frac < (0.45 if storage == "float32" else 0.23), frac
    short = A.Plan(S.FULL_CONFIG, compact_workspace=True)
    assert short.tap_info("down_h.0", 2, 4)[1] == 4 * 24 * 4 * S.FULL_CONFIG.hop


def test_plan_rejects_bad_config():
    with pytest.raises(ValueError):
        A.Plan(S.GeneratorConfig(in_channels=0))
    with pytest.raises(ValueError):
        A.Plan(S.GeneratorConfig(mid_channels=(8, 4), upsampling_scales=(2, 2, 2)))


def _unpack_conv(blob, w_off, cout, cin, ntaps, MW, KC):
    """Inverse of the documented fragment order (fastsvc_plan.cpp): returns W[co][ci][tap]."""
    cinp = (cin + 3) // 4 * 4
    nchunks = (cinp + KC - 1) // KC
    kg = KC // 4
    Q = ntaps * nchunks * kg
    W = np.zeros((cout, cin, ntaps), np.float32)
    for co in range(cout):
        grp, m, l15 = co // (16 * MW), (co % (16 * MW)) // 16, co % 16
        for ci in range(cin):
            ch, g, lhi = ci // KC, (ci % KC) // 4, ci % 4
            for tap in range(ntaps):
                q = (ch * ntaps + tap) * kg + g
                lane = lhi * 16 + l15
                W[co, ci, tap] = blob[w_off + ((grp * Q + q) * 64 + lane) * MW + m]
    return W


def _unpack_hx(blob, off_floats, cout, cin, MW, prec):
    """Inverse of the split-half / bf16 fragment order (fastsvc_plan.cpp, fastsvc_hx.hip): returns
    W[co][ci][tap] as float64 = hi + lo (prec 0, binary16 pieces) or the bf16 value (prec 1)."""
    np_ = 2 if prec == 0 else 1
    nch = (cin + 31) // 32
    ngroups = (cout + 16 * MW - 1) // (16 * MW)
    halves = blob[off_floats: off_floats + ngroups * nch * 3 * MW * np_ * 256].view(np.uint16)
    W = np.zeros((cout, cin, 3))
    for co in range(cout):
        grp, m, l15 = co // (16 * MW), (co % (16 * MW)) // 16, co % 16
        for ci in range(cin):
            ch, lhi, e = ci // 32, (ci % 32) // 8, ci % 8
            for tap in range(3):
                frag = ((((grp * nch + ch) * 3 + tap) * MW + m) * np_) * 512
                lane = lhi * 16 + l15
                if prec == 0:
                    W[co, ci, tap] = float(halves[frag + lane * 8 + e: frag + lane * 8 + e + 1].view(np.float16)[0]) + \
                                     float(halves[frag + 512 + lane * 8 + e: frag + 512 + lane * 8 + e + 1].view(np.float16)[0])
                else:
                    W[co, ci, tap] = float((halves[frag + lane * 8 + e: frag + lane * 8 + e + 1].astype(np.uint32) << 16).view(np.float32)[0])
    return W


def test_pack_first_layer_fragment_order_and_fold():
    """The first allocation in the blob is down stage 0's raw 1x1 pair, then raw c1 pair, then the
    packed c2 pair: check the packed c2 (24->24, MW=2, KC=24) of the lft chain against the folded
    reference-layout weight."""
    cfg = S.FULL_CONFIG
    sd = S.synth_state_dict(cfg, 5)
    plan = A.Plan(cfg)
    blob = plan.pack(sd).numpy()
    folded = S.fold_weight_norm(sd)
    # raw section: r_raw[2] w (24 -> 64 each), b (64 each), c1_raw w (72 -> 128 each), b (64 each)
    assert np.array_equal(blob[0:24], folded["downsampling_lft.0.residual_block.0.weight"].ravel())
    assert np.array_equal(blob[64:88], folded["downsampling_sine.0.residual_block.0.weight"].ravel())
    # (each layer is followed by its (l1, bmax) pair - largest absolute row sum, largest |bias| - in a 64-float granule)
    w1x1 = folded["downsampling_lft.0.residual_block.0.weight"].reshape(24, -1)
    assert np.allclose(blob[4 * 64: 4 * 64 + 2], [np.abs(w1x1).sum(axis=1).max(),
                                                   np.abs(folded["downsampling_lft.0.residual_block.0.bias"]).max()], rtol=1e-6)
    off_c1 = 4 * 64 + 2 * 64
    assert np.allclose(blob[off_c1:off_c1 + 72], folded["downsampling_lft.0.downsample_block.2.weight"].ravel(), atol=2e-7)
    off_c2 = off_c1 + 2 * 128 + 2 * 64 + 2 * 64
    W = _unpack_conv(blob, off_c2, 24, 24, 3, 2, 24)
    assert np.abs(W - folded["downsampling_lft.0.downsample_block.4.weight"]).max() <= 2e-7
    # the same layer's split-half (binary16 hi + lo) and bfloat16 fragments: after the two plain copies, the two
    # bias rows and the two Winograd copies of the pair
    want = folded["downsampling_lft.0.downsample_block.4.weight"].astype(np.float64)
    off_hx = off_c2 + 2 * 2304 + 2 * 64 + 2 * 64 + 2 * 3072
    # (binary16 pieces hold w * 2^e[co], the channel's largest magnitude moved into [2^14, 2^15); the exact inverse
    # factors follow the two bfloat16 copies: ConvParams::whx_inv)
    off_inv = off_hx + 2 * 3072 + 2 * 1536
    inv = blob[off_inv: off_inv + 24].astype(np.float64)
    assert np.all(np.log2(inv) == np.round(np.log2(inv)))
    Ws = _unpack_hx(blob, off_hx, 24, 24, 2, 0)
    top = np.abs(Ws).reshape(24, -1).max(axis=1)
    assert np.all((top >= 2.0 ** 14) & (top < 2.0 ** 15))
    Wh = Ws * inv[:, None, None]
    assert np.abs(Wh - want).max() <= np.abs(want).max() * 2.0 ** -20
    # per channel: 22 significand bits relative to the CHANNEL's largest weight, whatever its absolute scale
    assert np.all(np.abs(Wh - want).reshape(24, -1).max(axis=1) <= np.abs(want).reshape(24, -1).max(axis=1) * 2.0 ** -21)
    Wb = _unpack_hx(blob, off_hx + 2 * 3072, 24, 24, 2, 1)
    assert np.abs(Wb - want).max() <= np.abs(want).max() * 2.0 ** -8 and np.abs(Wb - want).max() > 0
    # both key layouts pack to the same blob (float sections compared as floats; the half-precision
    # sections, where a last-bit difference of the fold moves a 16-bit pattern, through their decoded values)
    blob2 = plan.pack(folded).numpy()
    assert np.abs(blob[:off_hx] - blob2[:off_hx]).max() <= 2e-7
    assert np.abs(_unpack_hx(blob2, off_hx, 24, 24, 2, 0) * blob2[off_inv: off_inv + 24].astype(np.float64)[:, None, None] - Wh).max() <= 2e-7


def test_pack_is_strict():
    cfg = S.TINY_CONFIG
    sd = S.synth_state_dict(cfg, 5)
    plan = A.Plan(cfg)
    bad = dict(sd)
    bad.pop("film_sine.2.conv_shift.bias")
    with pytest.raises(KeyError):
        plan.pack(bad)
    bad = dict(sd)
    bad["conv_last.weight_v"] = bad["conv_last.weight_v"][..., :0]
    with pytest.raises(KeyError):
        plan.pack(bad)


def test_module_surface_matches_reference():
    g = A.FastSVCGenerator()
    assert list(g.state_dict().keys()) == S.state_dict_keys(S.FULL_CONFIG, weight_norm=True)
    assert sum(v.numel() for v in g.state_dict().values()) == 2_751_554
    assert g.in_channels == 144 and list(g.mid_channels) == [192, 96, 48, 24]
    assert list(g.upsampling_scales) == [2, 4, 4, 5]
    g.remove_weight_norm()
    assert list(g.state_dict().keys()) == S.state_dict_keys(S.FULL_CONFIG, weight_norm=False)
    assert sum(v.numel() for v in g.state_dict().values()) == 2_744_353
    g.apply_weight_norm()
    assert list(g.state_dict().keys()) == S.state_dict_keys(S.FULL_CONFIG, weight_norm=True)
    for name in ("forward", "inference", "remove_weight_norm", "apply_weight_norm", "state_dict",
                 "load_state_dict", "parameters", "eval", "train", "to"):
        assert callable(getattr(g, name))
    assert "FastSVCGenerator" in repr(g)


def test_constructor_does_not_mutate_arguments_and_accepts_yaml_kwargs():
    mid, scales = [192, 96, 48, 24], [2, 4, 4, 5]
    params = dict(in_channels=144, out_channels=1, mid_channels=mid, upsampling_scales=scales,
                  spk_emb_size=512, use_spk_emb=True)                       # fastsvc.yaml:23-29
    g = A.FastSVCGenerator(**params)
    assert mid == [192, 96, 48, 24] and scales == [2, 4, 4, 5]
    g2 = A.FastSVCGenerator(use_spk_emb=False)
    assert not any("emb_projector" in k for k in g2.state_dict())


def test_reference_style_checkpoint_loads_strict():
    sd = S.synth_state_dict(S.FULL_CONFIG, 11)
    g = A.FastSVCGenerator()
    res = g.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    # conv2d weights stay 4-D, weight_g keeps its (Cout,1,1,1) shape
    assert g.state_dict()["upsampling_nets.0.conv_first.weight_v"].shape == (192, 144, 1, 3)
    assert g.state_dict()["upsampling_nets.0.conv_first.weight_g"].shape == (192, 1, 1, 1)
    assert g.state_dict()["film_lft.1.conv.weight_g"].shape == (48, 1, 1)


def test_harana_namespace_resolution():
    """train_fastsvc.py:700-704 / utils.py:266-275: getattr(harana.models, "FastSVCGenerator")."""
    import sys
    saved = {k: v for k, v in sys.modules.items() if k == "harana" or k.startswith("harana.")}
    try:
        A.install_into_harana()
        import harana.models
        cls = getattr(harana.models, "FastSVCGenerator")
        assert cls is A.FastSVCGenerator
    finally:
        for k in [m for m in sys.modules if m == "harana" or m.startswith("harana.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_product_path_fails_loudly_on_cpu():
    g = A.FastSVCGenerator().eval()
    x, s, l = torch.zeros(1, 144, 4), torch.zeros(1, 1, 640), torch.zeros(1, 1, 640)
    with pytest.raises(A.FastSVCError):
        g(x, s, l, torch.zeros(1, 512))
    with pytest.raises(A.FastSVCError):              # training mode too: the forward is the HIP path
        g.train()(x, s, l, torch.zeros(1, 512))


def test_product_code_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "svcc23_fastsvc_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, f


def test_launch_shape_table_roundtrip_and_shipped_file():
    """fastsvc_tuned_set/get are host-only: entries round-trip in key order, replace on re-insert,
    and the shipped MI355X table parses and only names shapes the pipelined kernel is built for."""
    import json
    from svcc23_fastsvc_amd.engine import TUNED_TABLE_PATH
    plan = A.Plan(S.FULL_CONFIG, load_shipped_table=False)
    assert plan.tuned_shapes() == {}
    plan.load_tuned({"up.0.d3|8|1200": [1, 2, 2, 1], "film.2.heads|8|4800": [2, 2, 2, 1]})
    plan.load_tuned({"up.0.d3|8|1200": [2, 2, 2, 3, 1]})           # 5th entry: algorithm (0 when absent)
    assert plan.tuned_shapes() == {"film.2.heads|8|4800": [2, 2, 2, 1, 0], "up.0.d3|8|1200": [2, 2, 2, 3, 1]}
    doc = json.load(open(TUNED_TABLE_PATH))
    table = doc["tables"][plan.config_signature()]
    assert len(table) > 40
    for key, (nw, wm, wn, tpw, algo) in table.items():
        layer, b, t, *storage = key.split("|")                      # "...|b": entries of the bfloat16-storage mode
        assert int(b) >= 1 and int(t) >= 1 and layer and storage in ([], ["b"])
        # algo 0 / 1 / 2: f32-MFMA direct / Winograd (48- / 32-channel groups); 3: half-precision MFMA (fastsvc_hx.hip)
        # 4 / 5: the conditioning stages' phase kernel / layer pipeline; 6: the wide-layer kernel (fastsvc_wx.hip: eight waves)
        assert nw in (1, 2, 3, 4, 6, 8) and wm * wn == (8 if algo == 6 else 4) and 1 <= tpw <= 24 and algo in (0, 1, 2, 3, 6)
    shipped = A.Plan(S.FULL_CONFIG)
    assert shipped.tuned_shapes() == {k: list(v) for k, v in table.items()}
    # the bfloat16-storage plan holds the same table; its launches look up the "|b" keys
    assert any(k.endswith("|b") for k in table) and any(not k.endswith("|b") for k in table)
    assert A.Plan(S.FULL_CONFIG, storage="bfloat16").tuned_shapes() == shipped.tuned_shapes()


def test_table_switches_for_fused_launches_set_the_documented_keys():
    """`keep_last_block_output`, `keep_block_heads_separate` and `keep_residual_convs_separate` are table entries with
    algorithm 0 under the keys INTEGRATION.md documents (conv_last|B|T, up.<i>.head|B|T_in, up.<i>.d3x|B|T_out, both
    storages); the shipped table says "fused" (algorithm 3) for every up.<i>.d3x entry it holds."""
    cfg = S.FULL_CONFIG
    plan = A.Plan(cfg, load_shipped_table=False)
    B, F = 3, 40
    plan.keep_residual_convs_separate(B, F)
    t = plan.tuned_shapes()
    T = F
    for i, sc in enumerate(cfg.upsampling_scales):
        T *= sc
        for sfx in ("", "|b"):
            assert t[f"up.{i}.d3x|{B}|{T}{sfx}"][4] == 0
    assert len(t) == 2 * cfg.n_stages
    plan.keep_block_heads_separate(B, F)
    plan.keep_last_block_output(B, F)
    t = plan.tuned_shapes()
    assert t[f"up.0.head|{B}|{F}"][4] == 0 and t[f"conv_last|{B}|{F * cfg.hop}"][4] == 0
    shipped = A.Plan(cfg).tuned_shapes()
    d3x = {k: v for k, v in shipped.items() if ".d3x|" in k}
    assert len(d3x) >= 24 and all(v[4] == 3 for v in d3x.values()), {k: v for k, v in d3x.items() if v[4] != 3}


def test_decode_harness_f0_statistics_match_reference_golden(tmp_path):
    """F0Statistics.estimate / .convert vs the live reference (decode_chain.npz), the
    device variant of convert, PCM-16 writer round trip, feature-container loader."""
    import wave
    from conftest import load_golden
    from svcc23_fastsvc_amd import decode as Dc
    g = load_golden("decode_chain.npz")
    cfg = S.FULL_CONFIG
    frames = [int(v) for v in g["frames"]]
    batches = [S.synth_batch(cfg, 1, F, 400 + i) for i, F in enumerate(frames)]
    f0s = [b.f0[0, 0].astype(np.float64) for b in batches]
    fs = Dc.F0Statistics()
    assert np.allclose(fs.estimate(f0s), g["src_stats"], rtol=0, atol=1e-12)
    for i, f0 in enumerate(f0s):
        cv = fs.convert(f0, g["srcstats"], g["trgstats"])
        assert np.allclose(cv, g[f"cvf0.{i}"], rtol=1e-12, atol=0)
        assert np.array_equal(cv == 0, f0 == 0)                       # unvoiced frames stay unvoiced
        cvd = Dc.convert_f0_device(torch.from_numpy(f0), g["srcstats"], g["trgstats"]).numpy()
        assert np.allclose(cvd, cv.astype(np.float32), rtol=1e-6)
    y = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 1.7, -3.0, 1e-5], dtype=np.float32)
    pcm = Dc.to_pcm16(y)
    assert pcm.dtype == np.int16 and list(pcm) == [0, 16384, -16384, 32767, -32767, 32767, -32768, 0]
    path = str(tmp_path / "a.wav")
    Dc.write_wav(path, y, 24000)
    with wave.open(path, "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 24000, len(y))
        assert np.array_equal(np.frombuffer(w.readframes(len(y)), dtype=np.int16), pcm)
    feat = str(tmp_path / "u.npz")
    np.savez(feat, f0=batches[0].f0[0].T, ppg=batches[0].ppg[0].T, lft=batches[0].lft[0].T)
    u = Dc.load_features(feat)
    assert u["f0"].shape == (frames[0], 1) and u["ppg"].shape == (frames[0], 144) and u["lft"].shape == (frames[0] * 160, 1)


def test_packed_weight_cache_is_invalidated_and_module_copies(tmp_path):
    """the packed blob must not outlive the parameters it was built from, and a module that
    has a plan / blob must still deepcopy and torch.save (the ctypes handle is dropped, not pickled)."""
    import copy
    import io
    g = A.FastSVCGenerator(in_channels=8, mid_channels=[16, 8, 8, 4], upsampling_scales=[2, 4, 4, 5],
                           out_channels=1, spk_emb_size=16)
    b0 = g.packed_weights("cpu")
    assert g.packed_weights("cpu") is b0
    g2 = copy.deepcopy(g)
    assert g2._plan is None and g2._blob is None and torch.equal(g2.packed_weights("cpu"), b0)
    buf = io.BytesIO()
    torch.save(g, buf)
    g.load_state_dict(g.state_dict())
    assert g._blob is None
    b1 = g.packed_weights("cpu")
    g.float()                                            # _apply re-homes parameters
    assert g._blob is None
    b2 = g.packed_weights("cpu")
    with torch.no_grad():
        next(g.parameters()).mul_(2.0)                   # in-place through the tensor: version counter moves
    b3 = g.packed_weights("cpu")
    assert b3 is not b2 and not torch.equal(b3, b2)
    g.remove_weight_norm()
    assert g._blob is None
    b4 = g.packed_weights("cpu")
    next(g.parameters()).data.mul_(2.0)                  # through .data: invisible (documented) ...
    assert g.packed_weights("cpu") is b4
    g.invalidate_packed_weights()                        # ... unless told, or fingerprinted
    assert not torch.equal(g.packed_weights("cpu"), b4)
    g.checksum_weights = True
    b5 = g.packed_weights("cpu")
    next(g.parameters()).data.mul_(0.5)
    assert not torch.equal(g.packed_weights("cpu"), b5)
    assert b1 is not None


def test_checkpoint_schema_roundtrip(tmp_path):
    """checkpoints in the reference trainer's schema (train_fastsvc.py:104-128) + config.yml."""
    from svcc23_fastsvc_amd import checkpoint as C
    params = dict(in_channels=8, mid_channels=[16, 8, 8, 4], upsampling_scales=[2, 4, 4, 5], out_channels=1,
                  spk_emb_size=16, use_spk_emb=True)
    g = A.FastSVCGenerator(**params)
    opt = torch.optim.SGD(g.parameters(), lr=0.1)
    path = str(tmp_path / "exp" / "checkpoint-5steps.pkl")
    C.save_checkpoint(path, g, optimizer={"generator": opt}, steps=5, epochs=1,
                      config={"generator_type": "FastSVCGenerator", "generator_params": params})
    raw = torch.load(path, map_location="cpu")
    assert set(raw) == {"optimizer", "scheduler", "steps", "epochs", "model"}
    assert set(raw["model"]) == {"generator", "discriminator"} and raw["steps"] == 5
    g2 = C.load_generator(path)
    for k, v in g.state_dict().items():
        assert torch.equal(v, g2.state_dict()[k])
    g3 = A.FastSVCGenerator(**params)
    info = C.load_checkpoint(path, g3, optimizer={"generator": torch.optim.SGD(g3.parameters(), lr=0.1)})
    assert info == {"steps": 5, "epochs": 1}
    assert torch.equal(g3.packed_weights("cpu"), g.packed_weights("cpu"))


def test_reference_load_model_and_decode_sequence_with_the_swapped_class(tmp_path):
    """A checkpoint written by the REFERENCE generator in the Trainer.save_checkpoint schema (train_fastsvc.py:104-128),
    loaded the way the reference's `load_model` does it (harana/utils/utils.py:243-280: config.yml beside the checkpoint,
    class looked up on harana.models by `generator_type`, strict load of ["model"]["generator"]) with this package's class
    installed as harana.models.FastSVCGenerator, then the decode_fastsvc.py:140-143 sequence (remove_weight_norm -> eval).
    The reference generator's own initialisation and its state dict after remove_weight_norm are stored data
    (tests/golden/ref_checkpoint.npz, written by make_golden.py from the live reference)."""
    import sys
    import yaml
    from svcc23_fastsvc_amd import checkpoint as C
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_checkpoint.npz"))
    ref_sd = {k[5:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("ckpt/")}
    ref_folded = {k[7:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("folded/")}
    params = dict(in_channels=8, mid_channels=[16, 8, 8, 4], upsampling_scales=[2, 4, 4, 5], out_channels=1,
                  spk_emb_size=16, use_spk_emb=True)
    ckpt = tmp_path / "exp" / "checkpoint-10steps.pkl"
    os.makedirs(ckpt.parent)
    torch.save({"model": {"generator": ref_sd, "discriminator": {}},
                "optimizer": {"generator": {}, "discriminator": {}},
                "scheduler": {"generator": {}, "discriminator": {}}, "steps": 10, "epochs": 1}, str(ckpt))
    with open(ckpt.parent / "config.yml", "w") as f:
        yaml.dump({"generator_type": "FastSVCGenerator", "generator_params": params}, f, Dumper=yaml.Dumper)
    saved = {m: sys.modules.get(m) for m in ("harana", "harana.models")}
    models = sys.modules.get("harana.models")
    original = getattr(models, "FastSVCGenerator", None) if models is not None else None
    try:
        A.install_into_harana()                          # the swap a maintainer makes
        ref_models = sys.modules["harana.models"]
        assert ref_models.FastSVCGenerator is A.FastSVCGenerator
        with open(ckpt.parent / "config.yml") as f:
            config = yaml.load(f, Loader=yaml.Loader)
        model = getattr(ref_models, config["generator_type"])(**config["generator_params"])
        model.load_state_dict(torch.load(str(ckpt), map_location="cpu")["model"]["generator"])
        assert isinstance(model, A.FastSVCGenerator)
        loaded = C.load_generator(str(ckpt))             # the package's own restatement of load_model
        for k, v in model.state_dict().items():
            assert torch.equal(v, loaded.state_dict()[k]), k
        model.remove_weight_norm()                       # decode_fastsvc.py:142
        model = model.eval()                             # :143 (.to(device) needs the GPU box)
        ours, theirs = model.state_dict(), ref_folded
        assert list(ours) == list(theirs)
        for k in theirs:
            assert torch.allclose(ours[k], theirs[k], atol=1e-7), k
        # and the packed blob built from it equals the one built from the weight-norm checkpoint
        plan = model.plan
        # (up to the last bit of the two folds: a last-bit difference moves the 16-bit pattern of a low piece, so the
        # blobs are compared by the share of identical words; test_pack_first_layer_fragment_order_and_fold
        # decodes the fragments and compares values)
        b1 = plan.pack(model.state_dict()).numpy()
        b2 = plan.pack(torch.load(str(ckpt))["model"]["generator"]).numpy()
        assert b1.shape == b2.shape and (b1.view(np.uint16) != b2.view(np.uint16)).mean() < 0.2
    finally:
        if original is not None:
            models.FastSVCGenerator = original
        for m, mod in saved.items():
            if mod is None:
                sys.modules.pop(m, None)
            else:
                sys.modules[m] = mod


def test_split_half_conversions_match_numpy():
    """The packer's binary16 / bfloat16 conversions (fastsvc_plan.cpp) against numpy / torch: normal range,
    subnormals, ties, the overflow edge, and the split x = hi + lo holding 22 significand bits."""
    lib = A.load_library()
    rng = np.random.default_rng(5)
    x = np.concatenate([
        rng.standard_normal(4096).astype(np.float32) * np.float32(10.0) ** rng.integers(-8, 5, 4096).astype(np.float32),
        np.array([0.0, -0.0, 1.0, -1.0, 65504.0, 65519.9, 65520.0, 1e5, 6.1035156e-05, 6.0e-05, 5.9604645e-08,
                  2.9802322e-08, 2.98e-08, 1.0009765625, 1.00048828125, 1.00146484375, 0.3, -0.1], dtype=np.float32)])
    n = x.size
    hi = np.zeros(n, np.uint16); lo = np.zeros(n, np.uint16); bf = np.zeros(n, np.uint16)
    lib.fastsvc_split_half(x.ctypes.data, n, hi.ctypes.data, lo.ctypes.data, bf.ctypes.data)
    with np.errstate(over="ignore"):
        want_hi = x.astype(np.float16)
        assert np.array_equal(hi, want_hi.view(np.uint16))
        fin = np.isfinite(want_hi)
        want_lo = (x[fin] - want_hi[fin].astype(np.float32)).astype(np.float16)
    assert np.array_equal(lo[fin], want_lo.view(np.uint16))
    want_bf = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(bf, want_bf)
    # the two pieces reproduce x to 2^-21 relative (or the subnormal step 2^-25 absolute)
    mid = fin & (np.abs(x) < 6e4)
    rec = hi.view(np.float16)[mid].astype(np.float64) + lo.view(np.float16)[mid].astype(np.float64)
    assert np.all(np.abs(rec - x[mid]) <= np.maximum(np.abs(x[mid]) * 2.0 ** -21, 2.0 ** -25))


def test_bench_defaults_follow_baseline_configs():
    """VERDICT r3 task 4: a bare `bench.py --gpus 1` measures BASELINE's largest single-GPU configuration in its stated
    dtype (cfg3, bfloat16), `--gpus N > 1` measures config 4 (the 512-utterance set, strong scaling) in the same
    storage; explicit flags win; the training step stays float32."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.resolve_workload(1, None, None) == ("cfg3", "bfloat16")
    for n in (2, 4, 8):
        assert bench.resolve_workload(n, None, None) == ("cfg4", "bfloat16")
    assert bench.resolve_workload(8, "cfg2", None) == ("cfg2", "bfloat16")
    assert bench.resolve_workload(1, "cfg2", "float32") == ("cfg2", "float32")
    assert bench.resolve_workload(8, "cfg5", None) == ("cfg5", "float32")
    # the 512-utterance set shards evenly over 2 / 4 / 8 ranks (64 utterances = one batch per rank at 8)
    from svcc23_fastsvc_amd import distributed as D
    frames = S.workload_frames("cfg4")
    for n in (2, 8):
        shards = D.shard_utterances(frames, n)
        assert sorted(i for sh in shards for i in sh) == list(range(512)) and {len(sh) for sh in shards} == {512 // n}
