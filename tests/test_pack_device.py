"""Device-side weight packer (fastsvc_pack_weights_device / Plan.pack_device), the part that needs no GPU: the ABI, the
host-side checks that precede every device call, and a pin on the HOST packer's bytes - the device packer's yardstick must
not move in the pull request that adds it.  The byte comparisons against a GPU run are tests/test_pack_device_gpu.py."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest
import torch

import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import synth as S
from svcc23_fastsvc_amd.engine import ABI_SYMBOLS, _Tensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_MISSING = -1, -2


@pytest.fixture(scope="module", autouse=True)
def _built():
    from svcc23_fastsvc_amd.build import build
    build()


def _tensor_array(sd):
    """ctypes table over HOST arrays: enough for everything that fails before a launch."""
    items = list(sd.items())
    arr = (_Tensor * len(items))()
    keep = []
    for i, (k, v) in enumerate(items):
        a = np.ascontiguousarray(v, dtype=np.float32)
        name = k.encode()
        keep.append((a, name))
        arr[i].name, arr[i].data, arr[i].numel = name, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), a.size
    return arr, len(items), keep


def test_library_exports_and_header_declares_the_device_packer():
    header = open(os.path.join(ROOT, "include", "fastsvc_hip.h")).read()
    declared = set(re.findall(r"\b(fastsvc_[a-z0-9_]+)\s*\(", header))
    lib = A.load_library()
    for sym in ("fastsvc_pack_device_scratch_bytes", "fastsvc_pack_weights_device"):
        assert sym in declared and sym in ABI_SYMBOLS and hasattr(lib, sym), sym
    assert lib.fastsvc_abi_version() == 1
    assert "#define FASTSVC_ABI_VERSION 1" in header
    for cfg in (A.TINY_CONFIG, A.FULL_CONFIG):
        plan = A.Plan(cfg)
        assert plan.pack_device_scratch_bytes > 0
        assert 0 < plan.pack_device_launches <= 16          # a handful, whatever the number of layers
    assert lib.fastsvc_pack_device_scratch_bytes(None) == 0
    # the launch count is a property of the kernel set, not of the generator's size
    assert A.Plan(A.TINY_CONFIG).pack_device_launches == A.Plan(A.FULL_CONFIG).pack_device_launches


def test_pack_device_refuses_cpu_tensors():
    plan = A.Plan(A.TINY_CONFIG)
    sd = {k: torch.from_numpy(v) for k, v in S.synth_state_dict(A.TINY_CONFIG, 77).items()}
    with pytest.raises(A.FastSVCError):
        plan.pack_device(sd)


@pytest.mark.parametrize("layout", ["weight_norm", "folded"])
def test_missing_and_mis_sized_tensors_fail_on_the_host_with_the_host_packers_message(layout):
    cfg = A.TINY_CONFIG
    plan = A.Plan(cfg)
    lib = plan.lib
    base = S.synth_state_dict(cfg, 77)
    if layout == "folded":
        base = S.fold_weight_norm(base)
    blob_host = np.empty(plan.blob_bytes, dtype=np.uint8)
    # the device call never gets as far as touching these two (they are host memory: it would fault if it did)
    blob = np.empty(plan.blob_bytes, dtype=np.uint8)
    scratch = np.empty(plan.pack_device_scratch_bytes, dtype=np.uint8)

    def both(sd):
        arr, n, keep = _tensor_array(sd)
        rc_h = lib.fastsvc_pack_weights(plan._h, arr, n, blob_host.ctypes.data)
        msg_h = lib.fastsvc_last_error().decode()
        rc_d = lib.fastsvc_pack_weights_device(plan._h, arr, n, blob.ctypes.data, scratch.ctypes.data, scratch.size, None)
        msg_d = lib.fastsvc_last_error().decode()
        return rc_h, msg_h, rc_d, msg_d

    wkey = ".weight_v" if layout == "weight_norm" else ".weight"
    victims = ["upsampling_nets.0.conv_first.bias", "film_lft.0.conv_scale" + wkey, "conv_last" + wkey,
               "downsampling_sine.0.downsample_block.2.bias"]
    if layout == "weight_norm":
        victims.append("upsampling_nets.1.conv_block2.1.weight_g")
    for key in victims:
        assert key in base, key
        missing = {k: v for k, v in base.items() if k != key}
        short = dict(base)
        short[key] = base[key].reshape(-1)[:-1]
        for sd in (missing, short):
            rc_h, msg_h, rc_d, msg_d = both(sd)
            assert rc_h == E_MISSING and rc_d == E_MISSING, (key, rc_h, rc_d)
            assert msg_d == msg_h and key.rsplit(".", 1)[0] in msg_d, (key, msg_h, msg_d)

    arr, n, keep = _tensor_array(base)
    sb = scratch.size
    assert lib.fastsvc_pack_weights_device(None, arr, n, blob.ctypes.data, scratch.ctypes.data, sb, None) == E_INVALID
    assert lib.fastsvc_pack_weights_device(plan._h, None, n, blob.ctypes.data, scratch.ctypes.data, sb, None) == E_INVALID
    assert lib.fastsvc_pack_weights_device(plan._h, arr, n, None, scratch.ctypes.data, sb, None) == E_INVALID
    assert lib.fastsvc_pack_weights_device(plan._h, arr, n, blob.ctypes.data, None, sb, None) == E_INVALID
    arr[3].data = None
    assert lib.fastsvc_pack_weights_device(plan._h, arr, n, blob.ctypes.data, scratch.ctypes.data, sb, None) == E_INVALID
    # (too small a scratch is refused on the host as well)
    arr, n, keep = _tensor_array(base)
    assert lib.fastsvc_pack_weights_device(plan._h, arr, n, blob.ctypes.data, scratch.ctypes.data, sb - 1, None) == -3


# SHA-256 of the host packer's blob on the commit before the device packer existed
HOST_BLOB_SHA256 = {
    ("tiny", 77): "1be9b34b20be6450f6b9a79e872c506eb2d1815e7d76549df96a453f588bee1c",
    ("full", 201): "c525262d206c50a6bad950edcdd95fa3318f8e2a43a8b7a623633eebcd8b72b4",
}


@pytest.mark.parametrize("which,seed", sorted(HOST_BLOB_SHA256))
def test_the_host_packer_did_not_move(which, seed):
    cfg = A.TINY_CONFIG if which == "tiny" else A.FULL_CONFIG
    plan = A.Plan(cfg)
    sd = S.synth_state_dict(cfg, seed)
    blob = plan.pack(sd)
    assert blob.numel() * 4 == plan.blob_bytes
    assert hashlib.sha256(blob.numpy().tobytes()).hexdigest() == HOST_BLOB_SHA256[(which, seed)]
    assert torch.equal(plan.pack(sd), blob)                 # the pool's jobs write disjoint regions


def test_generator_and_train_step_switches():
    """`pack_on_device` is off for the module (inference keeps the host route) and a TrainStep on the CPU leaves it off."""
    from svcc23_fastsvc_amd import training as TR
    assert A.FastSVCGenerator.pack_on_device is False
    cfg = A.TINY_CONFIG
    gen = A.FastSVCGenerator(in_channels=cfg.in_channels, mid_channels=list(cfg.mid_channels),
                             upsampling_scales=list(cfg.upsampling_scales), out_channels=cfg.out_channels,
                             spk_emb_size=cfg.spk_emb_size, use_spk_emb=cfg.use_spk_emb)
    assert set(dict(gen.named_parameters())) == set(gen.state_dict())      # what pack_device is handed
    disc = TR.MelGANMultiScaleDiscriminator(scales=1, discriminator_params=dict(
        in_channels=1, out_channels=1, kernel_sizes=[5, 3], channels=4, max_downsample_channels=8, downsample_scales=[2]))
    TR.TrainStep(gen, disc, dict(discriminator_train_start_steps=0))
    assert gen.pack_on_device is False
    gen.prefetch_packed_weights()                            # CPU parameters: nothing to do, nothing raised
