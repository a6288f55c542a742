"""The layer-local check of tests/layer_local.py on the CPU: its bound is SOUND (a float32 model of the kernels, in several
accumulation orders, passes every segment) and NOT VACUOUS (each of the classic kernel mistakes, planted in one segment of
that model, fails the segment's check).  The second property is what stands in for a hand-picked tolerance.

Reference layers: every convolution of `FastSVCGenerator` (harana/models/fastsvc.py:80-140, 164-232, 301-340)."""
import numpy as np
import pytest
import torch

import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import synth as S

import layer_local as LL

CFG = S.FULL_CONFIG
# 2 x 8 frames, the second utterance 5 frames long: rows of 16 ... 1280 columns (tile edges 127 / 128 exist from the 32-per-frame
# rate on), row ends at 1 and 2 mod 4, a padded width that differs from the length
B, F, LENS = 2, 8, [8, 5]
FORMATS = ("bfloat16", "float16")


@pytest.fixture(scope="module")
def weights():
    return S.fold_weight_norm(S.synth_state_dict(CFG, 301))


@pytest.fixture(scope="module")
def batch():
    return S.synth_batch(CFG, B, F, 302)


_TAPS = {}


def _model_taps(weights, batch, fmt, with_spk, order):
    """every segment run once by the float32 model, each on the model's own stored outputs of the segments before it"""
    key = (fmt, with_spk, order)
    if key not in _TAPS:
        taps = LL.empty_taps(CFG, B, F, batch.ppg, batch.sine, batch.lft, batch.spk_emb if with_spk else None)
        for seg in LL.segments(CFG):
            if seg.kind == "spk" and not with_spk:
                continue
            LL.model_segment(seg, taps, weights, fmt, B, F, LENS, with_spk, order)
        _TAPS[key] = taps
    return _TAPS[key]


def test_storage_rounding_agrees_with_the_packers_conversions():
    """`round_storage` against `fastsvc_split_half` (pinned by tests/test_boundary.py::test_split_half_conversions_match_numpy)"""
    lib = A.load_library()
    rng = np.random.default_rng(11)
    x = np.concatenate([
        rng.standard_normal(8192).astype(np.float32) * np.float32(10.0) ** rng.integers(-8, 5, 8192).astype(np.float32),
        np.array([0.0, 1.0, -1.0, 65504.0, 65519.9, 65520.0, 6.1035156e-05, 6.0e-05, 5.9604645e-08, 2.9802322e-08, 2.98e-08,
                  1.0009765625, 1.00048828125, 1.00146484375, 1.00390625, 1.01171875, 0.3, -0.1], dtype=np.float32)])
    hi = np.zeros(x.size, np.uint16); bf = np.zeros(x.size, np.uint16)
    lib.fastsvc_split_half(x.ctypes.data, x.size, hi.ctypes.data, None, bf.ctypes.data)
    want_bf = torch.from_numpy(bf.view(np.int16)).view(torch.bfloat16).double().numpy()
    with np.errstate(over="ignore"):
        want_hi = hi.view(np.float16).astype(np.float64)
    for fmt, want in (("bfloat16", want_bf), ("float16", want_hi)):
        got, ulp = LL.round_storage(x.astype(np.float64), fmt)
        assert np.array_equal(got, want), fmt
        fin = np.isfinite(want) & (x != 0)
        assert np.all(np.abs(got[fin] - x[fin]) <= 0.5 * ulp[fin]), fmt


def test_segment_table_covers_the_workspace():
    """every tensor of the helper's tap list is the output of exactly one single-layer segment, the compact decimated copies
    `down_hd.k` of the whole-stage segments (tests/test_layer_local_gpu.py holds the list against the plan's own layout)"""
    outs = [t for s in LL.segments(CFG) for t in s.outputs]
    assert len(outs) == len(set(outs))
    stats = {s.st_out[0] for s in LL.segments(CFG) if s.st_out}
    hd = {s.y for n, s in LL.fused_segments(CFG).items() if n.endswith(".hd")}
    assert hd == {"down_hd.1", "down_hd.2"}
    assert set(outs) | stats | hd == set(LL.tap_shapes(CFG, B, F))


@pytest.mark.parametrize("with_spk,order", [(True, 0), (True, 1), (True, 2), (False, 0)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_bound_is_sound_for_a_float32_model_in_any_accumulation_order(weights, batch, fmt, with_spk, order):
    taps = _model_taps(weights, batch, fmt, with_spk, order)
    bad = []
    for seg in LL.segments(CFG):
        if seg.kind == "spk" and not with_spk:
            continue
        rep = LL.check_segment(seg, taps, weights, fmt, B, F, LENS, with_spk)
        assert rep.checked == LL.expected_elements(seg, CFG, B, F, LENS, with_spk) > 0, seg.name      # nothing is sampled
        if order == 0:
            print(f"LAYERLOCAL {fmt} spk={int(with_spk)} {seg.name}: {rep.checked} elements, bound within one ulp for "
                  f"{100 * rep.share:.1f} %, worst {rep.worst:.2f} bounds")
        if rep.failed:
            bad.append(rep.message)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("mut", LL.MUTATIONS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_each_mutation_fails_the_check_of_every_segment_it_fits(weights, batch, fmt, mut):
    """one output column at a tile edge from taps one column off | the last column of a ragged row without its zero padding |
    one channel's bias dropped | two input channels of a 32-channel chunk swapped in the weights | LeakyReLU slope 0.1 | the
    stretched operand read one input column late | the operand rounded to the other 2-byte type | InstanceNorm statistics
    over the padded width"""
    clean = _model_taps(weights, batch, fmt, True, 0)
    slipped, ran = [], 0
    for seg in LL.segments(CFG):
        if not LL.applicable(seg, mut, True):
            continue
        taps = dict(clean)
        for t in seg.outputs + ((seg.st_out[0],) if seg.st_out else ()):
            taps[t] = clean[t].copy()
        LL.model_segment(seg, taps, weights, fmt, B, F, LENS, True, 0, mut)
        rep = LL.check_segment(seg, taps, weights, fmt, B, F, LENS, True)
        ran += 1
        if not rep.failed:
            slipped.append(f"{seg.name}: worst {rep.worst:.2f} bounds")
    assert ran > 0
    assert not slipped, f"{mut} slipped through in {fmt}: " + "; ".join(slipped)


# (fused segment, layer of its chain, mutation) triples whose planted mutation stays inside the segment's bound in the CPU
# model at this file's shapes - out of reach of that segment's check, in either storage unless a format is named.  All but two
# lie in the whole-stage `cond.1` launch: `cond.1.ss` spans five layers at C = 48 / 96 with no tap in between and its linear
# bound has a median of 26 ulp in bfloat16 (122 ulp in float16; up to 1e-1 / 2e-2 of the tap's maximum) - the class of bound
# this file set out to replace, and no sound way past it without a tap the product does not expose; `cond.1.hd` holds
# c1 -> c2 -> c3 of the same launch to 0.6 / 1.4 ulp, but only at every 4th column.  The list is asserted EXACTLY: a triple
# that starts to fail its check must be taken off it.
OUT_OF_REACH = {
    # cond.1.hd sees every 4th column only: the last column of a row (odd) never reaches a column it keeps
    ("cond.1.hd", "cond.1.c1", "no_pad"), ("cond.1.hd", "cond.1.c2", "no_pad"),
    # cond.1.ss, the layers cond.1.hd also holds (it catches all of these but `no_pad` above)
    ("cond.1.ss", "cond.1.c1", "bias"), ("cond.1.ss", "cond.1.c1", "no_pad"), ("cond.1.ss", "cond.1.c1", "other_type"),
    ("cond.1.ss", "cond.1.c1", "slope"), ("cond.1.ss", "cond.1.c2", "bias"), ("cond.1.ss", "cond.1.c2", "other_type"),
    ("cond.1.ss", "cond.1.c2", "slope"), ("cond.1.ss", "cond.1.c2", "tile_edge"), ("cond.1.ss", "cond.1.h", "bias"),
    ("cond.1.ss", "cond.1.h", "other_type"), ("cond.1.ss", "cond.1.h", "slope"), ("cond.1.ss", "cond.1.h", "tile_edge"),
    ("cond.1.ss", "cond.1.c1", "swap_w", "bfloat16"), ("cond.1.ss", "cond.1.c2", "swap_w", "bfloat16"),
    ("cond.1.ss", "cond.1.c2", "no_pad", "bfloat16"),
    # cond.1.ss, the layers nothing else holds in that launch: its FiLM conv and heads
    ("cond.1.ss", "cond.1.u", "bias"), ("cond.1.ss", "cond.1.u", "other_type"), ("cond.1.ss", "cond.1.ss", "other_type"),
    # two-layer chains at C = 192: a median-sized bias / a half-ulp operand change in the first layer
    ("film.3.chain", "film.3.conv", "bias"), ("down.3.c23", "down.3.c2_d2", "other_type", "bfloat16"),
}


@pytest.mark.parametrize("fmt", FORMATS)
def test_fused_segments_sound_and_not_vacuous(weights, batch, fmt):
    """the multi-layer segments of the fused routes (c2 -> c3, c1 -> c2 -> c3, FiLM conv -> heads, d3x, conv_last on the last
    block, the whole-stage conditioning launches): the float32 model of each, fed the stored taps of the single-layer model,
    passes in every accumulation order; every mutation, planted in EACH layer of the chain it fits, fails the segment's
    check - except exactly the triples of OUT_OF_REACH"""
    clean = dict(_model_taps(weights, batch, fmt, True, 0))
    for name in ("cond.0.hd", "cond.1.hd"):               # the compact copies no single-layer segment writes: stage 1 reads the first
        seg = LL.fused_segments(CFG)[name]
        clean[seg.y] = clean[seg.y].copy()
        LL.model_segment(seg, clean, weights, fmt, B, F, LENS, True, 0)
    bad, slipped = [], set()

    def run(seg, order, mut):
        taps = dict(clean)
        for t in seg.outputs + ((seg.st_out[0],) if seg.st_out else ()):
            taps[t] = clean[t].copy()
        LL.model_segment(seg, taps, weights, fmt, B, F, LENS, True, order, mut)
        rep = LL.check_segment(seg, taps, weights, fmt, B, F, LENS, True)
        assert rep.checked == LL.expected_elements(seg, CFG, B, F, LENS, True) > 0, seg.name
        return rep

    for name, seg in LL.fused_segments(CFG).items():
        for order in (0, 1, 2):
            rep = run(seg, order, None)
            if order == 0:
                print(f"LAYERLOCAL {fmt} spk=1 {name}: {rep.checked} elements, bound within one ulp for {100 * rep.share:.1f} %, median "
                      f"bound {rep.bound_ulps:.1f} ulp, largest {rep.bound_of_max:.1e} of the tap's maximum, worst {rep.worst:.2f} bounds")
            if rep.failed:
                bad.append(rep.message)
        for layer in LL.chain_layers(seg):
            for mut in LL.MUTATIONS:
                if LL.applicable(layer, mut, True) and not run(seg, 0, (mut, layer.name, seg.y_dec)).failed:
                    slipped.add((name, layer.name, mut))
    assert not bad, "\n".join(bad)
    want = {t[:3] for t in OUT_OF_REACH if len(t) == 3 or t[3] == fmt}
    assert slipped == want, f"slipped but not listed: {sorted(slipped - want)}; listed but caught: {sorted(want - slipped)}"
