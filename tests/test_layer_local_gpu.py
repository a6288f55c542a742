"""Teacher-forced per-layer parity of the 2-byte storages (-m gpu): every layer of the yaml generator is fed what the GPU
itself stored as its input, restated in float64 (tests/layer_local.py) and compared element by element with what the GPU
stored as its output, within a derived bound of about one ulp of the storage type.  One forward per (route, storage,
speaker mode, batch); the float64 references run on the CPU on copies of its workspace.

Route A: every layer its own launch (non-compact workspace, no shipped table, every fused route switched off).
Route B: the default launch selection - `d3x`, the fused c2 -> c3 / c1 -> c2 -> c3 / FiLM launches, `conv_last` on the last
block - each fused launch checked by a multi-layer segment between the taps that still exist.
Route S: what ships - the default plan with the shipped table, then the compact workspace with the whole-stage conditioning
launches `cond.0` / `cond.1` (from the signals to `ss.k` and the compact decimated copies `down_hd.k`).
Route C: Route A with the wide-layer kernel (csrc/fastsvc_wx.hip) and the two-per-CU conv_hx instances forced on, checked on
the layers they take over - a reference for those kernels that is not another kernel.

Reference layers: every convolution of `FastSVCGenerator` (harana/models/fastsvc.py:80-140, 164-232, 301-340)."""
import numpy as np
import pytest
import torch

import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import synth as S

import layer_local as LL

pytestmark = pytest.mark.gpu

CFG = S.FULL_CONFIG
SFX = {"bfloat16": ("|b",), "float16": ("|b", "|h")}
TAG = {"bfloat16": "x1", "float16": "h1"}
# the smallest shapes at which tiles, chunks and row ends all occur: 3840 - 4480 columns at the last block's rate
BATCHES = {"full": (2, 24, None), "ragged": (5, 28, [28, 25, 22, 7, 1])}      # lengths: n mod 4 in {0, 1, 2, 3} and one frame
FUSED = ("c23", "c123", "chain", "d3x", "head")
WIDE_LAYERS = {"film.2.heads", "down.3.c2_d2", "down.3.c3_d4", "film.3.conv", "film.3.heads", "up.0.conv_first", "up.0.d9", "up.0.d27"}
TWO_CU = {"up.2.d9": "conv_hx<3,2,1,4,0,4,1,%s>"}
TWO_CU_B = {"up.2.d3x": "conv_hx<3,2,1,4,0,4,4,%s>", "up.2.d9": "conv_hx<3,2,1,4,0,4,1,%s>"}      # Route B: d3x stays fused
# launches of the shipped table that run on the f32-input MFMA family (csrc/fastsvc_kernels.hip: float32 weights and
# operands, which the 2-byte segment table does not describe): the ones WITHOUT a float64 reference here
UNREFERENCED = {"down.1.c1_res1x1", "up.3.conv_first", "up.3.up_stretch"}
WHOLE_STAGE = {"cond.0": {"down.0.c123", "film.0.chain"}, "cond.1": {"down.1.c1_res1x1", "down.1.c23", "film.1.chain"}}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    A.load_library()
    return torch.device("cuda:0")


_CACHE = {}


def _weights():
    if "w" not in _CACHE:
        _CACHE["w"] = S.fold_weight_norm(S.synth_state_dict(CFG, 311))       # folded: the packer takes `.weight` verbatim
    return _CACHE["w"]


def _rates():
    """columns per frame of conditioning stage k"""
    down = [1] + list(CFG.upsampling_scales)[::-1][:-1]
    out, r = [], CFG.hop
    for k in range(CFG.n_stages):
        r //= down[k]
        out.append(r)
    return out


def _table(route, storage, B, F):
    t = {}
    for sfx in SFX[storage]:
        for k, r in enumerate(_rates()):
            t[f"down.{k}.c23|{B}|{r * F}{sfx}"] = [3, 1, 4, 1, 0]             # c2 / c3 as separate launches
            t[f"film.{k}.chain|{B}|{r * F}{sfx}"] = [3, 1, 4, 1, 0]           # FiLM conv / heads likewise
        t[f"down.0.c123|{B}|{CFG.hop * F}{sfx}"] = [3, 1, 4, 1, 0]
        if route == "C":
            for layer, T in [("film.2.heads", 8 * F), ("down.3.c2_d2", 2 * F), ("down.3.c3_d4", 2 * F), ("film.3.conv", 2 * F),
                             ("film.3.heads", 2 * F), ("up.0.conv_first", F), ("up.0.d9", 2 * F), ("up.0.d27", 2 * F)]:
                t[f"{layer}|{B}|{T}{sfx}"] = [6, 4, 2, 2, 6]                  # conv_wx (algorithm 6)
            t[f"up.2.d9|{B}|{32 * F}{sfx}"] = [2, 1, 4, 2, 3]                 # the instance budgeted for two workgroups per CU
    return t


def _run(dev, route, storage, with_spk, batch):
    key = (route, storage, with_spk, batch)
    if key in _CACHE:
        return _CACHE[key]
    B, F, lens = BATCHES[batch]
    if route == "B":                                  # the default launch selection: every fused route; the C = 48 instances
        plan = A.Plan(CFG, storage=storage, load_shipped_table=False)     # budgeted for two workgroups per CU forced
        plan.load_tuned({f"{layer}|{B}|{32 * F}{sfx}": [2, 1, 4, 2, 3] for layer in TWO_CU_B for sfx in SFX[storage]})
    elif route == "S":                                                         # what ships: the default plan and its table
        plan = A.Plan(CFG, storage=storage)
    elif route in ("SC", "SP"):                                                # ... and the compact workspace the module and bench.py run
        plan = A.Plan(CFG, storage=storage, compact_workspace=True)
        if route == "SP":                             # the layer pipelines, which long batches get (algorithm 5 under the stage's key)
            plan.load_tuned({f"cond.{k}|{B}|{_rates()[k] * F}{sfx}": [1, 1, 1, 1, 5] for k in (0, 1) for sfx in SFX[storage]})
    else:
        plan = A.Plan(CFG, storage=storage, load_shipped_table=False)
        plan.keep_residual_convs_separate(B, F)
        plan.keep_block_heads_separate(B, F)
        plan.keep_last_block_output(B, F)
        plan.load_tuned(_table(route, storage, B, F))
    if ("blob", storage) not in _CACHE:
        _CACHE[("blob", storage)] = plan.pack(_weights()).to(dev)
    if ("ins", batch) not in _CACHE:
        b = S.synth_batch(CFG, B, F, 312)
        ppg, sine, lft = (np.array(a, np.float32) for a in (b.ppg, b.sine, b.lft))
        if lens is not None:                                                   # poison the inputs' padding
            rng = np.random.default_rng(313)
            for j, n in enumerate(lens):
                ppg[j, :, n:] = 1e3 * rng.standard_normal(ppg[j, :, n:].shape)
                sine[j, :, n * CFG.hop:] = 1e3
                lft[j, :, n * CFG.hop:] = -1e3
        _CACHE[("ins", batch)] = (ppg, sine, lft, np.array(b.spk_emb, np.float32))
    ppg, sine, lft, emb = _CACHE[("ins", batch)]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ws = torch.empty(plan.workspace_bytes(B, F), dtype=torch.uint8, device=dev)
    ws.fill_(0xFF)
    recs = []
    y = plan.forward(_CACHE[("blob", storage)], to(ppg), to(sine), to(lft), to(emb) if with_spk else None, workspace=ws,
                     profile=recs, lengths=lens)
    torch.cuda.synchronize()
    taps = {"ppg": ppg.astype(np.float64), "sig": np.concatenate([lft, sine], 0).astype(np.float64), "wave": y.cpu().double().numpy()}
    if with_spk:
        taps["spk_emb"] = emb.astype(np.float64)
    written = {t for r in recs for t in _written(r["layer"])} | {"ppg_act"} if route in ("B", "S") else None
    if route in ("SC", "SP"):                         # (shared buffers hold their last user's tensor: only these are read)
        last = CFG.n_stages - 1                       # ... the whole-stage launches' outputs, and the last block's tensors
        written = {"ss.0", "ss.1", "down_hd.1", "down_hd.2"} | {f"up.{last}.{t}" for t in ("a", "u1", "xmid", "u2", "u3", "spk", "stats")}
    for name, shape in LL.tap_shapes(CFG, B, F).items():
        if name == "wave" or (not with_spk and name.endswith((".spk", ".stats"))):
            continue
        if written is not None and name not in written and (route in ("SC", "SP") or not name.endswith((".spk", ".stats"))):
            continue                                                           # (a fused route never writes it)
        taps[name] = plan.tap(name, B, F, ws).cpu().double().numpy().reshape(shape)
    del ws
    _CACHE[key] = (taps, recs)
    return _CACHE[key]


def _segments_of(layer):
    """the segments a launch of the shipped routes is checked by: a fused launch's multi-layer segment, else the single layers"""
    fused = LL.fused_segments(CFG)
    if layer in fused:
        return [fused[layer]]
    if layer.startswith("cond."):
        return [fused[layer + ".hd"], fused[layer + ".ss"]]
    if layer == "spk_proj":
        return [s for s in LL.segments(CFG) if s.kind == "spk"]
    return [s for s in LL.segments(CFG) if layer in s.layers]


def _written(layer):
    return [t for s in _segments_of(layer) for t in s.outputs]


def _check(taps, recs, segs, storage, with_spk, batch, label):
    B, F, lens = BATCHES[batch]
    bad = []
    for seg in segs:
        rep = LL.check_segment(seg, taps, _weights(), storage, B, F, lens, with_spk, recs)
        assert rep.checked == LL.expected_elements(seg, CFG, B, F, lens, with_spk) > 0, (seg.name, rep.checked)   # nothing sampled
        print(f"LAYERLOCAL {label} {storage} spk={int(with_spk)} {batch} {seg.name} [{rep.kernel}]: {rep.checked} elements, "
              f"bound within one ulp for {100 * rep.share:.1f} %, median bound {rep.bound_ulps:.1f} ulp, largest {rep.bound_of_max:.1e} of the "
              f"tap's maximum, worst {rep.worst:.2f} bounds")
        if rep.failed:
            bad.append(rep.message)
    assert not bad, "\n".join(bad)


def _mfma_kernels_only(segs, recs):
    """the segment table models 2-byte operands: every convolution ran on the half-precision MFMA kernels (conv_hx /
    conv_wx), the stretched ones in their polyphase mode"""
    kernels = {r["layer"]: r["kernel"] for r in recs}
    for seg in segs:
        if seg.kind not in ("direct", "poly"):
            continue
        kn = next(kernels[l] for l in seg.layers if l in kernels)
        assert kn.startswith(("conv_hx<", "conv_wx<")), (seg.name, kn)
        if seg.kind == "poly":
            assert kn.startswith("conv_hx<") and kn.split(",")[4] == "3", (seg.name, kn)
            if seg.y2:                                # the reference models the staged FiLM-affine epilogue only
                assert LL.poly_staged(kn), (seg.name, kn)


CASES = [(st, spk, bt) for st in ("bfloat16", "float16") for spk in (True, False) for bt in ("full", "ragged")]
IDS = [f"{st}-{'spk' if spk else 'nospk'}-{bt}" for st, spk, bt in CASES]


@pytest.mark.parametrize("storage,with_spk,batch", CASES, ids=IDS)
def test_route_a_every_layer_its_own_launch(dev, storage, with_spk, batch):
    taps, recs = _run(dev, "A", storage, with_spk, batch)
    layers = [r["layer"] for r in recs]
    assert not [l for l in layers if l.rsplit(".", 1)[-1] in FUSED or l.startswith("cond.")], layers
    assert "conv_last" in layers
    segs = [s for s in LL.segments(CFG) if with_spk or s.kind != "spk"]
    for seg in segs:                                                  # each segment's launch ran (ppg_act's copy is not profiled)
        assert seg.name == "ppg_act" or LL.kernel_of(seg, recs) != "?", seg.name
    _check(taps, recs, segs, storage, with_spk, batch, "A")
    _mfma_kernels_only(segs, recs)


@pytest.mark.parametrize("storage,with_spk,batch", CASES, ids=IDS)
def test_route_c_wide_and_two_per_cu_instances(dev, storage, with_spk, batch):
    B, F, lens = BATCHES[batch]
    taps, recs = _run(dev, "C", storage, with_spk, batch)
    kernels = {r["layer"]: r["kernel"] for r in recs}
    on_wx = {l for l, k in kernels.items() if k.startswith("conv_wx<")}
    # (a ragged batch: rows at the frame rate or twice it may end inside a group of 4 - those launches stay on conv_hx's
    # row-end instances; the 8F-rate layer is eligible)
    # (conv_wx has its FiLM-affine epilogue only behind the InstanceNorm prologue: without a speaker up.0.d9 stays on conv_hx)
    wide = WIDE_LAYERS if with_spk else WIDE_LAYERS - {"up.0.d9"}
    assert on_wx == (wide if lens is None else {"film.2.heads"}), sorted(on_wx)
    for layer, kn in TWO_CU.items():
        assert kernels[layer] == kn % TAG[storage], (layer, kernels[layer])
    taken = on_wx | set(TWO_CU)
    segs = [s for s in LL.segments(CFG) if s.name in taken]
    assert len(segs) == len(taken)
    _check(taps, recs, segs, storage, with_spk, batch, "C")


@pytest.mark.parametrize("storage,with_spk,batch", CASES, ids=IDS)
def test_route_b_fused_launches(dev, storage, with_spk, batch):
    """The default launch selection (non-compact workspace, no table): the fused launches run, each checked by its
    multi-layer segment between the taps that still exist - xmid / u2 behind `d3x` (the stretched residual accumulated
    inside), `down_h.k` behind the fused c2 -> c3 / c1 -> c2 -> c3 launches, `ss.k` behind the fused FiLM nets, the waveform
    behind `conv_last` on the last block - and every other launch by its single-layer segment."""
    B, F, lens = BATCHES[batch]
    taps, recs = _run(dev, "B", storage, with_spk, batch)
    layers = [r["layer"] for r in recs]
    fused = {l for l in layers if l.rsplit(".", 1)[-1] in FUSED}
    # every fused launch the shape allows: stages 2 / 3 of the FiLM nets and stage 3's pair have no fused variant; in the
    # ragged batch up.0's rows (twice the frame rate) end inside a group of 4, where d3x has no instance
    expect = {"down.0.c123", "film.0.chain", "down.1.c23", "film.1.chain", "down.2.c23", "up.1.d3x", "up.2.d3x", "up.3.d3x"}
    if lens is None:
        expect.add("up.0.d3x")
    assert fused == expect, sorted(fused ^ expect)
    kernels = {r["layer"]: r["kernel"] for r in recs}
    for layer, kn in TWO_CU_B.items():
        assert kernels[layer] == kn % TAG[storage], (layer, kernels[layer])
    assert "conv_last" not in layers                                     # (it rode on the last block's final launch)
    segs = _shipped_segments(layers)                                      # (the last block's launch wrote the waveform, not `out`)
    _check(taps, recs, segs, storage, with_spk, batch, "B")
    _mfma_kernels_only(segs, recs)


def _shipped_segments(layers, skip=()):
    segs = [LL.Seg("ppg_act", ("ppg_act",), "convert", "ppg", y="ppg_act")]
    for layer in layers:
        if layer in skip:
            continue
        found = _segments_of(layer)
        assert found, f"launch {layer} has no segment"
        segs += [s for s in found if s not in segs]
    last = f"up.{CFG.n_stages - 1}.d27"
    return [s for s in segs if s.name != last] + [LL.fused_segments(CFG)["conv_last.fused"]]


def _f32_family(kernels):
    return {l for l, k in kernels.items() if k.startswith("conv_mfma")}


@pytest.mark.parametrize("storage,with_spk,batch", CASES, ids=IDS)
def test_route_s_shipped_table(dev, storage, with_spk, batch):
    """The default plan with the shipped launch table (non-compact workspace, so that every tap exists): every launch on the
    half-precision MFMA kernels or the VALU kernels is checked by its segment; the launches the table puts on the f32-input
    MFMA family are exactly UNREFERENCED."""
    taps, recs = _run(dev, "S", storage, with_spk, batch)
    kernels = {r["layer"]: r["kernel"] for r in recs}
    assert "conv_last" not in kernels and any(l.endswith(".d3x") for l in kernels), sorted(kernels)
    for layer, kn in kernels.items():                                    # every launch is of a family this file knows
        assert kn.startswith(("conv_hx<", "conv_wx<", "conv_mfma", "in1_conv", "spk_proj")), (layer, kn)
    assert _f32_family(kernels) == UNREFERENCED, sorted(_f32_family(kernels) ^ UNREFERENCED)
    segs = _shipped_segments(list(kernels), skip=UNREFERENCED)
    _check(taps, recs, segs, storage, with_spk, batch, "S")
    _mfma_kernels_only(segs, recs)


@pytest.mark.parametrize("pipelines", [False, True], ids=["phase", "pipe"])
@pytest.mark.parametrize("storage,with_spk,batch", CASES, ids=IDS)
def test_route_s_compact_workspace_whole_stage_launches(dev, storage, with_spk, batch, pipelines):
    """The plan the module and bench.py run (shipped table, compact workspace): conditioning stages 0 and 1 are one launch
    each, checked from the raw signals to `ss.0` / `down_hd.1` and from `down_hd.1` to `ss.1` / `down_hd.2`.  The buffers of
    the other launches are shared between stages there; they run the kernels of the non-compact plan, which checks them.
    Both kernels of each stage: the phase kernels these short batches get, and the layer pipelines of long batches, forced."""
    taps, recs = _run(dev, "SP" if pipelines else "SC", storage, with_spk, batch)
    kernels = {r["layer"]: r["kernel"] for r in recs}
    assert set(WHOLE_STAGE) <= set(kernels), sorted(kernels)
    for k in (0, 1):
        assert kernels[f"cond.{k}"].startswith(f"cond_stage{k}_pipe<") == pipelines, kernels[f"cond.{k}"]
    _, recs_s = _run(dev, "S", storage, with_spk, batch)
    kernels_s = {r["layer"]: r["kernel"] for r in recs_s}
    replaced = set().union(*WHOLE_STAGE.values())
    rest = {l: k for l, k in kernels.items() if l not in WHOLE_STAGE}
    assert rest == {l: k for l, k in kernels_s.items() if l not in replaced}
    fused = LL.fused_segments(CFG)
    segs = [fused[f"{c}.{o}"] for c in sorted(WHOLE_STAGE) for o in ("hd", "ss")]
    # Equal kernels do not cover the compact layout's buffer sharing.  The last block's tensors are the last users of their
    # shared buffers and still intact: its launches are checked here as well, in the shared layout, down to the waveform ...
    last = CFG.n_stages - 1
    segs += [fused[f"up.{last}.d3x"], next(s for s in LL.segments(CFG) if s.name == f"up.{last}.d9"), fused["conv_last.fused"]]
    # ... and the layer pipelines give the phase kernels' bits (same products in the same order), so the two compact runs
    # agree bit for bit on the waveform.  (Route S's waveform is NOT comparable that way: there the stages run as c123 /
    # c23 / FiLM-chain launches, whose roundings differ from the whole-stage kernels'.)
    if pipelines:
        other, _ = _run(dev, "SC", storage, with_spk, batch)
        assert np.array_equal(taps["wave"], other["wave"])
    _check(taps, recs, segs, storage, with_spk, batch, "SP" if pipelines else "SC")


def test_segment_table_names_the_plans_own_tensors():
    """every tap of the helper's list is a tensor of the plan's workspace layout, with the helper's shape (the library's
    `fastsvc_workspace_tap` answers from the layout itself, in both workspace modes)"""
    for compact in (False, True):
        plan = A.Plan(CFG, storage="bfloat16", compact_workspace=compact)
        for B, F, _ in BATCHES.values():
            for name, shape in LL.tap_shapes(CFG, B, F).items():
                if name == "wave" or (compact and not name.startswith(("ss.", "down_hd.", "ppg_act")) and not name.endswith((".out", ".spk", ".stats"))):
                    continue
                _, numel, _ = plan.tap_info(name, B, F)
                if not (compact and numel == 0):                         # (compact: a tensor no launch writes has size 0)
                    assert numel == int(np.prod(shape)), (name, numel, shape)
