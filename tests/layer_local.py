"""Teacher-forced, layer-local parity for the 2-byte activation storages (bfloat16, float16).

Every layer of the yaml generator (`S.FULL_CONFIG`) is one SEGMENT: the workspace taps it reads, the taps it writes, and a
float64 restatement of that one layer built from the oracle's pieces (`oracle/fastsvc_oracle.py`: `_conv`, `_lrelu`,
`_squeeze`, `_stretch`, `_speaker_bias`; InstanceNorm as the kernels apply it, below).  A check feeds a segment the values
the GPU itself stored as the layer's input and requires every valid element the GPU stored as its output to lie within a
DERIVED bound of the float64 result - so rounding noise does not accumulate with depth and the bound per element is about one
ulp of the storage type, not a few percent of the tensor's maximum.  Nothing here is a measured tolerance.

Rounding points, read from the kernels (csrc/fastsvc_device.inc, fastsvc_hx_common.inc, fastsvc_hx.hip, fastsvc_wx.hip,
fastsvc_kernels.hip, the packer in fastsvc_plan.cpp / fastsvc_pack.hip); `r16` = round to nearest even into the storage type:

* weights of the MFMA layers: `r16(w)` of the folded float32 weight (the packer's 2-byte fragment sets; a state dict that
  already holds `.weight` is taken verbatim).  Polyphase stretch convs (`up.i.res_stretch`, `up.i.up_stretch`) hold
  `r16(W0)`, `r16(float32(W0 + W1 + W2))`, `r16(W2)` and multiply `x[j-1]`, `x[j]`, `x[j+1]` and the sign-flipped `x[j]`
  separately: out[s j + ph] = Wsum x[j] + [ph = 0] (W0 x[j-1] - W0 x[j]) + [ph = s-1] (W2 x[j+1] - W2 x[j]).
  Biases, the rank-1 residual of stage 0, `down.0.c1` (VALU), `conv_last` (VALU) and the speaker projection read float32.
  The FiLM heads' bias is float32(b_lft + b_sine).
* operands: a stored tensor enters as it is stored.  Where the staging waves transform it, the operand is
  `r16(lrelu(fma(u, A, Bc)))` with `A = float32(rstd)`, `Bc = float32(p - mean rstd)`, `mean = s1 / n`,
  `var = max(s2 / n - mean^2, 0)`, `rstd = 1 / sqrt(var + 1e-5)` in float64 from the float64 sums `(s1, s2)` of the
  producer's UNROUNDED u over the utterance's own n columns (the `up.i.stats` tap) and the float32 speaker bias p (the
  `up.i.spk` tap); without a speaker embedding `(A, Bc) = (1, 0)`; `lrelu(v) = max(v, 0.2f v)` in float32.
* epilogue: `v = acc + bias` [, `lrelu`] [, `+ residual` as stored | `+ r1w x + r1b` in float32]; `y = r16(v)`;
  `y2 = r16(scale v + shift)` from the UNROUNDED float32 v and the stored scale / shift; the InstanceNorm sums add the unrounded
  `scale v + shift` (float32 per tile, float64 across tiles).  `conv_last` writes float32.  One exception, which the
  issue's list did not have: the polyphase FiLM-affine instances whose tile fits the wave's 16 KB LDS patch (`poly_staged`; all
  four `up.i.up_stretch` launches of the yaml generator) round the finished tile into the patch first,
  `y2 = r16(scale r16(v) + shift)`, and sum that `scale r16(v) + shift`.

The bound of one output element (all terms float64, computed beside the reference):

    bound = 0.5 ulp16(|ref| + d) + d,     d = gamma (|x^| * |w|) + sum_near-tie |w| ulp16(x^) + epilogue term

* `|x^| * |w|`: the same convolution on absolute values (every product the kernel forms, the polyphase kernels' cancelling
  pairs included).  Products of two 2-byte values are exact in float32 (8 + 8 or 11 + 11 significand bits <= 24).
* `gamma`: the float32 summation bound.  A sum of n exact terms in ANY order is within (n - 1) 2^-24 sum |terms| of the
  exact sum to first order (Higham, Accuracy and Stability, 4.2): `(n_terms + 4) 2^-24` with n_terms = K C_in is sound
  whatever the hardware does, and is what the VALU layers (`down.0.c1`, `conv_last`: inexact products, one more rounding
  each, counted in the + 4 with the bias) use.  For the MFMA layers it is too loose: at C = 192 it is 580 2^-24 ~ 0.4 ulp
  of bfloat16 after the cancellation of a 576-term sum, and the mutation "operand rounded to the other type" then slips
  through the widest layers (tests/test_layer_local.py).  They use the blocked count that follows the K loop instead: one
  `v_mfma_f32_16x16x32` adds 32 exact products to its accumulator; the bound assumes no more than the instruction's 8
  K-steps of 4 products (the K of the architecture's smallest matrix instruction) each rounding the accumulator once, the 4
  products of a step joined by at most 3 additions.  A product that enters at step p of instruction j of N then passes
  at most 3 + (8 - p) + 8 (N - j) <= 8 N + 3 roundings, so `gamma = (8 N + 8) 2^-24`, N = K ceil(C_in / 32) instructions
  per output tile (polyphase: 5 per chunk - the sum tap, and both outer taps with their sign-flipped twins), + 5 for the
  bias that may start the accumulator and the polyphase joins.  A single rounding per instruction (N), or a pairwise
  tree (N + 5), lie inside it; only a fully sequential 32-term chain per instruction would not.  This is an ASSUMPTION
  about how the hardware rounds inside one instruction, not a theorem: nothing public specifies it.  The GPU runs of
  tests/test_layer_local_gpu.py are what validates it (every element of every segment inside the bound on an MI355X);
  if a later run fails by a small factor across many elements of the wide layers only, suspect this term first - the
  flat count is the sound fallback.
* near-tie: the float32 evaluation of the operand transform is within `e = 2^-23 (|u A| + |Bc|) + 2^-23 |v|` of its
  float64 value (one FMA or a multiply and an add, the slope's product, and 0.2f against 0.2); an operand whose float64
  value is within e of a rounding boundary may come out one ulp16 away, which moves the output by at most |w| ulp16(x^).
* epilogue term: 2^-24 (magnitude of the operands) per float32 operation behind the accumulator (bias, slope product,
  residual add; three for the rank-1 term; two for scale v + shift, scaled by |scale| for what v carries).
* 0.5 ulp16 is taken at |ref| + d: the GPU's unrounded value may sit in the next binade.  float32 outputs: ulp32.

InstanceNorm sums: `|s1 - sum u_ref| <= sum d_u + 512 2^-24 sum |u|` and `|s2 - sum u_ref^2| <= sum (2 |u| d_u + d_u^2)
+ 514 2^-24 sum u^2` (+ 2^-50 relative for the float64 joins): a lane's float32 partial sum spans one tile of at most 512
columns (NW <= 8 tiles of 16 columns times WN <= 4 waves), partial sums are joined in float64.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from oracle import fastsvc_oracle as O

U32 = 2.0 ** -24
SIG_BITS = {"bfloat16": 8, "float16": 11}
OTHER = {"bfloat16": "float16", "float16": "bfloat16"}
TORCH_DT = {"bfloat16": torch.bfloat16, "float16": torch.float16}
SLOPE32 = np.float32(O.LRELU_SLOPE)
TILE_COLS = 512                     # upper bound of the columns one float32 partial InstanceNorm sum spans
MUTATIONS = ("tile_edge", "no_pad", "bias", "swap_w", "slope", "stretch_late", "other_type", "stats_width")


# ---------------------------------------------------------------------------------------------------------------
# storage rounding
# ---------------------------------------------------------------------------------------------------------------
def round_storage(x, fmt: str) -> Tuple[np.ndarray, np.ndarray]:
    """float64 -> (nearest `fmt` value, round to nearest even, as float64; the ulp of `fmt` at x).  Agrees with
    `fastsvc_split_half`'s bf16 / f16_hi outputs on float32 inputs (tests/test_layer_local.py); binary16 subnormals have
    the fixed ulp 2^-24, magnitudes that round past 65504 become infinities; zero has ulp 0 (binary16: 2^-24)."""
    x = np.asarray(x, np.float64)
    p = SIG_BITS[fmt]
    _, e = np.frexp(x)                                   # |x| in [2^(e-1), 2^e)
    ulp = np.ldexp(1.0, e - p)
    if fmt == "float16":
        ulp = np.maximum(ulp, 2.0 ** -24)
    else:
        ulp = np.where(x == 0.0, 0.0, ulp)
    with np.errstate(invalid="ignore", divide="ignore"):
        val = np.where(ulp > 0.0, np.rint(x / np.where(ulp > 0.0, ulp, 1.0)) * ulp, 0.0)
    if fmt == "float16":
        val = np.where(np.abs(val) > 65504.0, np.copysign(np.inf, val), val)
    return val, ulp


def ulp32(x) -> np.ndarray:
    _, e = np.frexp(np.asarray(x, np.float64))
    return np.ldexp(1.0, e - 24)


def _t(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))[None]


def _conv64(x: np.ndarray, w: np.ndarray, dil: int) -> np.ndarray:
    """(C_in, T) x (C_out, C_in, K) -> (C_out, T): the oracle's `_conv` (zero 'same' padding) without a bias."""
    wd = {"p.weight": torch.from_numpy(np.ascontiguousarray(w, np.float64)), "p.bias": torch.zeros(w.shape[0], dtype=torch.float64)}
    return O._conv(_t(x), wd, "p", dil)[0].numpy()


def _lrelu64(x: np.ndarray) -> np.ndarray:
    return O._lrelu(torch.from_numpy(np.ascontiguousarray(x, np.float64))).numpy()


# ---------------------------------------------------------------------------------------------------------------
# the segment table
# ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Seg:
    name: str                       # the launch of Route A that runs it (`profile=` layer name)
    layers: Tuple[str, ...]         # launches that may run it, first match names the kernel
    kind: str                       # direct | poly | in1 | pointwise | convert | spk
    x: str                          # input tap
    w: Tuple[str, ...] = ()         # weight prefixes: (lft, sine) for the conditioning layers, else one
    layout: str = "up"              # up: (B, C, T) | cond: (2B, C, T), weights per signal | film: cond in, (B, 2C, T) out | heads
    K: int = 3
    dil: int = 1
    dec: int = 1                    # the input is read every `dec`-th column (Squeeze2d)
    stretch: int = 1                # Stretch2d factor of the polyphase convs
    rate: int = 1                   # input columns per frame (after the decimation)
    pre: str = "none"               # none | lrelu | norm (InstanceNorm + speaker bias where a speaker is given, then lrelu)
    post_lrelu: bool = False
    res: Optional[str] = None       # residual tap, added as stored
    rank1: Tuple[str, ...] = ()     # stage 0: the 1x1 residual conv of the raw signal, float32 (weight prefixes per signal)
    ss: Optional[str] = None        # FiLM scale / shift tap -> y2, InstanceNorm sums
    y: Optional[str] = None
    y2: Optional[str] = None
    st_in: Optional[Tuple[str, int]] = None
    st_out: Optional[Tuple[str, int]] = None
    block: int = -1                 # up block (speaker tap `up.<block>.spk`)
    first: Optional["Seg"] = None   # fused launches: the layer whose output stays in LDS / registers and feeds this one
    x2: Optional[str] = None        # d3x: second operand tap (the raw `a`), stretched `stretch2` times through `w2`'s plain taps
    w2: Tuple[str, ...] = ()        # (one prefix, or one per signal)
    stretch2: int = 1
    y_dec: int = 1                  # the output tap holds every `y_dec`-th column (the compact decimated copy `down_hd.k`)

    @property
    def outputs(self) -> Tuple[str, ...]:
        return tuple(t for t in (self.y, self.y2) if t)


def segments(cfg) -> List[Seg]:
    """Single-layer segments of a generator, in execution order: every workspace tensor of the non-compact layout is the
    output of one of them (`down_hd.k`, which only the whole-stage conditioning launches write, excepted)."""
    n = cfg.n_stages
    scales = list(cfg.upsampling_scales)
    mids = list(cfg.mid_channels)
    hop = int(np.prod(scales))
    down_scales = [1] + scales[::-1][:-1]
    segs = [Seg("ppg_act", ("ppg_act",), "convert", "ppg", y="ppg_act")]
    for i in range(n):
        segs.append(Seg(f"up.{i}.spk", ("spk_proj",), "spk", "spk_emb", (f"upsampling_nets.{i}.emb_projector",), y=f"up.{i}.spk", block=i))
    rate = hop
    for k in range(n):
        rate //= down_scales[k]
        dn = tuple(f"downsampling_{s}.{k}" for s in ("lft", "sine"))
        fl = tuple(f"film_{s}.{k}" for s in ("lft", "sine"))
        if k == 0:
            segs.append(Seg("down.0.c1", ("down.0.c1",), "in1", "sig", tuple(p + ".downsample_block.2" for p in dn), "cond",
                            rate=rate, pre="lrelu", y="down_c1.0"))
        else:
            segs.append(Seg(f"down.{k}.c1", (f"down.{k}.c1_res1x1", f"down.{k}.c1"), "direct", f"down_h.{k - 1}",
                            tuple(p + ".downsample_block.2" for p in dn), "cond", dec=down_scales[k], rate=rate, pre="lrelu", y=f"down_c1.{k}"))
            segs.append(Seg(f"down.{k}.r", (f"down.{k}.c1_res1x1", f"down.{k}.res1x1"), "direct", f"down_h.{k - 1}",
                            tuple(p + ".residual_block.0" for p in dn), "cond", K=1, dec=down_scales[k], rate=rate, y=f"down_r.{k}"))
        segs.append(Seg(f"down.{k}.c2_d2", (f"down.{k}.c2_d2",), "direct", f"down_c1.{k}", tuple(p + ".downsample_block.4" for p in dn),
                        "cond", dil=2, rate=rate, pre="lrelu", y=f"down_c2.{k}"))
        segs.append(Seg(f"down.{k}.c3_d4", (f"down.{k}.c3_d4",), "direct", f"down_c2.{k}", tuple(p + ".downsample_block.6" for p in dn),
                        "cond", dil=4, rate=rate, pre="lrelu", res=None if k == 0 else f"down_r.{k}",
                        rank1=tuple(p + ".residual_block.0" for p in dn) if k == 0 else (), y=f"down_h.{k}"))
        segs.append(Seg(f"film.{k}.conv", (f"film.{k}.conv",), "direct", f"down_h.{k}", tuple(p + ".conv" for p in fl), "film",
                        rate=rate, post_lrelu=True, y=f"film_u.{k}"))
        segs.append(Seg(f"film.{k}.heads", (f"film.{k}.heads",), "direct", f"film_u.{k}", fl, "heads", rate=rate, y=f"ss.{k}"))
    rate = 1
    for i in range(n):
        k = n - 1 - i
        s = scales[i]
        up = f"upsampling_nets.{i}"
        st = f"up.{i}.stats"
        ss = f"ss.{k}"
        segs.append(Seg(f"up.{i}.conv_first", (f"up.{i}.conv_first",), "direct", "ppg_act" if i == 0 else f"up.{i - 1}.out",
                        (up + ".conv_first",), rate=rate, y=f"up.{i}.a"))
        segs.append(Seg(f"up.{i}.res_stretch", (f"up.{i}.res_stretch",), "poly", f"up.{i}.a", (up + ".residual_block.1",),
                        stretch=s, rate=rate, y=f"up.{i}.xr"))
        segs.append(Seg(f"up.{i}.up_stretch", (f"up.{i}.up_stretch",), "poly", f"up.{i}.a", (up + ".upsample_block0.2",),
                        stretch=s, rate=rate, pre="lrelu", post_lrelu=True, ss=ss, y2=f"up.{i}.u1", st_out=(st, 0)))
        rate *= s
        segs.append(Seg(f"up.{i}.d3", (f"up.{i}.d3",), "direct", f"up.{i}.u1", (up + ".conv_block1.1",), dil=3, rate=rate, pre="norm",
                        res=f"up.{i}.xr", ss=ss, y=f"up.{i}.xmid", y2=f"up.{i}.u2", st_in=(st, 0), st_out=(st, 1), block=i))
        segs.append(Seg(f"up.{i}.d9", (f"up.{i}.d9",), "direct", f"up.{i}.u2", (up + ".conv_block2.1",), dil=9, rate=rate, pre="norm",
                        ss=ss, y2=f"up.{i}.u3", st_in=(st, 1), st_out=(st, 2), block=i))
        segs.append(Seg(f"up.{i}.d27", (f"up.{i}.d27",), "direct", f"up.{i}.u3", (up + ".conv_block3.1",), dil=27, rate=rate, pre="norm",
                        res=f"up.{i}.xmid", y=f"up.{i}.out", st_in=(st, 2), block=i))
    segs.append(Seg("conv_last", ("conv_last",), "pointwise", f"up.{n - 1}.out", ("conv_last",), K=1, rate=rate, y="wave"))
    return segs


def fused_segments(cfg) -> Dict[str, Seg]:
    """launch name -> the multi-layer segment of a fused route, between the taps that still exist: the single-layer
    references chained, the tensor between them rounded where the kernel rounds it (the LDS tile of the c2 -> c3 / c1 ->
    c2 -> c3 / FiLM conv -> heads launches: `r16(lrelu(acc + bias))`, csrc/fastsvc_hx.hip hx_chain_store), not at all where
    it does not (`d3x`: the stretched residual conv's products join the d = 3 conv's accumulator, the biases add in
    float32; `conv_last` on the last block: a float32 dot product of the finished, unrounded block output)."""
    from dataclasses import replace
    by = {s.name: s for s in segments(cfg)}
    n = cfg.n_stages
    out = {}
    for k in range(n):
        c2, c3 = by[f"down.{k}.c2_d2"], by[f"down.{k}.c3_d4"]
        out[f"down.{k}.c23"] = replace(c3, name=f"down.{k}.c23", layers=(f"down.{k}.c23",), first=c2)
        out[f"film.{k}.chain"] = replace(by[f"film.{k}.heads"], name=f"film.{k}.chain", layers=(f"film.{k}.chain",), first=by[f"film.{k}.conv"])
    out["down.0.c123"] = replace(by["down.0.c3_d4"], name="down.0.c123", layers=("down.0.c123",),
                                 first=replace(by["down.0.c2_d2"], name="down.0.c12", first=by["down.0.c1"]))
    for i in range(n):
        out[f"up.{i}.d3x"] = replace(by[f"up.{i}.d3"], name=f"up.{i}.d3x", layers=(f"up.{i}.d3x",), res=None, x2=f"up.{i}.a",
                                     w2=(f"upsampling_nets.{i}.residual_block.1",), stretch2=int(cfg.upsampling_scales[i]))
    # The whole-stage conditioning launches (csrc/fastsvc_cond.hip; the compact workspace): c1 -> c2 -> c3 -> film.conv -> heads
    # on LDS planes, every plane `r16(lrelu(acc))` (p0_layer_chunk / q1_layer_chunk KIND 0 / 2) except h, `r16(acc)` (KIND 1),
    # which film.conv reads and whose every s'-th column is copied out as `down_hd.<k+1>`.  Stage 1 reads the compact copy;
    # its 1x1 residual conv's products join c3's accumulator (never rounded), the biases add in float32.
    # How much these segments hold: `cond.k.hd` (three layers) and `cond.0.ss` stay near one ulp; `cond.1.ss` - five layers at
    # C = 48 / 96 with no tap in between - has a linear bound of about 20 ulp in bfloat16 and 100 ulp in float16 (median; up to
    # 6e-2 / 2e-2 of the tap's maximum on the GPU batches), so it catches gross faults of stage 1's FiLM net only; which planted
    # mistakes stay inside it is listed, exactly, in tests/test_layer_local.py (OUT_OF_REACH).
    down = [1] + list(cfg.upsampling_scales)[::-1][:-1]
    if n > 2:
        h0 = replace(out["down.0.c123"], name="cond.0.h", layers=("cond.0",), y=None)
        c1 = replace(by["down.1.c1"], name="cond.1.c1", layers=("cond.1",), x="down_hd.1", dec=1)
        c2 = replace(by["down.1.c2_d2"], name="cond.1.c2", layers=("cond.1",), first=c1)
        h1 = replace(by["down.1.c3_d4"], name="cond.1.h", layers=("cond.1",), first=c2, res=None, x2="down_hd.1",
                     w2=tuple(f"downsampling_{s}.1.residual_block.0" for s in ("lft", "sine")), y=None)
        for k, h in ((0, h0), (1, h1)):
            out[f"cond.{k}.hd"] = replace(h, name=f"cond.{k}.hd", y=f"down_hd.{k + 1}", y_dec=down[k + 1])
            out[f"cond.{k}.ss"] = replace(by[f"film.{k}.heads"], name=f"cond.{k}.ss", layers=(f"cond.{k}",),
                                          first=replace(by[f"film.{k}.conv"], name=f"cond.{k}.u", first=h))
    out["conv_last.fused"] = replace(by["conv_last"], name="conv_last.fused", layers=(f"up.{n - 1}.d27",), first=by[f"up.{n - 1}.d27"])
    return out


def chain_layers(seg: Seg) -> List[Seg]:
    """the layers of a (fused) segment, last one first"""
    return [seg] + (chain_layers(seg.first) if seg.first is not None else [])


def applicable(seg: Seg, mut: str, with_spk: bool) -> bool:
    """Which of the mutations of tests/test_layer_local.py a layer has the code for.  (Whether a mutation that fits is also
    within reach of a multi-layer segment's bound is not decided here: tests/test_layer_local.py plants every mutation in
    every layer of every chain and lists the triples that slip through.)"""
    if seg.kind in ("convert", "spk"):
        return False
    if mut == "tile_edge":
        return True
    if mut == "no_pad":
        return seg.K == 3 and seg.y_dec == 1                  # (the last column is not one the decimated copy keeps)
    if mut == "bias":
        return True
    if mut == "swap_w":
        return seg.kind != "in1"
    if mut == "slope":
        return (seg.pre != "none" or seg.post_lrelu) and not (seg.first is not None and seg.pre == "none")
    if mut == "stretch_late":
        return seg.kind == "poly" or seg.x2 is not None
    if mut == "other_type":
        return (seg.pre != "none" or seg.first is not None) and seg.kind not in ("in1", "pointwise")
    if mut == "stats_width":
        return seg.pre == "norm" and with_spk
    raise KeyError(mut)


# ---------------------------------------------------------------------------------------------------------------
# weights as the kernels hold them
# ---------------------------------------------------------------------------------------------------------------
def _w3(weights, prefix) -> np.ndarray:
    w = np.asarray(weights[prefix + ".weight"], np.float32)
    if w.ndim == 4:
        w = w[:, :, 0, :]
    return w


def layer_weights(seg: Seg, weights, sig: Optional[int], fmt: str) -> Dict[str, np.ndarray]:
    """{'w': (C_out, C_in, K) float64 as multiplied, 'wabs': what bounds the products' magnitudes, 'b': bias}"""
    if seg.layout == "heads":
        parts = {}
        for s, name in enumerate(seg.w):
            parts[s] = (_w3(weights, name + ".conv_scale"), _w3(weights, name + ".conv_shift"))
        w = np.concatenate([np.concatenate([parts[0][0], parts[1][0]], 1), np.concatenate([parts[0][1], parts[1][1]], 1)], 0)
        b = np.concatenate([np.asarray(weights[seg.w[0] + ".conv_scale.bias"], np.float32) + np.asarray(weights[seg.w[1] + ".conv_scale.bias"], np.float32),
                            np.asarray(weights[seg.w[0] + ".conv_shift.bias"], np.float32) + np.asarray(weights[seg.w[1] + ".conv_shift.bias"], np.float32)])
    else:
        name = seg.w[sig if len(seg.w) > 1 else 0]
        w = _w3(weights, name)
        b = np.asarray(weights[name + ".bias"], np.float32)
    out = {"b": b.astype(np.float64)}
    if seg.kind in ("in1", "pointwise"):
        out["w"] = w.astype(np.float64)
        out["wabs"] = np.abs(out["w"])
    elif seg.kind == "poly":
        w0 = round_storage(w[:, :, 0], fmt)[0]
        w2 = round_storage(w[:, :, 2], fmt)[0]
        ws = round_storage((w[:, :, 0].astype(np.float64) + w[:, :, 1].astype(np.float64) + w[:, :, 2].astype(np.float64)).astype(np.float32), fmt)[0]
        out["poly"] = (w0, ws, w2)
        # taps on the STRETCHED axis with the kernel's values at every phase (module docstring)
        out["w"] = np.stack([w0, ws - w0 - w2, w2], -1)
        out["wabs"] = np.stack([np.abs(w0), np.abs(ws) + np.abs(np.abs(w0) - np.abs(w2)), np.abs(w2)], -1)
    else:
        out["w"] = round_storage(w, fmt)[0]
        out["wabs"] = np.abs(out["w"])
    if seg.w2:
        name2 = seg.w2[sig if len(seg.w2) > 1 else 0]
        out["w2"] = round_storage(_w3(weights, name2), fmt)[0]
        out["b"] = (b + np.asarray(weights[name2 + ".bias"], np.float32)).astype(np.float64)       # one accumulator, float32 sum
    if seg.rank1:
        name = seg.rank1[sig]
        out["r1w"] = np.asarray(weights[name + ".weight"], np.float64).reshape(-1)
        out["r1b"] = np.asarray(weights[name + ".bias"], np.float64).reshape(-1)
    return out


# ---------------------------------------------------------------------------------------------------------------
# tap access (full padded arrays, float64)
# ---------------------------------------------------------------------------------------------------------------
def instances(seg: Seg, B: int):
    if seg.layout in ("cond", "film"):
        return [(s, b) for s in (0, 1) for b in range(B)]
    return [(None, b) for b in range(B)]


def _row(seg: Seg, taps, name: str, sig, b: int, B: int, out: bool):
    t = taps[name]
    if seg.layout == "cond" or (seg.layout == "film" and not out):
        return t[sig * B + b]
    if seg.layout == "film":
        C = t.shape[1] // 2
        return t[b, sig * C:(sig + 1) * C]
    return t[b]


def norm_coefficients(stats_row: np.ndarray, spk_row: np.ndarray, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """(A, Bc) exactly as the staging code computes them: float64 from the sums, then rounded to float32."""
    mean = stats_row[:, 0] / float(n)
    var = np.maximum(stats_row[:, 1] / float(n) - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + O.IN_EPS)
    A = rstd.astype(np.float32)
    Bc = (spk_row.astype(np.float64) - mean * rstd).astype(np.float32)
    return A, Bc


def _lens(B, F, lens):
    return [F] * B if lens is None else [int(v) for v in lens]


# ---------------------------------------------------------------------------------------------------------------
# the float64 reference of one instance (one utterance [, one signal]) and its bound
# ---------------------------------------------------------------------------------------------------------------
def _operand_ref(seg: Seg, xs: np.ndarray, fmt: str, coef, xerr=None):
    """input (C, n) -> (operand x^, how far the operand the kernel multiplies may lie from x^).  `xerr` None: xs is a stored
    tensor (exact).  Else xs is the unrounded float64 value of a fused launch's inner layer, known to `xerr`: the kernel
    rounds its own float32 value of it into the LDS tile, which may land one or more ulp16 away."""
    if seg.pre == "none" and xerr is None:
        return xs, np.zeros_like(xs)
    v, err = xs, (np.zeros_like(xs) if xerr is None else xerr)
    if coef is not None:
        A, Bc = (c.astype(np.float64)[:, None] for c in coef)
        v = xs * A + Bc
        err = np.abs(A) * err + 2 * U32 * (np.abs(xs * A) + np.abs(Bc))
    if seg.pre != "none":
        v = _lrelu64(v)                                      # (1-Lipschitz: err carries over)
        err = err + 2 * U32 * np.abs(v)
    if seg.kind in ("in1", "pointwise"):                     # float32 VALU layers: the operand is not rounded to 2 bytes
        return v, err
    return _round_known_to(v, err, fmt)


def _round_known_to(v: np.ndarray, err: np.ndarray, fmt: str):
    """r16 of a float32 value known only to `err` around the float64 v -> (r16(v), how far the kernel's r16 may lie from it)"""
    xh, ulp = round_storage(v, fmt)
    dist = 0.5 * ulp - np.abs(v - xh)                        # to the nearest rounding boundary
    with np.errstate(invalid="ignore", divide="ignore"):
        flips = np.where(err >= dist, np.floor((err - dist) / np.where(ulp > 0, ulp, 1.0)) + 1.0, 0.0)
    return xh, np.where(ulp > 0, flips * ulp, 2 * err)


_WCACHE: Dict[tuple, Dict[str, np.ndarray]] = {}


def _cached_weights(seg: Seg, weights, sig, fmt: str):
    key = (id(weights), seg.name, sig, fmt)
    if key not in _WCACHE:
        _WCACHE[key] = layer_weights(seg, weights, sig, fmt)
    return _WCACHE[key]


def gamma(seg: Seg, cin: int) -> float:
    """the float32 summation bound of a segment's accumulator, relative to sum |products| (module docstring)"""
    if seg.kind in ("direct", "poly"):
        units = (5 if seg.kind == "poly" else seg.K) * ((cin + 31) // 32)
        if seg.x2:
            units += 3 * ((cin + 31) // 32)                  # the second operand's products join the same accumulator
        return (8 * units + 8) * U32
    return (seg.K * cin + 4) * U32


def _value(seg: Seg, taps, weights, fmt: str, B: int, F: int, lens, with_spk: bool, sig, b: int):
    """-> (v, d, n_out): the float64 value of the layer's epilogue over the instance's own columns BEFORE it is rounded
    into storage, and how far the kernel's float32 value of it may lie from v"""
    n = _lens(B, F, lens)[b] * seg.rate
    L = _cached_weights(seg, weights, sig, fmt)
    if seg.first is not None:                                # fused launch: the inner layer's value never reached memory
        if seg.layout == "heads":
            parts = [_value(seg.first, taps, weights, fmt, B, F, lens, with_spk, s, b) for s in (0, 1)]
            xs, xerr = (np.concatenate([p[i] for p in parts], 0) for i in (0, 1))
        else:
            xs, xerr, _ = _value(seg.first, taps, weights, fmt, B, F, lens, with_spk, sig, b)
    else:
        xs, xerr = _row(seg, taps, seg.x, sig, b, B, False), None
        xs = O._squeeze(torch.from_numpy(xs), seg.dec).numpy()[:, :n] if seg.dec > 1 else xs[:, :n]
    coef = None
    if seg.pre == "norm" and with_spk:
        coef = norm_coefficients(taps[seg.st_in[0]][seg.st_in[1] * B + b], taps[f"up.{seg.block}.spk"][b], n)
    xh, dev = _operand_ref(seg, xs, fmt, coef, xerr)
    if seg.kind == "poly":
        xh, dev = (O._stretch(torch.from_numpy(a), seg.stretch).numpy() for a in (xh, dev))
    acc = _conv64(xh, L["w"], seg.dil)
    mag = _conv64(np.abs(xh), L["wabs"], seg.dil)
    d = _conv64(dev, L["wabs"], seg.dil) if dev.any() else np.zeros_like(acc)
    if seg.x2:                                               # d3x: the raw `a`, stretched, through the residual conv's taps
        s2 = seg.stretch2
        x2 = O._stretch(torch.from_numpy(_row(seg, taps, seg.x2, sig, b, B, False)[:, :n // s2]), s2).numpy()
        acc = acc + _conv64(x2, L["w2"], 1)
        mag = mag + _conv64(np.abs(x2), np.abs(L["w2"]), 1)
    bias = L["b"][:, None]
    d = d + gamma(seg, xh.shape[0]) * (mag + np.abs(bias))   # (the bias may start the accumulator: it is in every partial sum)
    v = acc + bias
    d = d + U32 * (np.abs(acc) + np.abs(bias))
    if seg.post_lrelu:
        v = _lrelu64(v)
        d = d + 2 * U32 * np.abs(v)
    no = n * seg.stretch
    if seg.res:
        r = _row(seg, taps, seg.res, sig, b, B, True)[:, :no]
        v = v + r
        d = d + U32 * (np.abs(v) + d)
    if seg.rank1:
        x1 = taps["sig"][sig * B + b][:, :no]
        r = L["r1w"][:, None] * x1 + L["r1b"][:, None]
        v = v + r
        d = d + 3 * U32 * (np.abs(L["r1w"][:, None] * x1) + np.abs(L["r1b"][:, None]) + np.abs(v))
    return v, d, no


def poly_staged(kernel: str) -> bool:
    """Whether a polyphase conv_hx instance runs its epilogue through the wave's LDS patch (csrc/fastsvc_hx.hip,
    hx_poly_staged: the patch of MW 16 rows of NW 16 S elements + 16 bytes fits 16 KB) - the finished tile is then rounded
    into the patch BEFORE the FiLM affine: y2 = r16(scale r16(v) + shift).  The reference models only this form: the GPU
    test asserts that every polyphase FiLM-affine launch it checks is such an instance.  Instance name: conv_hx<MW,NW,WM,WN,3,EPI,S,...>."""
    if not kernel.startswith("conv_hx<"):
        return False
    f = kernel[len("conv_hx<"):].split(",")
    mw, nw, s = int(f[0]), int(f[1]), int(f[6])
    return mw * 16 * (nw * 16 * s * 2 + 16) <= 16 * 1024


def reference(seg: Seg, taps, weights, fmt: str, B: int, F: int, lens, with_spk: bool, sig, b: int):
    """-> {tap: (ref, bound)} over the instance's own columns, and {'s1': (ref, bound), 's2': ...} for the sums"""
    n = _lens(B, F, lens)[b] * seg.rate
    if seg.kind == "convert":
        ref = taps[seg.x][b][:, :n]
        return {seg.y: (ref, 0.5 * round_storage(ref, fmt)[1])}, {}
    if seg.kind == "spk":
        w = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in weights.items() if k.startswith(seg.w[0])}
        e = taps[seg.x][b:b + 1]
        ref = O._speaker_bias(torch.from_numpy(e), w, seg.w[0].rsplit(".", 1)[0])[0, :, 0].numpy()
        en = np.abs(e[0]) / max(np.sqrt((e[0] ** 2).sum()), O.L2_EPS)
        mag = np.abs(np.asarray(weights[seg.w[0] + ".weight"], np.float64)) @ en + np.abs(np.asarray(weights[seg.w[0] + ".bias"], np.float64))
        E = e.shape[1]
        # float32: the norm (E + 2 operations), the division, an E-term dot product, the bias
        bound = 2 * (E + 4) * U32 * mag + 0.5 * ulp32(np.abs(ref) + 2 * (E + 4) * U32 * mag)
        return {seg.y: (ref[:, None], bound[:, None])}, {}
    v, d, no = _value(seg, taps, weights, fmt, B, F, lens, with_spk, sig, b)
    if seg.y_dec > 1:
        v, d = v[:, ::seg.y_dec], d[:, ::seg.y_dec]
    out, sums = {}, {}
    if seg.y:
        if seg.kind == "pointwise":
            out[seg.y] = (v, d + 0.5 * ulp32(np.abs(v) + d))
        else:
            out[seg.y] = (v, d + 0.5 * round_storage(np.abs(v) + d, fmt)[1])
    if seg.y2:
        ssr = taps[seg.ss][b]
        C = ssr.shape[0] // 2
        sc, sh = ssr[:C, :no], ssr[C:, :no]
        if seg.kind == "poly":                               # (see poly_staged: the affine reads the rounded tile)
            v, d = _round_known_to(v, d, fmt)
        u = sc * v + sh
        du = np.abs(sc) * d + 2 * U32 * (np.abs(sc * v) + np.abs(sh))
        out[seg.y2] = (u, du + 0.5 * round_storage(np.abs(u) + du, fmt)[1])
        if seg.st_out and with_spk:
            a1, a2 = np.abs(u).sum(1), (u * u).sum(1)
            sums["s1"] = (u.sum(1), du.sum(1) + TILE_COLS * U32 * a1 + 2.0 ** -50 * a1)
            sums["s2"] = (a2, (2 * np.abs(u) * du + du * du).sum(1) + (TILE_COLS + 2) * U32 * a2 + 2.0 ** -50 * a2)
    return out, sums


# ---------------------------------------------------------------------------------------------------------------
# the check
# ---------------------------------------------------------------------------------------------------------------
@dataclass
class Report:
    seg: str
    kernel: str
    checked: int = 0
    failed: int = 0
    within_one_ulp: int = 0          # elements whose bound is at most one ulp of the output type at the reference
    worst: float = 0.0               # largest deviation in units of the bound
    bound_ulps: float = 0.0          # median bound in ulps of the output type at the reference
    bound_of_max: float = 0.0        # largest bound as a fraction of the largest |reference| of its tap
    message: str = ""

    @property
    def share(self) -> float:
        return self.within_one_ulp / max(1, self.checked)


def expected_elements(seg: Seg, cfg, B: int, F: int, lens, with_spk: bool) -> int:
    """how many elements a check of `seg` must reach: every utterance's own columns of every output, and its sums"""
    shapes = tap_shapes(cfg, B, F)
    ln = _lens(B, F, lens)
    n = 0
    for tap in seg.outputs:
        shp = shapes[tap]
        if len(shp) == 2:
            n += shp[0] * shp[1]
        else:
            C = shp[1] // 2 if seg.layout == "film" else shp[1]
            rows = 2 * shp[0] if seg.layout == "film" else shp[0]
            n += sum(C * (shp[2] // F) * ln[r % B] for r in range(rows))
    if seg.st_out and with_spk:
        n += 2 * B * shapes[seg.st_out[0]][1]
    return n


def kernel_of(seg: Seg, records) -> str:
    names = {r["layer"]: r["kernel"] for r in (records or [])}
    for layer in seg.layers:
        if layer in names:
            return f"{layer}: {names[layer]}"
    return "?"


def check_segment(seg: Seg, taps, weights, fmt: str, B: int, F: int, lens, with_spk: bool, records=None) -> Report:
    """Every valid element of every output of `seg` against its float64 reference; `taps` hold float64 copies of the
    workspace tensors (full padded shapes), 'ppg', 'sig' (2B, 1, T: lft batch then sine batch), 'spk_emb' and 'wave'."""
    rep = Report(seg.name, kernel_of(seg, records))
    worst = None
    sizes, peaks = [], {}
    for sig, b in instances(seg, B):
        out, sums = reference(seg, taps, weights, fmt, B, F, lens, with_spk, sig, b)
        for tap, (ref, bound) in out.items():
            got = _row(seg, taps, tap, sig, b, B, True)
            got = got.reshape(ref.shape[0], -1)[:, :ref.shape[1]]
            dev = np.abs(got - ref)
            bad = ~(dev <= bound)                            # (a NaN fails)
            unit = ulp32(ref) if seg.kind in ("pointwise", "spk") else round_storage(ref, fmt)[1]
            rep.checked += dev.size
            rep.failed += int(bad.sum())
            rep.within_one_ulp += int((bound <= unit).sum())
            sizes.append((bound / np.where(unit > 0, unit, np.inf)).reshape(-1))
            peaks[tap] = (max(peaks.get(tap, (0.0, 0.0))[0], float(np.max(bound))), max(peaks.get(tap, (0.0, 0.0))[1], float(np.max(np.abs(ref)))))
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(bound > 0, dev / np.where(bound > 0, bound, 1.0), np.where(dev > 0, np.inf, 0.0))
            ratio = np.where(np.isnan(ratio), np.inf, ratio)
            c, t = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            if worst is None or ratio[c, t] > worst[0]:
                row = b if sig is None else sig * B + b
                worst = (float(ratio[c, t]), tap, row, int(c), int(t), float(got[c, t]), float(ref[c, t]), float(bound[c, t]))
        for j, key in enumerate(("s1", "s2")):
            if key not in sums:
                continue
            ref, bound = sums[key]
            got = taps[seg.st_out[0]][seg.st_out[1] * B + b][:, j]
            dev = np.abs(got - ref)
            bad = ~(dev <= bound)
            rep.checked += dev.size
            rep.failed += int(bad.sum())
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = dev / bound
            ratio = np.where(np.isnan(ratio), np.inf, ratio)
            c = int(np.argmax(ratio))
            if worst is None or ratio[c] > worst[0]:
                worst = (float(ratio[c]), f"{seg.st_out[0]}[{seg.st_out[1]}].{key}", b, c, -1, float(got[c]), float(ref[c]), float(bound[c]))
    if sizes:
        rep.bound_ulps = float(np.median(np.concatenate(sizes)))
        rep.bound_of_max = max(bd / mx for bd, mx in peaks.values() if mx > 0)
    if worst is not None:
        rep.worst = worst[0]
        r, tap, row, c, t, g, f, bd = worst
        rep.message = (f"segment {seg.name} [{rep.kernel}] {fmt}: {rep.failed} of {rep.checked} elements outside the bound; worst {tap} "
                       f"(row {row}, channel {c}, column {t}; column mod 128 = {t % 128 if t >= 0 else '-'}, mod 192 = {t % 192 if t >= 0 else '-'}): "
                       f"gpu {g!r} ref {f!r} bound {bd:.3e} = {r:.2f} bounds")
    return rep


# ---------------------------------------------------------------------------------------------------------------
# a float32 CPU model of the kernels (tests/test_layer_local.py: soundness of the bound, mutations)
# ---------------------------------------------------------------------------------------------------------------
def _r16_32(x: np.ndarray, fmt: str) -> np.ndarray:
    """float32 -> storage type -> float32, by torch's conversion (round to nearest even)"""
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(TORCH_DT[fmt]).to(torch.float32).numpy()


def _conv32(x: np.ndarray, w: np.ndarray, dil: int, order: int, no_pad_tail: Optional[np.ndarray] = None) -> np.ndarray:
    """float32 products and sums; 32-channel chunks, taps and the 4-channel steps inside a chunk visited in an order
    picked by `order` (0: ascending, 1: descending, 2: a fixed shuffle) - the accumulation order of a kernel is not the
    reference's business."""
    Co, Ci, K = w.shape
    T = x.shape[1]
    pad = (K // 2) * dil
    xp = np.zeros((Ci, T + 2 * pad), np.float32)
    xp[:, pad:pad + T] = x
    if no_pad_tail is not None and pad:
        xp[:, pad + T:] = no_pad_tail[:, None]
    units = [(c0, k) for c0 in range(0, Ci, 32) for k in range(K)]
    steps = list(range(0, 32, 4))
    if order == 1:
        units, steps = units[::-1], steps[::-1]
    elif order == 2:
        rng = np.random.default_rng(7)
        units = [units[i] for i in rng.permutation(len(units))]
        steps = [steps[i] for i in rng.permutation(8)]
    acc = np.zeros((Co, T), np.float32)
    w = w.astype(np.float32)
    for c0, k in units:                                    # one matrix instruction: 8 K-steps of 4 products
        for c4 in steps:
            c = c0 + c4
            if c < Ci:
                acc = acc + w[:, c:c + 4, k] @ xp[c:c + 4, k * dil:k * dil + T]
    return acc


def _lrelu32(v: np.ndarray, slope) -> np.ndarray:
    v = v.astype(np.float32)
    return np.maximum(v, (np.float32(slope) * v).astype(np.float32))


def _model_value(seg: Seg, taps, weights, fmt: str, B: int, F: int, lens, with_spk: bool, order, mut, sig, b: int):
    """-> (float32 value of the layer's epilogue before it is rounded into storage, its valid width)"""
    f32 = np.float32
    inner, align = None, seg.y_dec
    if isinstance(mut, tuple):                                # (mutation, the layer of the chain it is planted in, the segment's y_dec)
        align = mut[2]
        inner = mut if mut[1] != seg.name else None
        mut = mut[0] if mut[1] == seg.name else None
    n = _lens(B, F, lens)[b] * seg.rate
    L = _cached_weights(seg, weights, sig, fmt)
    w, bias = L["w"].astype(f32), L["b"].astype(f32).copy()
    if seg.kind == "poly":
        w0, ws, w2 = (a.astype(f32) for a in L["poly"])
    if seg.first is not None:                                 # fused launch: the inner layer stays in float32
        if seg.layout == "heads":
            xs = np.concatenate([_model_value(seg.first, taps, weights, fmt, B, F, lens, with_spk, order, inner, s, b)[0] for s in (0, 1)], 0)
        else:
            xs = _model_value(seg.first, taps, weights, fmt, B, F, lens, with_spk, order, inner, sig, b)[0]
    else:
        xs = _row(seg, taps, seg.x, sig, b, B, False)
        xs = xs[:, ::seg.dec][:, :n].astype(f32)
    pre_slope = f32(0.1) if (mut == "slope" and seg.pre != "none") else SLOPE32
    post_slope = f32(0.1) if (mut == "slope" and seg.pre == "none") else SLOPE32
    v = xs
    if seg.pre == "norm" and with_spk:
        n_norm = F * seg.rate if mut == "stats_width" else n
        A, Bc = norm_coefficients(taps[seg.st_in[0]][seg.st_in[1] * B + b], taps[f"up.{seg.block}.spk"][b], n_norm)
        v = (xs * A[:, None] + Bc[:, None]).astype(f32)
    if seg.pre != "none":
        v = _lrelu32(v, pre_slope)
    if (seg.pre != "none" or seg.first is not None) and seg.kind not in ("in1", "pointwise"):
        v = _r16_32(v, OTHER[fmt] if mut == "other_type" else fmt)
    xh = v
    if mut == "swap_w" and w.shape[1] >= 2:
        w = w.copy(); w[:, [0, 1]] = w[:, [1, 0]]
        if seg.kind == "poly":
            w0, ws, w2 = (a.copy() for a in (w0, ws, w2))
            for a in (w0, ws, w2):
                a[:, [0, 1]] = a[:, [1, 0]]
    if mut == "bias":
        bias[int(np.argsort(np.abs(bias))[len(bias) // 2])] = 0.0
    x2 = None
    if seg.x2:
        x2 = np.repeat(_row(seg, taps, seg.x2, sig, b, B, False)[:, :n // seg.stretch2].astype(f32), seg.stretch2, 1)
        if mut == "stretch_late":                             # the stretched operand read one input column late
            x2 = np.concatenate([x2[:, seg.stretch2:], np.zeros_like(x2[:, :seg.stretch2])], 1)

    def accumulate(xh, tail=None):
        if seg.kind == "poly":
            xm = xh
            if mut == "stretch_late":
                xm = np.concatenate([xh[:, 1:], np.zeros_like(xh[:, :1])], 1)
            prev = np.concatenate([np.zeros_like(xm[:, :1]), xm[:, :-1]], 1)
            nxt = np.concatenate([xm[:, 1:], np.zeros_like(xm[:, :1]) if tail is None else tail[:, None]], 1)
            one = lambda m, a: _conv32(a, m[:, :, None], 1, order)
            a0 = (one(w0, prev) + one(-w0, xm)).astype(f32)
            a2 = (one(w2, nxt) + one(-w2, xm)).astype(f32)
            zz = (one(ws, xm) + bias[:, None]).astype(f32)
            full = np.repeat(zz, seg.stretch, 1)
            full[:, ::seg.stretch] = (full[:, ::seg.stretch] + a0).astype(f32)
            full[:, seg.stretch - 1::seg.stretch] = (full[:, seg.stretch - 1::seg.stretch] + a2).astype(f32)
            return full
        acc = _conv32(xh, w, seg.dil, order, tail)
        if x2 is not None:
            acc = (acc + _conv32(x2, L["w2"].astype(f32), 1, order)).astype(f32)
        return (acc + bias[:, None]).astype(f32)

    vv = accumulate(xh)
    no = n * seg.stretch
    if mut == "no_pad" and seg.K == 3:
        vv[:, -1] = accumulate(xh, xh[:, -1])[:, -1]
    if mut == "tile_edge":
        c0 = 127 if no > 129 else no // 2
        c0 -= c0 % align                                      # (a column the decimated copy keeps)
        shifted = accumulate(np.concatenate([xh[:, 1:], np.zeros_like(xh[:, :1])], 1))
        vv[:, c0] = shifted[:, c0]
    if seg.post_lrelu:
        vv = _lrelu32(vv, post_slope)
    if seg.res:
        vv = (vv + _row(seg, taps, seg.res, sig, b, B, True)[:, :no].astype(f32)).astype(f32)
    if seg.rank1:
        x1 = taps["sig"][sig * B + b][:, :no].astype(f32)
        vv = (vv + (L["r1w"].astype(f32)[:, None] * x1 + L["r1b"].astype(f32)[:, None]).astype(f32)).astype(f32)
    return vv, no


def model_segment(seg: Seg, taps, weights, fmt: str, B: int, F: int, lens, with_spk: bool, order: int = 0, mut: Optional[str] = None):
    """Run one segment as the kernels do - float32 arithmetic, storage rounding at their points - on `taps` and write
    its outputs into `taps` (own columns only).  `mut`: one of MUTATIONS, applied to every instance it fits - in a fused
    launch to its last layer, or `(mutation, layer name, seg.y_dec)` to plant it in one layer of the chain (`chain_layers`)."""
    f32 = np.float32
    ln = _lens(B, F, lens)
    for sig, b in instances(seg, B):
        n = ln[b] * seg.rate
        if seg.kind == "convert":
            taps[seg.y][b][:, :n] = _r16_32(taps[seg.x][b][:, :n], fmt)
            continue
        if seg.kind == "spk":
            e = taps[seg.x][b].astype(f32)
            e = e / max(f32(np.sqrt((e * e).sum(dtype=f32))), f32(1e-12))
            taps[seg.y][b] = ((np.asarray(weights[seg.w[0] + ".weight"], f32) @ e) + np.asarray(weights[seg.w[0] + ".bias"], f32)).astype(f32)
            continue
        vv, no = _model_value(seg, taps, weights, fmt, B, F, lens, with_spk, order, mut, sig, b)
        if seg.y and seg.y_dec > 1:
            vd = _r16_32(vv, fmt)[:, ::seg.y_dec]
            _row(seg, taps, seg.y, sig, b, B, True)[:, :vd.shape[1]] = vd
        elif seg.y:
            _row(seg, taps, seg.y, sig, b, B, True)[:, :no] = vv if seg.kind == "pointwise" else _r16_32(vv, fmt)
        if seg.y2:
            ssr = taps[seg.ss][b]
            C = ssr.shape[0] // 2
            if seg.kind == "poly":                               # (the staged polyphase epilogue: see poly_staged)
                vv = _r16_32(vv, fmt)
            u = (ssr[:C, :no].astype(f32) * vv + ssr[C:, :no].astype(f32)).astype(f32)
            _row(seg, taps, seg.y2, sig, b, B, True)[:, :no] = _r16_32(u, fmt)
            if seg.st_out and with_spk:
                st = taps[seg.st_out[0]][seg.st_out[1] * B + b]
                parts = [u[:, t:t + 128] for t in range(0, no, 128)]
                st[:, 0] = sum(p.sum(1, dtype=f32).astype(np.float64) for p in parts)
                st[:, 1] = sum((p * p).sum(1, dtype=f32).astype(np.float64) for p in parts)


def empty_taps(cfg, B: int, F: int, ppg, sine, lft, spk_emb, fill=np.nan) -> Dict[str, np.ndarray]:
    """the tensors of the non-compact workspace as float64 arrays filled with `fill`, plus the inputs"""
    taps = {"ppg": np.asarray(ppg, np.float64), "sig": np.concatenate([np.asarray(lft, np.float64), np.asarray(sine, np.float64)], 0)}
    if spk_emb is not None:
        taps["spk_emb"] = np.asarray(spk_emb, np.float64)
    for name, shp in tap_shapes(cfg, B, F).items():
        taps[name] = np.full(shp, fill, np.float64)
    return taps


def tap_shapes(cfg, B: int, F: int) -> Dict[str, Tuple[int, ...]]:
    n = cfg.n_stages
    scales = list(cfg.upsampling_scales)
    mids = list(cfg.mid_channels)
    hop = int(np.prod(scales))
    down_scales = [1] + scales[::-1][:-1]
    out = {"ppg_act": (B, cfg.in_channels, F), "wave": (B, cfg.out_channels, F * hop)}
    T = F * hop
    for k in range(n):
        T //= down_scales[k]
        C = mids[n - 1 - k]
        for name in ("down_c1", "down_c2", "down_h") + (("down_r",) if k else ()):
            out[f"{name}.{k}"] = (2 * B, C, T)
        if k + 1 < n and k < 2 and n > 2:                      # the compact decimated copy the whole-stage launches write
            out[f"down_hd.{k + 1}"] = (2 * B, C, T // down_scales[k + 1])
        out[f"film_u.{k}"] = (B, 2 * C, T)
        out[f"ss.{k}"] = (B, 2 * C, T)
    T = F
    for i in range(n):
        C = mids[i]
        out[f"up.{i}.a"] = (B, C, T)
        T *= scales[i]
        for name in ("xr", "u1", "xmid", "u2", "u3", "out"):
            out[f"up.{i}.{name}"] = (B, C, T)
        out[f"up.{i}.spk"] = (B, C)
        out[f"up.{i}.stats"] = (3 * B, C, 2)
    return out
