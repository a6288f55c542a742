"""Training step of the FastSVC recipe around the HIP generator (BASELINE config 5).

What the reference's trainer runs per step (``harana/bin/train_fastsvc.py:157-240``, recipe
``egs/svcc23/fastsvc1/conf/fastsvc.yaml``):

    y_ = G(*x)                                   generator forward (this repo: HIP kernels)
    L_G = mean_r(SC_r + MAG_r)(y_, y)            multi-resolution STFT loss, 6 resolutions (stft_loss.py:21-180)
          [+ lambda_adv * mean_d MSE(D_d(y_), 1)  once the discriminator trains] (adversarial_loss.py:16-60)
    clip_grad_norm_(G, 10); RAdam step; StepLR step
    y_ = G(*x) under no_grad                     second forward ("re-compute y_ which leads better quality")
    L_D = mean_d MSE(D_d(y), 1) + mean_d MSE(D_d(y_), 0)      (adversarial_loss.py:63-127)
    clip_grad_norm_(D, 1); RAdam step; StepLR step

restated here from scratch: `MultiResolutionSTFTLoss`, `MelGANMultiScaleDiscriminator` (the yaml's discriminator,
``harana/models/fastsvc.py:386-640``; same module tree / state-dict keys so the reference's checkpoints load),
the two adversarial losses, `RAdam` (``harana/optimizers/radam.py:14-99``; one fused update per step through
``torch._foreach``), and `TrainStep` with a flat-bucket RCCL gradient all-reduce for data-parallel training (the
reference trains on ONE GPU; BASELINE config 5 asks for 8).

Honest scope: the generator FORWARD runs on the fused HIP path; its BACKWARD is an autograd graph over the restated
dataflow (``autograd.py``) whose heavy nodes are hand-written HIP kernels (``conv_grad.py``: convolution forward /
backward-data / backward-weight, FiLM + InstanceNorm + LeakyReLU, the all-layer weight-norm) and whose
remaining elementwise glue is PyTorch-ROCm; the multi-resolution STFT loss is HIP forward and backward
(``stft_loss.py``) on the GPU (the torch composition below serves the CPU tests); the discriminators, the adversarial
losses and RAdam are PyTorch-ROCm operators.  Discriminators restated here: the yaml's `MelGANMultiScaleDiscriminator`
and the HiFiGAN multi-period / multi-scale family BASELINE config 5 names (``fastsvc.py:631-1143``).  Everything is
pinned against the LIVE reference by ``tests/golden/train_step.npz``, ``train_recipe.npz`` and ``hifigan_disc.npz``
(``tests/golden/make_golden.py train | train_recipe | hifigan``).
"""
from __future__ import annotations

import contextlib

import math
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .gconv import ConvAct, GroupedConv1d

RECIPE = {
    # egs/svcc23/fastsvc1/conf/fastsvc.yaml
    "stft_loss_params": dict(fft_sizes=[2048, 1024, 512, 256, 128, 64], hop_sizes=[512, 256, 128, 64, 32, 16],
                             win_lengths=[2048, 1024, 512, 256, 128, 64], window="hann_window"),
    "discriminator_params": dict(in_channels=1, out_channels=1, scales=3, kernel_sizes=[5, 3], channels=16,
                                 max_downsample_channels=512, downsample_scales=[4, 4, 4], negative_slope=0.2,
                                 use_weight_norm=True),
    "lambda_adv": 2.5, "lambda_aux": 1.0,
    "batch_size": 32, "batch_length": 16000,
    "generator_optimizer_params": dict(lr=1e-3, eps=1e-6, weight_decay=0.0),
    "discriminator_optimizer_params": dict(lr=1e-3, eps=1e-6, weight_decay=0.0),
    "generator_scheduler_params": dict(step_size=100000, gamma=0.5),
    "discriminator_scheduler_params": dict(step_size=100000, gamma=0.5),
    "generator_grad_norm": 10.0, "discriminator_grad_norm": 1.0,
    "generator_train_start_steps": 0, "discriminator_train_start_steps": 100000,
}


# ------------------------------------------------------------------------------------------------------------
# multi-resolution STFT loss (stft_loss.py:21-180)
# ------------------------------------------------------------------------------------------------------------
def stft_magnitude(x: torch.Tensor, fft_size: int, hop: int, win_length: int, window: torch.Tensor) -> torch.Tensor:
    """(B, T) -> (B, frames, fft_size // 2 + 1): sqrt(clamp(re^2 + im^2, 1e-7)), centred reflect-padded frames."""
    spec = torch.stft(x, fft_size, hop, win_length, window, center=True, onesided=True, return_complex=True)
    power = spec.real * spec.real + spec.imag * spec.imag
    return torch.sqrt(torch.clamp(power, min=1e-7)).transpose(2, 1)


class MultiResolutionSTFTLoss(nn.Module):
    """``(sc, mag) = loss(y_hat, y)``: spectral convergence ``||Y - X||_F / ||Y||_F`` and log-magnitude L1, each averaged
    over the resolutions.  Same constructor surface and buffer names as the reference module."""

    def __init__(self, fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50), win_lengths=(600, 1200, 240),
                 window: str = "hann_window"):
        super().__init__()
        if not (len(fft_sizes) == len(hop_sizes) == len(win_lengths)):
            raise ValueError("fft_sizes, hop_sizes and win_lengths must have the same length")
        self.resolutions = [(int(f), int(h), int(w)) for f, h, w in zip(fft_sizes, hop_sizes, win_lengths)]
        self.stft_losses = nn.ModuleList()
        for _, _, w in self.resolutions:
            holder = nn.Module()
            holder.register_buffer("window", getattr(torch, window)(w))
            self.stft_losses.append(holder)

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if x.dim() == 3:
            x = x.reshape(-1, x.size(2))
            y = y.reshape(-1, y.size(2))
        sc_total = x.new_zeros(())
        mag_total = x.new_zeros(())
        for (nfft, hop, wl), holder in zip(self.resolutions, self.stft_losses):
            xm = stft_magnitude(x, nfft, hop, wl, holder.window)
            ym = stft_magnitude(y, nfft, hop, wl, holder.window)
            sc_total = sc_total + torch.linalg.norm(ym - xm) / torch.linalg.norm(ym)
            mag_total = mag_total + (torch.log(ym) - torch.log(xm)).abs().mean()
        n = len(self.resolutions)
        return sc_total / n, mag_total / n


# ------------------------------------------------------------------------------------------------------------
# MelGAN multi-scale discriminator (fastsvc.py:386-640) - module tree chosen so that state-dict keys match
# ------------------------------------------------------------------------------------------------------------
def _melgan_scale(in_channels: int, out_channels: int, kernel_sizes: Sequence[int], channels: int,
                  max_channels: int, downsample_scales: Sequence[int], slope: float) -> nn.ModuleList:
    k0, k1 = int(kernel_sizes[0]), int(kernel_sizes[1])
    if k0 % 2 == 0 or k1 % 2 == 0:
        raise ValueError("kernel sizes must be odd")
    first = k0 * k1
    layers = nn.ModuleList()
    layers.append(nn.Sequential(nn.ReflectionPad1d((first - 1) // 2), nn.Conv1d(in_channels, channels, first),
                                nn.LeakyReLU(slope)))
    c = channels
    for s in downsample_scales:
        c_out = min(c * s, max_channels)
        # (GroupedConv1d / ConvAct: nn.Conv1d + LeakyReLU under the reference's keys, one HIP launch forward and three backward
        # on the GPU for the recipe's shape - k = 41, stride 4, four input channels per group; gconv.py)
        layers.append(ConvAct(GroupedConv1d(c, c_out, kernel_size=10 * s + 1, stride=s, padding=5 * s, groups=c // 4),
                              nn.LeakyReLU(slope)))
        c = c_out
    c_out = min(c * 2, max_channels)
    layers.append(nn.Sequential(nn.Conv1d(c, c_out, k0, padding=(k0 - 1) // 2), nn.LeakyReLU(slope)))
    layers.append(nn.Conv1d(c_out, out_channels, k1, padding=(k1 - 1) // 2))
    return layers


class _Scale(nn.Module):
    def __init__(self, layers: nn.ModuleList):
        super().__init__()
        self.layers = layers

    def forward(self, x):
        outs = []
        for f in self.layers:
            x = f(x)
            outs.append(x)
        return outs


class MelGANMultiScaleDiscriminator(nn.Module):
    """``D(x)`` -> list (per scale) of lists (per layer) of feature maps; scale k sees the input average-pooled k
    times (kernel 4, stride 2, padding 1, count_include_pad=False).  Weight-norm on every conv, N(0, 0.02) init."""

    def __init__(self, in_channels=1, out_channels=1, scales=3, kernel_sizes=(5, 3), channels=16,
                 max_downsample_channels=1024, downsample_scales=(4, 4, 4, 4), negative_slope=0.2,
                 use_weight_norm=True, downsample_pooling_params=None, **_ignored):
        super().__init__()
        self.discriminators = nn.ModuleList(
            _Scale(_melgan_scale(in_channels, out_channels, kernel_sizes, channels, max_downsample_channels,
                                 downsample_scales, negative_slope)) for _ in range(scales))
        pp = dict(kernel_size=4, stride=2, padding=1, count_include_pad=False)
        pp.update(downsample_pooling_params or {})
        self.pooling = nn.AvgPool1d(**pp)
        if use_weight_norm:
            self.apply_weight_norm()
        for m in self.modules():
            if isinstance(m, nn.Conv1d):
                # (legacy weight_norm: `weight` is recomputed from g / v at every forward; the reference resets
                # `.weight.data` after applying weight-norm, which therefore changes nothing - kept for the folded case)
                if not hasattr(m, "weight_g"):
                    m.weight.data.normal_(0.0, 0.02)

    def apply_weight_norm(self):
        for m in self.modules():
            if isinstance(m, nn.Conv1d) and not hasattr(m, "weight_g"):
                nn.utils.weight_norm(m)

    def remove_weight_norm(self):
        for m in self.modules():
            if isinstance(m, nn.Conv1d) and hasattr(m, "weight_g"):
                nn.utils.remove_weight_norm(m)

    def forward(self, x):
        outs = []
        for d in self.discriminators:
            outs.append(d(x))
            x = self.pooling(x)
        return outs


# ------------------------------------------------------------------------------------------------------------
# HiFiGAN multi-period / multi-scale discriminators (fastsvc.py:631-1143): what BASELINE config 5 names.  Same module
# trees / state-dict keys as the reference classes, so its checkpoints load; `D(x)` -> list of final outputs, one per
# sub-discriminator (scales first, then periods), `return_fmaps=True` adds the flat list of hidden feature maps.
# ------------------------------------------------------------------------------------------------------------
def _activation(name: str, params: Optional[dict]) -> nn.Module:
    return getattr(nn, name)(**(params or {}))


class HiFiGANPeriodDiscriminator(nn.Module):
    """(B, C, T) is reflect-padded to a multiple of `period`, folded to (B, C, T / period, period) and run through
    Conv2d layers with (k, 1) kernels - every column of the fold is a 1-D signal of stride `period` (fastsvc.py:631-760).
    The output conv has kernel ``kernel_sizes[1] - 1`` with padding ``(kernel_sizes[1] - 1) // 2`` (so it is one row
    LONGER than its input for the default 3) - as the reference builds it."""

    def __init__(self, in_channels=1, out_channels=1, period=3, kernel_sizes=(5, 3), channels=32,
                 downsample_scales=(3, 3, 3, 3, 1), max_downsample_channels=1024, bias=True,
                 nonlinear_activation="LeakyReLU", nonlinear_activation_params=None, use_weight_norm=True,
                 use_spectral_norm=False):
        super().__init__()
        k0, k1 = int(kernel_sizes[0]), int(kernel_sizes[1])
        if len(kernel_sizes) != 2 or k0 % 2 == 0 or k1 % 2 == 0:
            raise ValueError("kernel_sizes must be two odd numbers")
        if use_weight_norm and use_spectral_norm:
            raise ValueError("Either use use_weight_norm or use_spectral_norm.")
        act = nonlinear_activation_params if nonlinear_activation_params is not None else {"negative_slope": 0.1}
        self.period = int(period)
        self.convs = nn.ModuleList()
        c_in, c_out = in_channels, channels
        for sc in downsample_scales:
            self.convs.append(nn.Sequential(nn.Conv2d(c_in, c_out, (k0, 1), (int(sc), 1), padding=((k0 - 1) // 2, 0)),
                                            _activation(nonlinear_activation, act)))
            c_in, c_out = c_out, min(c_out * 4, max_downsample_channels)
        # (c_out has already been advanced once more: the reference's output conv reads `out_chs`, not `in_chs` - equal
        # whenever the last hidden width sits at the cap, which the constructor requires of a loadable configuration)
        self.output_conv = nn.Conv2d(c_out, out_channels, (k1 - 1, 1), 1, padding=((k1 - 1) // 2, 0))
        # (the reference never hands `bias` to these Conv2d layers, fastsvc.py:631-700: they always have one - a
        # period_discriminator_params with bias=False must give the same module tree and state-dict keys as the reference's)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                if use_weight_norm:
                    nn.utils.weight_norm(m)
                elif use_spectral_norm:
                    nn.utils.spectral_norm(m)

    def forward(self, x, return_fmaps: bool = False):
        b, c, t = x.shape
        if t % self.period:
            pad = self.period - t % self.period
            x = F.pad(x, (0, pad), "reflect")
            t += pad
        x = x.view(b, c, t // self.period, self.period)
        fmaps = []
        for f in self.convs:
            x = f(x)
            fmaps.append(x)
        out = torch.flatten(self.output_conv(x), 1, -1)
        return (out, fmaps) if return_fmaps else out


class HiFiGANMultiPeriodDiscriminator(nn.Module):
    def __init__(self, periods=(2, 3, 5, 7, 11), discriminator_params=None):
        super().__init__()
        params = dict(discriminator_params or {})
        params.pop("period", None)
        self.discriminators = nn.ModuleList(HiFiGANPeriodDiscriminator(period=int(p), **params) for p in periods)

    def forward(self, x, return_fmaps: bool = False):
        outs, fmaps = [], []
        for d in self.discriminators:
            if return_fmaps:
                o, fm = d(x, True)
                fmaps.extend(fm)
            else:
                o = d(x)
            outs.append(o)
        return (outs, fmaps) if return_fmaps else outs


class HiFiGANScaleDiscriminator(nn.Module):
    """Conv1d stack: k = 15 input conv, grouped strided k = 41 convs (groups 4, 16, ... <= max_groups; channels doubling up
    to the cap), a k = 5 conv and the k = 3 output conv (fastsvc.py:835-975).

    Reference quirk kept on purpose (SURVEY.md §8 e): its `apply_weight_norm` / `apply_spectral_norm` test
    ``isinstance(m, nn.Conv2d)`` on this Conv1d-only stack (fastsvc.py:957-975), so NEITHER norm is ever applied and the
    state dict holds plain `weight` / `bias` - whatever `use_weight_norm`, `use_spectral_norm` or the multi-scale
    wrapper's `follow_official_norm` say.  `reference_norm_quirk=False` applies the norm the flags ask for instead."""

    def __init__(self, in_channels=1, out_channels=1, kernel_sizes=(15, 41, 5, 3), channels=128,
                 max_downsample_channels=1024, max_groups=16, bias=True, downsample_scales=(2, 2, 4, 4, 1),
                 nonlinear_activation="LeakyReLU", nonlinear_activation_params=None, use_weight_norm=True,
                 use_spectral_norm=False, reference_norm_quirk: bool = True):
        super().__init__()
        ks = [int(k) for k in kernel_sizes]
        if len(ks) != 4 or any(k % 2 == 0 for k in ks):
            raise ValueError("kernel_sizes must be four odd numbers")
        if use_weight_norm and use_spectral_norm:
            raise ValueError("Either use use_weight_norm or use_spectral_norm.")
        act = nonlinear_activation_params if nonlinear_activation_params is not None else {"negative_slope": 0.1}
        self.layers = nn.ModuleList()
        self.layers.append(nn.Sequential(nn.Conv1d(in_channels, channels, ks[0], bias=bias, padding=(ks[0] - 1) // 2),
                                         _activation(nonlinear_activation, act)))
        c_in, c_out, groups = channels, channels, 4
        for sc in downsample_scales:
            self.layers.append(nn.Sequential(nn.Conv1d(c_in, c_out, kernel_size=ks[1], stride=int(sc), padding=(ks[1] - 1) // 2,
                                                       groups=groups, bias=bias), _activation(nonlinear_activation, act)))
            c_in = c_out
            c_out = min(c_in * 2, max_downsample_channels)
            groups = min(groups * 4, max_groups)
        c_out = min(c_in * 2, max_downsample_channels)
        self.layers.append(nn.Sequential(nn.Conv1d(c_in, c_out, kernel_size=ks[2], stride=1, padding=(ks[2] - 1) // 2, bias=bias),
                                         _activation(nonlinear_activation, act)))
        self.last_layer = nn.Conv1d(c_out, out_channels, kernel_size=ks[3], stride=1, padding=(ks[3] - 1) // 2, bias=bias)
        if not reference_norm_quirk:
            for m in self.modules():
                if isinstance(m, nn.Conv1d):
                    if use_weight_norm:
                        nn.utils.weight_norm(m)
                    elif use_spectral_norm:
                        nn.utils.spectral_norm(m)

    def forward(self, x, return_fmaps: bool = False):
        fmaps = []
        for f in self.layers:
            x = f(x)
            fmaps.append(x)
        out = self.last_layer(x)
        return (out, fmaps) if return_fmaps else out


class HiFiGANMultiScaleDiscriminator(nn.Module):
    """Scale k sees the input pooled k times (AvgPool1d kernel 4, stride 2, padding 2: torch's default count_include_pad)."""

    def __init__(self, scales=3, downsample_pooling="AvgPool1d", downsample_pooling_params=None, discriminator_params=None,
                 follow_official_norm=False, reference_norm_quirk: bool = True):
        super().__init__()
        self.discriminators = nn.ModuleList()
        for i in range(int(scales)):
            params = dict(discriminator_params or {})
            if follow_official_norm:
                params["use_weight_norm"], params["use_spectral_norm"] = (i != 0), (i == 0)
            self.discriminators.append(HiFiGANScaleDiscriminator(reference_norm_quirk=reference_norm_quirk, **params))
        pp = downsample_pooling_params if downsample_pooling_params is not None else dict(kernel_size=4, stride=2, padding=2)
        self.pooling = getattr(nn, downsample_pooling)(**pp)

    def forward(self, x, return_fmaps: bool = False):
        outs, fmaps = [], []
        for d in self.discriminators:
            if return_fmaps:
                o, fm = d(x, True)
                fmaps.extend(fm)
            else:
                o = d(x)
            outs.append(o)
            x = self.pooling(x)
        return (outs, fmaps) if return_fmaps else outs


class HiFiGANMultiScaleMultiPeriodDiscriminator(nn.Module):
    """`msd` + `mpd` (fastsvc.py:1056-1143): outputs of the scales, then of the periods."""

    def __init__(self, scales=3, scale_downsample_pooling="AvgPool1d", scale_downsample_pooling_params=None,
                 scale_discriminator_params=None, follow_official_norm=True, periods=(2, 3, 5, 7, 11),
                 period_discriminator_params=None, reference_norm_quirk: bool = True):
        super().__init__()
        self.msd = HiFiGANMultiScaleDiscriminator(scales=scales, downsample_pooling=scale_downsample_pooling,
                                                  downsample_pooling_params=scale_downsample_pooling_params,
                                                  discriminator_params=scale_discriminator_params,
                                                  follow_official_norm=follow_official_norm,
                                                  reference_norm_quirk=reference_norm_quirk)
        self.mpd = HiFiGANMultiPeriodDiscriminator(periods=periods, discriminator_params=period_discriminator_params)

    def forward(self, x, return_fmaps: bool = False):
        if return_fmaps:
            so, sf = self.msd(x, True)
            po, pf = self.mpd(x, True)
            return so + po, sf + pf
        return self.msd(x) + self.mpd(x)


def discriminator_is_per_sample_stateless(d: nn.Module) -> bool:
    """True when `D(cat([a, b]))` equals `cat([D(a), D(b)])` and a forward mutates nothing: no BatchNorm (cross-sample
    statistics) and no spectral norm (a power iteration per training forward) anywhere in the module."""
    for m in d.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            return False
        for hook in getattr(m, "_forward_pre_hooks", {}).values():
            if type(hook).__name__ == "SpectralNorm":
                return False
        if hasattr(m, "parametrizations"):
            for plist in m.parametrizations.values():
                if any(type(q).__name__ == "_SpectralNorm" for q in plist):
                    return False
    return True


# ------------------------------------------------------------------------------------------------------------
# adversarial losses, MSE flavour (adversarial_loss.py:16-127); `outs`: list per discriminator of per-layer lists
# ------------------------------------------------------------------------------------------------------------
def _final(outs):
    return [o[-1] if isinstance(o, (list, tuple)) else o for o in outs] if isinstance(outs, (list, tuple)) else [outs]


def generator_adversarial_loss(outs_hat) -> torch.Tensor:
    finals = _final(outs_hat)
    return sum(((o - 1.0) ** 2).mean() for o in finals) / len(finals)


def discriminator_adversarial_loss(outs_hat, outs) -> Tuple[torch.Tensor, torch.Tensor]:
    fh, fr = _final(outs_hat), _final(outs)
    real = sum(((o - 1.0) ** 2).mean() for o in fr) / len(fr)
    fake = sum((o ** 2).mean() for o in fh) / len(fh)
    return real, fake


# ------------------------------------------------------------------------------------------------------------
# RAdam (radam.py:14-99): rectified Adam; the variance rectification depends on the step count only
# ------------------------------------------------------------------------------------------------------------
class RAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @staticmethod
    def rectified_step_size(t: int, beta1: float, beta2: float) -> Tuple[float, bool]:
        """(step size without lr, whether the adaptive denominator is used) at step t >= 1."""
        b2t = beta2 ** t
        n_max = 2.0 / (1.0 - beta2) - 1.0
        n_t = n_max - 2.0 * t * b2t / (1.0 - b2t)
        if n_t >= 5.0:
            r = math.sqrt((1.0 - b2t) * (n_t - 4.0) / (n_max - 4.0) * (n_t - 2.0) / n_t * n_max / (n_max - 2.0))
            return r / (1.0 - beta1 ** t), True
        return 1.0 / (1.0 - beta1 ** t), False

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            by_step: Dict[int, Tuple[list, list, list, list]] = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("RAdam does not support sparse gradients")
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, dtype=torch.float32)
                    st["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32)
                st["step"] += 1
                ps, gs, ms, vs = by_step.setdefault(st["step"], ([], [], [], []))
                ps.append(p); gs.append(p.grad.float()); ms.append(st["exp_avg"]); vs.append(st["exp_avg_sq"])
            for t, (ps, gs, ms, vs) in by_step.items():
                torch._foreach_mul_(vs, beta2)
                torch._foreach_addcmul_(vs, gs, gs, value=1.0 - beta2)
                torch._foreach_mul_(ms, beta1)
                torch._foreach_add_(ms, gs, alpha=1.0 - beta1)
                size, adaptive = self.rectified_step_size(t, beta1, beta2)
                if group["weight_decay"] != 0:
                    torch._foreach_mul_(ps, 1.0 - group["weight_decay"] * group["lr"])
                if adaptive:
                    denom = torch._foreach_sqrt(vs)
                    torch._foreach_add_(denom, group["eps"])
                    torch._foreach_addcdiv_(ps, ms, denom, value=-size * group["lr"])
                else:
                    torch._foreach_add_(ps, ms, alpha=-size * group["lr"])
        return loss


# ------------------------------------------------------------------------------------------------------------
# data-parallel gradient exchange: flat buckets, one all-reduce each (RCCL when the tensors are on a GPU)
# ------------------------------------------------------------------------------------------------------------
def all_reduce_gradients(params: Iterable[torch.nn.Parameter], group=None, bucket_bytes: int = 64 << 20) -> int:
    """Average `.grad` over the ranks of `group`.  Gradients are packed into flat float32 buckets of at most
    `bucket_bytes` (generator 11 MB, yaml discriminator 17 MB: one bucket each) so that the ring is per-link bound
    on few large messages, not on hundreds of small ones.  Returns the number of collectives issued."""
    import torch.distributed as dist
    if not dist.is_available() or not dist.is_initialized() or dist.get_world_size(group) == 1:
        return 0
    world = dist.get_world_size(group)
    grads = [p.grad for p in params if p.grad is not None]
    buckets: List[List[torch.Tensor]] = [[]]
    size = 0
    for g in grads:
        nbytes = g.numel() * 4
        if buckets[-1] and size + nbytes > bucket_bytes:
            buckets.append([])
            size = 0
        buckets[-1].append(g)
        size += nbytes
    n = 0
    for b in buckets:
        if not b:
            continue
        flat = torch.cat([g.reshape(-1).float() for g in b])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        flat.div_(world)
        off = 0
        for g in b:
            g.copy_(flat[off: off + g.numel()].view_as(g))
            off += g.numel()
        n += 1
    return n


class TrainStep:
    """One optimisation step of generator and discriminator, the reference trainer's `_train_step`
    (train_fastsvc.py:157-240) with an optional data-parallel gradient all-reduce in front of each clip."""

    def __init__(self, generator: nn.Module, discriminator: nn.Module, config: Optional[dict] = None,
                 group=None, steps: int = 0):
        cfg = dict(RECIPE)
        cfg.update(config or {})
        self.config = cfg
        self.generator, self.discriminator = generator, discriminator
        self.group = group
        self.steps = int(steps)
        dev = next(generator.parameters()).device
        # on the GPU the criterion is the HIP one (stft_loss.py: forward and backward kernels, csrc/fastsvc_stftloss.hip);
        # the torch composition below serves the CPU host-logic / gloo tests and `stft_loss_impl: "torch"` A/B runs
        impl = cfg.get("stft_loss_impl", "hip" if dev.type == "cuda" else "torch")
        if impl == "hip":
            from .stft_loss import MultiResolutionSTFTLoss as HipMultiResolutionSTFTLoss
            self.stft = HipMultiResolutionSTFTLoss(**cfg["stft_loss_params"]).to(dev)
        else:
            self.stft = MultiResolutionSTFTLoss(**cfg["stft_loss_params"]).to(dev)
        self.opt_g = RAdam(generator.parameters(), **cfg["generator_optimizer_params"])
        self.opt_d = RAdam(discriminator.parameters(), **cfg["discriminator_optimizer_params"])
        self.sched_g = torch.optim.lr_scheduler.StepLR(self.opt_g, **cfg["generator_scheduler_params"])
        self.sched_d = torch.optim.lr_scheduler.StepLR(self.opt_d, **cfg["discriminator_scheduler_params"])
        # BASELINE config 5's dtype: `autocast_dtype: "bfloat16"` runs the forward computations of the step - generator
        # (HIP forward in bfloat16 activation storage when the module says so; its PyTorch backward re-evaluates the
        # dataflow under the same autocast, see autograd.py), discriminator, adversarial losses - under
        # torch.autocast; master weights, optimizer state, InstanceNorm statistics and the STFT loss stay float32
        # (the reference has no AMP: train_fastsvc.py:157-240 - this is what "bf16 train step" can mean for it).
        # The DISCRIMINATOR stays float32 unless `autocast_discriminator: True`: on this ROCm (7.0 / MIOpen of torch 2.10)
        # the bf16 backward-data of the MelGAN discriminator's first conv (1 -> 16 channels, k = 15:
        # `MIOpenDriver convbfp16 -n 32 -c 1 -W 4014 -k 16 -x 15 -F 2`) intermittently dies with a GPU memory access
        # fault, depending on which solver MIOpen's find step picked (caught with MIOPEN_ENABLE_LOGGING_CMD=1)
        ac = cfg.get("autocast_dtype")
        self.autocast_dtype = getattr(torch, ac) if isinstance(ac, str) else ac
        # fake + real through the discriminator as ONE batch, and its parameters frozen for the generator's adversarial term:
        # only for discriminators whose forward is stateless per sample (weight-norm convolutions, LeakyReLU, pooling - the
        # MelGAN and HiFiGAN families as the reference builds them); a BatchNorm or spectral-norm discriminator gets the
        # reference's two calls in its order (train_fastsvc.py:207-211)
        self._stateless_d = discriminator_is_per_sample_stateless(discriminator)
        # the optimizer invalidates the generator's packed weights every step: re-pack them on the GPU (HIP kernels, the
        # host packer's bytes - so no loss or parameter changes with this key) instead of download, host pack, upload
        if dev.type == "cuda" and hasattr(type(generator), "pack_on_device"):
            generator.pack_on_device = bool(cfg.get("pack_on_device", True))

    def _autocast(self, discriminator: bool = False):
        dev = next(self.generator.parameters()).device
        if self.autocast_dtype is None or dev.type != "cuda" or (discriminator and not self.config.get("autocast_discriminator", False)):
            return contextlib.nullcontext()
        return torch.autocast(device_type="cuda", dtype=self.autocast_dtype)

    def step(self, batch, log: bool = True) -> Dict[str, float]:
        """batch = ((ppg, sine, lft[, spk_emb]), y) - the Collater's layout (train_fastsvc.py:537-551).
        `log=False` skips the host read-back of the loss values (each one synchronises the stream)."""
        x, y = batch
        cfg = self.config
        logd: Dict[str, torch.Tensor] = {}
        train_d = self.steps > cfg["discriminator_train_start_steps"]
        if self.steps > cfg.get("generator_train_start_steps", 0):
            with self._autocast():
                y_ = self.generator(*x)
            sc, mag = self.stft(y_.float(), y.float())
            gen_loss = (sc + mag) * cfg.get("lambda_aux", 1.0)
            logd["spectral_convergence_loss"], logd["log_stft_magnitude_loss"] = sc.detach(), mag.detach()
            if train_d:
                # the generator's adversarial term needs d loss / d y_ only: the reference's backward also fills the
                # DISCRIMINATOR's parameter gradients here and zeroes them before they are used (train_fastsvc.py:183,
                # 224: optimizer["discriminator"].zero_grad() precedes dis_loss.backward()) - a third of the discriminator's
                # backward work (its weight gradients) and as many launches; frozen for this one call, same updates
                # (HIP-graph replay of the discriminator's own update, torch.cuda.make_graphed_callables, was measured
                # too: 53.6 ms against 52.0 ms launch by launch - not kept)
                d_params = [p for p in self.discriminator.parameters() if p.requires_grad] if self._stateless_d else []
                for p in d_params:
                    p.requires_grad_(False)
                try:
                    with self._autocast(discriminator=True):
                        adv = generator_adversarial_loss(self.discriminator(y_))
                finally:
                    for p in d_params:
                        p.requires_grad_(True)
                logd["adversarial_loss"] = adv.detach()
                gen_loss = gen_loss + cfg["lambda_adv"] * adv.float()
            logd["generator_loss"] = gen_loss.detach()
            self.opt_g.zero_grad()
            gen_loss.backward()
            all_reduce_gradients(self.generator.parameters(), self.group)
            if cfg["generator_grad_norm"] > 0:
                torch.nn.utils.clip_grad_norm_(self.generator.parameters(), cfg["generator_grad_norm"])
            self.opt_g.step()
            self.sched_g.step()
            if train_d and hasattr(self.generator, "prefetch_packed_weights"):
                self.generator.prefetch_packed_weights()     # parameters -> host while the GPU runs the real batch below
        if train_d:
            if cfg.get("batch_discriminator_inputs", True) and self._stateless_d:
                # fake and real batch through the discriminator as ONE batch of 2B: it has no cross-sample operator (weight-norm
                # convolutions, LeakyReLU, average pooling), so the outputs are those of two calls - and the step, which is bound
                # by the host's launch path once the generator's kernels are hand-written, issues half as many discriminator
                # launches (MIOpen's convolution_backward costs the host 0.2 ms a call)
                with torch.no_grad():
                    y_ = self.generator(*x)              # second forward, with the updated generator
                nb = y.shape[0]
                with self._autocast(discriminator=True):
                    finals = _final(self.discriminator(torch.cat([y_.detach(), y], dim=0)))
                    real, fake = discriminator_adversarial_loss([o[:nb] for o in finals], [o[nb:] for o in finals])
            elif self._stateless_d:
                # (the real batch first: it does not depend on the generator, and the host re-packs the updated generator
                # weights while the GPU is busy with it - same losses as `D(y_), D(y)` in the reference's order)
                with self._autocast(discriminator=True):
                    p_real = self.discriminator(y)
                with torch.no_grad():
                    y_ = self.generator(*x)              # second forward, with the updated generator
                with self._autocast(discriminator=True):
                    real, fake = discriminator_adversarial_loss(self.discriminator(y_.detach()), p_real)
            else:
                # a discriminator with state (spectral norm's power iteration, BatchNorm): the reference's calls, in its order
                with torch.no_grad():
                    y_ = self.generator(*x)
                with self._autocast(discriminator=True):
                    p_real = self.discriminator(y)
                    real, fake = discriminator_adversarial_loss(self.discriminator(y_.detach()), p_real)
            dis_loss = real.float() + fake.float()
            logd["real_loss"], logd["fake_loss"], logd["discriminator_loss"] = real.detach(), fake.detach(), dis_loss.detach()
            self.opt_d.zero_grad()
            dis_loss.backward()
            all_reduce_gradients(self.discriminator.parameters(), self.group)
            if cfg["discriminator_grad_norm"] > 0:
                torch.nn.utils.clip_grad_norm_(self.discriminator.parameters(), cfg["discriminator_grad_norm"])
            self.opt_d.step()
            self.sched_d.step()
        self.steps += 1
        return {k: float(v) for k, v in logd.items()} if log else {}

    @torch.no_grad()
    def eval_step(self, batch) -> Dict[str, float]:
        """The reference trainer's `_eval_step` (train_fastsvc.py:266-311) on one batch of the `step` layout: both modules in
        `.eval()` for the call (their previous modes are restored), no gradient, and - as in the reference - every term
        whatever `discriminator_train_start_steps` says: `y_ = G(*x)`, the STFT loss, `adv = gen_adv(D(y_))`,
        `gen = lambda_aux * (sc + mag) + lambda_adv * adv`, `real, fake = dis_adv(D(y_), D(y))`.  Returns the seven values
        under `step`'s key names (the reference logs them as `eval/<name>`).  Parameters, gradients, optimizer and
        scheduler state and `steps` are left as they are."""
        x, y = batch
        cfg = self.config
        modes = [(m, m.training) for m in (self.generator, self.discriminator)]
        try:
            for m, _ in modes:
                m.eval()
            with self._autocast():
                y_ = self.generator(*x)
            sc, mag = self.stft(y_.float(), y.float())
            with self._autocast(discriminator=True):
                p_ = self.discriminator(y_)
                adv = generator_adversarial_loss(p_)
                real, fake = discriminator_adversarial_loss(p_, self.discriminator(y))
            gen = (sc + mag) * cfg.get("lambda_aux", 1.0) + cfg["lambda_adv"] * adv.float()
            logd = {"spectral_convergence_loss": sc, "log_stft_magnitude_loss": mag, "adversarial_loss": adv,
                    "generator_loss": gen, "real_loss": real, "fake_loss": fake, "discriminator_loss": real.float() + fake.float()}
            return {k: float(v) for k, v in logd.items()}
        finally:
            for m, was_training in modes:
                m.train(was_training)
