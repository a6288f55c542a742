"""``f0_extract`` - F0 by YIN (de Cheveigne & Kawahara 2002) on the frames ``loudness_extract`` uses, computed by a HIP
kernel (``csrc/fastsvc_f0.hip``: one workgroup per frame, the 2048 samples in LDS, the difference function computed
directly in float32).  The recipe's F0 is ``pyworld.harvest``'s, a whole-file CPU algorithm; this is a per-frame definition
 that ``StreamSession(f0="audio")`` computes frame by frame with the same bits.  GPU tensors only."""
from __future__ import annotations

import ctypes

import torch

from .engine import FastSVCError, _check, f0_lags, load_library


@torch.no_grad()
def f0_extract(audio: torch.Tensor, sample_rate: int, hop: int, f0_floor: float = 70.0, f0_ceil: float = 340.0,
               threshold: float = 0.15) -> torch.Tensor:
    """audio (T,) or (B, T) float on the GPU -> (frames,) or (B, frames) float32, frames = 1 + T // hop
    (``loudness_extract``'s frames: frame f is the 2048 samples centred on ``f hop``, reflection at both ends), one F0 in
    Hz per frame and 0 where the frame is unvoiced.  ``f0_floor`` and ``f0_ceil`` bound the search (lags ``f0_lags``;
    ``ValueError`` when ``ceil(sample_rate / f0_floor) > 1024``), ``threshold`` is YIN's on the normalised difference.
    Every row of a batch is one utterance; a frame's value depends on its own 2048 samples alone."""
    if not isinstance(audio, torch.Tensor) or not audio.is_cuda:
        raise FastSVCError("f0_extract (HIP) needs a GPU tensor; there is no CPU fallback")
    single = audio.dim() == 1
    a = (audio[None] if single else audio).to(torch.float32).contiguous()
    if a.dim() != 2 or a.shape[1] < 2:
        raise ValueError(f"audio must be (T,) or (B, T) with T >= 2, got {tuple(audio.shape)}")
    hop = int(hop)
    if hop < 1 or not float(threshold) > 0.0:
        raise ValueError(f"f0_extract needs hop >= 1 and threshold > 0, got {hop} and {threshold}")
    f0_lags(sample_rate, f0_floor, f0_ceil)
    lib = load_library()
    B, T = a.shape
    frames = int(lib.fastsvc_loudness_frames(T, hop))
    out = torch.empty((B, frames), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _check(lib, lib.fastsvc_f0_extract(ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, T, hop,
                                           ctypes.c_float(float(sample_rate)), ctypes.c_float(float(f0_floor)),
                                           ctypes.c_float(float(f0_ceil)), ctypes.c_float(float(threshold)),
                                           ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)), "fastsvc_f0_extract")
    return out[0] if single else out
