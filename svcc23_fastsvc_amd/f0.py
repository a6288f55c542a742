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
               threshold: float = 0.15, track=None) -> torch.Tensor:
    """audio (T,) or (B, T) float on the GPU -> (frames,) or (B, frames) float32, frames = 1 + T // hop
    (``loudness_extract``'s frames: frame f is the 2048 samples centred on ``f hop``, reflection at both ends), one F0 in
    Hz per frame and 0 where the frame is unvoiced.  ``f0_floor`` and ``f0_ceil`` bound the search (lags ``f0_lags``;
    ``ValueError`` when ``ceil(sample_rate / f0_floor) > 1024``), ``threshold`` is YIN's on the normalised difference.
    Every row of a batch is one utterance; a frame's value depends on its own 2048 samples alone.

    ``track=decode.F0Track(...)``: the fixed-lag Viterbi track over the frames' candidates (``f0_candidates``) in
    place of the per-frame pick - two launches (csrc/fastsvc_f0.hip: candidates, one workgroup per frame; the tracker, one
    per row), the value of frame f a function of the frames ``<= f + track.lag``; ``track.unvoiced=None`` takes ``threshold``
    as the unvoiced state's cost.  ``None`` (the default): the launch and the bits as before."""
    if track is not None:
        from .decode import F0Track
        if not isinstance(track, F0Track):
            raise ValueError(f"track must be None or a decode.F0Track, got {track!r}")
        if not float(threshold) > 0.0:
            raise ValueError(f"f0_extract needs threshold > 0, got {threshold}")
        cands = f0_candidates(audio, sample_rate, hop, f0_floor, f0_ceil, track.cand_threshold)
        return f0_track(cands, f0_lags(sample_rate, f0_floor, f0_ceil)[1], sample_rate, track,
                        float(threshold) if track.unvoiced is None else track.unvoiced)
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


@torch.no_grad()
def f0_candidates(audio: torch.Tensor, sample_rate: int, hop: int, f0_floor: float = 70.0, f0_ceil: float = 340.0,
                  cand_threshold: float = 0.5) -> torch.Tensor:
    """audio (T,) or (B, T) float on the GPU -> (frames, 4, 2) or (B, frames, 4, 2) float32: per frame of ``f0_extract`` up to
    four candidates ``(tau_hat, s)`` of the tracker (``decode.F0Track``) - the local minima of YIN's d' under
    ``cand_threshold`` in ``[max(tau_min, 2), tau_max]``, the four with the smallest d' (ties: the smaller lag) in ascending
    lag, each with the pick's parabola as ``tau_hat`` and ``s = d'``; absent entries are ``(0, inf)``.  One HIP launch
    (fastsvc_f0_candidates).  GPU tensors only."""
    if not isinstance(audio, torch.Tensor) or not audio.is_cuda:
        raise FastSVCError("f0_candidates (HIP) needs a GPU tensor; there is no CPU fallback")
    single = audio.dim() == 1
    a = (audio[None] if single else audio).to(torch.float32).contiguous()
    if a.dim() != 2 or a.shape[1] < 2:
        raise ValueError(f"audio must be (T,) or (B, T) with T >= 2, got {tuple(audio.shape)}")
    hop = int(hop)
    if hop < 1 or not float(cand_threshold) > 0.0:
        raise ValueError(f"f0_candidates needs hop >= 1 and cand_threshold > 0, got {hop} and {cand_threshold}")
    f0_lags(sample_rate, f0_floor, f0_ceil)
    lib = load_library()
    B, T = a.shape
    frames = int(lib.fastsvc_loudness_frames(T, hop))
    out = torch.empty((B, frames, 4, 2), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _check(lib, lib.fastsvc_f0_candidates(ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, T, hop,
                                              ctypes.c_float(float(sample_rate)), ctypes.c_float(float(f0_floor)),
                                              ctypes.c_float(float(f0_ceil)), ctypes.c_float(float(cand_threshold)),
                                              ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)),
               "fastsvc_f0_candidates")
    return out[0] if single else out


@torch.no_grad()
def f0_track(cands: torch.Tensor, tau_max: int, sample_rate: float, track, unvoiced: float) -> torch.Tensor:
    """``decode.f0_track_rule`` on the device: cands (frames, 4, 2) or (B, frames, 4, 2) float32 on the GPU -> (frames,) or (B,
    frames) float32, the tracked F0 of every row (fastsvc_f0_track: one workgroup per row, one lane runs the recurrence, all
    lanes trace back).  ``track``: a ``decode.F0Track``; ``unvoiced``: the unvoiced state's cost."""
    if not isinstance(cands, torch.Tensor) or not cands.is_cuda:
        raise FastSVCError("f0_track (HIP) needs a GPU tensor; there is no CPU fallback")
    single = cands.dim() == 3
    c = (cands[None] if single else cands).to(torch.float32).contiguous()
    if c.dim() != 4 or tuple(c.shape[2:]) != (4, 2) or c.shape[1] < 1:
        raise ValueError(f"cands must be (frames, 4, 2) or (B, frames, 4, 2) with frames >= 1, got {tuple(cands.shape)}")
    lib = load_library()
    B, frames = int(c.shape[0]), int(c.shape[1])
    out = torch.empty((B, frames), dtype=torch.float32, device=c.device)
    scratch = torch.empty(int(lib.fastsvc_f0_track_scratch_bytes(B, frames)), dtype=torch.uint8, device=c.device)
    with torch.cuda.device(c.device):
        _check(lib, lib.fastsvc_f0_track(ctypes.c_void_p(c.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                         ctypes.c_void_p(scratch.data_ptr()), B, frames, int(tau_max),
                                         ctypes.c_float(float(sample_rate)), int(track.lag), float(track.lag_bias),
                                         float(track.jump), float(track.switch), float(unvoiced),
                                         ctypes.c_void_p(torch.cuda.current_stream(c.device).cuda_stream)), "fastsvc_f0_track")
    return out[0] if single else out
