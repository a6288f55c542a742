"""Float64 reference of the F0 estimator (svcc23_fastsvc_amd.f0.f0_extract, decode.StreamSession(f0="audio"), DESIGN.md
4.10): YIN per frame on the loudness frame, stated in numpy.  Plus a float32 MODEL of the kernel's arithmetic (the order of
csrc/fastsvc_f0.inc, fused multiply-adds included) that the margins of the GPU tests are measured with on the CPU, and the
test signals the F0 tests share.

    x[k], k in [0, 2048): sample f hop - 1024 + k of the audio, np.pad reflection at both ends, no window
    tau_min = floor(sr / f0_ceil), tau_max = ceil(sr / f0_floor), W = 2048 - tau_max
    d(tau)  = sum over 1 <= j < W of (x[j] - x[j + tau])^2               (x[0] is never read)
    d'(tau) = d(tau) tau / (d(1) + ... + d(tau));  d(1) == 0 -> unvoiced
    tau     = smallest lag in [tau_min, tau_max] with d'(tau) < threshold, walked right while d'(tau + 1) < d'(tau)
    parabola over d'(tau - 1), d'(tau), d'(tau + 1) when both neighbours exist and d'(tau) is the smallest of the three
    f0      = sr / tau_hat, 0 when unvoiced
"""
import math
from typing import NamedTuple

import numpy as np

SR = 24000
N_FFT = 2048
F0_FLOOR, F0_CEIL, THRESHOLD = 70.0, 340.0, 0.15


def lags(sr=SR, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL):
    sr, lo, hi = (float(np.float32(v)) for v in (sr, f0_floor, f0_ceil))
    return int(math.floor(sr / hi)), int(math.ceil(sr / lo))


def reflect_index(i, T):
    """np.pad(mode="reflect") as an index map, for any i (several reflections when T is short)."""
    i = np.asarray(i, dtype=np.int64)
    if T == 1:
        return np.zeros_like(i)
    period = 2 * (T - 1)
    i = np.mod(i, period)
    return np.where(i < T, i, period - i)


def frame(audio, f: int, hop: int) -> np.ndarray:
    """The 2048 samples of frame f, in the audio's dtype."""
    audio = np.asarray(audio)
    return audio[reflect_index(f * hop - N_FFT // 2 + np.arange(N_FFT), len(audio))]


class Pick(NamedTuple):
    f0: float          # Hz, 0.0 when unvoiced
    tau: int           # the lag picked (after the walk), 0 when unvoiced
    margin: float      # the smallest distance of any comparison that decided `tau` from flipping: |d'(t) - threshold| for
                       # every lag up to the first one under the threshold (all lags when unvoiced), |d'(t + 1) - d'(t)|
                       # for every step of the walk and the one that stopped it; inf for a constant frame


def _pick(dn, tau_min, tau_max, threshold, sr, flat, dtype):
    """The decision on d' (index = lag), in ``dtype`` arithmetic."""
    if flat:
        return Pick(0.0, 0, float("inf"))
    seg = dn[tau_min: tau_max + 1]
    under = np.nonzero(seg < threshold)[0]
    if under.size == 0:
        return Pick(0.0, 0, float(np.min(np.abs(seg.astype(np.float64) - threshold))))
    first = tau_min + int(under[0])
    margin = float(np.min(np.abs(dn[tau_min: first + 1].astype(np.float64) - threshold)))
    tau = first
    while tau + 1 <= tau_max:
        margin = min(margin, abs(float(dn[tau + 1]) - float(dn[tau])))
        if not dn[tau + 1] < dn[tau]:
            break
        tau += 1
    tau_hat = dtype(tau)
    if tau - 1 >= 1 and tau + 1 <= tau_max:
        s0, s1, s2 = dn[tau - 1], dn[tau], dn[tau + 1]
        den = (s0 - s1) + (s2 - s1)
        if s1 <= s0 and s1 <= s2 and den > 0:
            tau_hat = tau_hat + (dtype(0.5) * (s0 - s2)) / den
    return Pick(float(dtype(sr) / tau_hat), tau, margin)


def yin_frame(x, sr=SR, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL, threshold=THRESHOLD, full: bool = False):
    """The reference: frame x (2048 samples) -> Pick, in float64.  ``full``: -> (Pick, d' indexed by lag)."""
    tau_min, tau_max = lags(sr, f0_floor, f0_ceil)
    W = N_FFT - tau_max
    x = np.asarray(x, dtype=np.float64)
    V = np.lib.stride_tricks.sliding_window_view(x[1:], W - 1)[: tau_max + 1]       # V[tau, j - 1] = x[j + tau]
    d = np.zeros(tau_max + 1)
    d[1:] = ((V[0][None, :] - V[1:]) ** 2).sum(axis=1)
    flat = d[1] == 0.0
    dn = np.ones(tau_max + 1)
    if not flat:
        dn[1:] = d[1:] * np.arange(1, tau_max + 1) / np.cumsum(d[1:])
    p = _pick(dn, tau_min, tau_max, float(np.float32(threshold)), float(np.float32(sr)), flat, np.float64)
    return (p, dn) if full else p


def yin_frame_f32(x, sr=SR, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL, threshold=THRESHOLD, full: bool = False):
    """The float32 MODEL of csrc/fastsvc_f0.inc: four partial sums by j mod 4, each a chain of fused multiply-adds in
    ascending j (a product of two float32 is exact in float64, so float32(float64 sum) is the fused result up to a rare
    double rounding), (p0 + p1) + (p2 + p3), the running sum in ascending lag, every other operation rounded to float32."""
    f32 = np.float32
    tau_min, tau_max = lags(sr, f0_floor, f0_ceil)
    W = N_FFT - tau_max
    x = np.asarray(x, dtype=f32)
    V = np.lib.stride_tricks.sliding_window_view(x, W)[: tau_max + 1]               # V[tau, j] = x[j + tau]
    E = (V[0][None, :] - V[1:]).astype(f32)                                         # E[tau - 1, j], rounded to float32
    E64 = E.astype(np.float64)
    part = np.zeros((4, tau_max), dtype=f32)
    for j in range(1, W):
        part[j & 3] = (E64[:, j] * E64[:, j] + part[j & 3].astype(np.float64)).astype(f32)
    d = np.zeros(tau_max + 1, dtype=f32)
    d[1:] = (part[0] + part[1]) + (part[2] + part[3])
    flat = d[1] == 0.0
    dn = np.ones(tau_max + 1, dtype=f32)
    if not flat:
        c = np.cumsum(d[1:], dtype=f32)                                             # (sequential: ascending lag)
        dn[1:] = (d[1:] * np.arange(1, tau_max + 1, dtype=f32)) / c
    p = _pick(dn, tau_min, tau_max, f32(threshold), f32(sr), flat, f32)
    return (p, dn) if full else p


def f0_frames(audio, hop: int, n_frames=None, model=yin_frame, **kw):
    """-> list of Pick, one per frame: ``1 + len(audio) // hop`` frames (the whole-file function) or the first ``n_frames``."""
    audio = np.asarray(audio)
    n = 1 + len(audio) // hop if n_frames is None else int(n_frames)
    return [model(frame(audio, f, hop), **kw) for f in range(n)]


# ------------------------------------------------------------------------------------------------------------ signals

def harmonic_tone(freq, n: int, phase: float = 0.0) -> np.ndarray:
    """A sine with three harmonics (0.5, 0.25, 0.125) whose frequency follows ``freq`` (a number or n values), float32."""
    f = np.broadcast_to(np.asarray(freq, dtype=np.float64), (n,))
    ph = phase + 2.0 * np.pi * np.cumsum(f) / SR
    return (0.5 * np.sin(ph) + 0.25 * np.sin(2.0 * ph) + 0.125 * np.sin(3.0 * ph)).astype(np.float32)


TONES = (70.5, 110.0, 220.0, 339.0)
TONE_SAMPLES = 4800                                  # 0.2 s
GLIDE_SAMPLES = 9600                                 # 0.4 s, 110 -> 220 Hz (linear in time)


def glide_freq() -> np.ndarray:
    return np.linspace(110.0, 220.0, GLIDE_SAMPLES)


def f0_signals() -> dict:
    """name -> float32 audio, each a file of its own: the four steady tones, the glide, voiced -> silence -> voiced, white
    noise at 1e-3, digital silence."""
    sig = {f"tone{f:g}": harmonic_tone(f, TONE_SAMPLES) for f in TONES}
    sig["glide"] = harmonic_tone(glide_freq(), GLIDE_SAMPLES)
    gap = np.concatenate([harmonic_tone(150.0, 3200), np.zeros(3200, dtype=np.float32), harmonic_tone(150.0, 3200)])
    sig["gap"] = gap
    sig["noise"] = (1e-3 * np.random.default_rng(7).standard_normal(TONE_SAMPLES)).astype(np.float32)
    sig["zeros"] = np.zeros(TONE_SAMPLES, dtype=np.float32)
    return sig


def interior_frames(n_samples: int, hop: int):
    """The frames whose 2048 samples all lie inside the audio: no reflection."""
    return [f for f in range(1 + n_samples // hop) if f * hop - N_FFT // 2 >= 0 and f * hop + N_FFT // 2 <= n_samples]


def voiced_stream(F: int, hop: int, seed: int = 0) -> np.ndarray:
    """F hop samples for the stream tests: a harmonic tone that wanders between 120 and 200 Hz, a silent stretch in the
    middle of streams of 30 frames and more (14 frames: longer than a frame, so some frames hold nothing but the noise
    and are unvoiced), over 1e-5 noise.  float32."""
    T = F * hop
    rng = np.random.default_rng(seed)
    f = 160.0 + 40.0 * np.sin(2.0 * np.pi * (np.arange(T) / SR) * (0.6 + 0.1 * seed) + seed)
    y = harmonic_tone(f, T, phase=float(seed))
    if F >= 30:
        y[T // 2 - 7 * hop: T // 2 + 7 * hop] = 0.0
    return (y + 1e-5 * rng.standard_normal(T)).astype(np.float32)
