"""Float64 reference of the running source F0 statistics of live streams (decode.RunningF0Stats), written
from the rule and not from the package: it imports nothing of svcc23_fastsvc_amd.

A stream has six constants - prior mean m_p, prior std s_p > 0, prior weight n0 > 0 (frames), decay g = exp(-1 / horizon) or
exactly 1.0, target mean m_t, target std s_t - and a state (w, S1, S2) = (0, 0, 0).  Frames in order; raw F0 v:

    v <= 0: the output is 0, the state unchanged
    else    d = log((double) v) - m_p;  w = w g + 1;  S1 = S1 g + d;  S2 = S2 g + d d;  N = n0 + w;  mu = S1 / N
            var = (n0 s_p s_p + S2) / N - mu mu;  out = exp((s_t / sqrt(var)) (d - mu) + m_t)

every operation a separately rounded float64 operation.  ``running_loop`` is the ten-line loop (any decay); ``running_closed``
the closed form without a horizon, by np.cumsum over the voiced frames.  Both return a ``Track``.
"""
import math
from typing import NamedTuple

import numpy as np


class Track(NamedTuple):
    out: np.ndarray       # (F,) float64: the shifted F0, 0 on unvoiced frames
    mean: np.ndarray      # (V,) per voiced frame: m_p + mu, the mean of log F0 it was shifted with
    var: np.ndarray       # (V,) ... and the variance
    w: np.ndarray         # (V,) the weight after the frame
    s1: np.ndarray        # (V,)
    s2: np.ndarray        # (V,)


def decay(horizon=None) -> float:
    return 1.0 if horizon is None else math.exp(-1.0 / horizon)


def constants(trg, prior=None, prior_frames=100.0, horizon=None):
    """(m_p, s_p, n0, g, m_t, s_t); no prior: the target's statistics."""
    m_t, s_t = float(trg[0]), float(trg[1])
    m_p, s_p = (m_t, s_t) if prior is None else (float(prior[0]), float(prior[1]))
    return m_p, s_p, float(prior_frames), decay(horizon), m_t, s_t


def running_loop(f0, consts) -> Track:
    m_p, s_p, n0, g, m_t, s_t = consts
    f0 = np.asarray(f0).reshape(-1)
    voiced = f0 > 0
    d = np.log(f0[voiced].astype(np.float64)) - m_p
    V = d.size
    mu, var, ws, a1, a2 = (np.empty(V) for _ in range(5))
    w = s1 = s2 = 0.0
    for k, dk in enumerate(d.tolist()):
        w = w * g + 1.0
        s1 = s1 * g + dk
        s2 = s2 * g + dk * dk
        N = n0 + w
        mu[k] = s1 / N
        var[k] = (n0 * s_p * s_p + s2) / N - mu[k] * mu[k]
        ws[k], a1[k], a2[k] = w, s1, s2
    out = np.zeros(f0.size)
    out[voiced] = np.exp((s_t / np.sqrt(var)) * (d - mu) + m_t)
    return Track(out, m_p + mu, var, ws, a1, a2)


def running_closed(f0, consts) -> Track:
    """Without a horizon (g == 1): w_k = k, S1 and S2 the running sums of d and d d."""
    m_p, s_p, n0, g, m_t, s_t = consts
    assert g == 1.0
    f0 = np.asarray(f0).reshape(-1)
    voiced = f0 > 0
    d = np.log(f0[voiced].astype(np.float64)) - m_p
    w = np.arange(1, d.size + 1, dtype=np.float64)
    s1, s2 = np.cumsum(d), np.cumsum(d * d)
    N = n0 + w
    mu = s1 / N
    var = (n0 * s_p * s_p + s2) / N - mu * mu
    out = np.zeros(f0.size)
    out[voiced] = np.exp((s_t / np.sqrt(var)) * (d - mu) + m_t)
    return Track(out, m_p + mu, var, w, s1, s2)


def estimate(f0):
    """[mean, population std] of log F0 over the voiced frames (np.std: what F0Statistics.estimate uses)."""
    f0 = np.asarray(f0).reshape(-1)
    logs = np.log(f0[f0 > 0].astype(np.float64))
    return np.array([np.mean(logs), np.std(logs)])


def fixed_convert(f0, src, trg):
    """The fixed Gaussian shift (F0Statistics.convert), float64."""
    f0 = np.asarray(f0).reshape(-1)
    out = np.zeros(f0.size)
    voiced = f0 > 0
    out[voiced] = np.exp((trg[1] / src[1]) * (np.log(f0[voiced].astype(np.float64)) - src[0]) + trg[0])
    return out


def wandering_track(F: int, seed: int = 0, unvoiced: float = 0.15) -> np.ndarray:
    """F frames of F0 (float32) whose log wanders between 120 and 200 Hz - two incommensurate slow sines and a little
    jitter - with stretches of unvoiced frames (0) that cover about ``unvoiced`` of the track."""
    rng = np.random.default_rng(seed)
    t = np.arange(F, dtype=np.float64)
    lo, hi = math.log(120.0), math.log(200.0)
    mid, amp = 0.5 * (lo + hi), 0.5 * (hi - lo)
    x = 0.62 * np.sin(2.0 * np.pi * t / 173.0 + seed) + 0.33 * np.sin(2.0 * np.pi * t / 61.0 + 1.0) + 0.05 * rng.uniform(-1, 1, F)
    f0 = np.exp(mid + amp * x)
    if unvoiced > 0:
        gate = np.sin(2.0 * np.pi * t / 47.0 + 0.5 * seed) > math.cos(math.pi * unvoiced)
        f0[gate] = 0.0
    assert f0[f0 > 0].min() >= 120.0 and f0.max() <= 200.0
    return f0.astype(np.float32)


def ulps32(a, b) -> np.ndarray:
    """|a - b| in float32 units in the last place (both positive float32 arrays)."""
    a, b = (np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    return np.abs(a - b)
