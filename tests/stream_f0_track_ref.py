"""Float64 reference of the fixed-lag Viterbi F0 tracker (decode.F0Track, decode.f0_track_rule, f0.f0_candidates, DESIGN.md
4.10), written from the definition alone and in another form than the rule on the host: the candidates of a frame from the
d' of stream_f0_ref.yin_frame(..., full=True), the recurrence as 5 x 5 matrices in numpy.  Plus the signals the tracker's
tests share and the measures the GPU test's margins are taken with.

    candidates   lags t in [max(tau_min, 2), tau_max] with d'(t) < cand_threshold, d'(t) < d'(t - 1) and t == tau_max or d'(t)
                 <= d'(t + 1); the four with the smallest d' (ties: the smaller lag) in ascending lag; (tau_hat, s): the
                 estimator's parabola under its conditions, s = d'(t); absent (0, inf); a flat frame has none
    local        c_k = s_k + lag_bias ((tau_hat_k - tau_hat_0) / tau_max); state 4 (unvoiced): `unvoiced`; absent: inf
    transition   4 -> 4: 0; voiced <-> 4: switch; a -> b: jump (|ta - tb| / min(ta, tb))
    recurrence   C_0 = local; C'[j] = (min_a C[a] + tr(a, j)) + local[j], ties to the smallest a; C = C' - min C'
    output       e = min(f + lag, F - 1): argmin C_e (ties: smallest index) followed back to f; f0 = sr / tau_hat or 0
"""
from typing import NamedTuple

import numpy as np

import stream_f0_ref as R

K = 4
DEFAULTS = dict(lag=8, cand_threshold=0.5, lag_bias=0.2, jump=1.0, switch=0.3, unvoiced=R.THRESHOLD)


class Cands(NamedTuple):
    pairs: np.ndarray      # (4, 2): (tau_hat, s), absent (0, inf), in the dtype of d'
    lags: list             # the integer lags kept, ascending
    margin: list           # per kept lag: the smallest distance of a decision that made it one from flipping - d' against
                           # cand_threshold, against its two neighbours, and against the fifth-best local minimum (inf: none)
    minima: np.ndarray     # every lag that is a local minimum under the threshold, kept or not


def candidates(dn, tau_min, tau_max, cand_threshold=0.5, flat=False) -> Cands:
    """The candidates of one frame from its d' (index = lag), in the arithmetic of ``dn.dtype``."""
    dtype = dn.dtype.type
    pairs = np.zeros((K, 2), dtype=dn.dtype)
    pairs[:, 1] = np.inf
    if flat:
        return Cands(pairs, [], [], np.zeros(0, dtype=np.int64))
    thr = dtype(np.float32(cand_threshold))
    t = np.arange(max(tau_min, 2), tau_max + 1)
    right = np.append(dn[t[:-1] + 1], dtype(np.inf))          # (t == tau_max: no right neighbour to lose against)
    is_min = (dn[t] < thr) & (dn[t] < dn[t - 1]) & (dn[t] <= right)
    minima = t[is_min]
    order = minima[np.lexsort((minima, dn[minima]))]           # by d', then by lag
    kept = np.sort(order[:K])
    fifth = float(dn[order[K]]) if order.size > K else float("inf")
    margin = []
    for k, tau in enumerate(kept.tolist()):
        s0, s1 = dn[tau - 1], dn[tau]
        tau_hat = dtype(tau)
        m = min(float(thr) - float(s1), float(s0) - float(s1), fifth - float(s1))
        if tau + 1 <= tau_max:
            s2 = dn[tau + 1]
            m = min(m, float(s2) - float(s1))
            den = (s0 - s1) + (s2 - s1)
            if s1 <= s0 and s1 <= s2 and den > 0:
                tau_hat = tau_hat + (dtype(0.5) * (s0 - s2)) / den
        pairs[k] = (tau_hat, s1)
        margin.append(m)
    return Cands(pairs, kept.tolist(), margin, minima)


def frame_candidates(x, cand_threshold=0.5, model=R.yin_frame, **kw):
    """Frame x (2048 samples) -> (Pick, Cands, d') with ``model`` = yin_frame (float64) or yin_frame_f32; ``kw``: the model's
    (``f0_floor=24.0`` widens the search to tau_max = 1000, where a tone offers far more than four minima)."""
    pick, dn = model(x, full=True, **kw)
    tau_min, tau_max = R.lags(*(kw.get(k, d) for k, d in (("sr", R.SR), ("f0_floor", R.F0_FLOOR), ("f0_ceil", R.F0_CEIL))))
    flat = bool(np.all(dn[1:] == 1))                           # (d(1) == 0: the models leave d' at 1 everywhere)
    return pick, candidates(dn, tau_min, tau_max, cand_threshold, flat), dn


def audio_candidates(audio, hop, cand_threshold=0.5, model=R.yin_frame, **kw):
    """-> (picks, list of Cands, list of d') for the ``1 + len(audio) // hop`` frames of the whole-file function."""
    out = [frame_candidates(R.frame(audio, f, hop), cand_threshold, model, **kw) for f in range(1 + len(audio) // hop)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def _costs(pairs, ppairs, tau_max, lag_bias, jump, switch, unvoiced):
    """Local costs (5,) of a frame and the transition matrix (5, 5) from the frame before (None: no matrix)."""
    inf = np.inf
    tau, s = pairs[:, 0].astype(np.float64), pairs[:, 1].astype(np.float64)
    on = np.isfinite(s)
    local = np.full(K + 1, inf)
    local[:K][on] = s[on] + lag_bias * ((tau[on] - tau[0]) / float(tau_max))
    local[K] = unvoiced
    if ppairs is None:
        return local, None
    ptau, pon = ppairs[:, 0].astype(np.float64), np.isfinite(ppairs[:, 1])
    both = pon[:, None] & on[None, :]
    ta, tb = np.where(both, ptau[:, None], 1.0), np.where(both, tau[None, :], 1.0)
    tr = np.full((K + 1, K + 1), inf)
    tr[:K, :K] = np.where(both, jump * (np.abs(ta - tb) / np.minimum(ta, tb)), inf)
    tr[:K, K] = np.where(pon, switch, inf)
    tr[K, :K] = np.where(on, switch, inf)
    tr[K, K] = 0.0
    return local, tr


def forward(cands, tau_max, lag_bias, jump, switch, unvoiced):
    """The recurrence over ``cands (F, 4, 2)`` -> (best state per frame (F,), backpointers (F, 5))."""
    F = len(cands)
    best, back = np.zeros(F, dtype=np.int64), np.zeros((F, K + 1), dtype=np.int64)
    C = None
    for f in range(F):
        local, tr = _costs(cands[f], cands[f - 1] if f else None, tau_max, lag_bias, jump, switch, unvoiced)
        if f == 0:
            C = local
        else:
            tot = C[:, None] + tr                              # (a, j); an absent a or j is inf: it never wins against state 4
            back[f] = np.argmin(tot, axis=0)                   # (the first of equals: the smallest a)
            C = tot[back[f], np.arange(K + 1)] + local
            C = C - C.min()
        best[f] = int(np.argmin(C))
    return best, back


def states(cands, tau_max, lag=8, lag_bias=0.2, jump=1.0, switch=0.3, unvoiced=R.THRESHOLD):
    """The fixed-lag state of every frame: traced back from ``min(f + lag, F - 1)``."""
    best, back = forward(cands, tau_max, lag_bias, jump, switch, unvoiced)
    F = len(cands)
    out = np.zeros(F, dtype=np.int64)
    for f in range(F):
        e = min(f + lag, F - 1)
        s = best[e]
        for g in range(e, f, -1):
            s = back[g, s]
        out[f] = s
    return out


def viterbi_states(cands, tau_max, lag_bias=0.2, jump=1.0, switch=0.3, unvoiced=R.THRESHOLD):
    """Plain Viterbi: ONE trace from the last frame's best state."""
    best, back = forward(cands, tau_max, lag_bias, jump, switch, unvoiced)
    F = len(cands)
    out = np.zeros(F, dtype=np.int64)
    s = best[F - 1]
    for f in range(F - 1, -1, -1):
        out[f] = s
        s = back[f, s]
    return out


def f0_of(cands, st, sr=R.SR):
    """States -> F0 in the candidates' dtype: sr / tau_hat, 0 when unvoiced."""
    cands = np.asarray(cands)
    out = np.zeros(len(cands), dtype=cands.dtype)
    v = st < K
    out[v] = cands.dtype.type(sr) / cands[np.nonzero(v)[0], st[v], 0]
    return out


def track(cands, tau_max, sr=R.SR, **kw):
    """cands (F, 4, 2) -> the tracked F0 (F,), in the candidates' dtype."""
    cands = np.asarray(cands)
    kw.pop("cand_threshold", None)
    return f0_of(cands, states(cands, tau_max, **kw), sr)


def track_audio(audio, hop, **kw):
    """-> (per-frame reference F0, tracked reference F0, cands (F, 4, 2)) of the audio, float64."""
    p = dict(DEFAULTS, **kw)
    picks, cs, _ = audio_candidates(audio, hop, p["cand_threshold"])
    cands = np.stack([c.pairs for c in cs])
    return np.array([q.f0 for q in picks]), track(cands, R.lags()[1], **p), cands


# ------------------------------------------------------------------------------------------------------------ signals

T_TRACK = 96 * 256
BURST_F0, SUB_F0 = 150.0, 160.0
SUBHARMONICS = ((0.3, 0.4, 0.6), (0.6, 0.47, 0.53))           # (a, lo, hi): gated;  (1.0, 0.47, 0.53) is reported only


def burst_signal() -> np.ndarray:
    """A 150 Hz harmonic tone with a 20 ms noise burst of amplitude 0.2 in its middle, float32."""
    y = R.harmonic_tone(BURST_F0, T_TRACK).astype(np.float64)
    y[T_TRACK // 2: T_TRACK // 2 + 480] += 0.2 * np.random.default_rng(3).standard_normal(480)
    return y.astype(np.float32)


def subharmonic_signal(a: float, lo: float, hi: float) -> np.ndarray:
    """A 160 Hz harmonic tone whose amplitude is modulated at 80 Hz under a Hann envelope over [lo T, hi T), float32."""
    T = T_TRACK
    phi = 2.0 * np.pi * SUB_F0 * np.arange(T) / R.SR
    env = np.zeros(T)
    i0, i1 = int(lo * T), int(hi * T)
    env[i0:i1] = np.hanning(i1 - i0)
    y = (0.5 * np.sin(phi) + 0.25 * np.sin(2 * phi) + 0.125 * np.sin(3 * phi)) * (1.0 + a * env * np.cos(phi / 2.0))
    return (y + 1e-5 * np.random.default_rng(1).standard_normal(T)).astype(np.float32)


def bad_frames(f0, true: float) -> int:
    """Frames that are unvoiced or more than 1 % from the true frequency."""
    f0 = np.asarray(f0, dtype=np.float64)
    return int(np.sum(~((f0 > 0) & (np.abs(f0 - true) <= 0.01 * true))))


def track_signals() -> dict:
    """name -> (float32 audio, true frequency or None): the tracker's own signals and stream_f0_ref.f0_signals()."""
    sig = {"burst": (burst_signal(), BURST_F0)}
    for a, lo, hi in SUBHARMONICS:
        sig[f"sub{a:g}"] = (subharmonic_signal(a, lo, hi), SUB_F0)
    for name, y in R.f0_signals().items():
        sig[name] = (y, None)
    return sig


WIDE_FLOOR = 24.0           # f0_floor of the WIDE cases: tau_max = 1000, so that frames offer more than four local minima


def wide_signals() -> dict:
    """name -> float32 audio for the candidate SELECTION: searched down to 24 Hz (tau_max 1000) a 339 Hz tone has up to 14
    local minima of d' under 0.5 in a frame, the glide up to 8, a 220 Hz tone in 0.02 noise up to 9 - the four smallest are
    kept and a fifth-best exists."""
    sig = R.f0_signals()
    noisy = sig["tone220"].astype(np.float64) + 0.02 * np.random.default_rng(5).standard_normal((2, sig["tone220"].size))[1]
    return {"tone339": sig["tone339"], "glide": sig["glide"], "tone220n": noisy.astype(np.float32)}


def measure_float32_model(cases, every: int = 1) -> dict:
    """What the GPU test of the candidates takes its bounds from: the float32 model of the kernel's d' (yin_frame_f32) given
    to the candidate rule in float32, against float64, over every ``every``-th frame of ``cases = [(audio, hop, f0_floor),
    ...]``.  -> dict(dn: largest |d'_32 - d'_64|, s, tau: largest differences of a candidate both have, lost: the largest
    reference margin of a candidate the model does not have, gained: candidates of the model the reference does not have,
    most: the most local minima in one frame).  Minutes over all frames of all signals; the CPU test samples."""
    out = dict(dn=0.0, s=0.0, tau=0.0, lost=0.0, gained=0, most=0)
    for y, hop, floor in cases:
        for f in range(0, 1 + len(y) // hop, every):
            x = R.frame(y, f, hop)
            _, c64, d64 = frame_candidates(x, f0_floor=floor)
            _, c32, d32 = frame_candidates(x, model=R.yin_frame_f32, f0_floor=floor)
            out["dn"] = max(out["dn"], float(np.max(np.abs(d32.astype(np.float64) - d64))))
            out["most"] = max(out["most"], len(c64.minima))
            for k, t in enumerate(c64.lags):
                if t in c32.lags:
                    j = c32.lags.index(t)
                    out["s"] = max(out["s"], abs(float(c32.pairs[j, 1]) - float(c64.pairs[k, 1])))
                    out["tau"] = max(out["tau"], abs(float(c32.pairs[j, 0]) - float(c64.pairs[k, 0])))
                else:
                    out["lost"] = max(out["lost"], c64.margin[k])
            out["gained"] += sum(1 for t in c32.lags if t not in c64.lags)
    return out


def measured_cases():
    """Every (audio, hop, f0_floor) the bounds of tests/test_f0_candidates_gpu.py were measured over."""
    cases = [(y, hop, R.F0_FLOOR) for y, _ in track_signals().values() for hop in (160, 256)]
    return cases + [(y, hop, WIDE_FLOOR) for y in wide_signals().values() for hop in (160, 256)]


if __name__ == "__main__":                             # python tests/stream_f0_track_ref.py: the full measurement
    narrow = [c for c in measured_cases() if c[2] == R.F0_FLOOR]
    wide = [c for c in measured_cases() if c[2] == WIDE_FLOOR]
    print("f0_floor 70:", measure_float32_model(narrow))
    print("f0_floor 24:", measure_float32_model(wide))
