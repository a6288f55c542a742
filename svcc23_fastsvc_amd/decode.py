"""Decode harness - the caller on the other side of the generator boundary.

Mirrors what ``harana/bin/decode_fastsvc.py:120-206`` does per utterance - F0 mean shift
(``harana/utils/features.py:41-108``, std forced to 1 at ``decode_fastsvc.py:165,176``), sine
excitation, ``inference()``, PCM-16 wav - but batches the utterances: they are grouped by similar
length, zero-padded, and run as ragged batches (``lengths``), with the excitation synthesised on the
device.  Each utterance's waveform equals what the reference's one-at-a-time loop produces
(``tests/golden/decode_chain.npz`` is made by that loop on the live reference).

Feature containers follow the reference's dump layout (``audio_feats_dataset.py:30-34``), time-major:
``f0 (F, 1)``, ``ppg (F, C)``, ``lft (T, 1)``, optionally ``spk_emb``; ``.npz`` files with those keys
are read here (``.h5`` as well when h5py is importable - it is not a dependency).

    python -m svcc23_fastsvc_amd.decode --dumpdir feats/ --checkpoint ckpt.pkl --config conf.yaml \\
        --outdir wav/ --spk-emb embs.npz --srcf0stats src_stats/ --trgf0stats trg_stats/

``--resident`` keeps the features on the device across target speakers (``DecodeSession``); with it, ``--fanout N`` converts
the speakers in groups of N whose batches hold (utterance, speaker) rows (``convert_many``: for small source sets), ``--checked
[--fallback bfloat16,float32]`` reports per utterance what the PCM-16 conversion hides and re-runs in a fallback storage the
batches whose output is not finite, and ``--storage auto`` is float16 storage with ``--checked --fallback bfloat16``.
``--window CORE[,CONTEXT[,FADE]]`` decodes every utterance as overlapping windows (``convert_windowed``): recordings longer
than one forward takes, in buffers sized by the window.  ``--stream PUSH[,CORE[,CONTEXT[,FADE]]] [--streams N]`` feeds the
dumps as N concurrent simulated LIVE streams, PUSH frames per call (``StreamSession``: features arrive chunk by chunk,
samples come back as soon as their window has its context); ``--stream-norm running`` normalises every window by the
statistics of all frames its stream has delivered so far, carried on the GPU, instead of by the window's own, and
``--stream-horizon FRAMES`` forgets those statistics exponentially; ``--checked``, ``--fallback`` and ``--storage auto`` work
on streams too: every window is checked, and re-run in a fallback storage, before its samples or its running statistics
are used (``StreamSession(checked=True)``).
"""
from __future__ import annotations

import argparse
import glob
import math
import os
import time
import wave
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .distributed import bucket_ragged


class F0Statistics:
    """Same surface as ``harana.utils.features.F0Statistics`` (features.py:41-108)."""

    def estimate(self, f0list: Sequence[np.ndarray]) -> np.ndarray:
        """[mean, std] of log F0 over the voiced (non-zero) frames of all sequences."""
        logs = [np.log(np.asarray(f0)[np.nonzero(f0)]) for f0 in f0list]
        f0s = np.concatenate(logs) if logs else np.zeros(0)
        return np.array([np.mean(f0s), np.std(f0s)])

    def convert(self, f0: np.ndarray, orgf0stats: Sequence[float], tarf0stats: Sequence[float]) -> np.ndarray:
        """Gaussian-normalised log-F0 transform of the voiced frames; unvoiced frames stay 0."""
        f0 = np.asarray(f0)
        cvf0 = np.zeros(len(f0))
        voiced = f0 > 0
        cvf0[voiced] = np.exp((tarf0stats[1] / orgf0stats[1]) * (np.log(f0[voiced]) - orgf0stats[0]) + tarf0stats[0])
        return cvf0


@dataclass(frozen=True)
class RunningF0Stats:
    """Source F0 statistics a live stream makes for itself: pass it to ``StreamSession.open`` as ``src_f0_stats`` where a
    ``[mean, std]`` of log F0 over a corpus goes, which a live microphone does not have (``StreamSession``'s docstring and
    DESIGN.md 4.10 have the rule).  ``prior``: ``[mean, std]`` of log F0 the stream starts from, finite with ``std > 0``, or
    None for the target's statistics - the stream then begins almost unshifted; ``prior_frames``: the voiced frames the prior
    counts as, finite and ``> 0`` (it is never forgotten); ``horizon``: None, or the voiced frames after which a frame counts
    with 1 / e, finite and ``>= 1``.  Immutable; a ``ValueError`` for anything else."""
    prior: Optional[Tuple[float, float]] = None
    prior_frames: float = 100.0
    horizon: Optional[float] = None

    def __post_init__(self):
        if self.prior is not None:
            try:
                mean, std = (float(v) for v in self.prior)
            except (TypeError, ValueError) as e:
                raise ValueError(f"prior must be None or [mean, std] of log F0, got {self.prior!r}") from e
            if not (math.isfinite(mean) and math.isfinite(std) and std > 0.0):
                raise ValueError(f"prior must be a finite [mean, std] with std > 0, got {self.prior!r}")
            object.__setattr__(self, "prior", (mean, std))
        try:
            frames = float(self.prior_frames)
            horizon = None if self.horizon is None else float(self.horizon)
        except (TypeError, ValueError) as e:
            raise ValueError("prior_frames and horizon must be numbers") from e
        if not (math.isfinite(frames) and frames > 0.0):
            raise ValueError(f"prior_frames must be finite and > 0, got {self.prior_frames!r}")
        if horizon is not None and not (math.isfinite(horizon) and horizon >= 1.0):
            raise ValueError(f"horizon must be None or finite and >= 1 (voiced frames), got {self.horizon!r}")
        object.__setattr__(self, "prior_frames", frames)
        object.__setattr__(self, "horizon", horizon)

    @property
    def decay(self) -> float:
        """``g``: what a voiced frame multiplies the sums before it by - ``exp(-1 / horizon)``, exactly 1.0 without one."""
        return 1.0 if self.horizon is None else math.exp(-1.0 / self.horizon)

    def constants(self, trg_f0_stats: Sequence[float]) -> Tuple[float, float, float, float, float, float]:
        """The rule's six constants for a target ``[mean, std]``: ``(m_p, s_p, n0, g, m_t, s_t)``."""
        try:
            m_t, s_t = (float(v) for v in list(trg_f0_stats)[:2])
        except (TypeError, ValueError) as e:
            raise ValueError(f"trg_f0_stats must be [mean, std] of log F0, got {trg_f0_stats!r}") from e
        if not (math.isfinite(m_t) and math.isfinite(s_t)):
            raise ValueError(f"trg_f0_stats must be finite, got {trg_f0_stats!r}")
        m_p, s_p = (m_t, s_t) if self.prior is None else self.prior
        if not s_p > 0.0:
            raise ValueError(f"without a prior the target's std is the prior's and must be > 0, got {s_p}")
        return m_p, s_p, self.prior_frames, self.decay, m_t, s_t


def running_f0_convert(f0: np.ndarray, running: RunningF0Stats, trg_f0_stats: Sequence[float]) -> np.ndarray:
    """The running shift of a whole F0 track on the host - for ``RunningF0Stats`` what ``F0Statistics.convert`` is for fixed
    statistics, and what a stream opened with ``running`` applies frame by frame on the device.  Frames in order, from ``(w,
    S1, S2) = (0, 0, 0)``; an unvoiced frame (``f0 <= 0``) is 0 and changes nothing; a voiced one, every operation a separately
    rounded float64 operation::

        d = log(f0) - m_p;  w = w g + 1;  S1 = S1 g + d;  S2 = S2 g + d d;  N = n0 + w;  mu = S1 / N
        var = (n0 s_p s_p + S2) / N - mu mu;  out = exp((s_t / sqrt(var)) (d - mu) + m_t)

    Returns float64 (the device rounds it to float32)."""
    m_p, s_p, n0, g, m_t, s_t = running.constants(trg_f0_stats)
    f0 = np.asarray(f0).reshape(-1)
    out = np.zeros(f0.size)
    voiced = f0 > 0
    d = np.log(f0[voiced].astype(np.float64)) - m_p
    mu, var = np.empty(d.size), np.empty(d.size)
    prior = n0 * s_p * s_p
    w = s1 = s2 = 0.0
    for k, dk in enumerate(d.tolist()):              # (Python floats: IEEE doubles, one rounding per operation)
        w, s1, s2 = w * g + 1.0, s1 * g + dk, s2 * g + dk * dk
        N = n0 + w
        m = s1 / N
        mu[k], var[k] = m, (prior + s2) / N - m * m
    out[voiced] = np.exp((s_t / np.sqrt(var)) * (d - mu) + m_t)
    return out


F0_CANDIDATES = 4             # K: the candidates a frame offers the tracker - a constant of the definition, not a parameter
F0_TRACK_MAX_LAG = 64


@dataclass(frozen=True)
class F0Track:
    """Fixed-lag Viterbi tracking of the F0 over YIN candidates: pass it to ``StreamSession(f0="audio", f0_track=...)`` or
    ``f0_extract(track=...)`` (DESIGN.md 4.10 and ``f0_track_rule`` have the rule).  ``lag``: the frames the tracker looks
    ahead, ``0 <= lag <= 64`` - the value of frame f is a function of the audio of the frames ``<= f + lag`` alone, and a live
    stream delivers it ``lag`` frames later; ``cand_threshold > 0``: d' a local minimum must lie under to be a candidate;
    ``lag_bias``: what a candidate costs per ``tau_max`` of lag above the frame's smallest-lag candidate (it keeps the tracker
    off a sub-harmonic); ``jump``: the cost of an octave between voiced frames; ``switch``: of a change of voicing;
    ``unvoiced``: the unvoiced state's cost per frame, or None for the session's ``f0_threshold``.  Costs are finite and ``>=
    0``.  Immutable; a ``ValueError`` for anything else."""
    lag: int = 8
    cand_threshold: float = 0.5
    lag_bias: float = 0.2
    jump: float = 1.0
    switch: float = 0.3
    unvoiced: Optional[float] = None

    def __post_init__(self):
        try:
            lag = int(self.lag)
            if lag != self.lag:
                raise ValueError
            costs = {k: float(getattr(self, k)) for k in ("cand_threshold", "lag_bias", "jump", "switch")}
            if self.unvoiced is not None:
                costs["unvoiced"] = float(self.unvoiced)
        except (TypeError, ValueError) as e:
            raise ValueError("F0Track needs an integer lag and numbers for its costs") from e
        if not 0 <= lag <= F0_TRACK_MAX_LAG:
            raise ValueError(f"lag must be in [0, {F0_TRACK_MAX_LAG}] frames, got {self.lag!r}")
        for k, v in costs.items():
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"{k} must be finite and >= 0, got {getattr(self, k)!r}")
            object.__setattr__(self, k, v)
        if not costs["cand_threshold"] > 0.0:
            raise ValueError(f"cand_threshold must be > 0, got {self.cand_threshold!r}")
        object.__setattr__(self, "lag", lag)


def f0_track_rule(cands, tau_max: int, sample_rate: float, track: F0Track, unvoiced: float) -> np.ndarray:
    """The tracker on the host - for ``F0Track`` what ``running_f0_convert`` is for the running statistics, and what
    fastsvc_f0_track and a tracked stream compute on the device.  ``cands (F, 4, 2)``: per frame up to four ``(tau_hat, s)`` in
    ascending lag, absent entries ``(0, inf)`` (``f0.f0_candidates``).  Viterbi over the states {candidate 0..3, 4 = unvoiced},
    in float64 (Python floats: one rounding per operation)::

        local[k] = s_k + lag_bias ((tau_hat_k - tau_hat_0) / tau_max);  local[4] = unvoiced;  absent: inf
        tr(4, 4) = 0;  tr(a, 4) = tr(4, b) = switch;  tr(a, b) = jump (|ta - tb| / min(ta, tb))
        C_0 = local;  C'[j] = (min over a of C[a] + tr(a, j)) + local[j], ties to the smallest a (the backpointer; absent
        states take no part);  C = C' - min C'

    Frame f: the argmin of ``C_e`` (ties: the smallest index), ``e = min(f + lag, F - 1)``, followed back to f; ``f0 =
    sample_rate / tau_hat`` or 0 when unvoiced, in the dtype of ``cands`` (float32 candidates: the device's bits).  Returns
    ``(F,)`` of that dtype."""
    cands = np.asarray(cands)
    if cands.ndim != 3 or cands.shape[1:] != (F0_CANDIDATES, 2):
        raise ValueError(f"cands must be (F, {F0_CANDIDATES}, 2), got {cands.shape}")
    dtype = cands.dtype if cands.dtype in (np.float32, np.float64) else np.dtype(np.float64)
    F, K, inf = cands.shape[0], F0_CANDIDATES, float("inf")
    tmax, bias, jump, sw, uv, lag = float(int(tau_max)), track.lag_bias, track.jump, track.switch, float(unvoiced), track.lag
    back = np.zeros((F, K + 1), dtype=np.int64)
    best = np.zeros(F, dtype=np.int64)
    C, ptau = [], []
    for f in range(F):
        tau = [float(v) for v in cands[f, :, 0]]
        sc = [float(v) for v in cands[f, :, 1]]
        local = [sc[k] + bias * ((tau[k] - tau[0]) / tmax) if sc[k] < inf else inf for k in range(K)] + [uv]
        if f == 0:
            nxt = list(local)
        else:
            nxt = []
            for j in range(K + 1):
                top, src = inf, 0
                for a in range(K + 1) if local[j] < inf else ():
                    if not C[a] < inf:
                        continue
                    if a == K and j == K:
                        tr = 0.0
                    elif a == K or j == K:
                        tr = sw
                    else:
                        tr = jump * (abs(ptau[a] - tau[j]) / min(ptau[a], tau[j]))
                    v = C[a] + tr
                    if v < top:
                        top, src = v, a
                nxt.append(top + local[j])
                back[f, j] = src
            m = min(nxt)
            nxt = [v - m for v in nxt]
        C, ptau = nxt, tau
        best[f] = min(range(K + 1), key=lambda j: (C[j], j))
    out = np.zeros(F, dtype=dtype)
    sr = dtype.type(sample_rate)
    for f in range(F):
        e = min(f + lag, F - 1)
        st = best[e]
        for g in range(e, f, -1):
            st = back[g, st]
        if st < K:
            out[f] = sr / cands[f, st, 0].astype(dtype)
    return out


def convert_f0_device(f0: torch.Tensor, orgf0stats: Sequence[float], tarf0stats: Sequence[float]) -> torch.Tensor:
    """``F0Statistics.convert`` on a device tensor of any shape (float64 inside, like numpy)."""
    f = f0.to(torch.float64)
    voiced = f > 0
    safe = torch.where(voiced, f, torch.ones_like(f))
    cv = torch.exp((float(tarf0stats[1]) / float(orgf0stats[1])) * (torch.log(safe) - float(orgf0stats[0]))
                   + float(tarf0stats[0]))
    return torch.where(voiced, cv, torch.zeros_like(cv)).to(torch.float32)


def to_pcm16(y) -> np.ndarray:
    """float waveform -> int16: round-to-nearest of y * 32767 (libsndfile's float normalisation, which
    is what ``sf.write(..., "PCM_16")`` at decode_fastsvc.py:195-200 applies), saturated instead of
    wrapped when |y| > 1."""
    if isinstance(y, torch.Tensor):
        y = y.detach().to("cpu", torch.float32).numpy()
    return np.clip(np.rint(np.asarray(y, dtype=np.float64).reshape(-1) * 32767.0), -32768, 32767).astype(np.int16)


def output_report(y, lens: Optional[Sequence[int]] = None):
    """What ``to_pcm16`` hides, per row: ``(nonfinite, clipped, max_abs)``, int32, int32 and float32 arrays with one entry
    per row of ``y`` - a (B, width) / (B, 1, width) array or tensor, or a sequence of 1-D waveforms (what
    ``decode_utterances`` returns) - over each row's first ``lens[b]`` samples (default: the whole row):

        nonfinite  NaN / +-inf samples (``to_pcm16`` saturates the infinities; a NaN has no defined int16 value);
        clipped    finite samples whose PCM-16 value saturates: rint(float64(y) * 32767.0) outside [-32768, 32767], with
                   ``to_pcm16``'s own float64 arithmetic (so -32768 itself, reached from -1 - 2^-15, is a value, not a clip);
        max_abs    the largest |y| over the finite samples, 0 when there is none.

    The host reference of ``engine.output_check`` / ``pcm16_pack(report=)``, which give the same numbers bit for bit."""
    if isinstance(y, torch.Tensor):
        y = y.detach().to("cpu", torch.float32).numpy()
    rows = [np.asarray(r, dtype=np.float32).reshape(-1) for r in y]
    B = len(rows)
    if lens is None:
        lens = [r.size for r in rows]
    elif len(lens) != B:
        raise ValueError("output_report needs one length per row")
    nonfinite, clipped, max_abs = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.float32)
    for b, row in enumerate(rows):
        n = int(lens[b])
        if n < 0 or n > row.size:
            raise ValueError(f"row {b}: length {n} outside [0, {row.size}]")
        v = row[:n]
        finite = np.isfinite(v)
        v = v[finite]
        r = np.rint(v.astype(np.float64) * 32767.0)
        nonfinite[b] = n - int(finite.sum())
        clipped[b] = int(((r < -32768.0) | (r > 32767.0)).sum())
        max_abs[b] = np.abs(v).max() if v.size else 0.0
    return nonfinite, clipped, max_abs


def flagged_batches(batches: Sequence[Sequence[int]], flagged, among: Optional[Sequence[int]] = None) -> List[int]:
    """Indices, ascending, of the batches that hold at least one utterance of ``flagged`` - the batches a checked
    ``DecodeSession`` runs again, each as a whole.  ``among``: look at these batch indices only (a later round looks at the
    batches of the round before, with the utterances that are still flagged)."""
    flagged = set(int(i) for i in flagged)
    ks = range(len(batches)) if among is None else sorted(set(int(k) for k in among))
    return [k for k in ks if any(int(i) in flagged for i in batches[k])]


def storage_fallback(model, fallback: Sequence[str], n_units: int, is_flagged, rerun):
    """The storage fallback of every checked convert: ``(storage, tried, still)`` for the units ``0 .. n_units - 1`` of a
    pass (utterances, or (utterance, speaker) rows) that has just run in the model's own storage.  ``is_flagged(i)`` says
    whether unit i's latest result has non-finite samples.  For every name of ``fallback``, while units are flagged, the
    model is switched to that storage and ``rerun(name, flagged)`` has to run the flagged units again, each of them, and
    have ``is_flagged`` see the new results; what it runs beside them is its own business.  ``storage[i]`` is the storage
    unit i's result comes from, ``tried[i]`` the storages that left it flagged before, in order, ``still`` the units
    flagged after the last fallback.  The model is back in its first storage afterwards, also when ``rerun`` raises, and
    is never touched when nothing is flagged.  No device work in here: a pure host function."""
    first = getattr(model, "activation_storage", "float32")
    storage, tried = [first] * n_units, [[] for _ in range(n_units)]
    flagged = [i for i in range(n_units) if is_flagged(i)]
    try:
        for name in fallback:
            if not flagged:
                break
            model.use_activation_storage(name)
            rerun(name, flagged)
            for i in flagged:
                tried[i].append(storage[i])
                storage[i] = name
            flagged = [i for i in flagged if is_flagged(i)]
    finally:
        if getattr(model, "activation_storage", first) != first:
            model.use_activation_storage(first)
    return storage, tried, flagged


def _rerun_in_batches(row_batches: Sequence[Sequence[int]], run):
    """``storage_fallback``'s ``rerun`` for a pass whose units sit in batches that run as a whole (``row_batches[k]``: the
    units of batch k): every round ``run`` gets ``[(k, positions in batch k of its flagged units), ...]`` for the batches,
    among those of the round before, that hold a flagged unit (``flagged_batches``) - a unit flagged in a round was
    flagged in every round before, so its batch is always among them."""
    again = None

    def rerun(name, flagged):
        nonlocal again
        again = flagged_batches(row_batches, flagged, again)
        hit = set(flagged)
        run([(k, [j for j, r in enumerate(row_batches[k]) if r in hit]) for k in again])
    return rerun


def _report_dicts(rep, storage: Sequence[str], tried: Sequence[List[str]]) -> List[Dict[str, object]]:
    """``last_report``'s dicts, one per unit, from the units' downloaded report rows (n, 4)."""
    from .engine import report_arrays
    nonfinite, clipped, max_abs = report_arrays(rep)
    return [dict(storage=storage[i], nonfinite=int(nonfinite[i]), clipped=int(clipped[i]), max_abs=float(max_abs[i]),
                 tried=tried[i]) for i in range(len(storage))]


def _raise_still_nonfinite(model, fallback: Sequence[str], units: str, still) -> None:
    from .engine import FastSVCError
    raise FastSVCError(f"{units} {still} still have non-finite samples after storages "
                       f"{[getattr(model, 'activation_storage', 'float32')] + list(fallback)} (strict=True)")


def fanout_batches(frames: Sequence[int], n_speakers: int, max_batch: int = 32,
                   pad_tolerance: float = 0.125) -> List[List[Tuple[int, int]]]:
    """Batches of ``(utterance, speaker)`` rows for ``DecodeSession.convert_many``: ``bucket_ragged`` over the expanded row
    list ``r = utterance * n_speakers + speaker`` with ``n_frames[r] = frames[utterance]``, mapped back to pairs.  Longest
    first; the rows of one utterance are adjacent, speaker ascending - they share a length and pad nothing - and the
    utterances follow each other in ``bucket_ragged``'s own order, so with ``n_speakers == 1`` the batches are exactly
    ``bucket_ragged(range(len(frames)), frames, ...)``'s."""
    S = int(n_speakers)
    if S < 1:
        raise ValueError("fanout_batches needs at least one speaker")
    n = len(frames) * S
    rows = bucket_ragged(range(n), [int(frames[r // S]) for r in range(n)], max_batch, pad_tolerance)
    return [[(r // S, r % S) for r in chunk] for chunk in rows]


def fanout_layout(chunk: Sequence[Tuple[int, int]], counts: Sequence[int], offsets: Sequence[int]):
    """Where the rows of one fan-out batch go: ``(row_offsets, runs, total)``.  The batch's packed buffer is laid
    ``[speaker][utterance]``: ``row_offsets[j]`` is where row j's ``counts[utterance]`` elements start in it.  A
    speaker's utterances of one batch follow each other in the session's packing order (``offsets``: ``pack_layout`` in
    ``bucket_ragged``'s order, which is the order of ``fanout_batches``' utterances, and only a batch's first and last
    utterance can lack speakers), so each speaker is one contiguous run both there and in its own packed result:
    ``runs`` holds ``(speaker, first element in the speaker's result, start in the batch's buffer, count)``."""
    by_spk: Dict[int, List[int]] = {}
    for j, (_, sp) in enumerate(chunk):
        by_spk.setdefault(sp, []).append(j)
    row_offsets, runs, pos = [0] * len(chunk), [], 0
    for sp in sorted(by_spk):
        start = pos
        for j in by_spk[sp]:
            row_offsets[j] = pos
            pos += int(counts[chunk[j][0]])
        runs.append((sp, int(offsets[chunk[by_spk[sp][0]][0]]), start, pos - start))
    return row_offsets, runs, pos


def receptive_field_frames(cfg) -> int:
    """Frames of input on either side of an output frame that can influence it, for a generator WITHOUT a speaker
    embedding (with one, InstanceNorm couples a row's whole time axis): run on the frames ``[lo - R, hi + R)`` of an
    utterance, the generator's output on ``[lo, hi)`` is the whole-utterance result.  Derived from the layer table
    (``synth.layer_table``: a k = 3 convolution of dilation d reaches d samples of its own rate to either side), walking
    the dataflow backwards from ``conv_last`` with the reach held in samples of the current rate:

        up block i (output rate r_i = prod(scales[:i + 1]) samples a frame), reach H of its output:
            its stretched input is read to  H + d(conv_block3) + d(conv_block2) + d(conv_block1) + d(upsample_block0 /
            residual_block) samples; a stretch by s turns a reach of h into ceil(h / s) (window edges are frame edges, so
            they are multiples of s at every rate), and conv_first adds its own;
            the FiLM scale / shift are read to  H + d(conv_block3) + d(conv_block2) + d(conv_block1); the FiLM net adds
            conv and conv_scale / conv_shift, the down net of that rate its three convolutions, every decimation by s
            turns a reach of h into h * s, and the down nets of the higher rates add theirs, up to the full rate.

    The answer is the largest of the reaches at the frame rate (ppg) and at the full rate (lft and the excitation, rounded
    up to whole frames): 33 for the recipe's generator (scales 2, 4, 4, 5)."""
    from .synth import layer_table
    reach = {L.name: (L.ksize // 2) * L.dilation for L in layer_table(cfg) if L.kind != "linear"}
    scales = [int(v) for v in cfg.upsampling_scales]
    down_scales = [int(v) for v in cfg.down_scales]
    n = len(scales)
    hop = int(np.prod(scales))

    def down_reach(k: int) -> int:
        p = f"downsampling_lft.{k}"
        return max(reach[f"{p}.residual_block.0"],
                   reach[f"{p}.downsample_block.2"] + reach[f"{p}.downsample_block.4"] + reach[f"{p}.downsample_block.6"])

    need = 0                                             # frames
    H = reach["conv_last"]                               # reach of the last block's output, in its own samples
    for i in range(n - 1, -1, -1):
        p, k = f"upsampling_nets.{i}", n - 1 - i
        blocks = reach[f"{p}.conv_block3.1"] + reach[f"{p}.conv_block2.1"] + reach[f"{p}.conv_block1.1"]
        # conditioning: FiLM k at this block's rate, then down nets k, k - 1, ..., 0 back to the full rate
        h = H + blocks + reach[f"film_lft.{k}.conv"] + max(reach[f"film_lft.{k}.conv_scale"], reach[f"film_lft.{k}.conv_shift"])
        for j in range(k, -1, -1):
            h = (h + down_reach(j)) * down_scales[j]
        need = max(need, -(-h // hop))
        # the block's own input, one rate down
        h = H + blocks + max(reach[f"{p}.upsample_block0.2"], reach[f"{p}.residual_block.1"])
        H = -(-h // scales[i]) + reach[f"{p}.conv_first"]
    return max(need, H)


def _check_window_sizes(core: int, context: int, fade: Optional[int] = None) -> None:
    if core < 4 or core % 4 or context < 0 or context % 4:
        raise ValueError(f"core and context must be multiples of 4 with core >= 4, got core {core}, context {context}")
    if fade is not None and (fade < 0 or fade % 2 or fade > min(core, 2 * context)):
        raise ValueError(f"fade must be even with 0 <= fade <= min(core, 2 * context) = {min(core, 2 * context)}, got {fade}")


def window_plan(frames: Sequence[int], core: int, context: int) -> List[Tuple[int, int, int, int, int]]:
    """Rows ``(utt, in_lo, in_hi, core_lo, core_hi)``, in frames, for ``DecodeSession.convert_windowed``: utterance u of F
    frames has K = ceil(F / core) windows; window k owns the core ``[k core, min((k + 1) core, F))`` and reads ``[max(0, k
    core - context), min(F, (k + 1) core + context))``.  An utterance with K = 1 is one row, the whole utterance.  Rows are
    in utterance order, an utterance's windows ascending.  ``core`` and ``context`` are multiples of 4, ``core >= 4``."""
    core, context = int(core), int(context)
    _check_window_sizes(core, context)
    rows = []
    for u, F in enumerate(frames):
        F = int(F)
        if F < 1:
            raise ValueError(f"utterance {u} has no frames")
        for k in range(-(-F // core)):
            lo, hi = k * core, min((k + 1) * core, F)
            rows.append((u, max(0, lo - context), min(F, hi + context), lo, hi))
    return rows


def window_batches(rows: Sequence[Tuple[int, int, int, int, int]], max_batch: int = 32,
                   pad_tolerance: float = 0.125) -> List[List[int]]:
    """Batches of row indices into ``rows``: ``bucket_ragged`` over the rows' lengths ``in_hi - in_lo``, so windows of many
    utterances share batches (longest first; rows of one length in ``rows``' order, which keeps an utterance's
    consecutive windows next to each other)."""
    return list(bucket_ragged(range(len(rows)), [r[2] - r[1] for r in rows], max_batch, pad_tolerance))


def grouped_window_batches(rows: Sequence[Tuple[int, int, int, int, int]], max_batch: int = 32) -> List[List[int]]:
    """Batches of row indices into ``rows`` that hold WHOLE utterances, for ``convert_windowed(norm="utterance")``: all
    windows of an utterance sit in one batch, adjacent and ascending, so that one forward sees every row whose InstanceNorm
    sums it pools.  Utterances are packed first-fit by window count, most windows first (ties in utterance order); a
    batch is as wide as its longest row and ragged through ``lengths``.  An utterance with more windows than ``max_batch``
    raises ``ValueError``: its intermediates would have to be kept across batches, which is not built, and per-window
    statistics are never substituted silently."""
    max_batch = int(max_batch)
    by_utt = _window_groups(rows)
    batches: List[List[int]] = []
    for u in sorted(by_utt, key=lambda u: (-len(by_utt[u]), u)):
        rs = by_utt[u]
        if len(rs) > max_batch:
            raise ValueError(f"utterance {u} has {len(rs)} windows but max_batch is {max_batch}: with norm=\"utterance\" all "
                             f"windows of an utterance run in one batch - a larger core or a larger max_batch fits it")
        for chunk in batches:
            if len(chunk) + len(rs) <= max_batch:
                chunk.extend(rs)
                break
        else:
            batches.append(list(rs))
    return batches


def pool_norm_sums(s1, s2, owned: Sequence[int], lens: Sequence[int], group: Sequence[int]):
    """The numpy reference of the pool-and-scatter rule of csrc/fastsvc_normgroup.hip, float64.  ``s1``, ``s2`` (B, C): the
    sums of u and of u^2 over the columns each row OWNS; ``owned[b]`` that many columns, ``lens[b]`` the row's own valid
    columns, ``group[b]`` the index of the first row of b's group.  Returns ``(q1, q2)`` (B, C): for every row the sums of
    its group, added in ascending row order, times ``lens[b] / N`` with N the group's owned columns - so that ``q1 /
    lens[b]`` is the group's mean and ``q2 / lens[b] - mean^2`` its biased variance, whatever the row's own length.  A row
    alone in its group that owns all its columns keeps its own sums, bit for bit."""
    s1, s2 = np.asarray(s1, dtype=np.float64), np.asarray(s2, dtype=np.float64)
    B = len(group)
    q1, q2 = s1.copy(), s2.copy()
    for b in range(B):
        members = [r for r in range(B) if group[r] == group[b]]
        if members == [b] and int(owned[b]) == int(lens[b]):
            continue
        N = sum(int(owned[r]) for r in members)
        t1, t2 = np.zeros_like(s1[b]), np.zeros_like(s2[b])
        for r in members:
            t1 = t1 + s1[r]
            t2 = t2 + s2[r]
        q1[b] = t1 * float(lens[b]) / float(N)
        q2[b] = t2 * float(lens[b]) / float(N)
    return q1, q2


NORM_CHUNK = 2048             # columns of one partial sum (NORMGROUP_CHUNK of csrc/fastsvc_kernels.h)


def chunk_sums(u, lo: int, hi: int, chunk: int = NORM_CHUNK) -> np.ndarray:
    """``(n_chunks, C, 2)`` float64: sum u and sum u^2 of the columns ``[lo, hi)`` of ``u`` (C, T), cut into chunks of
    ``chunk`` columns from ``lo`` - the partial sums of csrc/fastsvc_normgroup.hip up to the order inside a chunk.  An empty
    range has no chunks."""
    u = np.asarray(u, dtype=np.float64)
    parts = [np.stack([u[:, a: min(a + chunk, hi)].sum(axis=1), (u[:, a: min(a + chunk, hi)] ** 2).sum(axis=1)], axis=-1)
             for a in range(int(lo), int(hi), int(chunk))]
    return np.stack(parts) if parts else np.zeros((0, u.shape[0], 2))


def pool_running_sums(core, look, lens: Sequence[int], slot: Sequence[int], own_lo: Sequence[int], prior: Sequence[int],
                      reset: Sequence[int], carry: Dict[int, np.ndarray], decay: Optional[Sequence[float]] = None,
                      weight: Optional[Sequence[float]] = None):
    """The numpy reference of the RUNNING pool of csrc/fastsvc_normgroup.hip (``StreamSession(norm="running")``), float64.
    Row b of one forward is a window of the stream in carry slot ``slot[b]``; ``core[b]`` and ``look[b]`` are the chunk
    sums ``(n_chunks, C, 2)`` of its core and of its look-ahead (``chunk_sums``; the look-ahead may have none), ``lens[b]``
    its valid length, ``own_lo[b]`` where its core starts in it and ``prior[b]`` what the stream holds in front of the
    core - the three in one unit, frames or columns.  ``carry[s]`` (C, 2) holds the sums of the cores of all earlier
    windows of slot s; a ``reset`` row starts its stream: it and the slot's rows behind it in the batch take the carry as
    zero without looking.  Per row, added in THIS order: the carry; the core chunks of the rows q < b of the slot,
    ascending (row, chunk); b's own core chunks, which gives the slot's new carry; b's look-ahead chunks, which gives S.
    The row's statistics are ``S * lens[b] / N`` with ``N = prior[b] + lens[b] - own_lo[b]``, every frame of the stream up
    to the row's right edge: ``[..., 0] / lens[b]`` is their mean.  The left fold makes carry and statistics the same bits
    however a stream's windows fall into forwards.

    With a FORGETTING HORIZON (``decay`` and ``weight``, one float per row, both or neither; ``running_horizon_rows`` makes
    them): the running sum is multiplied by ``decay[q]`` in front of the core chunks of EVERY row q of the fold, b's own
    included - one rounding at a fixed place, so the bits still do not depend on the forwards - and ``N = weight[b]``, in
    the unit of ``lens``.  ``decay`` all 1 and ``weight[b] = prior[b] + lens[b] - own_lo[b]`` give the bits of the call
    without them.

    Returns ``(stats, new_carry)``: per row ``(C, 2)``, or ``None`` for a PASS-THROUGH row (reset, ``own_lo == 0``: window 0
    of a stream, whose statistics stay the producer's own), and ``carry`` updated with every slot of the batch (a new
    dict)."""
    B = len(slot)
    if (decay is None) != (weight is None):
        raise ValueError("decay and weight go together")
    stats: List[Optional[np.ndarray]] = []
    new_carry = dict(carry)
    for b in range(B):
        C = np.asarray(core[b]).shape[1]
        first = min(q for q in range(B) if slot[q] == slot[b])          # (a stream that starts in this batch starts from zero)
        s = np.zeros((C, 2)) if reset[first] else np.array(carry[slot[b]], dtype=np.float64)
        for q in range(b + 1):
            if slot[q] == slot[b]:
                if decay is not None:
                    s = s * float(decay[q])
                for part in np.asarray(core[q], dtype=np.float64):
                    s = s + part
        new_carry[slot[b]] = s                               # (the slot's last row of the batch has the last word)
        if reset[b] and int(own_lo[b]) == 0:
            stats.append(None)
            continue
        for part in np.asarray(look[b], dtype=np.float64):
            s = s + part
        N = int(prior[b]) + int(lens[b]) - int(own_lo[b]) if weight is None else float(weight[b])
        stats.append(s * float(lens[b]) / float(N))
    return stats, new_carry


def check_horizon(horizon, core: int) -> Optional[float]:
    """A forgetting horizon in frames: ``None``, or a positive finite float of at least ``core`` -> ``None`` or the float."""
    if horizon is None:
        return None
    try:
        h = float(horizon)
    except (TypeError, ValueError):
        raise ValueError(f"horizon must be None or a number of frames, got {horizon!r}") from None
    if not math.isfinite(h) or h <= 0.0:
        raise ValueError(f"horizon must be positive and finite, got {horizon!r}")
    if h < int(core):
        raise ValueError(f"horizon {h:g} is shorter than the core of {int(core)} frames")
    return h


def running_horizon_rows(windows: Sequence[Tuple[int, int, int, int]], horizon: Optional[float], w_prev: Optional[float],
                         core: Optional[int] = None):
    """The host side of a forgetting horizon, pure float64: for a stream's NEXT windows ``(in_lo, in_hi,
    core_lo, core_hi)``, ascending and adjacent, and ``w_prev``, the stream's weighted frame count after the window in
    front of them (ignored when the first one is window 0, ``core_lo == 0``), returns ``(decay, weight, bound, w_new)`` -
    three lists of one float per window, as ``fastsvc_forward_running_decay`` takes them, and the count after the last.

    With c = core_hi - core_lo, la = in_hi - core_hi and H = ``horizon``: ``decay = exp(-c / H)`` (one ``math.exp`` value:
    the device multiplies by exactly this double), ``w = decay w_prev + c`` (window 0: ``w = c``, its decay is 1 and
    multiplies nothing), ``weight = w + la`` - the weighted frames the window is normalised over - and ``bound = weight /
    wmin`` with ``wmin = exp(-(core_hi - core_hi_j) / H)`` the weight of the window's lightest column: core j holds
    ``in_lo``.  ``core``: the size of the stream's full cores (every core but a stream's last is full); ``None`` takes the
    longest core of ``windows``, which is right unless they are a stream's short last window alone.  ``horizon=None`` is
    the rule without forgetting: decay 1, ``w = core_hi``, ``weight = bound = in_hi``."""
    H = None if horizon is None else float(horizon)
    if core is None and windows:
        core = max(int(w[3]) - int(w[2]) for w in windows)
    decay, weight, bound = [], [], []
    w = None if w_prev is None else float(w_prev)
    for in_lo, in_hi, lo, hi in windows:
        in_lo, in_hi, lo, hi = int(in_lo), int(in_hi), int(lo), int(hi)
        c, la = hi - lo, in_hi - hi
        if not (0 <= in_lo <= lo < hi <= in_hi and c <= core and lo % core == 0):
            raise ValueError(f"window ({in_lo}, {in_hi}, {lo}, {hi}) is not a window of cores of {core} frames")
        if lo == 0:
            d, w = 1.0, float(c)
        else:
            if w is None:
                raise ValueError("w_prev is needed in front of a window that is not a stream's first")
            d = 1.0 if H is None else math.exp(-c / H)
            w = d * w + c
        hi_j = (in_lo // core + 1) * core                    # (the right edge of the core that holds in_lo)
        wmin = 1.0 if H is None or hi_j >= hi else math.exp(-(hi - hi_j) / H)
        decay.append(d)
        weight.append(w + la)
        bound.append(max((w + la) / wmin, w + la))
    return decay, weight, bound, w


def _window_groups(rows):
    """utterance -> its row indices, ascending window."""
    by_utt: Dict[int, List[int]] = {}
    for r, row in enumerate(rows):
        by_utt.setdefault(int(row[0]), []).append(r)
    for u, rs in by_utt.items():
        rs.sort(key=lambda r: rows[r][3])
        for a, b in zip(rs, rs[1:]):
            if rows[a][4] != rows[b][3]:
                raise ValueError(f"utterance {u}: the cores of its windows do not follow each other")
        if rows[rs[0]][3] != 0:
            raise ValueError(f"utterance {u}: its first core does not start at frame 0")
    return by_utt


def _check_fade(rows, by_utt, hop: int, fade: int) -> int:
    """``fade`` against the rows: even, at most the core, and both windows of every boundary cover its zone.  -> half a
    zone in samples."""
    fade = int(fade)
    if fade < 0 or fade % 2:
        raise ValueError(f"fade must be even and >= 0, got {fade}")
    half = fade * hop // 2
    for u, rs in by_utt.items():
        F = rows[rs[-1]][4]
        for a, b in zip(rs, rs[1:]):
            edge = rows[a][4]
            if fade > rows[a][4] - rows[a][3]:
                raise ValueError(f"fade {fade} is longer than the core of {rows[a][4] - rows[a][3]} frames")
            if rows[b][1] * hop > edge * hop - half or rows[a][2] * hop < min(edge * hop + half, F * hop):
                raise ValueError(f"fade {fade} needs {fade // 2} frames of context on both sides of frame {edge} of "
                                 f"utterance {u}")
    return half


def stitch_windows(ys: Sequence[np.ndarray], rows: Sequence[Tuple[int, int, int, int, int]], hop: int,
                   fade: int) -> List[np.ndarray]:
    """The numpy reference of the stitch, float64: ``ys[r]`` is the waveform of row r of ``rows`` (``window_plan``), its
    ``(in_hi - in_lo) * hop`` samples; returns one float64 array per utterance (ascending utterance).  Outside the fade
    zones, sample t of an utterance is the owning window's sample.  Around every interior boundary b = k core hop, with
    fh = fade hop, the zone ``[b - fh / 2, b + fh / 2)`` (clipped to the utterance) holds ``(1 - w) y_{k-1} + w y_k`` with
    ``w = (t - (b - fh / 2) + 0.5) / fh``: the two weights sum to 1 and neither reaches 0 or 1.  ``fade`` is even, ``0 <=
    fade <= min(core, 2 context)``; ``fade = 0`` is plain concatenation of the cores.  PCM-16 of the result is
    ``to_pcm16``'s rule on these float64 values; its float32 form is their rounding (``astype(np.float32)``)."""
    hop = int(hop)
    by_utt = _window_groups(rows)
    half = _check_fade(rows, by_utt, hop, fade)
    fh = 2 * half
    out = []
    for u in sorted(by_utt):
        rs = by_utt[u]
        T = rows[rs[-1]][4] * hop
        res = np.empty(T, dtype=np.float64)
        for r in rs:
            _, in_lo, in_hi, lo, hi = rows[r]
            y = np.asarray(ys[r]).reshape(-1)
            if y.size < (in_hi - in_lo) * hop:
                raise ValueError(f"row {r}: {y.size} samples, {(in_hi - in_lo) * hop} expected")
            res[lo * hop: hi * hop] = y[(lo - in_lo) * hop: (hi - in_lo) * hop]
        for a, b in zip(rs, rs[1:]):
            z0 = rows[a][4] * hop - half
            z1 = min(z0 + fh, T)
            if z1 <= z0:
                continue
            w = (np.arange(z1 - z0, dtype=np.float64) + 0.5) / fh
            ya = np.asarray(ys[a], dtype=np.float64).reshape(-1)[z0 - rows[a][1] * hop: z1 - rows[a][1] * hop]
            yb = np.asarray(ys[b], dtype=np.float64).reshape(-1)[z0 - rows[b][1] * hop: z1 - rows[b][1] * hop]
            with np.errstate(invalid="ignore"):
                res[z0:z1] = (1.0 - w) * ya + w * yb
        out.append(res)
    return out


NONE, STAGE, FROM_STAGE, FROM_Y, SKIP = range(5)     # a window side's mode in ``fastsvc_window_stitch`` (``STITCH_*``)


def _emit_rows(specs, hop: int, half: int, width: int, grow_left, grow_right):
    """The stitch layout dict of one batch (see ``stitch_layout``) from its rows' ``(u, T, in_lo, in_hi, core_lo, core_hi,
    left_mode, right_mode, left_src, right_src)``: window of utterance / stream ``u``, which has ``T`` samples; the window in
    frames.  The run a row writes is its core, moved OUT by half a zone on a side whose mode is in ``grow_left`` /
    ``grow_right`` (the row writes that zone), IN by half a zone on any other side that has a neighbour, and clipped to
    the utterance; the runs lie back to back in the batch's buffer."""
    d = {key: [] for key in ("n_samples", "core_lo", "core_hi", "left_mode", "right_mode", "left_src", "right_src",
                             "dst_off", "utt", "runs")}
    pos = 0
    for u, T, in_lo, in_hi, lo, hi, lm, rm, ls, rs in specs:
        t_lo = lo * hop - half if lm in grow_left else min(lo * hop + half, T) if lm != NONE else lo * hop
        t_hi = min(hi * hop + half, T) if rm in grow_right else hi * hop - half if rm != NONE else hi * hop
        t_hi = max(t_hi, t_lo)
        d["n_samples"].append((in_hi - in_lo) * hop)
        d["core_lo"].append((lo - in_lo) * hop)
        d["core_hi"].append((hi - in_lo) * hop)
        d["left_mode"].append(lm)
        d["right_mode"].append(rm)
        d["left_src"].append(ls)
        d["right_src"].append(rs)
        d["dst_off"].append(pos)
        d["utt"].append(u)
        d["runs"].append((u, t_lo, t_hi))
        pos += -(-(t_hi - t_lo) // 8) * 8                # (every run starts on a 16-byte boundary of both destinations)
    d["total"], d["width"], d["half"] = pos, width, half
    return d


def stitch_layout(rows: Sequence[Tuple[int, int, int, int, int]], batches: Sequence[Sequence[int]], hop: int, fade: int):
    """How ``engine.window_stitch`` resolves every fade zone when the rows run batch by batch, in ``batches``' order:
    ``(per_batch, stage_elems)``.  ``per_batch[k]`` is a dict of per-row lists for batch k (in the batch's row order) -
    ``n_samples``, ``core_lo``, ``core_hi`` (samples of the row), ``left_mode`` / ``right_mode`` / ``left_src`` /
    ``right_src`` (see ``fastsvc_window_stitch``), ``dst_off`` (the rows' written runs laid back to back in a per-batch
    buffer of ``total`` samples), ``utt``, and ``runs``: per row ``(utt, t_lo, t_hi)``, the samples of the utterance it
    writes - plus ``width`` (the batch's row length in samples) and ``half``.  Both windows of a boundary in one batch: the
    left one blends straight from the forward's output.  In different batches: the one that runs first stages its zone
    samples in a slot of ``2 half`` floats, the later one blends; ``stage_elems`` is the size of that buffer."""
    hop = int(hop)
    by_utt = _window_groups(rows)
    half = _check_fade(rows, by_utt, hop, fade)
    fh = 2 * half
    where = {}
    for k, chunk in enumerate(batches):
        for j, r in enumerate(chunk):
            if r in where:
                raise ValueError(f"row {r} is in two batches")
            where[r] = (k, j)
    widths = [max(rows[r][2] - rows[r][1] for r in chunk) * hop for chunk in batches]
    lmode, rmode, lsrc, rsrc = {}, {}, {}, {}
    slots = 0
    for u, rs in by_utt.items():
        if any(r not in where for r in rs):
            if all(r not in where for r in rs):
                continue
            raise ValueError(f"utterance {u}: only some of its windows are in the batches")
        if not half:
            continue
        for a, b in zip(rs, rs[1:]):
            (ka, ja), (kb, jb) = where[a], where[b]
            z0 = rows[a][4] * hop - half                 # the zone's first sample, in the utterance
            if ka == kb:
                rmode[a], rsrc[a] = FROM_Y, jb * widths[kb] + (z0 - rows[b][1] * hop)
                lmode[b] = SKIP
            elif ka < kb:
                rmode[a], rsrc[a] = STAGE, slots * fh
                lmode[b], lsrc[b] = FROM_STAGE, slots * fh
                slots += 1
            else:
                lmode[b], lsrc[b] = STAGE, slots * fh
                rmode[a], rsrc[a] = FROM_STAGE, slots * fh
                slots += 1
    # (whichever window of a boundary blends it, from the stage or from the forward's output, writes the zone)
    blends = (FROM_STAGE, FROM_Y)
    T = {u: rows[rs[-1]][4] * hop for u, rs in by_utt.items()}
    per_batch = []
    for k, chunk in enumerate(batches):
        specs = []
        for r in chunk:
            u, in_lo, in_hi, lo, hi = rows[r]
            specs.append((u, T[u], in_lo, in_hi, lo, hi, lmode.get(r, NONE), rmode.get(r, NONE), lsrc.get(r, 0), rsrc.get(r, 0)))
        per_batch.append(_emit_rows(specs, hop, half, widths[k], blends, blends))
    return per_batch, slots * fh


def stream_ready_rows(seen: int, ended: bool, core: int, context: int, done: int) -> List[Tuple[int, int, int, int]]:
    """The windows of a live stream that can run now: rows ``(in_lo, in_hi, core_lo, core_hi)``, in frames, for the windows
    ``done, done + 1, ...`` (``done`` windows ran before) that are READY when ``seen`` frames have arrived.  Window k is
    ready when ``(k + 1) core + context`` frames have arrived - everything it reads is there - or the stream has ended
    and ``k core < seen``; it reads ``[max(0, k core - context), min(seen, (k + 1) core + context))``.  Whatever the push
    schedule, a stream's rows are, one after the other, exactly ``window_plan([F], core, context)`` for its final length
    F: a window that runs before the end has all its context, one that runs at the end is clipped by F as the plan
    clips it."""
    seen, core, context, k = int(seen), int(core), int(context), int(done)
    rows = []
    while seen >= (k + 1) * core + context or (ended and k * core < seen):
        lo, hi = k * core, min((k + 1) * core, seen)
        rows.append((max(0, lo - context), min(seen, (k + 1) * core + context), lo, hi))
        k += 1
    return rows


def stream_ring_frames(core: int, context: int, max_push: int) -> int:
    """Frames a live stream retains on the device: ``core + 2 context + max_push`` rounded up to a multiple of 4.  After
    every push all ready windows run, so the oldest window that has not run, k, lacks a frame: ``seen < (k + 1) core +
    context``.  The next push brings at most ``max_push`` frames, and window k reads from ``k core - context``: the frames
    still needed span less than ``core + 2 context + max_push``, so a ring of that many never overwrites one."""
    return -(-(int(core) + 2 * int(context) + int(max_push)) // 4) * 4


LOUDNESS_HALF_FRAME = 1024      # samples a loudness frame reads on either side of its centre (n_fft 2048)


def stream_loudness_lag(hop: int) -> int:
    """Frames a live stream's loudness runs behind its audio: ``ceil(1024 / hop) - 1`` (6 at hop 160).  Frame f is the
    2048 samples centred on ``f hop``, so it reads samples up to ``f hop + 1023`` and is FINAL once ``seen hop >= f hop +
    1024``: with ``seen`` frames of audio the frames ``[0, seen - lag)`` are."""
    hop = int(hop)
    if hop < 1:
        raise ValueError(f"hop must be >= 1, got {hop}")
    return -(-LOUDNESS_HALF_FRAME // hop) - 1


def stream_final_frames(seen: int, ended: bool, hop: int) -> int:
    """Frames of a live stream whose loudness is final when ``seen`` frames of audio have arrived: ``max(0, seen - lag)``
    before the end, and all ``seen`` of them once the stream has ended (the last ones read reflected samples)."""
    seen = int(seen)
    return seen if ended else max(0, seen - stream_loudness_lag(hop))


def stream_loudness_ring_frames(core: int, context: int, max_push: int, hop: int) -> int:
    """Frames a live stream retains on the device with ``loudness="audio"``, ``lag = stream_loudness_lag(hop)``: the larger
    of two bounds, rounded up to a multiple of 4.

    FRAMES.  After every push all windows whose frames are final have run, so the oldest window that has not run, k, lacks
    a FINAL frame: ``final < (k + 1) core + context``, and ``seen <= final + lag``.  The next push brings at most
    ``max_push`` frames and window k reads from ``k core - context``: the frames still needed plus the next chunk span
    less than ``core + 2 context + max_push + lag`` - ``stream_ring_frames(core, context, max_push + lag)``.

    SAMPLES.  The audio ring holds ``cap hop`` samples, sample p at ``p % (cap hop)``.  The oldest frame that is not
    final, ``f0 >= seen - lag``, reads from sample ``f0 hop - 1024``; after the next push the ring ends at ``(seen +
    max_push) hop``.  So ``cap hop >= (max_push + lag) hop + 1024`` keeps every sample a frame still reads - the binding
    bound when ``core + 2 context`` is small."""
    core, context, max_push, hop = int(core), int(context), int(max_push), int(hop)
    lag = stream_loudness_lag(hop)
    frames = stream_ring_frames(core, context, max_push + lag)
    samples = -(-((max_push + lag) * hop + LOUDNESS_HALF_FRAME) // hop)
    return -(-max(frames, samples) // 4) * 4


def stream_tracked_frames(final: int, ended: bool, track_lag: int) -> int:
    """Frames of a live stream whose TRACKED F0 is final when ``final`` frames have their candidates (``f0_track=F0Track(lag=
    track_lag)``): frame f needs the frames up to ``f + track_lag``, so ``max(0, final - track_lag)`` before the end and all of
    them once the stream has ended."""
    final = int(final)
    return final if ended else max(0, final - int(track_lag))


def stream_track_ring_frames(core: int, context: int, max_push: int, hop: int, track_lag: int) -> int:
    """``stream_loudness_ring_frames`` for a session that tracks its F0 ``track_lag`` frames behind the final frames.  The
    FRAMES bound: the oldest window that has not run lacks a TRACKED frame, ``tracked < (k + 1) core + context``, and ``seen <=
    tracked + lag + track_lag`` - ``stream_ring_frames(core, context, max_push + lag + track_lag)``; the candidates and
    backpointers a frame's trace reads, the ``track_lag`` frames after it, lie inside that.  The SAMPLES bound is unchanged:
    candidates are made when a frame is final, as the F0 was."""
    core, context, max_push, hop = int(core), int(context), int(max_push), int(hop)
    lag = stream_loudness_lag(hop)
    frames = stream_ring_frames(core, context, max_push + lag + int(track_lag))
    samples = -(-((max_push + lag) * hop + LOUDNESS_HALF_FRAME) // hop)
    return -(-max(frames, samples) // 4) * 4


class StreamRow(NamedTuple):
    """Window ``k`` of the live stream in slot ``stream`` as a row of a forward: it reads the stream's frames ``[in_lo,
    in_hi)``, owns ``[core_lo, core_hi)`` of them, and is the stream's ``last`` window or not.  The row type of
    ``stream_push_rows``, of ``StreamStitchLayout.batch`` (which also takes the plain 7-tuple) and of a session's trace."""
    stream: int
    k: int
    in_lo: int
    in_hi: int
    core_lo: int
    core_hi: int
    last: bool

    frames = property(lambda r: r.in_hi - r.in_lo, doc="frames the row holds")
    own_lo = property(lambda r: r.core_lo - r.in_lo, doc="where its core starts, in frames of the row")
    own_hi = property(lambda r: r.core_hi - r.in_lo, doc="where its core ends, in frames of the row")


class StreamStitchLayout:
    """``stitch_layout``, incrementally: the streams' rows arrive batch by batch (a ``StreamSession.push`` is one batch
    per forward) and nobody knows the final length yet.  ``batch(rows, seen)`` returns for these rows what
    ``stitch_layout(rows_of_the_whole_streams, batches_so_far_and_later, hop, fade)`` puts into that batch's dict - the
    same ``n_samples``, ``core_lo``, ``core_hi``, modes, ``FROM_Y`` sources, ``dst_off``, ``runs``, ``total``, ``width``,
    ``half`` - except for where the staged zones live: every stream has TWO slots of ``2 half`` floats (``stage_elems``
    floats in all, allocated once).  A stream has at most one zone staged at a time, and a batch reads at most one slot
    of a stream (its first window of the batch, ``FROM_STAGE``) and writes at most one (its last, ``STAGE``) - in rows
    of one launch that nothing orders.  So a ``STAGE`` always takes the slot the stream did NOT write last: it is never
    the slot a row of the same batch reads.  ``pending[s]`` is the window of stream s whose right zone is staged and
    waits for its neighbour, ``written[s]`` the slot (0 / 1) it is in.

    A row is a ``StreamRow``, or the plain tuple ``(stream, k, in_lo, in_hi, core_lo, core_hi, last)``: window k of the
    stream, and whether it is the stream's last one.  Rows of a stream must come in window order; ``seen[stream]`` is
    the stream's frame count (its final one when it has ended), which clips a zone the stream ends in."""

    def __init__(self, n_streams: int, hop: int, fade: int):
        fade = int(fade)
        if fade < 0 or fade % 2:
            raise ValueError(f"fade must be even and >= 0, got {fade}")
        self.n_streams, self.hop, self.half = int(n_streams), int(hop), fade * int(hop) // 2
        self.stage_elems = self.n_streams * 2 * 2 * self.half
        self.pending: List[Optional[int]] = [None] * self.n_streams
        self.written = [1] * self.n_streams              # (the slot a stream staged into last; its first goes to slot 0)

    def reset(self, stream: int) -> None:
        """A new stream takes the slot: nothing is staged."""
        self.pending[stream] = None

    def slot(self, stream: int, which: int) -> int:
        """First element of slot ``which`` (0 / 1) of the stream."""
        return (2 * stream + which) * 2 * self.half

    def batch(self, rows, seen):
        hop, half = self.hop, self.half
        rows = [r if isinstance(r, StreamRow) else StreamRow(*r) for r in rows]
        where = {(r.stream, r.k): j for j, r in enumerate(rows)}
        if len(where) != len(rows):
            raise ValueError("a window is in the batch twice")
        width = max(r.frames for r in rows) * hop
        pending, written = list(self.pending), list(self.written)
        specs = []
        for r in rows:
            s, k = r.stream, r.k
            lm = rm = NONE
            ls = rs = 0
            if half and k > 0:
                if (s, k - 1) in where:
                    if where[(s, k - 1)] > where[(s, k)]:
                        raise ValueError(f"stream {s}: window {k} comes before window {k - 1}")
                    lm = SKIP
                elif pending[s] == k - 1:
                    lm, ls = FROM_STAGE, self.slot(s, written[s])
                    pending[s] = None
                else:
                    raise ValueError(f"stream {s}: window {k} runs, but window {k - 1} has not staged its fade zone")
            if half and not r.last:
                if (s, k + 1) in where:
                    j = where[(s, k + 1)]                # (the zone's other half is in the next window's row of this forward)
                    rm, rs = FROM_Y, j * width + (r.core_hi * hop - half - rows[j].in_lo * hop)
                else:
                    written[s] ^= 1                      # (not the slot the stream's first row of this batch may read)
                    rm, rs = STAGE, self.slot(s, written[s])
                    pending[s] = k
            specs.append((s, int(seen[s]) * hop, r.in_lo, r.in_hi, r.core_lo, r.core_hi, lm, rm, ls, rs))
        # (a stream's windows run in order: the left zone is written only when blended from the stage, the right one only
        # when blended from the forward's output)
        d = _emit_rows(specs, hop, half, width, (FROM_STAGE,), (FROM_Y,))
        self.pending, self.written = pending, written    # (only a batch that was laid out whole changes the state)
        return d


stream_stitch_layout = StreamStitchLayout           # (the incremental counterpart of ``stitch_layout``, under its name)


@dataclass
class _Stream:
    """What the host knows of one open stream of a ``StreamSession``.  Three of the fields say which entry of a two-entry
    record on the device is current: a launch reads entry p and writes entry ``p ^ 1``, and the field flips once that
    launch is enqueued."""
    id: int                          # what ``open`` returned
    slot: int                        # its row of every per-stream device buffer
    emb: bool                        # opened with a speaker embedding
    seed: int                        # keys the excitation's noise
    stats: Optional[tuple]           # ([mean, std] of the source's log F0, of the target's), or None: no F0 shift
    from_audio: bool = False         # the session makes the loudness (loudness="audio")
    seen: int = 0                    # frames that have arrived
    first: bool = True               # nothing has arrived: the sine phase starts at 0
    parity: int = 0                  # the phase record's current entry (flips with every stream_push; f0="audio": stream_f0)
    final: int = 0                   # loudness="audio": frames whose loudness is final
    loud_parity: int = 0             # the peak record's current entry (flips with every stream_loudness)
    done: int = 0                    # windows that ran
    norm_parity: int = 0             # norm="running": the carry record's current entry (flips with every forward)
    norm_w: float = 0.0              # ... and the weighted frames it holds (``running_horizon_rows``' w)
    totals: Optional[dict] = None    # a checked session: what its windows' reports add up to since ``open``
    running: Optional[tuple] = None  # RunningF0Stats' six constants (m_p, s_p, n0, g, m_t, s_t): the record at ``parity`` is its state
    track: bool = False              # the session tracks its F0 (f0_track): the excitation exists for the tracked frames only
    tracked: int = 0                 # ... frames whose tracked F0 and excitation are made (``parity`` flips with a call that makes some)
    track_parity: int = 0            # the tracker record's current entry (flips with every call that has newly final frames)

    @property
    def complete(self) -> int:
        """Frames whose features are complete - what a window is ready by: all that arrived or, when the session makes the
        loudness, those whose loudness is final or, when it tracks the F0, those whose tracked F0 is."""
        return self.tracked if self.track else self.final if self.from_audio else self.seen


def check_stream_chunks(chunks, end, open_ids, channels: int, hop: int, max_push: int, loudness: str = "given",
                        f0: str = "given"):
    """Everything ``StreamSession.push`` refuses, on the host alone: ``chunks = {id: dict(ppg, f0, lft | audio)}`` and the
    ids in ``end`` against the open ids, the ppg channels, ``hop``, ``max_push`` and the session's ``loudness`` and ``f0``
    modes.  Returns ``(parts, ids, end)``: ``parts[id] = (n, ppg (n, C), f0 (n,), lft or audio (n hop,))`` as numpy arrays
    in the order of ``chunks``, ``ids`` every id of ``chunks`` and ``end`` once, in that order, and ``end`` as a list of
    ints.  With ``f0="audio"`` (which needs ``loudness="audio"``) a chunk is ``dict(ppg, audio)``: an ``f0`` key is
    refused like any other mode's array, and ``parts[id][2]`` is None.  A ``ValueError`` names the first thing wrong;
    nothing is changed."""
    C, hop = int(channels), int(hop)
    sig, other = ("audio", "lft") if loudness == "audio" else ("lft", "audio")     # (the chunk's third array, and the other mode's)
    own_f0 = f0 == "audio"
    if own_f0 and loudness != "audio":
        raise ValueError("f0=\"audio\" needs loudness=\"audio\": the audio ring exists only there")
    end = [int(i) for i in end]
    for sid in list(chunks) + end:
        if sid not in open_ids:
            raise ValueError(f"stream {sid} is not open (unknown, or it has ended)")
    if len(set(end)) != len(end):
        raise ValueError("a stream is listed twice in end")
    parts = {}
    for sid, ch in chunks.items():
        try:
            ppg, lft = (np.asarray(ch[key]) for key in ("ppg", sig))
            pitch = None if own_f0 else np.asarray(ch["f0"])
            stray, stray_f0 = other in ch, own_f0 and "f0" in ch
        except (KeyError, TypeError) as e:
            raise ValueError(f"stream {sid}: a chunk is a dict with ppg{'' if own_f0 else ', f0'} and {sig}") from e
        if stray:
            raise ValueError(f"stream {sid}: the session was built with loudness=\"{loudness}\": a chunk carries {sig}, not {other}")
        if stray_f0:
            raise ValueError(f"stream {sid}: the session was built with f0=\"audio\": it makes the F0 from the audio, a chunk carries none")
        if ppg.ndim != 2 or ppg.shape[1] != C:
            raise ValueError(f"stream {sid}: ppg must be (n, {C}), got {ppg.shape}")
        n = int(ppg.shape[0])
        if n > max_push:
            raise ValueError(f"stream {sid}: {n} frames in one push, max_push is {max_push}")
        if pitch is not None and pitch.shape not in ((n,), (n, 1)):
            raise ValueError(f"stream {sid}: f0 must be ({n},) or ({n}, 1), got {pitch.shape}")
        if lft.shape not in ((n * hop,), (n * hop, 1)):
            raise ValueError(f"stream {sid}: {sig} must be ({n * hop},) or ({n * hop}, 1), got {lft.shape}")
        parts[sid] = (n, ppg, None if pitch is None else pitch.reshape(-1), lft.reshape(-1))
    return parts, list(dict.fromkeys(list(chunks) + end)), end


def stream_push_rows(streams: Sequence[_Stream], ended, core: int, context: int, running: bool = False,
                     horizon: Optional[float] = None):
    """The forwards' rows of one ``StreamSession.push``, planned on the host: ``streams`` are the records of the streams
    the push names, in slot order, ``ended`` the ids that end with it.  Returns ``(rows, forget)``.

    ``rows``: a ``StreamRow`` for every window that is ready now (``stream_ready_rows`` by the stream's ``complete``
    frames), stream after stream and a stream's ascending from window ``done`` - the order the forwards take them in;
    ``last`` is set on the window an ended stream stops in.

    ``forget``, with ``running`` (``norm="running"``): per row of a stream with an embedding - they all have one, or none
    has - ``(decay, weight, bound, w)``, ``running_horizon_rows``' three for the stream's ready windows behind its
    ``norm_w`` (one call per stream; ``horizon=None`` forgets nothing) and the weighted frames ``w`` the stream carries
    once the row has run.  Otherwise empty.

    Reads the records and changes none: the caller sets ``done`` to ``k + 1`` of a stream's last row, and ``norm_w`` to a
    row's ``w`` when its forward is enqueued."""
    rows: List[StreamRow] = []
    forget = []
    for st in streams:
        end, complete, k = st.id in ended, st.complete, st.done
        ready = stream_ready_rows(complete, end, core, context, k)
        for in_lo, in_hi, lo, hi in ready:
            rows.append(StreamRow(st.slot, k, in_lo, in_hi, lo, hi, end and hi == complete))
            k += 1
        if ready and running and st.emb:
            w = st.norm_w
            decay, weight, bound, _ = running_horizon_rows(ready, horizon, w, core)
            for (_, _, lo, hi), d, wt, bd in zip(ready, decay, weight, bound):
                w = d * w + (hi - lo) if lo else float(hi)       # (``running_horizon_rows``' w, after every window)
                forget.append((d, wt, bd, w))
    return rows, forget


def stream_check_spans(rows: Sequence[StreamRow], hop: int, half: int) -> Tuple[List[int], List[int]]:
    """The samples every window row of a stream forward CONTRIBUTES, ``(lo, hi)`` per row, in samples of the row - what a
    checked ``StreamSession`` judges a row on (``engine.stream_check``): the run it emits, the fade zone it stages for the
    stream's next window and the zone a neighbour row blends from it, and nothing else.  With ``half`` the half zone in
    samples (``fade * hop // 2``), window k of a stream contributes

        lo = max(0, own_lo hop - (half if k > 0 else 0)),    hi = min(frames hop, own_hi hop + (0 if last else half))

    - its core, grown by half a zone on every side that has a neighbour, clipped to the row (a stream may end inside a
    zone).  A non-finite sample of a row reaches ``stitch_windows``' result exactly when it lies in the row's span; the
    context outside it is read by the forward alone."""
    hop, half = int(hop), int(half)
    lo = [max(0, r.own_lo * hop - (half if r.k > 0 else 0)) for r in rows]
    hi = [min(r.frames * hop, r.own_hi * hop + (0 if r.last else half)) for r in rows]
    return lo, hi


def stream_rerun_rows(rows: Sequence[StreamRow], flagged) -> List[int]:
    """The rows of one stream forward a checked ``StreamSession`` runs again when the rows ``flagged`` (indices into
    ``rows``) are not finite: every row, in the forward's order, of every stream that has a flagged row.  A stream's windows
    of one forward chain through its carry record - the entry the forward leaves behind holds all of them - so they go
    together; rows of other streams never do: their carry must stay the one their delivered samples came from."""
    hit = {rows[int(i)].stream for i in flagged}
    return [j for j, r in enumerate(rows) if r.stream in hit]


def write_wav(path: str, y, sample_rate: int) -> None:
    """PCM-16 mono wav.  A float waveform goes through ``to_pcm16``; an int16 array (``DecodeSession.convert``) is
    written as it is."""
    if isinstance(y, np.ndarray) and y.dtype == np.int16:
        pcm = np.ascontiguousarray(y).reshape(-1)
    else:
        pcm = to_pcm16(y)
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(sample_rate))
        w.writeframes(pcm.tobytes())


def load_features(path: str) -> Dict[str, np.ndarray]:
    """One utterance's dump: {"f0": (F,1), "ppg": (F,C), "lft": (T,1)[, "spk_emb", "wave"]}."""
    if path.endswith(".npz"):
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    if path.endswith(".h5"):
        try:
            import h5py                     # optional; the reference's own container
        except ImportError as e:            # pragma: no cover - not installed in the build image
            raise RuntimeError("reading .h5 dumps needs h5py; convert to .npz with the same keys") from e
        with h5py.File(path, "r") as f:     # pragma: no cover
            return {k: f[k][()] for k in f.keys()}
    raise ValueError(f"unsupported feature container: {path}")


class _PinnedSet:
    """One batch worth of page-locked staging (inputs up, waveforms down), grown on demand and reused."""

    def __init__(self):
        self.bufs: Dict[str, torch.Tensor] = {}

    def get(self, key: str, shape) -> torch.Tensor:
        need = math.prod(shape)
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < need:
            buf = torch.empty(max(need, 1), dtype=torch.float32, pin_memory=True)
            self.bufs[key] = buf
        return buf[:need].view(*shape) if len(shape) > 1 else buf[:need]

    def samples(self, total: int, pcm16: bool, at: int = 0):
        """Room for the ``total`` samples of one download from word ``at`` of buffer "w" -> (the samples, the word behind
        them).  int16 samples are a view of the float32 words, so one buffer serves both kinds and every batch starts on a
        word boundary.  (A buffer that holds earlier batches, ``at > 0``, has to be large enough already: growing drops them.)"""
        end = at + ((total + 1) // 2 if pcm16 else total)
        words = self.get("w", (end,))
        if at:
            words = words[at:]
        return (words.view(torch.int16)[:total] if pcm16 else words), end


def _one_behind(stream, down, steps, enqueue, take) -> None:
    """The download pipeline of a pass.  For every entry of ``steps``, ``enqueue(pinned, *step)`` puts the step on
    ``stream``, whole - its downloads, into the page-locked set ``pinned = down[j & 1]``, last - and returns the
    arguments with which ``take`` copies the results out of the set.  ``take`` runs one step behind, once the event
    recorded behind the step's downloads has passed: while step j computes, step j - 1 is taken out, before step j + 1
    reuses its set.  Every step has been taken out when this returns."""
    behind = None
    for j, step in enumerate(steps):
        taken = enqueue(down[j & 1], *step)
        done = torch.cuda.Event()
        done.record(stream)
        if behind is not None:
            behind[0].synchronize()
            take(*behind[1])
        behind = (done, taken)
    if behind is not None:
        behind[0].synchronize()
        take(*behind[1])


def _stitch_to_host(y, lay, stage, pcm16: bool, pinned: _PinnedSet, report=None, at: int = 0):
    """One forward's window rows ``y`` stitched by the layout dict ``lay`` (``stitch_layout``, ``StreamStitchLayout``) into
    a new packed device buffer, int16 or float32, and its download queued on the current stream into ``pinned`` from word
    ``at`` -> ``pinned.samples``' pair: the ``lay["total"]`` samples there, row r's run at ``lay["dst_off"][r]``, and the word
    behind them.  ``report``: see ``engine.window_stitch``."""
    from .engine import window_stitch
    total = lay["total"]
    packed = torch.empty(max(total, 1), dtype=torch.int16 if pcm16 else torch.float32, device=y.device)
    window_stitch(y.view(len(lay["n_samples"]), lay["width"]), lay["n_samples"], lay["core_lo"], lay["core_hi"], lay["half"],
                  lay["left_mode"], lay["right_mode"], lay["left_src"], lay["right_src"], lay["dst_off"], stage=stage,
                  out_pcm=packed if pcm16 else None, out_float=None if pcm16 else packed, utt=lay["utt"], report=report)
    host, end = pinned.samples(total, pcm16, at)
    if total:
        host.copy_(packed[:total], non_blocking=True)
    return host, end


@torch.no_grad()
def decode_utterances(model, feats: Sequence[Dict[str, np.ndarray]], signal_generator, device,
                      trg_emb=None, src_f0_stats: Optional[Sequence[Sequence[float]]] = None,
                      trg_f0_stats: Optional[Sequence[float]] = None, max_batch: int = 32,
                      pad_tolerance: float = 0.125) -> List[np.ndarray]:
    """Waveforms (float32, (T,)) for every utterance, in order.

    model             ``FastSVCGenerator`` (eval, weight-norm removed or not) on ``device``
    feats             per utterance: time-major ``f0 (F,1)``, ``ppg (F,C)``, ``lft (T,1)``
    signal_generator  ``svcc23_fastsvc_amd.SignalGenerator`` (device excitation)
    trg_emb           target-speaker embedding (E,) / (1,E), or None
    src_f0_stats      per utterance [mean, std] of its SOURCE speaker's log F0, or None for no shift
    trg_f0_stats      [mean, std] of the target speaker (the reference forces both stds to 1)

    A three-stage pipeline over the length-bucketed batches, so that the GPU is the only thing the pass waits for:
    while batch k computes, the host assembles batch k+1 in page-locked memory (numpy row copies, F0 shift) and
    uploads it on a copy stream, and takes batch k-1's waveforms out of the page-locked buffer they were downloaded
    to.  Two staging sets each way; one at a time it was host-bound 5:1 (tools/decode_throughput.py)."""
    hop = signal_generator.hop_size
    frames = [int(np.asarray(u["ppg"]).shape[0]) for u in feats]
    out: List[Optional[np.ndarray]] = [None] * len(feats)
    if not feats:
        return []
    device = torch.device(device)
    emb_row = None
    if trg_emb is not None:
        emb_row = torch.as_tensor(np.asarray(trg_emb), dtype=torch.float32).reshape(1, -1).to(device)
    batches = list(bucket_ragged(range(len(feats)), frames, max_batch, pad_tolerance))
    cuda = device.type == "cuda"
    up_sets, down_sets = [_PinnedSet(), _PinnedSet()], [_PinnedSet(), _PinnedSet()]
    copy_stream = torch.cuda.Stream(device) if cuda else None
    up_free = [None, None]                    # event: the upload that last read this input set is done
    staged = {}

    def stage(k: int) -> None:
        chunk = batches[k]
        fmax, B = frames[chunk[0]], len(chunk)
        C = int(np.asarray(feats[chunk[0]]["ppg"]).shape[1])
        slot = k & 1
        if cuda and up_free[slot] is not None:
            up_free[slot].synchronize()
        shapes = {"ppg": (B, C, fmax), "f0": (B, 1, fmax), "lft": (B, 1, fmax * hop)}
        if cuda:
            host = {key: up_sets[slot].get(key, shp) for key, shp in shapes.items()}
        else:
            host = {key: torch.empty(shp, dtype=torch.float32) for key, shp in shapes.items()}
        hp, hf, hl = (host[key].numpy() for key in ("ppg", "f0", "lft"))
        for j, i in enumerate(chunk):
            u, n = feats[i], frames[i]
            hp[j, :, :n] = np.asarray(u["ppg"], dtype=np.float32).T
            hp[j, :, n:] = 0
            f = np.asarray(u["f0"], dtype=np.float64).reshape(-1)
            if src_f0_stats is not None and trg_f0_stats is not None:
                f = F0Statistics().convert(f, src_f0_stats[i], trg_f0_stats)
            hf[j, 0, :n] = f
            hf[j, 0, n:] = 0
            hl[j, 0, : n * hop] = np.asarray(u["lft"], dtype=np.float32).reshape(-1)[: n * hop]
            hl[j, 0, n * hop:] = 0
        if not cuda:
            staged[k] = (host["ppg"], host["f0"], host["lft"], None)
            return
        compute = torch.cuda.current_stream(device)
        with torch.cuda.stream(copy_stream):
            dev = {key: host[key].to(device, non_blocking=True) for key in shapes}
            ready = torch.cuda.Event()
            ready.record(copy_stream)
        for t in dev.values():
            t.record_stream(compute)            # allocated on the copy stream's pool, consumed on the compute stream
        up_free[slot] = ready
        staged[k] = (dev["ppg"], dev["f0"], dev["lft"], ready)

    pending = {}

    def compute(k: int) -> None:
        chunk = batches[k]
        ppg, f0, lft, ready = staged.pop(k)
        if ready is not None:
            torch.cuda.current_stream(device).wait_event(ready)
        sine = signal_generator(f0)
        emb = None if emb_row is None else emb_row.expand(len(chunk), -1).contiguous()
        y = model(ppg, sine, lft, emb, lengths=[frames[i] for i in chunk]).to(torch.float32)
        if cuda:
            host_y = down_sets[k & 1].get("y", tuple(y.shape))
            host_y.copy_(y, non_blocking=True)          # download queued behind the forward on the compute stream
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(device))
            pending[k] = (host_y, done)
        else:
            pending[k] = (y, None)

    def finish(k: int) -> None:
        host_y, done = pending.pop(k)
        if done is not None:
            done.synchronize()
        y = host_y.numpy()
        for j, i in enumerate(batches[k]):
            out[i] = y[j].reshape(-1)[: frames[i] * hop].copy()

    stage(0)
    for k in range(len(batches)):
        compute(k)                               # asynchronous: the host goes on while the GPU runs batch k
        if k + 1 < len(batches):
            stage(k + 1)
        if k >= 1:
            finish(k - 1)                        # (before compute(k + 1) reuses that download set)
    finish(len(batches) - 1)
    return out  # type: ignore[return-value]


def pack_layout(counts: Sequence[int], order: Sequence[int]):
    """Blocks of ``counts[i]`` elements laid back to back in ``order`` -> (offsets, total): ``offsets[i]`` is where
    utterance i's block starts (indexed by utterance, not by position)."""
    offsets = [0] * len(counts)
    pos = 0
    for i in order:
        offsets[i] = pos
        pos += int(counts[i])
    return offsets, pos


def pack_blocks(arrays: Sequence[np.ndarray], counts: Sequence[int], offsets: Sequence[int], dst: np.ndarray,
                indices: Optional[Sequence[int]] = None) -> None:
    """Copy the first ``counts[i]`` elements of every ``arrays[i]`` (flattened in its own C order - a time-major (F, C)
    array stays time-major: a plain contiguous copy, no transpose) to ``dst[offsets[i]:]``, converting to dst's dtype."""
    for i in (range(len(arrays)) if indices is None else indices):
        n = int(counts[i])
        a = np.asarray(arrays[i]).reshape(-1)
        if a.size < n:
            raise ValueError(f"utterance {i}: {a.size} elements, {n} expected")
        dst[offsets[i]: offsets[i] + n] = a[:n]


def _check_open(session) -> bool:
    """The prologue of every convert: a closed session raises ``RuntimeError``; -> whether there is anything to convert.
    (A function of the session, not a method: the converts are also called on stand-ins that have its attributes only.)"""
    if session._closed:
        raise RuntimeError("DecodeSession is closed")
    return bool(session.n)


class DecodeSession:
    """A data set kept on the device across target speakers: ``ppg`` and ``lft`` (99.7 % of the input bytes, the same for
    every speaker) cross the bus once, in the dump's own time-major layout and unpadded; every ``convert`` re-runs only
    what depends on the speaker and brings the waveforms back as unpadded int16.

        with DecodeSession(model, feats, sg, device, src_f0_stats) as s:
            for emb, stats in speakers:
                pcm = s.convert(emb, stats)          # list of int16 arrays, one per utterance, in the order of `feats`

    Results are bit-identical to ``decode_utterances`` (same arguments) followed by ``to_pcm16``: the batches are
    ``bucket_ragged``'s, in the same row order; the F0 shift stays on the host (``F0Statistics.convert``, float64, rounded
    to float32 by assignment into a float32 buffer, as ``decode_utterances`` does); the batches are assembled on the
    device by ``gather_time_major`` (ppg) and ``gather_padded`` (lft); ``pcm16_pack`` computes ``to_pcm16``'s value in
    float64.  F0 is uploaded already padded, (B, 1, Fmax) per batch, and needs no assembly.

    Constructor: packs ppg and lft batch by batch into page-locked memory (contiguous copies, no transposes) and queues
    each batch's upload on a copy stream as soon as it is packed, so the uploads overlap the packing of the later batches;
    it returns without waiting for them.  The first ``convert`` makes its compute stream wait per batch for that batch's
    upload only, so the first batches compute while the last are still in flight; the host packing itself is NOT
    overlapped with compute (it is finished when the constructor returns).  The page-locked staging is released after the
    first ``convert``.

    Assembled batches are not kept: every ``convert`` re-assembles them from the packed upload (two memory-bound launches
    per batch).  Device memory, with F_i frames per utterance, C ppg channels, hop samples per frame:
        held for the session's life    4 * sum_i F_i * (C + hop) bytes                         (packed ppg + lft)
        transient, one batch at a time 4 * B_k * Fmax_k * (C + 1 + 3 * hop) bytes              (ppg, f0, lft, sine, y)
                                       + 2 * hop * sum_{i in batch} F_i (packed int16) + the forward's workspace
    Page-locked host memory: the padded f0 of every batch (4 * sum_k B_k * Fmax_k bytes, for the session's life), the packed
    ppg + lft until the first pass, and TWO download sets used by batch parity, each grown to the largest batch it has
    taken - the packed int16 samples (or the float32 waveforms) of one batch.  ``convert``, ``convert_many`` and
    ``convert_windowed`` share them, and the checked ones a report buffer of 16 bytes a row.

    ``uploaded_bytes`` counts the host-to-device copies: ``["init"]`` by the constructor, ``["convert"]`` one entry per
    ``convert`` (the padded f0 of every batch plus the embedding).  Kernel descriptors (offsets, lengths: 12 - 16 bytes per
    utterance and launch) travel in kernel arguments and are not copies.

    ``checked=True`` (default False: nothing changes - launches, uploads, ``uploaded_bytes``, results): every batch is packed
    by the checked entry point (``pcm16_pack(report=)``; with ``pcm16=False`` the forward is followed by ``output_check``),
    and its reports, 16 bytes a row, come down on the same stream into page-locked memory next to the samples - no extra
    synchronisation per batch.  After the pass, every batch that holds a row with non-finite samples is run again AS A
    WHOLE - same rows, same order, same padded width and ``lengths`` - with the model switched
    (``use_activation_storage``) to the next entry of ``fallback``; only the flagged rows' samples and reports are
    replaced, and batches still flagged go on to the next entry.  The model's storage is restored afterwards, also when
    a forward raises.  So a float16-storage session returns, for exactly the utterances that left float16's range, what
    the fallback storage computes: a row that was never flagged has the bits of an unchecked session in the model's
    storage, a replaced row the bits of an unchecked session in the storage that replaced it (a ragged batch computes every
    row as if alone, and the forward is bit-reproducible).
    ``last_report``: after a checked ``convert``, one dict per utterance in the order of ``feats`` - ``storage`` (what
    produced the returned samples), ``nonfinite`` / ``clipped`` / ``max_abs`` (``output_report`` of those samples) and
    ``tried`` (the storages that gave non-finite samples before it).  ``forwards``: the forwards of the last ``convert``.
    ``strict=True`` raises ``FastSVCError`` naming the utterances still non-finite after the last fallback; otherwise
    their last result is returned and the report says so.
    What the check sees: an overflow of float16 storage that reaches the waveform - an infinity survives LeakyReLU, turns a
    convolution's sum into inf / NaN even through a zero weight and poisons InstanceNorm's mean, so it arrives as inf / NaN
    samples.  What it does not see: precision lost below 2^-14, and a tensor past the ceiling whose infinity is never
    read.  The range contract of float16 storage is unchanged; this detects its observable violations.

    Not thread-safe; one ``convert`` at a time.  ``out_channels`` must be 1."""

    def __init__(self, model, feats: Sequence[Dict[str, np.ndarray]], signal_generator, device,
                 src_f0_stats: Optional[Sequence[Sequence[float]]] = None, max_batch: int = 32,
                 pad_tolerance: float = 0.125, checked: bool = False, fallback: Sequence[str] = ("bfloat16",),
                 strict: bool = False):
        from .engine import STORAGE_CODES
        fallback = (fallback,) if isinstance(fallback, str) else tuple(fallback)
        for name in fallback:
            if name not in STORAGE_CODES:
                raise ValueError(f"fallback storage must be one of {sorted(STORAGE_CODES)}, got {name!r}")
        self.checked, self.fallback, self.strict = bool(checked), fallback, bool(strict)
        self.last_report: List[Dict[str, object]] = []
        self.forwards = 0
        self._h_rep = None
        self.model, self.signal_generator = model, signal_generator
        self.device = torch.device(device)
        self.hop = int(signal_generator.hop_size)
        self.src_f0_stats = src_f0_stats
        self.n = len(feats)
        self.frames = [int(np.asarray(u["ppg"]).shape[0]) for u in feats]
        self.batches: List[List[int]] = list(bucket_ragged(range(self.n), self.frames, max_batch, pad_tolerance)) if feats else []
        self._rows = [[(i, 0) for i in chunk] for chunk in self.batches]     # (convert's batches as the rows of a one-speaker fan-out)
        self.uploaded_bytes = {"init": 0, "convert": []}
        self.max_batch, self.pad_tolerance = int(max_batch), float(pad_tolerance)
        self._fan = None                             # (convert_many's resident extras, made by its first call)
        # set to a dict to have convert_windowed leave what it made there (tests): "excitation", one device tensor per
        # utterance, and "batches", per batch (its rows, the assembled excitation rows)
        self._window_trace: Optional[Dict[str, object]] = None
        self._closed = False
        self._ready = None
        self._h_ppg = self._h_lft = self._d_ppg = self._d_lft = self._h_f0 = None
        if not feats:
            return
        if int(getattr(model, "out_channels", 1)) != 1:
            raise ValueError("DecodeSession supports out_channels == 1 only")
        if src_f0_stats is not None and len(src_f0_stats) != self.n:
            raise ValueError("src_f0_stats needs one [mean, std] per utterance")
        if self.device.type != "cuda":
            from .engine import FastSVCError
            raise FastSVCError("DecodeSession needs a GPU device (no CPU fallback); got " + str(self.device))
        if checked and fallback and not hasattr(model, "use_activation_storage"):
            raise ValueError("a checked session with fallback storages needs a model with use_activation_storage() "
                             "(FastSVCGenerator); pass fallback=() to report only")
        hop, frames = self.hop, self.frames
        self.channels = C = int(np.asarray(feats[0]["ppg"]).shape[1])
        for i, u in enumerate(feats):
            if np.asarray(u["ppg"]).ndim != 2 or int(np.asarray(u["ppg"]).shape[1]) != C:
                raise ValueError(f"utterance {i}: ppg must be (F, {C}), got {np.asarray(u['ppg']).shape}")
        order = [i for chunk in self.batches for i in chunk]
        ppg_counts, lft_counts = [f * C for f in frames], [f * hop for f in frames]
        self._ppg_off, ppg_total = pack_layout(ppg_counts, order)
        self._lft_off, lft_total = pack_layout(lft_counts, order)          # (also where utterance i's int16 samples go)
        self._f0 = [np.asarray(u["f0"], dtype=np.float64).reshape(-1) for u in feats]
        self._f0_base, pos = [], 0
        for chunk in self.batches:
            self._f0_base.append(pos)
            pos += len(chunk) * frames[chunk[0]]
        self._h_f0 = torch.empty(max(pos, 1), dtype=torch.float32, pin_memory=True)
        self._h_ppg = torch.empty(max(ppg_total, 1), dtype=torch.float32, pin_memory=True)
        self._h_lft = torch.empty(max(lft_total, 1), dtype=torch.float32, pin_memory=True)
        self._d_ppg = torch.empty(max(ppg_total, 1), dtype=torch.float32, device=self.device)
        self._d_lft = torch.empty(max(lft_total, 1), dtype=torch.float32, device=self.device)
        self._copy_stream = torch.cuda.Stream(self.device)
        self._copy_stream.wait_stream(torch.cuda.current_stream(self.device))    # (the allocator may hand out blocks still in use there)
        self._d_ppg.record_stream(self._copy_stream)
        self._d_lft.record_stream(self._copy_stream)
        hp, hl = self._h_ppg.numpy(), self._h_lft.numpy()
        ppgs, lfts = [u["ppg"] for u in feats], [u["lft"] for u in feats]
        self._ready = []
        for chunk in self.batches:
            pack_blocks(ppgs, ppg_counts, self._ppg_off, hp, chunk)
            pack_blocks(lfts, lft_counts, self._lft_off, hl, chunk)
            with torch.cuda.stream(self._copy_stream):
                for h, d, off, counts in ((self._h_ppg, self._d_ppg, self._ppg_off, ppg_counts),
                                          (self._h_lft, self._d_lft, self._lft_off, lft_counts)):
                    lo, hi = off[chunk[0]], off[chunk[-1]] + counts[chunk[-1]]    # (a batch's blocks are contiguous)
                    if hi > lo:
                        d[lo:hi].copy_(h[lo:hi], non_blocking=True)
                        self.uploaded_bytes["init"] += 4 * (hi - lo)
                ev = torch.cuda.Event()
                ev.record(self._copy_stream)
            self._ready.append(ev)
        # (C = 1 rows for gather_padded: views of the packed upload, made once)
        self._lft_rows = [[self._d_lft[self._lft_off[i]: self._lft_off[i] + lft_counts[i]].view(1, -1) for i in chunk]
                          for chunk in self.batches]
        self._down = [_PinnedSet(), _PinnedSet()]    # (every pass's download staging, by batch parity)
        self._counts, self._total = lft_counts, lft_total            # (samples per utterance, and of one speaker's result)
        self._row_layouts = [fanout_layout(chunk, lft_counts, self._lft_off) for chunk in self._rows]   # (convert's batches never change)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self) -> None:
        """Wait for the session's device work and release its device and page-locked buffers."""
        if self._closed:
            return
        self._closed = True
        if self.n and self.device.type == "cuda":
            self._copy_stream.synchronize()
            torch.cuda.current_stream(self.device).synchronize()
        self._h_ppg = self._h_lft = self._d_ppg = self._d_lft = self._h_f0 = self._h_rep = None
        self._lft_rows = self._down = self._ready = self._fan = None

    def _emb_row(self, trg_emb) -> Optional[torch.Tensor]:
        """The target speaker's embedding as a (1, E) device tensor, or None."""
        if trg_emb is None:
            return None
        return torch.as_tensor(np.asarray(trg_emb), dtype=torch.float32).reshape(1, -1).to(self.device)

    def _wait_for_uploads(self, stream) -> None:
        """``stream`` waits for ALL the constructor's uploads, when no pass has waited for them yet."""
        for ev in self._ready or ():
            stream.wait_event(ev)

    def _uploads_waited(self) -> None:
        """After a pass's ``stream.synchronize()``: every upload of the constructor has been waited for, its staging can go."""
        if self._ready is not None:
            self._ready = None
            self._h_ppg = self._h_lft = None

    def _pack_f0(self, dst: np.ndarray, trg_f0_stats: Optional[Sequence[float]] = None) -> List[int]:
        """f0 packed like lft into ``dst`` (float32 by assignment) -> the offsets: utterance i's frames at ``_lft_off[i] /
        hop``.  With ``trg_f0_stats`` and source statistics, shifted on the host as ``convert`` shifts it."""
        f0_off = [o // self.hop for o in self._lft_off]
        shift = self.src_f0_stats is not None and trg_f0_stats is not None
        for i, f in enumerate(self._f0):
            n = self.frames[i]
            if f.size < n:
                raise ValueError(f"utterance {i}: {f.size} f0 values, {n} expected")
            if shift:
                f = F0Statistics().convert(f, self.src_f0_stats[i], trg_f0_stats)
            dst[f0_off[i]: f0_off[i] + n] = f[:n]
        return f0_off

    def _host_report(self, n_rows: int) -> torch.Tensor:
        """Page-locked room for the (n_rows, 4) reports of a checked pass, grown on demand and kept."""
        if self._h_rep is None or self._h_rep.shape[0] < n_rows:
            self._h_rep = torch.empty((n_rows, 4), dtype=torch.int32, pin_memory=True)
        return self._h_rep[:n_rows]

    def _row_pass(self, stream, batches: Sequence[Sequence[Tuple[int, int]]], n_spk: int, assemble, layout, pcm16: bool):
        """The pass under ``convert`` and ``convert_many``: the batches of ``(utterance, speaker)`` rows, one forward each,
        downloads one batch behind, and - a checked session - the storage fallback -> ``(out, reports, still)``:
        ``out[speaker][utterance]`` the arrays the two return, ``reports[speaker][utterance]`` the ``last_report`` dicts
        (None unless checked), ``still`` the pairs left non-finite.

        ``assemble(k, first_pass)`` puts batch k's inputs on the current stream and returns ``(ppg, f0, lft, emb, lens,
        fmax)`` (``first_pass`` False: a fallback run of the batch); ``layout(k)`` is batch k's ``fanout_layout``.  Then, per
        batch: the excitation, the forward, ``pcm16_pack`` into that layout (or ``output_check`` with ``pcm16=False``), the
        download of the samples and of the reports.  In the result, speaker s starts at ``s * total`` and is laid out as ``_lft_off`` says.
        A fallback run computes the batch whole and replaces the flagged rows' samples and reports only."""
        from .engine import output_check, pcm16_pack
        dev, hop, checked = self.device, self.hop, self.checked
        counts, total = self._counts, self._total    # (samples per utterance; one speaker's samples)
        if checked:
            row_batches, pos = [], 0                 # (batch k's rows as rows of the pass: where their reports go)
            for chunk in batches:
                row_batches.append(list(range(pos, pos + len(chunk))))
                pos += len(chunk)
            h_rep = self._host_report(pos)
        if pcm16:
            result = np.empty(n_spk * total, dtype=np.int16)
        else:
            out: List[List[Optional[np.ndarray]]] = [[None] * self.n for _ in range(n_spk)]

        def take(k: int, host: torch.Tensor, rows: Optional[Sequence[int]]) -> None:
            """Batch k's samples out of the page-locked buffer (``rows``: those rows of it only)."""
            chunk, h = batches[k], host.numpy()
            if pcm16:
                offs, runs, _ = layout(k)
                if rows is None:
                    for sp, first, start, count in runs:
                        result[sp * total + first: sp * total + first + count] = h[start: start + count]
                else:
                    for j in rows:
                        u, sp = chunk[j]
                        a = sp * total + self._lft_off[u]
                        result[a: a + counts[u]] = h[offs[j]: offs[j] + counts[u]]
                return
            for j in (range(len(chunk)) if rows is None else rows):
                u, sp = chunk[j]
                out[sp][u] = h[j].reshape(-1)[: counts[u]].copy()

        def enqueue(pinned: _PinnedSet, k: int, rows: Optional[Sequence[int]] = None):
            """Batch k on the stream, whole.  ``rows`` (a fallback run): only those rows' reports replace the first pass's."""
            R = len(batches[k])
            ppg, f0, lft, emb, lens, fmax = assemble(k, rows is None)
            sine = self.signal_generator(f0)
            emb = None if emb is None else emb.contiguous()      # (an expanded row becomes (R, E) here, behind the excitation)
            y = self.model(ppg, sine, lft, emb, lengths=lens).to(torch.float32)
            self.forwards += 1
            report = torch.empty((R, 4), dtype=torch.int32, device=dev) if checked else None
            if pcm16:
                offs, _, count = layout(k)
                packed = torch.empty(max(count, 1), dtype=torch.int16, device=dev)
                pcm16_pack(y.view(R, fmax * hop), [n * hop for n in lens], offs, out=packed, report=report)
                host = pinned.samples(count, True)[0]
                if count:
                    host.copy_(packed[:count], non_blocking=True)
            else:
                host = pinned.get("w", tuple(y.shape))
                host.copy_(y, non_blocking=True)
                if checked:
                    output_check(y.view(R, fmax * hop), [n * hop for n in lens], out=report)
            if checked:
                r0 = row_batches[k][0]
                if rows is None:
                    h_rep[r0: r0 + R].copy_(report, non_blocking=True)
                else:
                    for j in rows:
                        h_rep[r0 + j].copy_(report[j], non_blocking=True)
            return k, host, rows

        _one_behind(stream, self._down, [(k,) for k in range(len(batches))], enqueue, take)
        stream.synchronize()
        self._uploads_waited()
        reports, still = None, []
        if checked:
            rep = h_rep.numpy()
            pairs = [pair for chunk in batches for pair in chunk]            # (row of the pass -> (utterance, speaker))

            def run(work) -> None:                   # (the rare path; its events make ``rep`` current before it returns)
                _one_behind(stream, self._down, work, enqueue, take)

            storage, tried, flagged = storage_fallback(self.model, self.fallback, len(pairs), lambda r: rep[r, 0] > 0,
                                                       _rerun_in_batches(row_batches, run))
            reports = [[None] * self.n for _ in range(n_spk)]
            for (u, sp), d in zip(pairs, _report_dicts(rep, storage, tried)):
                reports[sp][u] = d
            still = [pairs[r] for r in flagged]
        if pcm16:
            out = [[result[sp * total + self._lft_off[i]: sp * total + self._lft_off[i] + counts[i]] for i in range(self.n)]
                   for sp in range(n_spk)]
        return out, reports, still

    @torch.no_grad()
    def convert(self, trg_emb=None, trg_f0_stats: Optional[Sequence[float]] = None, pcm16: bool = True) -> List[np.ndarray]:
        """Every utterance converted to one target speaker, in the order of ``feats``.

        pcm16=True   int16 arrays, equal to ``to_pcm16`` of what ``decode_utterances`` returns: views of ONE new array per
                     call, a copy of the page-locked download buffer (made batch by batch while later batches compute),
                     so they stay valid after the next ``convert`` and after ``close``.
        pcm16=False  float32 arrays, copies: exactly what ``decode_utterances`` returns."""
        if not _check_open(self):
            return []
        from .engine import FastSVCError, gather_padded, gather_time_major
        from .synth import TOO_LONG_HINT, max_forward_frames
        dev, hop, frames, C = self.device, self.hop, self.frames, self.channels
        cfg = getattr(self.model, "_cfg", None)
        if cfg is not None and max(frames) > max_forward_frames(cfg):        # (the forward's own limit and words, before any launch)
            i = int(np.argmax(frames))
            raise FastSVCError(f"utterance {i} ({frames[i]} frames) is too long for the 32-bit tensor descriptors of the "
                               f"kernels (one forward takes {max_forward_frames(cfg)} frames): split it" + TOO_LONG_HINT)
        stream = torch.cuda.current_stream(dev)
        self.forwards = 0
        emb_row = self._emb_row(trg_emb)
        up = 0 if emb_row is None else 4 * emb_row.numel()
        shift = self.src_f0_stats is not None and trg_f0_stats is not None
        hf_all = self._h_f0.numpy()

        def assemble(k: int, first_pass: bool):
            """f0 up, shifted on the host, and the batch out of the packed upload.  On a fallback run the padded f0 is still
            in its page-locked slot from the first pass."""
            nonlocal up
            chunk = self.batches[k]
            fmax, B = frames[chunk[0]], len(chunk)
            lens = [frames[i] for i in chunk]
            base = self._f0_base[k]
            if first_pass:
                hf = hf_all[base: base + B * fmax].reshape(B, 1, fmax)
                for j, i in enumerate(chunk):
                    f, n = self._f0[i], frames[i]
                    if shift:
                        f = F0Statistics().convert(f, self.src_f0_stats[i], trg_f0_stats)
                    hf[j, 0, :n] = f
                    hf[j, 0, n:] = 0
            f0 = self._h_f0[base: base + B * fmax].view(B, 1, fmax).to(dev, non_blocking=True)
            up += 4 * B * fmax
            if self._ready is not None:              # (the first pass: this batch's upload only, the later ones are in flight)
                stream.wait_event(self._ready[k])
            ppg = gather_time_major(self._d_ppg, [self._ppg_off[i] for i in chunk], lens, C, fmax)
            lft = gather_padded(self._lft_rows[k], fmax * hop)
            return ppg, f0, lft, None if emb_row is None else emb_row.expand(B, -1), lens, fmax

        out, reports, still = self._row_pass(stream, self._rows, 1, assemble, self._row_layouts.__getitem__, pcm16)
        if self.checked:
            self.last_report = reports[0]
        self.uploaded_bytes["convert"].append(up)
        if still and self.strict:
            _raise_still_nonfinite(self.model, self.fallback, "utterances", sorted(u for u, _ in still))
        return out[0]

    @torch.no_grad()
    def convert_windowed(self, trg_emb=None, trg_f0_stats: Optional[Sequence[float]] = None, core: int = 400,
                         context: Optional[int] = None, fade: int = 8, pcm16: bool = True,
                         norm: str = "window") -> List[np.ndarray]:
        """Every utterance converted to one target speaker as overlapping WINDOWS - for utterances longer than one
        forward takes (``synth.max_forward_frames``: 69 905 frames for the recipe's generator), and for sets whose
        lengths differ so much that ``bucket_ragged`` cannot fill batches.  Returns what ``convert`` returns: one array per
        utterance in the order of ``feats``, int16 (``pcm16=True``) or float32, views of one new array per call.

        ``window_plan(frames, core, context)`` cuts every utterance into windows that own ``core`` frames and read
        ``context`` more on each side (``context=None``: ``receptive_field_frames`` rounded up to a multiple of 4); an
        utterance of at most ``core`` frames is one row, the whole utterance, and runs as ``convert`` runs it.  The windows
        of ALL utterances are bucketed by length (``window_batches``), so device buffers are sized by ``max_batch x (core +
        2 context)`` frames, never by the longest utterance - apart from what is per sample of the whole set: the resident
        features, and this call's excitation (4 bytes a sample).  Per batch: one ``window_assemble``, one forward with
        ``lengths``, one ``window_stitch`` into a per-batch packed buffer; downloads run one batch behind.

        Excitation: the F0 shift (host, as in ``convert``) and the excitation are made ONCE per call for each whole
        utterance - one ``signal_generator`` call per utterance, in the order of ``feats`` - and the windows take slices:
        the sine phase and the noise are continuous across windows, and a window's excitation is bit for bit the slice of
        its utterance's.

        Stitching: ``stitch_windows``' rule - around every interior boundary the two windows are cross-faded linearly over
        ``fade`` frames in float64 (``fade`` even, ``<= min(core, 2 context)``; 0 concatenates the cores).

        What the result is.  Three cases.  WITHOUT a speaker embedding the generator is a convolution of
        finite reach, and with ``context >= receptive_field_frames`` every window's core IS the whole-utterance result (to
        float32 kernel arithmetic: the batching invariance the harness states), so the cross-fade blends two equal signals;
        ``norm`` changes nothing.  WITH an embedding and ``norm="window"`` (the default), InstanceNorm takes its statistics
        over the row: a window is normalised by ITS OWN mean and variance - as training normalises one-second crops - so
        the windowed decode is a different, well-defined function: exactly ``stitch_windows`` of every window run alone,
        NOT the whole-utterance result at any context.  WITH an embedding and ``norm="utterance"``, every norm point takes
        its sums over the frames each window OWNS (its core), pools them over the windows of the utterance and normalises
        every window by the utterance's mean and variance (``Generator.forward(norm_groups=...)``,
        csrc/fastsvc_normgroup.hip): InstanceNorm is then the same per-channel affine in every window, the generator is
        again of finite reach, and with ``context >= receptive_field_frames`` the result is the whole-utterance one, what
        ``convert`` returns, to float32 kernel arithmetic.  For that the windows of an utterance must share a forward:
        batches hold whole utterances (``grouped_window_batches``), and an utterance with more windows than ``max_batch``
        raises ``ValueError`` before anything runs - choose a larger ``core`` or ``max_batch``.  An utterance of one
        window runs exactly as in ``convert``.

        A checked session reports per UTTERANCE, over the stitched samples (``last_report`` as after ``convert``); an
        utterance with non-finite samples has ALL its windows run again in the next fallback storage, in batches of their
        own.  ``uploaded_bytes["convert_windowed"]`` gets one entry per call: the packed f0 (4 bytes a frame) and the
        embedding."""
        if not _check_open(self):
            return []
        from .engine import window_assemble
        dev, hop, frames, C = self.device, self.hop, self.frames, self.channels
        core = int(core)
        if context is None:
            cfg = getattr(self.model, "_cfg", None)
            if cfg is None:
                raise ValueError("convert_windowed needs context= for a model without a generator configuration")
            context = -(-receptive_field_frames(cfg) // 4) * 4
        context, fade = int(context), int(fade)
        _check_window_sizes(core, context, fade)
        if norm not in ("window", "utterance"):
            raise ValueError(f"norm must be \"window\" or \"utterance\", got {norm!r}")
        grouped = norm == "utterance"
        if len(getattr(self.signal_generator, "signal_types", ("sine",))) != 1:
            raise ValueError("convert_windowed needs a signal generator with one signal type")
        checked = self.checked
        stream = torch.cuda.current_stream(dev)
        self.forwards = 0
        rows = window_plan(frames, core, context)
        if grouped:
            grouped_window_batches(rows, self.max_batch)     # (an utterance that does not fit a batch: refused before anything runs)
        emb_row = self._emb_row(trg_emb)
        up = 0 if emb_row is None else 4 * emb_row.numel()
        total = sum(frames) * hop
        # ---- the excitation of every whole utterance, packed like lft
        f0_off = self._pack_f0(self._h_f0.numpy(), trg_f0_stats)     # (page-locked, at least sum(frames) floats)
        d_f0 = self._h_f0[: sum(frames)].to(dev, non_blocking=True)
        up += 4 * sum(frames)
        self._wait_for_uploads(stream)
        d_sine = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
        for i in range(self.n):
            n = frames[i]
            e = self.signal_generator(d_f0[f0_off[i]: f0_off[i] + n].view(1, 1, n))
            d_sine[self._lft_off[i]: self._lft_off[i] + n * hop].copy_(e.view(-1))
            del e
        trace = self._window_trace
        if trace is not None:
            trace.clear()
            trace.update(excitation=[d_sine[self._lft_off[i]: self._lft_off[i] + frames[i] * hop].clone() for i in range(self.n)],
                         batches=[])
        by_utt: Dict[int, List[int]] = {}
        for r, row in enumerate(rows):
            by_utt.setdefault(row[0], []).append(r)
        result = np.empty(total, dtype=np.int16 if pcm16 else np.float32)
        d_rep = torch.zeros((self.n, 4), dtype=torch.int32, device=dev) if checked else None
        # norm="utterance": the partial sums' scratch, once per call, for the largest batch any pass can form
        norm_scratch = None
        plan = getattr(self.model, "plan", None)
        if grouped and emb_row is not None and plan is not None:
            widest = max(r[2] - r[1] for r in rows)
            norm_scratch = torch.empty(max(plan.norm_group_scratch_bytes(min(self.max_batch, len(rows)), plan.padded_frames(widest)), 1),
                                       dtype=torch.uint8, device=dev)

        def run(row_ids: Sequence[int]) -> None:
            """One pass over these rows (all windows of their utterances), stitched into ``result``."""
            sub = [rows[r] for r in row_ids]
            batches = [[row_ids[j] for j in chunk] for chunk in
                       (grouped_window_batches(sub, self.max_batch) if grouped else window_batches(sub, self.max_batch, self.pad_tolerance))]
            layout, stage_elems = stitch_layout(rows, batches, hop, fade)
            stage = torch.empty(max(stage_elems, 1), dtype=torch.float32, device=dev)

            def take(host: torch.Tensor, lay) -> None:
                h = host.numpy()
                for (u, t_lo, t_hi), off in zip(lay["runs"], lay["dst_off"]):
                    a = self._lft_off[u]
                    result[a + t_lo: a + t_hi] = h[off: off + t_hi - t_lo]

            def enqueue(pinned: _PinnedSet, k: int):
                chunk, lay = batches[k], layout[k]
                lens = [rows[r][2] - rows[r][1] for r in chunk]
                width, B = max(lens), len(chunk)
                ppg, lft, sine = window_assemble(
                    self._d_ppg, self._d_lft, d_sine, [self._ppg_off[rows[r][0]] + rows[r][1] * C for r in chunk],
                    [self._lft_off[rows[r][0]] + rows[r][1] * hop for r in chunk], lens, C, hop, width)
                if trace is not None:
                    trace["batches"].append(([rows[r] for r in chunk], sine.clone()))
                emb = None if emb_row is None else emb_row.expand(B, -1).contiguous()
                if grouped:
                    # a row's group is its utterance; it owns its core, counted from its own first frame
                    first = {}
                    groups = ([first.setdefault(rows[r][0], j) for j, r in enumerate(chunk)],
                              [rows[r][3] - rows[r][1] for r in chunk], [rows[r][4] - rows[r][1] for r in chunk])
                    y = self.model(ppg, sine, lft, emb, lengths=lens, norm_groups=groups, norm_scratch=norm_scratch).to(torch.float32)
                else:
                    y = self.model(ppg, sine, lft, emb, lengths=lens).to(torch.float32)
                self.forwards += 1
                return _stitch_to_host(y, lay, stage, pcm16, pinned, d_rep)[0], lay

            _one_behind(stream, self._down, [(k,) for k in range(len(batches))], enqueue, take)
            stream.synchronize()

        run(list(range(len(rows))))
        self._uploads_waited()
        still: List[int] = []
        if checked:
            rep = d_rep.cpu().numpy()

            def rerun(name, flagged) -> None:        # (the rare path: batches of the flagged utterances' windows only)
                nonlocal rep
                d_rep[torch.as_tensor(flagged, device=dev)] = 0
                run([r for i in flagged for r in by_utt[i]])
                rep = d_rep.cpu().numpy()

            storage, tried, still = storage_fallback(self.model, self.fallback, self.n, lambda i: rep[i, 0] > 0, rerun)
            self.last_report = _report_dicts(rep, storage, tried)
        out = [result[self._lft_off[i]: self._lft_off[i] + frames[i] * hop] for i in range(self.n)]
        self.uploaded_bytes.setdefault("convert_windowed", []).append(up)
        if still and self.strict:
            _raise_still_nonfinite(self.model, self.fallback, "utterances", still)
        return out

    def _fanout_init(self) -> None:
        """convert_many's resident extras, made once: f0 packed like lft (utterance i's frames at ``_lft_off[i] / hop``),
        float32, the values ``convert`` uploads batch by batch; the (n, 2) float64 table of source statistics; and the
        layout as the ctypes arrays every ``fanout_assemble`` reads."""
        import ctypes
        frames = self.frames
        h = np.empty(max(sum(frames), 1), dtype=np.float32)
        f0_off = self._pack_f0(h)
        fan = {"f0": torch.from_numpy(h).to(self.device), "src": None}
        up = 4 * sum(frames)
        if self.src_f0_stats is not None:
            table = np.ascontiguousarray(np.asarray(self.src_f0_stats, dtype=np.float64).reshape(self.n, 2))
            fan["src"] = torch.from_numpy(table).to(self.device)
            up += table.nbytes
        fan["ppg_off"] = (ctypes.c_int64 * self.n)(*self._ppg_off)
        fan["lft_off"] = (ctypes.c_int64 * self.n)(*self._lft_off)
        fan["f0_off"] = (ctypes.c_int64 * self.n)(*f0_off)
        fan["frames"] = (ctypes.c_int32 * self.n)(*frames)
        self._fan = fan
        self.uploaded_bytes["fanout_init"] = up
        self.uploaded_bytes["convert_many"] = []

    @torch.no_grad()
    def convert_many(self, speakers: Sequence[Tuple[object, Optional[Sequence[float]]]], pcm16: bool = True):
        """Every utterance converted to every speaker of ``speakers``, a sequence of ``(trg_emb | None, trg_f0_stats |
        None)`` (all with an embedding or none, all with statistics or none): ``result[s][i]`` is utterance i (the order of
        ``feats``) for speaker s, the array kinds ``convert`` returns - int16 views of one new array per call
        (``pcm16=True``) or float32 copies.

        The batches are ``fanout_batches``': their rows are (utterance, speaker) pairs, so a source set smaller than
        ``max_batch`` still fills its batches, across the speaker axis (the forward couples no rows; it takes a per-row
        embedding and ``lengths``).  Each batch is one ``fanout_assemble`` launch per 64 rows - ppg, lft, the F0 shift in
        double precision on the device and the embedding rows, from the resident buffers - one ``signal_generator`` call
        (batches in order), one forward, and one ``pcm16_pack`` into the batch's ``[speaker][utterance]`` layout (or
        ``output_check`` with ``pcm16=False``); downloads run one batch behind.  The first call uploads the packed f0 (4
        bytes a frame) and the table of source statistics, counted once under ``uploaded_bytes["fanout_init"]``; after
        that a call uploads its speaker tables only (embeddings and statistics; one entry per call in
        ``uploaded_bytes["convert_many"]``) - no f0 crosses the bus again.  ``convert`` and its accounting do not change.

        Against ``convert``: with one speaker the batches are ``self.batches`` and, without an F0 shift, the result is
        ``convert``'s bit for bit.  With a shift the device's F0 is within one float32 ulp of the host's
        (``fastsvc_fanout_assemble``); with several speakers the batches differ, and the waveforms agree to the harness's
        batching invariance (2e-5 in float32 storage, tests/test_parity_gpu.py).  The excitation noise is seeded per
        ``signal_generator`` call and row, so with ``noise_amp > 0`` a fan-out pass draws other noise than sequential
        converts do - as two sequential converts of the same speaker already differ from each other.

        A checked session keeps ``convert``'s semantics per row: a fan-out batch that holds a row with non-finite samples
        is run again whole in the next fallback storage and only the flagged rows are replaced; ``last_report`` becomes
        a list per speaker of the per-utterance dicts; ``strict`` names the ``(utterance, speaker)`` pairs; the model's
        storage is restored also when a forward raises."""
        speakers = list(speakers)
        S = len(speakers)
        if not _check_open(self) or not S:
            return [[] for _ in speakers]
        from .engine import fanout_assemble
        dev, hop, frames, C = self.device, self.hop, self.frames, self.channels
        embs, stats = [e for e, _ in speakers], [t for _, t in speakers]
        for name, vals in (("an embedding", embs), ("F0 statistics", stats)):
            if any(v is None for v in vals) and not all(v is None for v in vals):
                raise ValueError(f"convert_many: every speaker of one call needs {name}, or none does")
        if self._fan is None:
            self._fanout_init()
        fan = self._fan
        up = 0
        self.forwards = 0
        emb_table = stats_table = None
        if embs[0] is not None:
            emb_table = torch.from_numpy(np.ascontiguousarray(
                np.stack([np.asarray(e, dtype=np.float32).reshape(-1) for e in embs]))).to(dev)
            up += 4 * emb_table.numel()
        shift = self.src_f0_stats is not None and stats[0] is not None
        if shift:
            stats_table = torch.from_numpy(np.ascontiguousarray(
                np.stack([np.asarray(t, dtype=np.float64).reshape(-1)[:2] for t in stats]))).to(dev)
            up += 8 * stats_table.numel()
        batches = fanout_batches(frames, S, self.max_batch, self.pad_tolerance)
        stream = torch.cuda.current_stream(dev)
        self._wait_for_uploads(stream)

        def assemble(k: int, first_pass: bool):
            chunk = batches[k]
            fmax = frames[chunk[0][0]]
            ppg, lft, f0, emb = fanout_assemble(self._d_ppg, self._d_lft, fan["f0"], fan["ppg_off"], fan["lft_off"],
                                                fan["f0_off"], fan["frames"], [u for u, _ in chunk], [sp for _, sp in chunk],
                                                C, hop, fmax, src_stats=fan["src"] if shift else None,
                                                spk_stats=stats_table, spk_emb=emb_table, n_spk=S)
            return ppg, f0, lft, emb, [frames[u] for u, _ in chunk], fmax

        layouts = {}

        def layout(k: int):
            if k not in layouts:
                layouts[k] = fanout_layout(batches[k], self._counts, self._lft_off)
            return layouts[k]

        out, reports, still = self._row_pass(stream, batches, S, assemble, layout, pcm16)
        if self.checked:
            self.last_report = reports
        self.uploaded_bytes["convert_many"].append(up)
        if still and self.strict:
            _raise_still_nonfinite(self.model, self.fallback, "(utterance, speaker) pairs", still)
        return out


class StreamSession:
    """Live conversion: features arrive a few frames at a time, for up to ``n_streams`` streams at once, and samples
    come back as soon as the windows that own them can run.

        with StreamSession(model, sg, device, n_streams=8) as s:
            a = s.open(trg_emb, src_stats, trg_stats)
            while ...:
                out = s.push({a: dict(ppg=..., f0=..., lft=...)})      # {a: int16 samples, possibly none yet}
            tail = s.end([a])[a]

    A stream is an utterance whose length F is unknown until it ends.  Its windows are ``window_plan([F], core,
    context)`` (``context=None``: ``receptive_field_frames`` rounded up to a multiple of 4; the sizes follow
    ``convert_windowed``'s rules), window k runs in the push after which it is ready (``stream_ready_rows``), and the
    windows are cross-faded by ``stitch_windows``' rule: everything a stream returned, concatenated, is samples ``[0, F
    hop)``, each exactly once, and equals ``stitch_windows`` of its windows.  WITHOUT a speaker embedding that is the
    whole-utterance result (to float32 kernel arithmetic); WITH one it is ``convert_windowed(norm="window")``'s function:
    InstanceNorm normalises every window by its own statistics.  Whole-utterance statistics need frames that have not
    arrived; ``norm="running"`` uses every frame that HAS: window k is normalised, at all norm points, by the mean and
    variance of the stream's frames ``[0, in_hi_k)`` - the float64 sums of the cores of windows 0..k-1, carried on the
    device from forward to forward (``Generator.forward(norm_running=...)``, csrc/fastsvc_normgroup.hip), plus the
    window's own core and look-ahead.  Window 0 is ``norm="window"``'s, bit for bit, so a stream that ends inside it
    returns the same bytes; later windows approach ``convert_windowed(norm="utterance")`` as the stream grows, and the
    result does not depend on how windows fall into forwards beyond the forward's batching invariance (DESIGN.md 4.10
    has the rule, its reference and its caveats).  It needs a model that takes an embedding; streams opened without
    one run as under ``"window"`` and carry nothing.

    ``horizon=H`` (frames, ``H >= core``; only with ``norm="running"``) makes the running statistics FORGET: the carried
    sums are multiplied by ``exp(-c / H)`` in front of every core of c frames, so a frame j cores back counts with
    ``exp(-j core / H)`` while the window's own core and look-ahead count in full.  The population a window is normalised
    by stays below ``core / (1 - exp(-core / H)) + context`` frames for as long as the stream lives - and with it the
    float32 headroom the mode costs - and a change of level is forgotten at that rate instead of never.
    One ``math.exp`` per window on the host (``running_horizon_rows``) feeds the device, the per-stream frame count ``w``
    (``norm_frames``) lives on the host; the same launches, one more multiplication per row in the pool.  ``None``: no
    forgetting, the launches and bytes as before.

    ``loudness="audio"`` takes the stream's raw audio instead of its loudness: a chunk is ``dict(ppg, f0, audio=(n hop,))``,
    and the A-weighted log loudness ``loudness_extract`` computes for whole files is made on the device, frame by frame, as
    the audio arrives (csrc/fastsvc_stream_loudness.hip).  Frame f is the whole-file function's frame f of the stream's
    audio ``y[0, F hop)`` - periodic Hann, 2048 samples centred on ``f hop``, reflection at both ends - with ONE departure:
    its 80 dB floor hangs under the RUNNING maximum of the power over the frames ``<= f``, not under the maximum of the
    whole utterance, which a live stream does not know.  That is a definition, not an approximation: it is causal and per
    frame, so it cannot depend on how the stream was cut into pushes, and it equals the whole-file value wherever the
    running maximum has reached the utterance's or no bin of the frame lies under either floor - for every frame of a
    stream whose loudest frame is its first - but a quiet passage BEFORE the utterance's peak is floored lower than the
    whole-file function floors it, and reads quieter (DESIGN.md 4.10 has figures).  A frame reads 1023 samples past its centre, so it is FINAL
    ``lag = stream_loudness_lag(hop)`` frames after it arrived (6 at hop 160) or at the stream's end; window k is ready
    when ``stream_ready_rows(final, ...)`` says so, ``final = stream_final_frames(seen, ended, hop)`` in ``seen``'s place,
    so a stream's rows are still ``window_plan([F], core, context)`` and stitching, running norms and horizons are
    untouched.  ``"given"`` (the default): launches, bytes and bits as before.

    ``f0="audio"`` (needs ``loudness="audio"``) makes the F0 from that audio as well: a chunk is ``dict(ppg, audio)`` and
    nothing else.  The recipe's F0 is ``pyworld.harvest``'s, a whole-file CPU algorithm; here the F0 is a DEFINITION, like
    the running loudness floor: YIN (de Cheveigne & Kawahara 2002) per frame on the loudness frame ``x[k] = y[f hop - 1024
    + k]``, ``k < 2048``, no window, reflection at 0 and - once the stream has ended - at ``F hop``.  With ``tau_min =
    floor(sr / f0_ceil)``, ``tau_max = ceil(sr / f0_floor)`` (70 and 343 at 24 kHz with the defaults 340 and 70 Hz; ``tau_max
    > 1024`` is a ``ValueError``) and ``W = 2048 - tau_max``: ``d(tau) = sum over 1 <= j < W of (x[j] - x[j + tau])^2`` for
    ``tau = 1..tau_max``, computed directly in float32 (no FFT: no cancellation; ``x[0]`` is never read - frame 0's is sample
    1024 by reflection, which has not arrived when the frame is final and hop divides 1024 - the loudness weights it by a
    Hann zero); ``d'(tau) = d(tau) tau / (d(1) + ... + d(tau))``, and a constant frame (``d(1) == 0``) is unvoiced: no NaN;
    the smallest ``tau`` in ``[tau_min, tau_max]`` with ``d'(tau) < f0_threshold`` (0.15), walked right while ``d'`` falls,
    refined by a parabola through its neighbours (skipped at the range's ends and when ``d'(tau)`` is not the smallest of
    the three); ``f0 = sr / tau_hat``, 0 when no lag qualifies.  The value is a function of the frame's 2048 samples alone -
    no running state, no departure from the whole-file function ``f0_extract`` (svcc23_fastsvc_amd/f0.py), whose bits a
    streamed frame has for every push schedule, slot and ring position.  The float64 reference is within 0.01 % of steady
    harmonic tones at 70.5 - 339 Hz, calls 1e-3 white noise and digital silence unvoiced on every frame, and is within 0.8
    % of a 110 -> 220 Hz glide over 0.4 s.  A frame's F0 is final when its loudness is, so the excitation
    of a chunk is no longer made by the push that delivers it: ``_finalise_f0`` (two ``stream_f0`` launches,
    csrc/fastsvc_stream_f0.hip) writes the raw F0 and the shifted F0 into two rings of ``cap`` frames and synthesises the
    frames' excitation from the carried phase; the F0 shift of ``src_f0_stats`` / ``trg_f0_stats`` runs there, on the
    device, in float64 (within one float32 ulp of ``F0Statistics.convert``).  Ring sizes, ``lag`` and latencies are
    ``loudness="audio"``'s.  ``"given"`` (the default): launches, kernel arguments, bytes and bits as before.

    ``open(trg_emb, src_f0_stats=RunningF0Stats(prior, prior_frames, horizon), trg_f0_stats=[m_t, s_t])`` (``f0="audio"``
    sessions) makes the source statistics of the F0 shift from the stream itself - a live microphone has no corpus to take
    them from.  Like the running loudness floor it is a DEFINITION: with the prior ``(m_p, s_p)`` (None: the target's), its
    weight ``n0 = prior_frames``, ``g = exp(-1 / horizon)`` (one ``math.exp`` at ``open``; exactly 1.0 without a horizon) and the
    state ``(w, S1, S2) = (0, 0, 0)`` at ``open``, the final frames are taken in order: raw F0 ``v <= 0`` gives 0 and leaves the
    state alone - silence neither counts nor forgets - and a voiced frame, in float64, every operation rounded separately::

        d = log(v) - m_p;  w = w g + 1;  S1 = S1 g + d;  S2 = S2 g + d d;  N = n0 + w;  mu = S1 / N
        var = (n0 s_p s_p + S2) / N - mu mu;  out = (float) exp((s_t / sqrt(var)) (d - mu) + m_t)

    Frame f is shifted by the statistics of the voiced frames ``<= f``, itself included, blended with a prior that counts as
    ``n0`` frames and is never forgotten; the voiced frame j voiced frames back counts with ``g^j``.  ``var >= n0 s_p^2 / N > 0``
    (Cauchy-Schwarz): no NaN, no division by zero, no floor parameter.  Without a horizon ``m_p + mu`` and ``var`` tend to the
    mean and population variance of the source's log F0, so the output tends to ``F0Statistics.convert(f0, estimate([f0 so
    far]), trg)`` - on 3000 frames wandering between 120 and 200 Hz the last fifth is within 9.0e-3 relative of ``convert`` with
    the whole track's ``estimate`` for ``prior_frames=1`` and 1.56e-1 for 100 (8.97e-2 and 4.06e-1 with ``horizon=200``: the
    prior keeps its share for ever, so a horizon wants a small ``prior_frames``).  With prior = target a stream
    begins almost unshifted and moves to the target's register as evidence arrives.  The value depends on the stream's
    frames alone, not on push sizes, slot or ring position.  On the device: a float64 record ``(n_streams, 2, 4)`` of ``(w, S1,
    S2, voiced frames)`` - allocated with ``f0="audio"``, never zeroed, a stream's frame 0 starts from zeros, addressed by the
    phase record's parity - and ONE more launch between the F0 and the excitation in a push where a stream with running
    statistics got final frames (``stream_f0_running``); streams with list statistics or none keep their meaning, and a
    push without a running stream its launches, kernel arguments and bytes.  All three kinds may be open at once.
    ``f0_stats(id)`` reads the record back; ``running_f0_convert`` is the rule on the host.  Within one float32 ulp of the
    float64 reference over the traced raw F0 (0 measured).

    ``f0_track=F0Track(lag=8, ...)`` (needs ``f0="audio"``) replaces the per-frame pick by fixed-lag Viterbi over YIN candidates
    (``F0Track``, ``f0_track_rule`` and DESIGN.md 4.10 have the rule): per frame up to four local minima of d' under
    ``cand_threshold``, across frames Viterbi over {4 candidates, unvoiced} in float64, the state of frame f traced back from the
    best state of frame ``min(f + lag, F - 1)`` - the value of frame f is a function of the audio of the frames ``<= f + lag``
    alone, so it does not depend on push sizes, slots or ring positions and equals ``f0_extract(track=...)``'s whole-file
    function over the stream's frames.  A frame's tracked F0, shift and excitation are made ``lag`` frames after it is final
    (all at the stream's end, also when that push finalises nothing): windows are ready by the TRACKED frames
    (``stream_tracked_frames``), ``latency_frames`` and ``latency_frames_max`` grow by ``lag`` and the rings hold
    ``stream_track_ring_frames`` frames.  ``_finalise_f0_tracked`` is one ``stream_f0_tracked``: the frames launch in candidate mode
    into a candidate ring, one block per stream for the recurrence (its costs in a float64 parity pair, backpointers in a
    ring) and the trace, then the running statistics and the excitation over the EMITTED frames.  All three kinds of F0
    statistics work with it.  Voicing has hysteresis at the edges of a voiced stretch.  ``None`` (the default): launches,
    kernel arguments, bytes and bits as before.

    State on the device, allocated once: per stream a ring of ``stream_ring_frames(core, context, max_push)`` frames of
    ppg, lft and excitation, the sine phase (float64) and two fade slots; an embedding table ``(n_streams, E)``; one
    upload buffer with a page-locked twin and one page-locked download buffer; with ``norm="running"`` per stream one
    carry record (``plan.norm_carry_bytes()``: two parity entries of every norm point's sums, never zeroed - a stream's
    first window resets it) and one scratch for the partial sums of a forward; with ``loudness="audio"`` the rings hold
    ``stream_loudness_ring_frames(core, context, max_push, hop)`` frames, and per stream there is a fourth ring, the audio
    (sample p at ``p % (cap hop)``), and the running maximum (a float32 parity pair, never zeroed - a stream's first frame
    starts it), plus one scratch for the power rows of the ``max_push + lag`` frames a push can finalise per stream.  A
    ``push`` is a driver over named steps, whose docstrings say what each launches: ``check_stream_chunks``, ``_append``
    (one upload, one ``stream_push``), with ``loudness="audio"`` ``_finalise_loudness`` (two ``stream_loudness`` launches, or
    none) and with ``f0="audio"`` ``_finalise_f0`` (two ``stream_f0`` launches when a frame became final, three with running F0
    statistics),
    ``stream_push_rows`` and, per ``max_batch`` ready rows, ``_forward_rows`` (``_run_rows``, a checked session's
    ``_check_rows``, ``_advance_carry``, the stitch); ``_collect`` waits once.  A push that
    completes no window runs no forward (``forwards`` counts them).

    Excitation: the phase is carried from push to push in float64 and equals the whole-utterance scan bit for bit, so
    with ``noise_amp == 0`` the streamed excitation IS ``signal_generator`` on the whole f0.  The noise is keyed by the
    stream's ``seed`` (mixed with the generator's) and the absolute sample index: it depends neither on the slot nor on
    the push sizes - and is another draw than ``signal_generator``'s, as ``convert_many``'s already is.  The F0 shift is
    ``F0Statistics.convert`` on the host per chunk, as in ``DecodeSession.convert`` (``f0="audio"``: on the device, when
    the frames are final).

    Latency, in frames of input (``latency_frames``, ``latency_frames_max``): a sample of frame t is returned by the
    push that delivers frame ``(t // core + 1) core + context - 1`` - its window's last context frame; the last ``fade /
    2`` frames of every core wait for the next window as well and return with frame ``(t // core + 2) core + context -
    1``; ``end`` returns everything still held; ``fade=0`` holds nothing back.  So ``core + context`` is the typical and
    ``2 core + context`` the worst delay.  With ``loudness="audio"`` every one of these is ``lag`` frames later: the push
    that delivers frame ``(t // core + 1) core + context - 1 + lag``, ``core + context + lag`` typical, ``2 core + context
    + lag`` worst.

    ``checked=True`` is ``DecodeSession``'s safety net for streams, which makes float16 activation storage usable live: every
    forward is judged before anything consumes it.  A stream needs that more than a file does.  With ``norm="running"`` a
    window that overflows the storage writes inf / NaN sums into the stream's carry record, every later window reads them,
    and the stream stays non-finite until it ends, with or without a horizon (``decay * inf`` is inf) - PCM-16 hides it, a
    NaN becomes 0 - and with any ``norm`` the fade zone a poisoned window stages leaks into the next push.  So after the
    model and before the stitch and the carry's flip, one launch (``engine.stream_check``, csrc/fastsvc_stream_check.hip)
    reports every row on the samples it contributes (``stream_check_spans``: context that is never emitted costs nothing)
    and counts the non-finite doubles of the carry entry the forward just wrote; the 16 bytes a row come down into
    page-locked memory and are waited for - the one synchronisation a checked forward adds (``_check_rows``).  A row with
    non-finite samples or carry is flagged, and all rows of its stream in that forward (``stream_rerun_rows``) run again in
    the next storage of ``fallback`` (names of ``STORAGE_CODES``, or one name; plans are built at construction): cut from
    the same rings, with the same parities and decays, so the re-run overwrites exactly those streams' carry entries,
    and copied over their rows on the device.  Rows of other streams are never run again and keep the bits of an unchecked
    session.  The decision is per forward, not per push: a stream's second forward of a push stages into the slot its
    first one read.  ``last_report`` is ``{id: [dict(window, storage, tried, nonfinite, clipped, max_abs,
    carry_nonfinite), ...]}`` for the windows that ran in the last push (empty lists included), the numbers those of the
    run whose samples were returned; ``totals(id)`` adds them up since ``open``, and the totals of a stream that ends are
    in that push's ``last_report["totals"][id]``.  There is no ``strict``: when the fallbacks are exhausted the samples are
    returned as they are and the report says so - ``nonfinite > 0`` and ``tried`` lists every storage, the last one
    included - because a live loop should not lose a push to an exception; a stream whose carry is still non-finite then
    STAYS non-finite.  ``fallback=()`` only reports.  The model is back in its first storage after every push, also when
    one raises.  ``checked=False`` (the default): no launch, wait, allocation or plan more than before.

    ``push`` validates everything before it uploads or enqueues anything: a ``ValueError`` leaves the session as it
    was, ``last_report`` included.  Not thread-safe.  ``out_channels`` must be 1 and the signal generator's only signal
    "sine".  Not built: graph capture of the per-push chain, several GPUs; for ``loudness="audio"`` a preset peak for
    calibration, a forgetting horizon for the maximum, ppg from audio (it needs an ASR model that lives outside this
    repository); ``f0="audio"`` without ``loudness="audio"``; a command-line flag for ``f0="audio"`` (the feature
    dumps hold no audio); for ``f0_track`` candidates beyond 4, a learned prior and tracking for ``f0="given"``; for ``RunningF0Stats`` a std
    floor or a mean-only mode, and ``f0="given"`` sessions (the host shifts per chunk there)."""

    def __init__(self, model, signal_generator, device, n_streams: int = 1, core: int = 32, context: Optional[int] = None,
                 fade: int = 8, max_push: Optional[int] = None, pcm16: bool = True, max_batch: int = 32, norm: str = "window",
                 horizon: Optional[float] = None, loudness: str = "given", checked: bool = False,
                 fallback: Sequence[str] = ("bfloat16",), f0: str = "given", f0_floor: float = 70.0, f0_ceil: float = 340.0,
                 f0_threshold: float = 0.15, f0_track: Optional[F0Track] = None):
        from .engine import FastSVCError
        self.model, self.signal_generator = model, signal_generator
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise FastSVCError("StreamSession needs a GPU device (no CPU fallback); got " + str(self.device))
        cfg = getattr(model, "_cfg", None)
        if cfg is None:
            raise ValueError("StreamSession needs a model with a generator configuration (FastSVCGenerator)")
        if int(getattr(model, "out_channels", 1)) != 1:
            raise ValueError("StreamSession supports out_channels == 1 only")
        if list(getattr(signal_generator, "signal_types", ["sine"])) != ["sine"]:
            raise ValueError("StreamSession needs a signal generator whose only signal type is \"sine\"")
        self.hop = int(signal_generator.hop_size)
        for name, value in self._check_args(cfg, self.hop, n_streams, core, context, fade, max_push, max_batch, norm, horizon,
                                            loudness, checked, fallback, f0, f0_floor, f0_ceil, f0_threshold,
                                            float(signal_generator.sample_rate), f0_track).items():
            setattr(self, name, value)
        if self.checked and self.fallback and not hasattr(model, "use_activation_storage"):
            raise ValueError("a checked session with fallback storages needs a model with use_activation_storage() "
                             "(FastSVCGenerator); pass fallback=() to report only")
        self.pcm16 = bool(pcm16)
        self._allocate(cfg)
        # a checked session: what the last push's windows reported, {id: [dict per window that ran]} (+ "totals")
        self.last_report: Optional[Dict[object, object]] = None
        self._slots: List[Optional[_Stream]] = [None] * self.n_streams        # per slot: the open stream's record
        self._ids: Dict[int, int] = {}                                       # open id -> slot
        self._next_id = 0
        self.forwards = 0
        # set to a dict to have push leave what it made there (tests): "excitation", per stream id the device tensors of
        # its chunks' excitation in order, "forwards", per forward (its rows, the assembled excitation rows), "y", per
        # forward (its rows, a clone of the waveforms that were stitched - after a checked session's fallbacks), and with
        # loudness="audio" "lft", per stream id the device tensors of its newly final frames' loudness in order; with
        # f0="audio" "f0" and "f0_shifted", likewise the frames' raw and shifted F0 (and "excitation" is per finalisation)
        self._stream_trace: Optional[Dict[str, object]] = None
        self._closed = False

    @staticmethod
    def _check_args(cfg, hop: int, n_streams: int = 1, core: int = 32, context: Optional[int] = None, fade: int = 8,
                    max_push: Optional[int] = None, max_batch: int = 32, norm: str = "window", horizon: Optional[float] = None,
                    loudness: str = "given", checked: bool = False, fallback: Sequence[str] = ("bfloat16",), f0: str = "given",
                    f0_floor: float = 70.0, f0_ceil: float = 340.0, f0_threshold: float = 0.15,
                    sample_rate: float = 24000.0, f0_track: Optional[F0Track] = None) -> Dict[str, object]:
        """The constructor's arguments against the generator configuration ``cfg`` and the signal generator's ``hop``, with
        no device: a ``ValueError`` for the first one that is refused, else the session's attributes they resolve to -
        the arguments as given or defaulted (``fallback`` a tuple of storage names; a string is one name), ``channels``,
        ``lag``, the rings' ``cap``, the floats ``_slice`` a stream takes
        of the upload buffer (16-byte aligned) and ``_down_elems``, the samples of the download buffer (a push returns at
        most the frames a ring holds per stream, every row's run padded to 8 samples)."""
        from .engine import STORAGE_CODES, STREAM_LOUDNESS_MAX_FRAMES, STREAM_MAX_PUSH, f0_lags
        fallback = (fallback,) if isinstance(fallback, str) else tuple(fallback)
        for name in fallback:
            if name not in STORAGE_CODES:
                raise ValueError(f"fallback storage must be one of {sorted(STORAGE_CODES)}, got {name!r}")
        core = int(core)
        context = -(-receptive_field_frames(cfg) // 4) * 4 if context is None else int(context)
        fade = int(fade)
        _check_window_sizes(core, context, fade)
        max_push = core if max_push is None else int(max_push)
        n_streams, max_batch = int(n_streams), int(max_batch)
        if n_streams < 1 or max_batch < 1:
            raise ValueError("StreamSession needs n_streams >= 1 and max_batch >= 1")
        if not 1 <= max_push <= STREAM_MAX_PUSH:
            raise ValueError(f"max_push must be in [1, {STREAM_MAX_PUSH}], got {max_push}")
        takes_emb = bool(cfg.use_spk_emb)
        if norm not in ("window", "running"):
            raise ValueError(f"norm must be \"window\" or \"running\", got {norm!r}")
        if norm == "running" and not takes_emb:
            raise ValueError("norm=\"running\" needs a model that takes a speaker embedding: without one nothing is normalised")
        if horizon is not None and norm != "running":
            raise ValueError("horizon forgets running statistics: it needs norm=\"running\"")
        horizon = check_horizon(horizon, core)
        if loudness not in ("given", "audio"):
            raise ValueError(f"loudness must be \"given\" or \"audio\", got {loudness!r}")
        if f0 not in ("given", "audio"):
            raise ValueError(f"f0 must be \"given\" or \"audio\", got {f0!r}")
        if f0 == "audio":
            if loudness != "audio":
                raise ValueError("f0=\"audio\" needs loudness=\"audio\": the audio ring exists only there")
            f0_lags(sample_rate, f0_floor, f0_ceil)      # (ValueError: tau_max > 1024, or no lag at all)
            if not float(f0_threshold) > 0.0:
                raise ValueError(f"f0_threshold must be > 0, got {f0_threshold}")
        if f0_track is not None:
            if not isinstance(f0_track, F0Track):
                raise ValueError(f"f0_track must be None or an F0Track, got {f0_track!r}")
            if f0 != "audio":
                raise ValueError("f0_track tracks the F0 the session makes: it needs f0=\"audio\" (tracking a given F0 is not built)")
        lag = stream_loudness_lag(hop) if loudness == "audio" else 0
        track_lag = 0 if f0_track is None else f0_track.lag
        cap = stream_ring_frames(core, context, max_push) if loudness == "given" else \
            stream_loudness_ring_frames(core, context, max_push, hop) if f0_track is None else \
            stream_track_ring_frames(core, context, max_push, hop, track_lag)
        if f0_track is not None and max_push + lag + track_lag > STREAM_LOUDNESS_MAX_FRAMES:
            raise ValueError(f"max_push + the loudness lag + the tracker's lag must be at most {STREAM_LOUDNESS_MAX_FRAMES} frames, "
                             f"got {max_push + lag + track_lag}")
        C = int(cfg.in_channels)
        return dict(core=core, context=context, fade=fade, max_push=max_push, n_streams=n_streams, max_batch=max_batch,
                    channels=C, _takes_emb=takes_emb, norm=norm, horizon=horizon, loudness=loudness, lag=lag, cap=cap,
                    checked=bool(checked), fallback=fallback, f0=f0, f0_floor=float(f0_floor), f0_ceil=float(f0_ceil),
                    f0_threshold=float(f0_threshold), f0_track=f0_track, track_lag=track_lag,
                    _slice=-(-max_push * (C + 1 + hop) // 4) * 4, _down_elems=n_streams * (cap * hop + 8 * (cap // core + 2)))

    def _allocate(self, cfg) -> None:
        """The session's device and page-locked buffers, sized by what ``_check_args`` resolved (the class docstring lists
        them)."""
        dev, n, cap, hop, C = self.device, self.n_streams, self.cap, self.hop, self.channels
        max_push, loudness, norm = self.max_push, self.loudness, self.norm
        self._ppg = torch.empty((n, cap, C), dtype=torch.float32, device=dev)
        self._lft = torch.empty((n, cap * hop), dtype=torch.float32, device=dev)
        self._exc = torch.empty((n, cap * hop), dtype=torch.float32, device=dev)
        self._phase = torch.empty((n, 2), dtype=torch.float64, device=dev)
        self._audio = self._peak = self._loud_scratch = None
        if loudness == "audio":
            from .engine import stream_loudness_scratch_bytes
            # the audio ring (sample p at p % (cap hop)), the running maximum's parity pair (never zeroed: a stream's
            # first frame starts it) and the power rows of the most frames a push can finalise per stream
            self._audio = torch.empty((n, cap * hop), dtype=torch.float32, device=dev)
            self._peak = torch.empty((n, 2), dtype=torch.float32, device=dev)
            self._loud_scratch = torch.empty(stream_loudness_scratch_bytes(n, max_push + self.lag), dtype=torch.uint8, device=dev)
        self._f0_raw = self._f0_shift = self._f0_rec = None
        if self.f0 == "audio":
            # the raw and the shifted F0 of the final frames (frame f at f % cap): what the excitation was made from
            self._f0_raw = torch.empty((n, cap), dtype=torch.float32, device=dev)
            self._f0_shift = torch.empty((n, cap), dtype=torch.float32, device=dev)
            # running source statistics: per stream two parity entries of (w, S1, S2, voiced frames), never zeroed - a stream's
            # first frame starts from zeros - addressed by the phase record's ``parity``
            self._f0_rec = torch.empty((n, 2, 4), dtype=torch.float64, device=dev)
        self._f0_cand = self._f0_back = self._f0_track_rec = None
        if self.f0_track is not None:
            # the tracker: the final frames' candidates (frame f at f % cap: 4 x (tau_hat, s)), their backpointers and best
            # state (8 bytes a frame) and per stream two parity entries of the recurrence's costs (5 of 8 doubles), never
            # zeroed - a stream's first frame starts fresh - addressed by ``track_parity``
            self._f0_cand = torch.empty((n, cap, 4, 2), dtype=torch.float32, device=dev)
            self._f0_back = torch.empty((n, cap, 8), dtype=torch.uint8, device=dev)
            self._f0_track_rec = torch.empty((n, 2, 8), dtype=torch.float64, device=dev)
        self._layout = StreamStitchLayout(n, hop, self.fade)
        self._stage = torch.empty(max(self._layout.stage_elems, 1), dtype=torch.float32, device=dev)
        self._emb = torch.zeros((n, max(int(cfg.spk_emb_size), 1)), dtype=torch.float32, device=dev)
        self._h_up = torch.empty(n * self._slice, dtype=torch.float32, pin_memory=True)
        self._d_up = torch.empty(n * self._slice, dtype=torch.float32, device=dev)
        self._h_down = _PinnedSet()
        self._h_down.get("w", (self._down_elems,))
        self._up_done: Optional[torch.cuda.Event] = None
        self._carry = self._norm_scratch = self._report = self._h_report = None
        plans = self._fallback_plans() if self.checked else None
        if norm == "running":
            plans = plans or [self.model.plan]
            plan = plans[0]
            if any(p.norm_carry_bytes() != plan.norm_carry_bytes() for p in plans):
                raise ValueError("the fallback storages' plans carry records of another size than the model's own")
            self._carry = torch.empty((n, plan.norm_carry_bytes() // 8), dtype=torch.float64, device=dev)
            scratch = max(p.norm_running_scratch_bytes(self.max_batch, p.padded_frames(self.core + 2 * self.context)) for p in plans)
            self._norm_scratch = torch.empty(max(scratch, 1), dtype=torch.uint8, device=dev)
        if self.checked:
            # one forward's row reports on the device and their page-locked twin (16 bytes a row)
            self._report = torch.empty((self.max_batch, 4), dtype=torch.int32, device=dev)
            self._h_report = torch.empty((self.max_batch, 4), dtype=torch.int32, pin_memory=True)
        self._emb_rows: Dict[tuple, torch.Tensor] = {}                       # row slots of a forward -> their index tensor

    def _fallback_plans(self) -> list:
        """A checked session: the model's own plan and that of every fallback storage, each built once here
        (``use_activation_storage`` keeps a plan per storage) so that the first fallback of a live stream builds nothing.
        The model is back in its first storage afterwards."""
        model = self.model
        plans = [model.plan]
        first = getattr(model, "activation_storage", "float32")
        try:
            for name in self.fallback:
                model.use_activation_storage(name)
                plans.append(model.plan)
        finally:
            if getattr(model, "activation_storage", first) != first:
                model.use_activation_storage(first)
        return plans

    latency_frames = property(lambda self: self.core + self.context + self.lag + self.track_lag,
                              doc="the typical delay, in frames of input: core + context (+ the loudness lag with loudness=\"audio\""
                                  ", + the tracker's lag with f0_track)")
    latency_frames_max = property(lambda self: 2 * self.core + self.context + self.lag + self.track_lag,
                                  doc="the worst delay (the last fade / 2 frames of a core): 2 core + context (+ the loudness lag, + "
                                      "the tracker's lag)")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self) -> None:
        """Wait for the session's device work and release its device and page-locked buffers."""
        if self._closed:
            return
        self._closed = True
        torch.cuda.current_stream(self.device).synchronize()
        self._ppg = self._lft = self._exc = self._phase = self._stage = self._emb = self._carry = self._norm_scratch = None
        self._report = self._h_report = None
        self._audio = self._peak = self._loud_scratch = self._f0_raw = self._f0_shift = self._f0_rec = None
        self._f0_cand = self._f0_back = self._f0_track_rec = None
        self._h_up = self._d_up = self._h_down = self._up_done = None
        self._slots, self._ids = [None] * self.n_streams, {}

    def open(self, trg_emb=None, src_f0_stats=None, trg_f0_stats: Optional[Sequence[float]] = None, seed: int = 0) -> int:
        """A new stream in a free slot -> its id (ids are never reused; a slot is, after ``end``).  ``trg_emb``: the target
        speaker's embedding or None - every open stream must agree on having one, because a forward takes ``spk_emb`` for
        all its rows or for none.  ``src_f0_stats`` and ``trg_f0_stats`` ([mean, std] of log F0): both or neither; a
        ``RunningF0Stats`` as ``src_f0_stats`` (``f0="audio"`` sessions) makes the stream run its own source statistics.  A
        ``ValueError`` leaves the session as it was."""
        if self._closed:
            raise RuntimeError("StreamSession is closed")
        free = [s for s in range(self.n_streams) if self._slots[s] is None]
        if not free:
            raise ValueError(f"all {self.n_streams} stream slots are busy")
        has_emb = trg_emb is not None
        if has_emb and not self._takes_emb:
            raise ValueError("the model does not take a speaker embedding")
        if any(st.emb != has_emb for st in self._slots if st is not None):
            raise ValueError("every open stream needs a speaker embedding, or none does")
        if (src_f0_stats is None) != (trg_f0_stats is None):
            raise ValueError("an F0 shift needs src_f0_stats and trg_f0_stats")
        running = None
        if isinstance(src_f0_stats, RunningF0Stats):
            if self.f0 != "audio":
                raise ValueError("running F0 statistics need a session with f0=\"audio\": with f0=\"given\" the host shifts "
                                 "every chunk (not built)")
            running, src_f0_stats, trg_f0_stats = src_f0_stats.constants(trg_f0_stats), None, None
        s = free[0]
        if has_emb:
            e = np.asarray(trg_emb, dtype=np.float32).reshape(-1)
            if e.size != self._emb.shape[1]:
                raise ValueError(f"trg_emb must hold {self._emb.shape[1]} values, got {e.size}")
            self._emb[s].copy_(torch.from_numpy(np.ascontiguousarray(e)))
        sid = self._next_id
        self._next_id += 1
        key = (int(getattr(self.signal_generator, "seed", 0)) * 0x9E3779B97F4A7C15 + int(seed)) & 0xFFFFFFFFFFFFFFFF
        self._slots[s] = _Stream(id=sid, slot=s, emb=has_emb, seed=key, from_audio=self.loudness == "audio",
                                 stats=None if src_f0_stats is None else (list(src_f0_stats), list(trg_f0_stats)),
                                 running=running, track=self.f0_track is not None)
        if self.checked:
            self._slots[s].totals = dict(windows=0, fell_back=0, nonfinite=0, clipped=0, max_abs=0.0, storages={})
        self._ids[sid] = s
        self._layout.reset(s)
        return sid

    def norm_frames(self, sid: int) -> float:
        """The weighted frames ``norm="running"`` carries for stream ``sid``: the frames of the cores that ran, each core
        multiplied by the decays of the cores behind it - without a ``horizon`` simply their count.  0.0 before the
        stream's first window and for a stream without an embedding, which carries nothing."""
        if self.norm != "running":
            raise ValueError("norm_frames needs norm=\"running\"")
        if sid not in self._ids:
            raise ValueError(f"stream {sid} is not open (unknown, or it has ended)")
        return float(self._slots[self._ids[sid]].norm_w)

    def f0_stats(self, sid: int) -> Dict[str, float]:
        """What a stream opened with ``RunningF0Stats`` knows of its source after the frames that are final: ``dict(mean, std,
        voiced_frames, weight, observed_mean, observed_std)``.  ``mean`` and ``std`` are the statistics of log F0 the last
        final voiced frame was shifted with (``m_p + mu``, ``sqrt(var)``: the prior's before the first one); ``weight`` is
        ``w``, ``voiced_frames`` their count; ``observed_mean`` and ``observed_std`` are the same without the prior (``m_p +
        S1 / w``, ``sqrt(S2 / w - (S1 / w)^2)``), NaN while ``w == 0`` - what to save for a speaker and hand back as ``prior``
        with a large ``prior_frames`` next time.  Reads the stream's current record on the device: one download of 32 bytes
        and a WAIT for everything enqueued before it - for the end of a conversation, not for the push loop.  ``ValueError``
        for a stream that is not open or runs no statistics."""
        if sid not in self._ids:
            raise ValueError(f"stream {sid} is not open (unknown, or it has ended)")
        st = self._slots[self._ids[sid]]
        if st.running is None:
            raise ValueError(f"stream {sid} was not opened with RunningF0Stats")
        m_p, s_p, n0, _, _, _ = st.running
        # (before the stream's first final frame the record holds whatever the slot's last stream left: the state is zeros)
        w, s1, s2, count = (0.0,) * 4 if st.first else self._f0_rec[st.slot, st.parity].cpu().tolist()
        N = n0 + w
        mu = s1 / N
        out = dict(mean=m_p + mu, std=math.sqrt((n0 * s_p * s_p + s2) / N - mu * mu), voiced_frames=int(count), weight=w,
                   observed_mean=float("nan"), observed_std=float("nan"))
        if w > 0.0:
            om = s1 / w
            out["observed_mean"], out["observed_std"] = m_p + om, math.sqrt(max(s2 / w - om * om, 0.0))
        return out

    def end(self, ids) -> Dict[int, np.ndarray]:
        """``push({}, end=ids)``: flush these streams and free their slots."""
        return self.push({}, end=ids)

    @torch.no_grad()
    def push(self, chunks, end=()) -> Dict[int, np.ndarray]:
        """Append a chunk to every stream of ``chunks`` - ``{id: dict(ppg=(n, C), f0=(n,) | (n, 1), lft=(n hop,) | (n hop,
        1))}``, ``0 <= n <= max_push``; with ``loudness="audio"`` the chunk carries ``audio=(n hop,) | (n hop, 1)`` in place of
        ``lft`` - run every window that became ready, and return ``{id: samples}`` for every id of
        ``chunks`` and ``end``: the stream's next samples, int16 (``pcm16``) or float32, a new array, empty when no
        window of the stream ran.  Streams in ``end`` end after their chunk: their remaining windows run in this call
        and their slots are free afterwards."""
        if self._closed:
            raise RuntimeError("StreamSession is closed")
        # nothing is touched before every chunk has passed
        parts, ids, end = check_stream_chunks(chunks, end, self._ids, self.channels, self.hop, self.max_push, self.loudness,
                                              self.f0)
        pushed = [sid for sid, part in parts.items() if part[0] > 0]
        if pushed:
            self._append(parts, pushed)
        if self.loudness == "audio":
            final = self._finalise_loudness(ids, end)
            if self.f0_track is not None:
                self._finalise_f0_tracked(final, ids, end)
            elif self.f0 == "audio" and final:
                self._finalise_f0(final)
        streams = sorted((self._slots[self._ids[sid]] for sid in ids), key=lambda st: st.slot)
        rows, forget = stream_push_rows(streams, end, self.core, self.context, self.norm == "running", self.horizon)
        for r in rows:
            self._slots[r.stream].done = r.k + 1
        # per slot, the frames whose features are complete: what the stitch layout clips a zone by and what the assembly may
        # cut rows from.  With loudness="audio" the ppg and excitation rings are `lag` frames ahead of that, and the ring
        # is sized for it (stream_loudness_ring_frames): a row still lies inside the frames they retain
        seen = [0 if st is None else st.complete for st in self._slots]
        for r in rows if self.loudness == "audio" else ():
            if r.in_lo < self._slots[r.stream].seen - self.cap:
                raise RuntimeError(f"stream slot {r.stream}: frame {r.in_lo} has left the ring of {self.cap} frames")
        down, off = [], 0
        report = {sid: [] for sid in ids} if self.checked else None
        for c0 in range(0, len(rows), self.max_batch):
            host, lay, off = self._forward_rows(rows[c0: c0 + self.max_batch], forget[c0: c0 + self.max_batch], seen, off, report)
            down.append((host, lay))
        out = self._collect(ids, down)
        if self.checked:
            if end:                                      # (a stream that ends leaves its totals here: its slot is freed below)
                report["totals"] = {sid: self.totals(sid) for sid in end}
            self.last_report = report
        for sid in end:
            s = self._ids.pop(sid)
            self._slots[s] = None
            self._layout.reset(s)
        return out

    def _append(self, parts, pushed: Sequence[int]) -> None:
        """The chunks of the streams ``pushed`` (ids, each with at least one frame; ``parts`` as ``check_stream_chunks``
        returns them) go into the rings: waits until the last upload has left the page-locked twin, shifts the F0 of a
        stream that has statistics, packs stream j's ppg, f0 and lft (or audio) into slice j, uploads the used slices in
        one copy and appends them, and synthesises their excitation, in one ``stream_push``.  Reads every stream's
        ``seen``, ``first`` and ``parity`` and leaves them advanced: ``seen`` by the chunk, the phase record's other entry
        current.  Traces the chunks' excitation.  With ``f0="audio"`` the slices hold ppg and audio only, the one
        ``stream_push`` copies and synthesises nothing, and only ``seen`` advances: ``_finalise_f0`` owns the phase record
        and the trace."""
        from .engine import stream_push
        hop, C, dev = self.hop, self.channels, self.device
        if self._up_done is not None:
            self._up_done.synchronize()                  # (the page-locked twin is still being read by the last upload)
        h = self._h_up.numpy()
        entries = []                                     # per stream (slot, n, up_off, pos, first, parity, seed), as stream_push takes them
        own_f0 = self.f0 == "audio"                     # (no f0 in the slice, nothing synthesised: ``_finalise_f0`` does that)
        for j, sid in enumerate(pushed):
            n, ppg, f0, lft = parts[sid]
            st = self._slots[self._ids[sid]]
            o = j * self._slice
            h[o: o + n * C] = ppg.reshape(-1)
            if own_f0:
                h[o + n * C: o + n * (C + hop)] = lft
            else:
                if st.stats is not None:
                    f0 = F0Statistics().convert(np.asarray(f0, dtype=np.float64), st.stats[0], st.stats[1])
                h[o + n * C: o + n * C + n] = f0
                h[o + n * C + n: o + n * (C + 1 + hop)] = lft
            entries.append((st.slot, n, o, st.seen, st.first, st.parity, st.seed))
        used = len(pushed) * self._slice
        self._d_up[:used].copy_(self._h_up[:used], non_blocking=True)
        self._up_done = torch.cuda.Event()
        self._up_done.record(torch.cuda.current_stream(dev))
        sg = self.signal_generator
        # (with loudness="audio" the chunk's third array is audio: the same copy appends it to the audio ring)
        stream_push(self._d_up, *zip(*entries), self._ppg, self._audio if self.loudness == "audio" else self._lft,
                    None if own_f0 else self._exc, None if own_f0 else self._phase, self.max_push, float(sg.sample_rate),
                    float(sg.sine_amp), float(sg.noise_amp))
        for sid in pushed:
            st = self._slots[self._ids[sid]]
            n = parts[sid][0]
            if own_f0:
                st.seen += n
                continue
            if self._stream_trace is not None:
                idx = (torch.arange(st.seen, st.seen + n, device=dev) % self.cap)
                self._stream_trace.setdefault("excitation", {}).setdefault(sid, []).append(
                    self._exc[st.slot].view(self.cap, hop)[idx].reshape(-1))
            st.seen += n
            st.first = False
            st.parity ^= 1                               # (enqueued: the other entry is the slot's phase now)

    def _finalise_loudness(self, ids: Sequence[int], end: Sequence[int]) -> None:
        """``loudness="audio"``: the frames of the streams ``ids`` that became final - by their audio's arrival, or by the
        stream's end (``end``), with or without a chunk - go from the audio ring into the lft ring: two launches for all
        streams (``stream_loudness``), none when no frame did.  Reads every stream's ``seen``, ``final`` and
        ``loud_parity`` and leaves ``final`` advanced and the peak record's other entry current.  Traces the frames'
        loudness.  Returns the entries it finalised, ``(slot, first_frame, n, seen, ended, parity)`` per stream."""
        from .engine import stream_loudness
        entries = []                                     # per stream (slot, first_frame, n, seen, ended, parity), as stream_loudness takes them
        for sid in ids:
            st = self._slots[self._ids[sid]]
            final = stream_final_frames(st.seen, sid in end, self.hop)
            if final > st.final:
                entries.append((st.slot, st.final, final - st.final, st.seen, sid in end, st.loud_parity))
        if not entries:
            return entries
        stream_loudness(self._audio, self._lft, self._peak, self._loud_scratch, *zip(*entries), self.cap, self.max_push + self.lag,
                        float(self.signal_generator.sample_rate))
        for s, f, n, _, _, _ in entries:
            st = self._slots[s]
            if self._stream_trace is not None:
                idx = (torch.arange(f, f + n, device=self.device) % self.cap)
                self._stream_trace.setdefault("lft", {}).setdefault(st.id, []).append(
                    self._lft[s].view(self.cap, self.hop)[idx].reshape(-1))
            st.final = f + n
            st.loud_parity ^= 1                          # (enqueued: the other entry is the slot's peak now)
        return entries

    def _finalise_f0(self, final) -> None:
        """``f0="audio"``: the frames ``_finalise_loudness`` just finalised (``final``, its entries) get their F0 from the
        audio ring, the F0 shift of a stream that has statistics - on the device, in float64 - and their excitation: two
        launches for all streams (``stream_f0``), three (``stream_f0_running``) when one of them runs its source statistics,
        whose record is read and written like the phase's.  Reads every stream's ``parity`` and leaves the phase record's
        other entry current.  Traces the frames' raw F0 (``"f0"``), shifted F0 (``"f0_shifted"``) and ``"excitation"``."""
        from .engine import stream_f0, stream_f0_running
        sg = self.signal_generator
        slots, first, n, seen, ended, _ = zip(*final)
        sts = [self._slots[s] for s in slots]
        rings = (self._audio, self._f0_raw, self._f0_shift, self._exc, self._phase)
        entries = (slots, first, n, seen, ended, [st.parity for st in sts], [st.seed for st in sts],
                   [None if st.stats is None else (*st.stats[0][:2], *st.stats[1][:2]) for st in sts])
        consts = (self.cap, self.max_push + self.lag, float(sg.sample_rate), self.f0_floor, self.f0_ceil, self.f0_threshold,
                  float(sg.sine_amp), float(sg.noise_amp))
        if any(st.running is not None for st in sts):
            stream_f0_running(*rings, self._f0_rec, *entries, [st.running for st in sts], *consts)
        else:
            stream_f0(*rings, *entries, *consts)
        for st, f, k in zip(sts, first, n):
            if self._stream_trace is not None:
                idx = (torch.arange(f, f + k, device=self.device) % self.cap)
                tr = self._stream_trace
                tr.setdefault("f0", {}).setdefault(st.id, []).append(self._f0_raw[st.slot][idx])
                tr.setdefault("f0_shifted", {}).setdefault(st.id, []).append(self._f0_shift[st.slot][idx])
                tr.setdefault("excitation", {}).setdefault(st.id, []).append(
                    self._exc[st.slot].view(self.cap, self.hop)[idx].reshape(-1))
            st.first = False
            st.parity ^= 1                               # (enqueued: the other entry is the slot's phase now)

    def _finalise_f0_tracked(self, final, ids: Sequence[int], end: Sequence[int]) -> None:
        """``_finalise_f0`` of a session with ``f0_track``: the frames ``_finalise_loudness`` just finalised (``final``) get their
        CANDIDATES from the audio ring and advance the tracker, and the frames whose tracked F0 became final with them
        (``stream_tracked_frames``: ``track_lag`` behind, all at a stream's end - also of a stream that ends in a push that
        finalises nothing) get it, its shift and their excitation: one ``stream_f0_tracked`` (the frames launch in candidate
        mode, the tracker, the running shift when a stream runs statistics, the excitation), or nothing when no stream has
        either.  Leaves ``tracked`` advanced, the tracker record's other entry current for a stream with new frames and the
        phase (and statistics) record's for a stream that emitted.  Traces the new frames' ``"f0_candidates"`` and the emitted
        frames' tracked raw F0 (``"f0"``), ``"f0_shifted"`` and ``"excitation"``."""
        from .engine import stream_f0_tracked
        sg, tk = self.signal_generator, self.f0_track
        new = {e[0]: (e[1], e[2]) for e in final}        # slot -> (first newly final frame, how many)
        work = []
        for sid in ids:
            st = self._slots[self._ids[sid]]
            first, n = new.get(st.slot, (st.final, 0))
            emit = stream_tracked_frames(st.final, sid in end, tk.lag) - st.tracked
            if n or emit:
                work.append((st, first, n, sid in end, emit))
        if not work:
            return
        sts = [w[0] for w in work]
        running = [st.running for st in sts] if any(st.running is not None for st in sts) else None
        stream_f0_tracked(self._audio, self._f0_cand, self._f0_back, self._f0_raw, self._f0_shift, self._exc, self._phase,
                          self._f0_rec if running is not None else None, self._f0_track_rec,
                          [st.slot for st in sts], [w[1] for w in work], [w[2] for w in work], [st.seen for st in sts],
                          [w[3] for w in work], [st.parity for st in sts], [st.track_parity for st in sts],
                          [st.tracked for st in sts], [w[4] for w in work], [st.seed for st in sts],
                          [None if st.stats is None else (*st.stats[0][:2], *st.stats[1][:2]) for st in sts], running,
                          self.cap, self.max_push + self.lag + self.track_lag, float(sg.sample_rate), self.f0_floor, self.f0_ceil,
                          tk.cand_threshold, tk.lag, tk.lag_bias, tk.jump, tk.switch,
                          self.f0_threshold if tk.unvoiced is None else tk.unvoiced, float(sg.sine_amp), float(sg.noise_amp))
        for st, first, n, _, emit in work:
            tr = self._stream_trace
            if tr is not None and n:
                idx = (torch.arange(first, first + n, device=self.device) % self.cap)
                tr.setdefault("f0_candidates", {}).setdefault(st.id, []).append(self._f0_cand[st.slot][idx])
            if tr is not None and emit:
                idx = (torch.arange(st.tracked, st.tracked + emit, device=self.device) % self.cap)
                tr.setdefault("f0", {}).setdefault(st.id, []).append(self._f0_raw[st.slot][idx])
                tr.setdefault("f0_shifted", {}).setdefault(st.id, []).append(self._f0_shift[st.slot][idx])
                tr.setdefault("excitation", {}).setdefault(st.id, []).append(
                    self._exc[st.slot].view(self.cap, self.hop)[idx].reshape(-1))
            if n:
                st.track_parity ^= 1                     # (enqueued: the other entry is the slot's tracker state now)
            if emit:
                st.tracked += emit
                st.first = False
                st.parity ^= 1                           # (enqueued: the other entry is the slot's phase now)

    def _forward_rows(self, chunk: Sequence[StreamRow], forget, seen: Sequence[int], off: int, report=None):
        """One forward over the rows ``chunk`` (at most ``max_batch``, as ``stream_push_rows`` orders them; ``forget``
        their entries, or nothing; ``seen`` per slot the frames rows may be cut from): lays out the stitch, cuts the rows
        from the rings and runs the model (``_run_rows``), a checked session then decides about every row before anything
        consumes it (``_check_rows``, which appends the rows' dicts to ``report``), the slots' carry records are made
        current (``_advance_carry``), and the rows are stitched into the page-locked download buffer from element ``off``.
        Without ``checked`` everything is enqueued and nothing waited for.  Returns ``(host, lay, off)``: the buffer's
        part, the batch's layout and the first element behind it.  Traces ``"y"``: the rows and a clone of the final ``y``."""
        lay = self._layout.batch(chunk, seen)
        y = self._run_rows(chunk, forget, seen, trace=True)
        if self.checked:
            self._check_rows(chunk, forget, seen, y, report)
        if self._stream_trace is not None:
            self._stream_trace.setdefault("y", []).append(
                ([(self._slots[r.stream].id, r.in_lo, r.in_hi, r.core_lo, r.core_hi) for r in chunk], y.clone()))
        self._advance_carry(chunk, forget)
        host, off = _stitch_to_host(y, lay, self._stage, self.pcm16, self._h_down, at=off)
        return host, lay, off

    def _carries(self, chunk: Sequence[StreamRow]) -> bool:
        """Whether the rows' streams carry running InstanceNorm sums (they all have an embedding, or none has)."""
        return self.norm == "running" and self._slots[chunk[0].stream].emb

    def _run_rows(self, chunk: Sequence[StreamRow], forget, seen: Sequence[int], trace: bool):
        """Cuts the rows ``chunk`` from the rings (``stream_assemble``) and runs the model in its current storage ->
        ``y`` (rows, 1, samples) float32.  With ``norm="running"`` and an embedding the forward reads entry
        ``norm_parity`` of the slots' carry records and writes the other one; the parities are NOT flipped here, so the
        same rows run again - a fallback - read the same sums and simply overwrite what the first run wrote.  Counts the
        forward and, with ``trace``, traces its rows and excitation."""
        from .engine import stream_assemble
        lens = [r.frames for r in chunk]
        slots = tuple(r.stream for r in chunk)
        ppg, lft, sine = stream_assemble(self._ppg, self._lft, self._exc, seen, slots, [r.in_lo for r in chunk], lens, max(lens))
        if trace and self._stream_trace is not None:
            self._stream_trace.setdefault("forwards", []).append(
                ([(self._slots[r.stream].id, r.in_lo, r.in_hi, r.core_lo, r.core_hi) for r in chunk], sine.clone()))
        emb = None
        if self._slots[slots[0]].emb:
            if slots not in self._emb_rows:              # (the steady state repeats one tuple: its index tensor is uploaded once)
                if len(self._emb_rows) >= 256:
                    self._emb_rows.clear()
                self._emb_rows[slots] = torch.as_tensor(slots, dtype=torch.int64, device=self.device)
            emb = self._emb.index_select(0, self._emb_rows[slots])
        if self._carries(chunk):
            # window k of a stream: its core starts own_lo frames into the row, core_lo frames of the stream lie in
            # front of it, window 0 resets the slot's carry; the slot's parity says which entry of its record is current
            running = (list(slots), [r.own_lo for r in chunk], [r.own_hi for r in chunk], [r.core_lo for r in chunk],
                       [int(r.k == 0) for r in chunk], [self._slots[s].norm_parity for s in slots])
            decay = None if self.horizon is None else tuple([f[i] for f in forget] for i in range(3))
            y = self.model(ppg, sine, lft, emb, lengths=lens, norm_running=running, norm_carry=self._carry,
                           norm_scratch=self._norm_scratch, norm_decay=decay).to(torch.float32)
        else:
            y = self.model(ppg, sine, lft, emb, lengths=lens).to(torch.float32)
        self.forwards += 1
        return y

    def _advance_carry(self, chunk: Sequence[StreamRow], forget) -> None:
        """The forward over ``chunk`` is enqueued and its samples are the ones that will be delivered: with
        ``norm="running"`` and an embedding the other entry of every slot's carry record is the current one now, and it
        holds the rows' weighted frames (``norm_w``).  Host state only."""
        if not self._carries(chunk):
            return
        slots = [r.stream for r in chunk]
        for s in dict.fromkeys(slots):                   # (enqueued: the other entry is the slot's carry now)
            self._slots[s].norm_parity ^= 1
        for s, f in zip(slots, forget):                  # (... and it holds this many weighted frames)
            self._slots[s].norm_w = f[3]

    def _check_rows(self, chunk: Sequence[StreamRow], forget, seen: Sequence[int], y: torch.Tensor, report) -> None:
        """A checked session's decision about one forward, between the model and everything that consumes ``y`` - the
        stitch, which stages a fade zone for the next push, and the carry record's flip.  ``stream_check`` reports every
        row on the span it contributes (``stream_check_spans``) and, with a carry, on the entry the forward just wrote;
        the report (16 bytes a row) comes down into page-locked memory and is WAITED for: the one synchronisation a
        checked forward adds.  A row is flagged by non-finite samples or a non-finite carry; every row of a flagged
        row's stream (``stream_rerun_rows``) runs again in the next storage of ``fallback`` (``storage_fallback``) - the
        same rows cut from the same rings, the same parities and decays, so the re-run overwrites exactly those streams'
        carry entries - is checked again and copied over its rows of ``y`` on the device.  Rows of streams that were
        not flagged are never run again.  Appends every row's dict to ``report[id]`` and adds it to the stream's totals."""
        from .engine import stream_check
        lo, hi = stream_check_spans(chunk, self.hop, self._layout.half)
        carried = self._carries(chunk)
        rep = np.zeros((len(chunk), 4), dtype=np.int32)
        again: List[int] = []                            # the rows to run again, by the latest reports

        def check(idx, yy) -> None:
            """Rows ``idx`` of the chunk, whose waveforms are the rows of ``yy``: their reports into ``rep``."""
            n, kw = len(idx), {}
            if carried:
                kw = dict(carry=self._carry, slots=[chunk[j].stream for j in idx], entry_doubles=self._carry.shape[1] // 2,
                          entries=[self._slots[chunk[j].stream].norm_parity ^ 1 for j in idx])
            stream_check(yy, [lo[j] for j in idx], [hi[j] for j in idx], out=self._report[:n], **kw)
            self._h_report[:n].copy_(self._report[:n], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
            rep[idx] = self._h_report[:n].numpy()
            bad = np.nonzero((rep[:, 0] > 0) | (rep[:, 3] > 0))[0]
            again[:] = stream_rerun_rows(chunk, bad) if bad.size else []

        def rerun(name, flagged) -> None:
            idx = stream_rerun_rows(chunk, flagged)      # (``again``: whole streams already)
            y2 = self._run_rows([chunk[j] for j in idx], [forget[j] for j in idx] if forget else forget, seen, trace=False)
            check(idx, y2)
            a = 0
            while a < len(idx):                          # (device copies, one per run of neighbouring rows)
                b = a + 1
                while b < len(idx) and idx[b] == idx[b - 1] + 1:
                    b += 1
                y[idx[a]: idx[a] + b - a, :, :y2.shape[-1]].copy_(y2[a:b])
                a = b

        check(list(range(len(chunk))), y)
        first = getattr(self.model, "activation_storage", "float32")
        storage, tried, still = storage_fallback(self.model, self.fallback, len(chunk), lambda i: i in again, rerun)
        for j in still if self.fallback else ():         # (fallbacks exhausted: ``tried`` lists every storage, the last included)
            tried[j] = tried[j] + [storage[j]]
        max_abs = rep[:, 2].copy().view(np.float32).tolist()
        for j, (r, (nonfinite, clipped, _, carry_bad)) in enumerate(zip(chunk, rep.tolist())):
            st = self._slots[r.stream]
            d = dict(window=r.k, storage=storage[j], tried=tried[j], nonfinite=nonfinite, clipped=clipped,
                     max_abs=max_abs[j], carry_nonfinite=carry_bad)
            report[st.id].append(d)
            t = st.totals
            t["windows"] += 1
            t["fell_back"] += int(d["storage"] != first)
            t["nonfinite"] += d["nonfinite"]
            t["clipped"] += d["clipped"]
            t["max_abs"] = max(t["max_abs"], d["max_abs"])
            t["storages"][d["storage"]] = t["storages"].get(d["storage"], 0) + 1

    def totals(self, sid: int) -> Dict[str, object]:
        """A checked session: what the windows of the open stream ``sid`` reported since ``open`` - ``windows`` that ran,
        how many ``fell_back`` to another storage, the sums of ``nonfinite`` and ``clipped`` samples, the largest
        ``max_abs``, and ``storages``: windows per storage their samples came from.  A copy.  (A stream that has ended:
        the ending push's ``last_report["totals"][sid]``.)"""
        if not self.checked:
            raise ValueError("totals needs checked=True")
        if sid not in self._ids:
            raise ValueError(f"stream {sid} is not open (unknown, or it has ended)")
        t = self._slots[self._ids[sid]].totals
        return dict(t, storages=dict(t["storages"]))

    def _collect(self, ids: Sequence[int], down) -> Dict[int, np.ndarray]:
        """Waits for the push's forwards, if any ran (one ``synchronize``), and copies every stream's runs out of their
        download buffers ``down = [(host, lay), ...]`` -> ``{id: samples}`` for ``ids``, new arrays, empty for a stream
        none of whose windows ran."""
        pieces: Dict[int, list] = {self._ids[sid]: [] for sid in ids}
        if down:
            torch.cuda.current_stream(self.device).synchronize()
        for host, lay in down:
            h = host.numpy()
            for (s, t_lo, t_hi), o in zip(lay["runs"], lay["dst_off"]):
                pieces[s].append(h[o: o + t_hi - t_lo])
        dtype = np.int16 if self.pcm16 else np.float32
        out = {}
        for sid in ids:
            ps = pieces[self._ids[sid]]
            out[sid] = np.concatenate(ps) if ps else np.empty(0, dtype=dtype)      # (a copy: never the page-locked buffer)
        return out


def _read_f0_mean(stats_dir: str, name: str) -> np.ndarray:
    import yaml
    with open(os.path.join(stats_dir, f"{name}.yml")) as f:
        y = yaml.safe_load(f)
    return np.array([float(y["stats"]["mean"]), 1.0])       # std forced to 1 (decode_fastsvc.py:165,176)


def main(argv=None) -> None:                                  # pragma: no cover - exercised on a GPU box
    import yaml
    from . import FastSVCGenerator, SignalGenerator
    ap = argparse.ArgumentParser(description="Batched FastSVC decoding (cf. harana-decode-fastsvc)")
    ap.add_argument("--dumpdir", required=True, help="directory of per-utterance feature dumps (.npz / .h5)")
    ap.add_argument("--checkpoint", required=True, help="reference checkpoint (.pkl with ['model']['generator'])")
    ap.add_argument("--config", required=True, help="recipe yaml (generator_params, hop_size, sampling_rate, ...)")
    ap.add_argument("--outdir", required=True)
    ap.add_argument("--spk-emb", default=None, help=".npz of target-speaker embeddings keyed by speaker")
    ap.add_argument("--srcf0stats", default=None)
    ap.add_argument("--trgf0stats", default=None)
    ap.add_argument("--max-batch", type=int, default=32)
    ap.add_argument("--storage", default="float32", choices=["float32", "bfloat16", "float16", "auto"],
                    help="activation storage of the generator's forward (FastSVCGenerator.activation_storage); auto: float16 "
                         "with --checked --fallback bfloat16 (needs --resident; also with --stream)")
    ap.add_argument("--checked", action="store_true",
                    help="with --resident: report non-finite and clipped samples per utterance and run the batches that "
                         "hold a non-finite utterance again in the --fallback storages (DecodeSession(checked=True)); with "
                         "--stream: per window, before its samples or its running statistics are used (StreamSession(checked=True))")
    ap.add_argument("--fallback", default=None,
                    help="comma-separated storages to fall back to, in order (default with --checked: bfloat16)")
    ap.add_argument("--resident", action="store_true",
                    help="keep the features on the device across target speakers (DecodeSession): ppg / lft are uploaded "
                         "once per group of dumps, PCM-16 is made on the device; same file names and contents")
    ap.add_argument("--resident-bytes", type=int, default=4 << 30,
                    help="device bytes of packed features one resident group may hold (default 4 GiB); a dump directory "
                         "larger than this is decoded group by group")
    ap.add_argument("--fanout", type=int, default=1,
                    help="with --resident: convert the target speakers in groups of N by DecodeSession.convert_many, whose "
                         "batches hold (utterance, speaker) rows - for source sets smaller than --max-batch; same file "
                         "names (default 1: one convert per speaker)")
    ap.add_argument("--window", default=None, metavar="CORE[,CONTEXT[,FADE]]",
                    help="with --resident: decode every utterance as overlapping windows of CORE frames "
                         "(DecodeSession.convert_windowed; CONTEXT frames read on each side, default the generator's "
                         "receptive field; cross-fade over FADE frames, default 8) - for recordings longer than one forward "
                         "takes; with a speaker embedding InstanceNorm then normalises per window, see --window-norm")
    ap.add_argument("--window-norm", choices=("window", "utterance"), default="window",
                    help="with --window: InstanceNorm statistics per window (default) or pooled over all windows of an "
                         "utterance, which reproduces the whole-utterance result; an utterance then needs at most "
                         "--max-batch windows")
    ap.add_argument("--stream", default=None, metavar="PUSH[,CORE[,CONTEXT[,FADE]]]",
                    help="with --resident: feed the dumps as simulated LIVE streams, PUSH frames per stream and call "
                         "(StreamSession: windows of CORE frames, default 32, run as soon as their CONTEXT has arrived, "
                         "default the generator's receptive field; cross-fade over FADE frames, default 8); same file names; "
                         "with a speaker embedding InstanceNorm normalises per window, as with --window (see --stream-norm)")
    ap.add_argument("--stream-norm", default="window", choices=["window", "running"],
                    help="with --stream and a speaker embedding: InstanceNorm statistics of each window alone (default) or "
                         "running - of every frame the stream has delivered up to the window's right edge, carried on the GPU "
                         "from push to push; approaches the whole-utterance result as the stream grows")
    ap.add_argument("--stream-horizon", type=float, default=None, metavar="FRAMES",
                    help="with --stream-norm running: forget the running statistics exponentially with this horizon, in "
                         "frames (at least CORE): a frame j cores back counts with exp(-j CORE / FRAMES), so a change of "
                         "level is forgotten and the population stays bounded however long the stream lives (default: never "
                         "forget)")
    ap.add_argument("--streams", type=int, default=1, help="with --stream: dumps converted side by side (default 1)")
    args = ap.parse_args(argv)
    if args.stream is not None:
        if not args.resident or args.fanout > 1 or args.window is not None:
            ap.error("--stream works on the --resident route, without --fanout and --window")
        try:
            parts = [int(v) for v in args.stream.split(",")]
            if not 1 <= len(parts) <= 4 or parts[0] < 1 or args.streams < 1:
                raise ValueError
        except ValueError:
            ap.error("--stream takes PUSH[,CORE[,CONTEXT[,FADE]]] in frames, --streams a count of at least 1")
        if args.stream_horizon is not None and args.stream_norm != "running":
            ap.error("--stream-horizon needs --stream-norm running")
        args.stream = dict(zip(("max_push", "core", "context", "fade"), parts), n_streams=args.streams, norm=args.stream_norm)
        if args.stream_horizon is not None:
            args.stream["horizon"] = args.stream_horizon
    elif args.streams != 1 or args.stream_norm != "window" or args.stream_horizon is not None:
        ap.error("--streams, --stream-norm and --stream-horizon need --stream")
    if args.window is not None:
        if not args.resident or args.fanout > 1:
            ap.error("--window works on the --resident route, without --fanout")
        try:
            parts = [int(v) for v in args.window.split(",")]
            if not 1 <= len(parts) <= 3:
                raise ValueError
        except ValueError:
            ap.error("--window takes CORE[,CONTEXT[,FADE]] in frames")
        args.window = dict(zip(("core", "context", "fade"), parts), norm=args.window_norm)
    elif args.window_norm != "window":
        ap.error("--window-norm needs --window")
    if args.fanout < 1:
        ap.error("--fanout needs a group size of at least 1")
    if args.fanout > 1 and not args.resident:
        ap.error("--fanout works on the --resident route")
    if args.storage == "auto":
        args.storage, args.checked = "float16", True
    if (args.checked or args.fallback is not None) and not args.resident:
        ap.error("--checked / --fallback / --storage auto work on the --resident route")
    if args.fallback is not None and not args.checked:
        ap.error("--fallback needs --checked")
    args.fallback = tuple(v for v in (args.fallback if args.fallback is not None else "bfloat16").split(",") if v)
    for name in args.fallback:
        if name not in ("float32", "bfloat16", "float16"):
            ap.error(f"--fallback: unknown storage {name!r}")
    with open(args.config) as f:
        config = yaml.safe_load(f)
    device = torch.device("cuda")
    model = FastSVCGenerator(**config["generator_params"])
    model.load_state_dict(torch.load(args.checkpoint, map_location="cpu")["model"]["generator"])
    model.remove_weight_norm()
    model.activation_storage = args.storage
    model = model.eval().to(device)
    sg_conf = config.get("signal_generator", {})
    sg = SignalGenerator(sample_rate=config["sampling_rate"], hop_size=config["hop_size"],
                         sine_amp=sg_conf.get("sine_amp", 0.1), noise_amp=sg_conf.get("noise_amp", 0.003),
                         signal_types=sg_conf.get("signal_types", ["sine"]))
    files = sorted(glob.glob(os.path.join(args.dumpdir, "*.npz")) + glob.glob(os.path.join(args.dumpdir, "*.h5")))
    if args.resident:
        os.makedirs(args.outdir, exist_ok=True)
        (_main_stream if args.stream is not None else _main_resident)(args, config, model, sg, device, files)
        return
    feats = [load_features(p) for p in files]
    utt_ids = [os.path.splitext(os.path.basename(p))[0] for p in files]
    os.makedirs(args.outdir, exist_ok=True)
    embs = dict(np.load(args.spk_emb)) if args.spk_emb else {}
    for trgspk in config.get("convert_to_speakers", [None]):
        trg_emb = embs.get(trgspk) if config["generator_params"].get("use_spk_emb") else None
        src_stats = trg_stats = None
        if args.srcf0stats and args.trgf0stats and trgspk is not None:
            trg_stats = _read_f0_mean(args.trgf0stats, trgspk)
            src_stats = [_read_f0_mean(args.srcf0stats, u.split("_")[0]) for u in utt_ids]
        t0 = time.time()
        ys = decode_utterances(model, feats, sg, device, trg_emb, src_stats, trg_stats, args.max_batch)
        torch.cuda.synchronize()
        dt = time.time() - t0
        total = sum(len(y) for y in ys)
        for utt, y in zip(utt_ids, ys):
            write_wav(os.path.join(args.outdir, f"{utt}_{trgspk}_gen.wav"), y, config["sampling_rate"])
        print(f"{len(ys)} utterances -> {trgspk}: RTF = {dt / (total / config['sampling_rate']):.5f}")


def resident_groups(files: Sequence[str], budget_bytes: int, hop: int, load=load_features):
    """Consecutive runs of ``files`` whose packed features (4 * F * (C + hop) bytes per utterance, what a DecodeSession
    holds) fit ``budget_bytes``; a single utterance above the budget is a group of its own.  Yields (paths, feats),
    loading one group at a time."""
    paths, feats, used = [], [], 0
    for p in files:
        u = load(p)
        ppg = np.asarray(u["ppg"])
        need = 4 * int(ppg.shape[0]) * (int(ppg.shape[1]) + hop)
        if paths and used + need > budget_bytes:
            yield paths, feats
            paths, feats, used = [], [], 0
        paths.append(p)
        feats.append(u)
        used += need
    if paths:
        yield paths, feats


def speaker_groups(speakers: Sequence, size: int, kind=lambda s: None) -> List[list]:
    """Consecutive runs of at most ``size`` speakers that share ``kind(speaker)`` - one ``convert_many`` call each (a call
    takes speakers that all have an embedding and statistics, or all have none)."""
    groups: List[list] = []
    for s in speakers:
        if groups and len(groups[-1]) < size and kind(groups[-1][0]) == kind(s):
            groups[-1].append(s)
        else:
            groups.append([s])
    return groups


def _main_resident(args, config, model, sg, device, files) -> None:      # pragma: no cover - exercised on a GPU box
    """The CLI's speaker loop with the features resident: one session per group of dumps, every target speaker inside it.
    A dump directory that fits one group runs the same batches as the default path, so the files are the same byte for
    byte; split into several groups the batches differ, and the waveforms agree to the harness's batching invariance
    (2e-5 in float, tests/test_parity_gpu.py) before the PCM rounding."""
    embs = dict(np.load(args.spk_emb)) if args.spk_emb else {}
    speakers = config.get("convert_to_speakers", [None])
    spent, samples = {s: 0.0 for s in speakers}, {s: 0 for s in speakers}
    reports = {s: [] for s in speakers}
    for paths, feats in resident_groups(files, args.resident_bytes, int(config["hop_size"])):
        utt_ids = [os.path.splitext(os.path.basename(p))[0] for p in paths]
        src_stats = None
        if args.srcf0stats and args.trgf0stats:
            src_stats = [_read_f0_mean(args.srcf0stats, u.split("_")[0]) for u in utt_ids]
        with DecodeSession(model, feats, sg, device, src_stats, args.max_batch, checked=args.checked,
                           fallback=args.fallback) as session:
            for group in (speaker_groups(speakers, args.fanout, lambda s: (embs.get(s) is None, s is None))
                          if args.fanout > 1 else []):
                trg = []
                for trgspk in group:
                    trg_emb = embs.get(trgspk) if config["generator_params"].get("use_spk_emb") else None
                    trg.append((trg_emb, _read_f0_mean(args.trgf0stats, trgspk) if src_stats is not None and trgspk is not None else None))
                t0 = time.time()
                pcms = session.convert_many(trg)
                dt = (time.time() - t0) / len(group)
                for k, (trgspk, pcm) in enumerate(zip(group, pcms)):
                    spent[trgspk] += dt
                    samples[trgspk] += sum(len(p) for p in pcm)
                    reports[trgspk] += session.last_report[k] if args.checked else []
                    for utt, p in zip(utt_ids, pcm):
                        write_wav(os.path.join(args.outdir, f"{utt}_{trgspk}_gen.wav"), p, config["sampling_rate"])
            for trgspk in (speakers if args.fanout == 1 else []):
                trg_emb = embs.get(trgspk) if config["generator_params"].get("use_spk_emb") else None
                trg_stats = None
                if src_stats is not None and trgspk is not None:
                    trg_stats = _read_f0_mean(args.trgf0stats, trgspk)
                t0 = time.time()
                pcm = session.convert(trg_emb, trg_stats) if args.window is None else \
                    session.convert_windowed(trg_emb, trg_stats, **args.window)
                spent[trgspk] += time.time() - t0
                samples[trgspk] += sum(len(p) for p in pcm)
                reports[trgspk] += session.last_report if args.checked else []
                for utt, p in zip(utt_ids, pcm):
                    write_wav(os.path.join(args.outdir, f"{utt}_{trgspk}_gen.wav"), p, config["sampling_rate"])
    for trgspk in speakers:
        if samples[trgspk]:
            print(f"{len(files)} utterances -> {trgspk}: RTF = {spent[trgspk] / (samples[trgspk] / config['sampling_rate']):.5f}")
        if args.checked:
            print(f"{trgspk}: " + summarize_reports(reports[trgspk], args.storage))


def _main_stream(args, config, model, sg, device, files) -> None:        # pragma: no cover - exercised on a GPU box
    """The CLI's speaker loop over simulated live streams: ``--streams`` dumps at a time run side by side through one
    ``StreamSession``, each delivering ``PUSH`` frames per call until it ends; the pieces a stream returned, concatenated,
    are its file."""
    embs = dict(np.load(args.spk_emb)) if args.spk_emb else {}
    hop, n, step = int(config["hop_size"]), args.stream["n_streams"], args.stream["max_push"]
    with StreamSession(model, sg, device, checked=args.checked, fallback=args.fallback, **args.stream) as session:
        for trgspk in config.get("convert_to_speakers", [None]):
            reports = []                                 # a checked session: one entry per stream, from its totals
            trg_emb = embs.get(trgspk) if config["generator_params"].get("use_spk_emb") else None
            shift = bool(args.srcf0stats and args.trgf0stats and trgspk is not None)
            trg_stats = _read_f0_mean(args.trgf0stats, trgspk) if shift else None
            spent, samples = 0.0, 0
            for g in range(0, len(files), n):
                paths = files[g: g + n]
                feats = [load_features(p) for p in paths]
                utt_ids = [os.path.splitext(os.path.basename(p))[0] for p in paths]
                frames = [int(np.asarray(u["ppg"]).shape[0]) for u in feats]
                t0 = time.time()
                ids = [session.open(trg_emb, _read_f0_mean(args.srcf0stats, u.split("_")[0]) if shift else None, trg_stats, seed=g + j)
                       for j, u in enumerate(utt_ids)]
                pieces = [[] for _ in paths]
                for a in range(0, max(frames), step):
                    live = [j for j, f in enumerate(frames) if a < f]
                    out = session.push({ids[j]: dict(ppg=np.asarray(feats[j]["ppg"])[a: a + step],
                                                     f0=np.asarray(feats[j]["f0"]).reshape(-1)[a: min(a + step, frames[j])],
                                                     lft=np.asarray(feats[j]["lft"]).reshape(-1)[a * hop: min(a + step, frames[j]) * hop])
                                        for j in live}, end=[ids[j] for j in live if a + step >= frames[j]])
                    for j in live:
                        pieces[j].append(out[ids[j]])
                    if args.checked:
                        reports += [stream_totals_report(t, args.storage) for t in session.last_report.get("totals", {}).values()]
                session.end([ids[j] for j, f in enumerate(frames) if f == 0])        # (a dump without frames: free its slot)
                spent += time.time() - t0
                for utt, ps in zip(utt_ids, pieces):
                    y = np.concatenate(ps) if ps else np.zeros(0, np.int16)
                    samples += y.size
                    write_wav(os.path.join(args.outdir, f"{utt}_{trgspk}_gen.wav"), y, config["sampling_rate"])
            if samples:
                print(f"{len(files)} streams -> {trgspk}: RTF = {spent / (samples / config['sampling_rate']):.5f}")
            if args.checked:
                print(f"{trgspk}: " + summarize_reports(reports, args.storage))


def stream_totals_report(totals: Dict[str, object], storage: str) -> Dict[str, object]:
    """A checked stream's totals (``StreamSession.totals``) as the one entry ``summarize_reports`` counts for an utterance:
    it fell back when one of its windows did - ``storage`` is then the last fallback storage among its windows', in the
    order they first ran - and its counts are the sums over its windows."""
    others = [name for name in totals["storages"] if name != storage]
    return dict(storage=others[-1] if others else storage, tried=[storage] if totals["fell_back"] else [],
                nonfinite=totals["nonfinite"], clipped=totals["clipped"], max_abs=totals["max_abs"])


def summarize_reports(reports: Sequence[Dict[str, object]], storage: str) -> str:
    """The CLI's closing line for one target speaker, from the ``last_report`` entries of its converts."""
    fell: Dict[str, int] = {}
    for r in reports:
        if r["tried"]:
            fell[str(r["storage"])] = fell.get(str(r["storage"]), 0) + 1
    bad = sum(1 for r in reports if r["nonfinite"])
    text = f"{len(reports)} utterances checked in {storage} storage; {sum(fell.values())} fell back"
    if fell:
        text += " (" + ", ".join(f"{n} to {name}" for name, n in sorted(fell.items())) + ")"
    if bad:
        text += f"; {bad} STILL NON-FINITE after the last fallback"
    text += f"; {sum(1 for r in reports if r['clipped'])} have clipped samples"
    return text + f"; largest max_abs {max((float(r['max_abs']) for r in reports), default=0.0):.4g}"


if __name__ == "__main__":                                    # pragma: no cover
    main()
