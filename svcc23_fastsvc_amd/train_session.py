"""Training-side data path: a corpus resident on the device, one HIP launch per batch.

The reference feeds its trainer through ``DataLoader`` workers: ``Collater.__call__``
(``harana/bin/train_fastsvc.py:484-551``) draws one random start frame per utterance, slices wave / lft / f0 / ppg in
numpy, stacks, transposes and synthesises the sine excitation on the CPU.  ``TrainSession`` is the counterpart of
``decode.DecodeSession``: the utterances are uploaded ONCE, in the dump's own time-major layout, and every batch is cut
out of them by ``engine.collate_crops`` (``csrc/fastsvc_collate.hip``: all five tensors in one launch, bit-identical
to the numpy slices) followed by the device excitation (``fastsvc_signal_generate``, the kernel behind
``SignalGenerator``) on the collated f0.

The sampler (``CropSampler``) is host-only and stateless: which utterances form global batch k of an epoch and where
each crop starts are pure functions of ``(seed, epoch, index)`` built on ``synth.hash_u64``, so resuming at a step and
sharding over data-parallel ranks need no bookkeeping.
"""
from __future__ import annotations

import ctypes
import warnings
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .synth import hash_u64, stream_id

_TYPE_CODE = {"noise": 0, "sine": 1, "uv": 2}


def round_batch_length(batch_length: int, hop_size: int) -> int:
    """``batch_length`` rounded down to a multiple of ``hop_size`` (train_fastsvc.py:461-465)."""
    batch_length, hop_size = int(batch_length), int(hop_size)
    if hop_size < 1 or batch_length < hop_size:
        raise ValueError(f"batch_length {batch_length} holds no frame of {hop_size} samples")
    return batch_length - batch_length % hop_size


def store_layout(n_frames: Sequence[int], align_frames: int = 1) -> Tuple[List[int], int]:
    """Frame offsets of the utterances' blocks in the packed store, in order -> (frame_off, total_frames).  Block u holds
    frames ``[frame_off[u], frame_off[u] + n_frames[u])``; with ``align_frames`` = 1 the blocks lie back to back, with 4
    every block starts on a multiple of 4 frames (16 bytes in every buffer: the kernel's 16-byte requests then apply
    whenever ``hop`` and ``D`` are multiples of 4), at most 3 unused frames between two blocks.  f0 is indexed in frames,
    ppg in ``frame * D`` elements, wave / lft in ``frame * hop`` samples."""
    align = max(int(align_frames), 1)
    offs, pos = [], 0
    for n in n_frames:
        pos = (pos + align - 1) // align * align
        offs.append(pos)
        pos += int(n)
    return offs, pos


def _flat(a, what: str, i: int) -> np.ndarray:
    a = np.asarray(a)
    if a.ndim == 2 and a.shape[1] == 1:
        a = a[:, 0]
    if a.ndim != 1:
        raise ValueError(f"utterance {i}: {what} must be (N,) or (N, 1), got {a.shape}")
    return a


def corpus_plan(feats: Sequence[Dict[str, np.ndarray]], batch_length: int, hop_size: int, aux_context_window: int = 0,
                use_spk_emb: bool = True) -> dict:
    """Host-only checks of a corpus (no device needed): the Collater's length checks for every utterance
    (train_fastsvc.py:553-557: ``len(wave) == len(ppg) * hop == len(lft) == len(f0) * hop``; ``ValueError`` naming the
    utterance otherwise) and which utterances can be cropped at all - one with ``n - 2 ctx <= frames`` cannot: the
    reference omits it with a warning (:522-527) and ``remove_short_samples`` filters it (:646-651).
    -> {"batch_length", "frames", "n_frames" (per utterance), "omitted", "eligible" (indices, file order), "D", "S"}."""
    hop, ctx = int(hop_size), int(aux_context_window)
    if ctx < 0:
        raise ValueError("aux_context_window must be >= 0")
    batch_length = round_batch_length(batch_length, hop)
    frames = batch_length // hop
    n_frames, omitted, eligible = [], [], []
    D = S = None
    for i, u in enumerate(feats):
        for key in ("wave", "f0", "ppg", "lft") + (("spk_emb",) if use_spk_emb else ()):
            if key not in u:
                raise ValueError(f"utterance {i}: no '{key}' in the dump")
        ppg = np.asarray(u["ppg"])
        if ppg.ndim != 2:
            raise ValueError(f"utterance {i}: ppg must be (F, D), got {ppg.shape}")
        n = int(ppg.shape[0])
        x, f0, lft = _flat(u["wave"], "wave", i), _flat(u["f0"], "f0", i), _flat(u["lft"], "lft", i)
        if len(x) != n * hop or len(x) != len(lft) or len(x) != len(f0) * hop:
            raise ValueError(f"utterance {i}: lengths do not agree: wave {len(x)}, lft {len(lft)}, f0 {len(f0)} and "
                             f"ppg {n} frames of {hop} samples")
        if D is None:
            D = int(ppg.shape[1])
        elif int(ppg.shape[1]) != D:
            raise ValueError(f"utterance {i}: ppg must be (F, {D}), got {ppg.shape}")
        if use_spk_emb:
            e = _flat(u["spk_emb"], "spk_emb", i)
            if S is None:
                S = len(e)
            elif len(e) != S:
                raise ValueError(f"utterance {i}: spk_emb must hold {S} values, got {len(e)}")
        n_frames.append(n)
        (eligible if n - 2 * ctx > frames else omitted).append(i)
    return {"batch_length": batch_length, "frames": frames, "n_frames": n_frames, "omitted": omitted,
            "eligible": eligible, "D": D or 0, "S": S or 0}


class CropSampler:
    """Which crops form which batch: a pure function of ``(seed, epoch, index)``, no hidden state.

    ``n_frames[i]`` frames per utterance (file order), ``eligible`` the indices that can be cropped.  An epoch visits
    every eligible utterance exactly once: ``shuffle=False`` in file order, ``shuffle=True`` in the order of their
    ``hash_u64`` keys for that epoch; consecutive groups of ``batch_size`` are the GLOBAL batches, the last one kept short
    (``DataLoader`` without ``drop_last``).  Utterance i's start frame in an epoch is uniform over the reference's
    half-open range ``[ctx, n_i - frames - ctx)`` (``np.random.randint``, train_fastsvc.py:502-504) and depends on
    ``(seed, epoch, i)`` only.  Rank r of ``world`` takes the global batches ``k % world == r``; every rank computes
    the same global list."""

    def __init__(self, n_frames: Sequence[int], eligible: Sequence[int], frames: int, batch_size: int,
                 aux_context_window: int = 0, seed: int = 0, shuffle: bool = True, rank: int = 0, world: int = 1):
        self.n_frames = [int(n) for n in n_frames]
        self.eligible = [int(i) for i in eligible]
        self.frames, self.ctx, self.batch_size = int(frames), int(aux_context_window), int(batch_size)
        self.seed, self.shuffle, self.rank, self.world = int(seed), bool(shuffle), int(rank), int(world)
        if self.batch_size < 1 or self.world < 1 or not 0 <= self.rank < self.world:
            raise ValueError("batch_size and world must be >= 1 and 0 <= rank < world")
        for i in self.eligible:
            if self.n_frames[i] - 2 * self.ctx <= self.frames:
                raise ValueError(f"utterance {i} ({self.n_frames[i]} frames) cannot be cropped to {self.frames} frames")

    @property
    def global_batches_per_epoch(self) -> int:
        return (len(self.eligible) + self.batch_size - 1) // self.batch_size

    def global_batches(self, epoch: int) -> List[Tuple[List[int], List[int]]]:
        """Every rank's batches of ``epoch``, in global order: [(utts, starts), ...]."""
        epoch = int(epoch)
        order = list(self.eligible)
        if self.shuffle and order:
            keys = hash_u64(self.seed, stream_id("train_session.order") + (epoch << 32), len(self.n_frames))
            order.sort(key=lambda i: (int(keys[i]), i))
        if order:
            h = hash_u64(self.seed, stream_id("train_session.start") + (epoch << 32), len(self.n_frames))
        starts = [self.ctx + int(h[i]) % (self.n_frames[i] - self.frames - 2 * self.ctx) for i in order]
        bs = self.batch_size
        return [(order[k: k + bs], starts[k: k + bs]) for k in range(0, len(order), bs)]

    def global_indices(self) -> List[int]:
        """The global batch numbers (within an epoch) this rank takes."""
        return list(range(self.rank, self.global_batches_per_epoch, self.world))

    def epoch_batches(self, epoch: int) -> List[Tuple[List[int], List[int]]]:
        """This rank's batches of ``epoch``: the global batches ``k % world == rank``."""
        g = self.global_batches(epoch)
        return [g[k] for k in self.global_indices()]


class TrainSession:
    """A training corpus kept on the device; batches cut out of it by one HIP launch each.

        session = TrainSession(feats, "cuda", batch_size=32, batch_length=16000, hop_size=160)
        for epoch in range(n):
            for batch in session.batches(epoch):
                step.step(batch)                       # TrainStep: ((ppg, sine, lft[, emb]), y)

    ``feats``: the dicts ``decode.load_features`` returns - ``wave (T,)`` / ``(T, 1)``, ``f0 (F,)`` / ``(F, 1)``,
    ``ppg (F, D)``, ``lft (T,)`` / ``(T, 1)``, ``spk_emb (S,)`` / ``(S, 1)``.  ``batch_length`` is rounded down to a
    multiple of ``hop_size``; every utterance must pass the Collater's length checks (``ValueError`` naming it);
    utterances too short to crop are left out and listed in ``omitted``.  Everything else is uploaded once through
    page-locked staging as five packed float32 buffers (``store_layout``, blocks aligned to 4 frames);
    ``resident_bytes`` is their size, and a ``budget_bytes`` below it raises instead of spilling.

    ``signal_generator_params``: ``sine_amp`` (0.1), ``noise_amp`` (0.003), ``signal_types`` (["sine"]) - the Collater's
    defaults (train_fastsvc.py:441-453).  The excitation noise of global batch k is seeded by ``(seed, k)`` alone.

    The batch tensors belong to the session: two alternating sets, so a batch stays valid until the next-but-one
    ``batch`` call.  Not thread-safe.  No CPU fallback: a non-GPU device raises ``FastSVCError``."""

    def __init__(self, feats: Sequence[Dict[str, np.ndarray]], device, batch_size: int, batch_length: int, hop_size: int,
                 sample_rate: int = 16000, aux_context_window: int = 0, signal_generator_params: Optional[dict] = None,
                 use_spk_emb: bool = True, seed: int = 0, shuffle: bool = True, rank: int = 0, world: int = 1,
                 budget_bytes: Optional[int] = None):
        from .engine import FastSVCError, load_library
        plan = corpus_plan(feats, batch_length, hop_size, aux_context_window, use_spk_emb)
        self.hop, self.ctx = int(hop_size), int(aux_context_window)
        self.batch_length, self.frames = plan["batch_length"], plan["frames"]
        self.batch_size, self.sample_rate = int(batch_size), float(sample_rate)
        self.use_spk_emb, self.seed = bool(use_spk_emb), int(seed)
        self.omitted: List[int] = plan["omitted"]
        if self.omitted:
            warnings.warn(f"{len(self.omitted)} utterances are shorter than the batch length and are left out: {self.omitted[:8]}")
        self.channels, self.emb_size = plan["D"], plan["S"]
        self.sampler = CropSampler(plan["n_frames"], plan["eligible"], self.frames, batch_size, self.ctx, seed, shuffle, rank, world)
        sg = dict(signal_generator_params or {})
        self.sine_amp, self.noise_amp = float(sg.get("sine_amp", 0.1)), float(sg.get("noise_amp", 0.003))
        self.signal_types = list(sg.get("signal_types", ["sine"]))
        for t in self.signal_types:
            if t not in _TYPE_CODE:
                raise ValueError(f"{t} is not a supported signal type (noise, sine, uv)")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise FastSVCError("TrainSession needs a GPU device (no CPU fallback); got " + str(self.device))
        if not plan["eligible"]:
            raise ValueError("no utterance is long enough to be cropped")
        self._lib = load_library()
        # ---- the store: eligible utterances only, in file order
        stored = plan["eligible"]
        self._slot = {u: j for j, u in enumerate(stored)}
        counts = [plan["n_frames"][u] for u in stored]
        self._frame_off, total = store_layout(counts, align_frames=4)
        self._n_frames = counts
        hop, D, S = self.hop, self.channels, self.emb_size
        sizes = {"f0": total, "ppg": total * D, "wave": total * hop, "lft": total * hop}
        if self.use_spk_emb:
            sizes["emb"] = len(stored) * S
        self.resident_bytes = 4 * sum(sizes.values())
        if budget_bytes is not None and self.resident_bytes > int(budget_bytes):
            raise ValueError(f"the corpus needs {self.resident_bytes} resident bytes, the budget is {int(budget_bytes)} "
                             "(streaming a larger corpus is not implemented)")
        host = {k: torch.zeros(max(n, 1), dtype=torch.float32, pin_memory=True) for k, n in sizes.items()}
        hv = {k: v.numpy() for k, v in host.items()}
        for j, u in enumerate(stored):
            f, o, n = feats[u], self._frame_off[j], counts[j]
            hv["f0"][o: o + n] = _flat(f["f0"], "f0", u)
            hv["ppg"][o * D: (o + n) * D] = np.asarray(f["ppg"]).reshape(-1)
            hv["wave"][o * hop: (o + n) * hop] = _flat(f["wave"], "wave", u)
            hv["lft"][o * hop: (o + n) * hop] = _flat(f["lft"], "lft", u)
            if self.use_spk_emb:
                hv["emb"][j * S: (j + 1) * S] = _flat(f["spk_emb"], "spk_emb", u)
        self._store = {k: v.to(self.device, non_blocking=True) for k, v in host.items()}
        torch.cuda.current_stream(self.device).synchronize()          # the staging goes when the constructor returns
        if self.use_spk_emb:
            self._store["emb"] = self._store["emb"].view(len(stored), S)
        self._off_c = (ctypes.c_int64 * len(stored))(*self._frame_off)
        self._nfr_c = (ctypes.c_int32 * len(stored))(*counts)
        self._sets: Dict[Tuple[int, int], dict] = {}
        self._calls = 0
        self.last_f0: Optional[torch.Tensor] = None

    # ---- sampling (host only) ----
    def epoch_batches(self, epoch: int) -> List[Tuple[List[int], List[int]]]:
        """This rank's ``(utts, starts)`` of ``epoch`` (``CropSampler.epoch_batches``): indices into ``feats``."""
        return self.sampler.epoch_batches(epoch)

    def batches(self, epoch: int, first: int = 0) -> Iterator[tuple]:
        """``batch(...)`` over ``epoch_batches(epoch)[first:]``; the noise of each is seeded by its global number
        ``epoch * global_batches_per_epoch + k``, so a resumed run draws what an uninterrupted one draws."""
        per_epoch = self.sampler.global_batches_per_epoch
        ks = self.sampler.global_indices()
        for i, (utts, starts) in enumerate(self.sampler.epoch_batches(epoch)):
            if i >= first:
                yield self.batch(utts, starts, step=int(epoch) * per_epoch + ks[i])

    # ---- assembly (device) ----
    def _buffers(self, B: int) -> dict:
        slot = self._calls & 1
        self._calls += 1
        key = (slot, B)
        if key not in self._sets:
            dev, T, W = self.device, self.frames * self.hop, self.frames + 2 * self.ctx
            e = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)        # noqa: E731
            self._sets[key] = {
                "y": e(B, 1, T), "lft": e(B, 1, T), "ppg": e(B, self.channels, W), "f0": e(B, 1, self.frames),
                "emb": e(B, self.emb_size) if self.use_spk_emb else None, "sine": e(B, len(self.signal_types), T),
                "scratch": torch.empty(max(int(self._lib.fastsvc_signal_scratch_bytes(B, self.frames)), 1),
                                       dtype=torch.uint8, device=dev)}
        return self._sets[key]

    @torch.no_grad()
    def batch(self, utts: Sequence[int], starts: Sequence[int], step: int = 0):
        """The batch of crops ``(utts[b], starts[b])`` - utterance indices into ``feats``, start frames with
        ``ctx <= start <= n - frames - ctx`` - as ``((ppg, sine, lft[, emb]), y)``, the layout ``TrainStep.step`` takes:
        one ``collate_crops`` launch, then the excitation from the collated f0, its noise seeded by ``(seed, step)``.
        The tensors are the session's own and are reused: a batch is valid until the next-but-one call of ``batch``."""
        from .engine import FastSVCError, collate_crops
        B = len(utts)
        if B == 0 or len(starts) != B:
            raise ValueError("batch needs at least one crop and one start per utterance")
        try:
            slots = [self._slot[int(u)] for u in utts]
        except KeyError as e:
            raise ValueError(f"utterance {e.args[0]} is not in the store (omitted or out of range)") from None
        buf = self._buffers(B)
        s = self._store
        collate_crops(s["wave"], s["lft"], s["ppg"], s["f0"], s.get("emb") if self.use_spk_emb else None,
                      self._off_c, self._nfr_c, slots, starts, self.channels, self.hop, self.frames, self.ctx,
                      out=(buf["y"], buf["lft"], buf["ppg"], buf["f0"], buf["emb"]))
        n = len(self.signal_types)
        types = (ctypes.c_int32 * n)(*[_TYPE_CODE[t] for t in self.signal_types])
        seed = int(hash_u64(self.seed, stream_id("train_session.noise"), 1, offset=int(step))[0])
        with torch.cuda.device(self.device):
            rc = self._lib.fastsvc_signal_generate(
                ctypes.c_void_p(buf["f0"].data_ptr()), ctypes.c_void_p(buf["sine"].data_ptr()),
                ctypes.c_void_p(buf["scratch"].data_ptr()), B, self.frames, self.hop,
                ctypes.c_float(self.sample_rate), ctypes.c_float(self.sine_amp), ctypes.c_float(self.noise_amp),
                types, n, ctypes.c_uint64(seed), ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        if rc != 0:
            raise FastSVCError(f"fastsvc_signal_generate failed ({rc})")
        self.last_f0 = buf["f0"]                                      # (B, 1, frames): what the excitation was made from
        x = (buf["ppg"], buf["sine"], buf["lft"]) + ((buf["emb"],) if self.use_spk_emb else ())
        return x, buf["y"]
