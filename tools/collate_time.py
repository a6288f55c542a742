"""Time per training batch of `TrainSession.batch` (resident corpus, one HIP launch + the device excitation) against the
host route the reference's Collater takes, restated here (train_fastsvc.py:500-543): numpy slices per utterance, stacked
and transposed into page-locked memory, uploaded, then the existing device `SignalGenerator` on the uploaded f0.

Recipe size: batch 32 x 16000 samples, D = 144, S = 512, hop 160, a corpus of COLLATE_UTTS (default 256) synthetic
utterances of 2 - 10 s.  Two measurements, the two routes alternated within the one run, COLLATE_REPS (default 5)
repetitions, medians; every timed region ends in a device synchronise:

    per batch   COLLATE_BATCHES (default 50) batches assembled back to back, nothing else on the device
    per step    COLLATE_STEPS (default 10) train steps (yaml-width generator, the yaml's discriminator, both networks
                training), each fed by a batch assembled in line by that route - no loader workers on either side

Before timing, the device route's ppg / lft / emb / y are checked to equal the host route's bit for bit.  The figures go to
profiles/train_session.txt.
    python tools/collate_time.py"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import synth as S, training as TR
from svcc23_fastsvc_amd.train_session import TrainSession

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dev = torch.device("cuda:0")
cfg = S.FULL_CONFIG
hop, D, S_emb, rate = cfg.hop, cfg.in_channels, cfg.spk_emb_size, 16000
B, batch_length = TR.RECIPE["batch_size"], TR.RECIPE["batch_length"]
frames = batch_length // hop
T = frames * hop
n_utts = int(os.environ.get("COLLATE_UTTS", "256"))
reps = max(int(os.environ.get("COLLATE_REPS", "5")), 1)
n_batches = int(os.environ.get("COLLATE_BATCHES", "50"))
n_steps = int(os.environ.get("COLLATE_STEPS", "10"))
rng = np.random.default_rng(7)
feats = []
for f in rng.integers(2 * rate // hop, 10 * rate // hop + 1, n_utts):
    f = int(f)
    f0 = np.where(rng.random((f, 1)) < 0.3, 0.0, rng.uniform(80, 400, (f, 1))).astype(np.float32)
    feats.append({"wave": (0.3 * rng.standard_normal(f * hop, dtype=np.float32)), "f0": f0,
                  "ppg": rng.standard_normal((f, D), dtype=np.float32),
                  "lft": rng.uniform(-9, 1, (f * hop, 1)).astype(np.float32),
                  "spk_emb": rng.standard_normal((S_emb, 1), dtype=np.float32)})
sg_params = dict(sine_amp=0.1, noise_amp=0.003, signal_types=["sine"])
session = TrainSession(feats, dev, B, batch_length, hop, sample_rate=rate, signal_generator_params=sg_params, seed=1)
sg = A.SignalGenerator(sample_rate=rate, hop_size=hop, **sg_params)
plan = [bt for e in range(8) for bt in session.epoch_batches(e) if len(bt[0]) == B]       # (utts, starts), full batches
pinned = [{k: torch.empty(s, dtype=torch.float32, pin_memory=True) for k, s in
           (("y", (B, 1, T)), ("lft", (B, 1, T)), ("ppg", (B, D, frames)), ("f0", (B, 1, frames)), ("emb", (B, S_emb)))}
          for _ in range(2)]
calls = [0]


def host_batch(utts, starts):
    """Collater.__call__ for given start frames: slices, np.array, transpose, FloatTensor - into page-locked memory (two
    alternating sets), one asynchronous upload per tensor, the excitation on the device."""
    ys, f0s, ppgs, lfts, embs = [], [], [], [], []
    for u, s in zip(utts, starts):
        f = feats[u]
        ys.append(f["wave"][s * hop: s * hop + T].astype(np.float32).reshape(-1, 1))
        f0s.append(f["f0"][s: s + frames].astype(np.float32).reshape(-1, 1))
        ppgs.append(f["ppg"][s: s + frames].astype(np.float32))
        lfts.append(f["lft"][s * hop: s * hop + T].astype(np.float32).reshape(-1, 1))
        embs.append(f["spk_emb"].astype(np.float32).squeeze(1))
    h = pinned[calls[0] & 1]
    calls[0] += 1
    h["y"].numpy()[:] = np.array(ys).transpose(0, 2, 1)
    h["f0"].numpy()[:] = np.array(f0s).transpose(0, 2, 1)
    h["ppg"].numpy()[:] = np.array(ppgs).transpose(0, 2, 1)
    h["lft"].numpy()[:] = np.array(lfts).transpose(0, 2, 1)
    h["emb"].numpy()[:] = np.array(embs)
    d = {k: v.to(dev, non_blocking=True) for k, v in h.items()}
    return (d["ppg"], sg(d["f0"]), d["lft"], d["emb"]), d["y"]


def device_batch(utts, starts, k=0):
    return session.batch(utts, starts, step=k)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


# the two routes cut the same batch
for utts, starts in plan[:3]:
    (p1, _, l1, e1), y1 = host_batch(utts, starts)
    (p2, _, l2, e2), y2 = device_batch(utts, starts)
    assert all(torch.equal(a, b) for a, b in ((p1, p2), (l1, l2), (e1, e2), (y1, y2))), "device route differs from the host route"

gen = A.FastSVCGenerator(in_channels=D, mid_channels=list(cfg.mid_channels), upsampling_scales=list(cfg.upsampling_scales),
                         out_channels=1, spk_emb_size=S_emb, use_spk_emb=True)
gen.load_state_dict({k: torch.from_numpy(v) for k, v in S.synth_state_dict(cfg, 201).items()})
gen = gen.to(dev).train()
disc = TR.MelGANMultiScaleDiscriminator(**TR.RECIPE["discriminator_params"]).to(dev).train()
step = TR.TrainStep(gen, disc, dict(discriminator_train_start_steps=0), steps=1)


def run_batches(route):
    for i in range(n_batches):
        route(*plan[i % len(plan)])


def run_steps(route):
    for i in range(n_steps):
        step.step(route(*plan[i % len(plan)]), log=False)


for route in (host_batch, device_batch):                     # warm both routes and the step
    run_batches(route)
    for i in range(3):
        step.step(route(*plan[i]), log=False)
t = {("batch", "host"): [], ("batch", "device"): [], ("step", "host"): [], ("step", "device"): []}
for _ in range(reps):
    for name, route in (("host", host_batch), ("device", device_batch)):
        t[("batch", name)].append(timed(lambda: run_batches(route)) / n_batches)
    for name, route in (("host", host_batch), ("device", device_batch)):
        t[("step", name)].append(timed(lambda: run_steps(route)) / n_steps)
lines = [f"collate_time: corpus of {n_utts} utterances of 2 - 10 s ({session.resident_bytes / 1e6:.1f} MB resident), batch {B} x {T} "
         f"samples, D {D}, S {S_emb}, hop {hop}; {reps} repetitions, routes alternated, medians; {torch.cuda.get_device_name(0)}",
         f"per batch: {n_batches} batches back to back; per step: {n_steps} train steps (both networks), the batch assembled in line",
         "device route's ppg / lft / emb / y equal the host route's bit for bit: True"]
labels = {"host": "host route (numpy slices, pinned upload, device sine)", "device": "TrainSession.batch (one launch + device sine)"}
for what in ("batch", "step"):
    for name in ("host", "device"):
        v = np.array(t[(what, name)]) * 1e3
        lines.append(f"per {what:5s} {labels[name]:56s} median {np.median(v):8.3f} ms  (min {v.min():8.3f}, max {v.max():8.3f})")
hb, db = np.median(t[("batch", "host")]), np.median(t[("batch", "device")])
lines.append(f"device route per batch / host route per batch = {db / hb:.3f}" +
             ("" if db <= hb else "  - the device route is NOT faster per batch"))
print("\n".join(lines), flush=True)
out = os.environ.get("COLLATE_OUT") or os.path.join(ROOT, "profiles", "train_session.txt")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
