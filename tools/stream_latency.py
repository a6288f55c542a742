"""Host-to-host time of one StreamSession.push that completes ONE window per stream - the steady state of live
conversion, where every stream delivers `core` frames per push - for 1, 8 and 32 streams, core 32 and 100, activation
storage float32 and bfloat16, speaker embedding, F0 shift on, int16 out.

Next to it, the yardstick: what the decode path could already do with the features RESIDENT on the device - one batch of
the same rows (one mid-utterance window of core + 2 context frames per stream) through convert_windowed's own chain:
window_assemble out of packed buffers that hold the features and a ready-made excitation, one forward with `lengths`,
window_stitch (one zone staged, one blended, as between pushes) and the download of the int16 samples, ending in a
synchronise.  The push does that and, before it, packs the chunk on the host, uploads it, appends it to the rings and
synthesises its excitation.

A repetition times STREAM_PUSHES (default 20) consecutive pushes, each host-to-host (a push ends in a synchronise), and
the same number of yardstick batches; the two legs alternate, STREAM_REPS (default 5) repetitions, and the medians of
the repetitions' means are reported with their spread.  Real-time factor: seconds of audio a push delivers (streams x
core x hop / sample rate) over the push time.  The figures go to profiles/decode_stream.txt.

--norm times another pair of legs instead: the same steady-state push in a StreamSession(norm="running") against a
StreamSession(norm="window") fed the same chunks - two sessions alive in one process, alternated repetition by repetition.
The running session carries its InstanceNorm sums on the device: one more read of the three FiLM-affined tensors of every
up block and 24 small launches per forward.  Its figures go to profiles/decode_stream_norm.txt.

--norm --horizon H: the pair is StreamSession(norm="running", horizon=H) against StreamSession(norm="running") - the same
launches, one more multiplication per row in the pool and three double arrays in the per-forward upload.  Its figures go
to profiles/decode_stream_horizon.txt.

--audio: the pair is StreamSession(loudness="audio") against StreamSession(loudness="given") on the same ppg and f0, 1, 8 and
32 streams at core 32 in both storages: the audio session is pushed samples and makes the loudness on the device (two more
launches per push, csrc/fastsvc_stream_loudness.hip).  Its figures go to profiles/decode_stream_loudness.txt.

--f0: the pair is StreamSession(f0="audio") against StreamSession(f0="given"), both with loudness="audio", on the same ppg and
audio, 1, 8 and 32 streams at core 32 in both storages: the f0 session is pushed no F0 and makes it, its shift and the
excitation on the device when the frames are final (two more launches per push, csrc/fastsvc_stream_f0.hip).  Reported, not
gated.  Its figures go to profiles/decode_stream_f0.txt.

--checked: the pair is StreamSession(checked=True) against StreamSession() in float16 activation storage on the same chunks, 1,
8 and 32 streams at core 32, with norm="window" and norm="running": the checked session adds one stream_check launch, a copy
of 16 bytes a row and ONE wait per forward (nothing falls back: the streams stay in range).  The difference is quoted next to
the spread of the unchecked leg; nothing is gated.  Its figures go to profiles/decode_stream_checked.txt.

--f0-stats: the pair is f0=audio streams opened with RunningF0Stats() (source statistics run on the device: one more launch
per push in which a frame became final, stream_f0_running_kernel) against the same streams opened with list statistics -
the path as it was - on the same ppg and audio, 1, 8 and 32 streams at core 32 in both storages.  Reported, not gated.  Its
figures go to profiles/decode_stream_f0_stats.txt.

--f0-track: the pair is f0=audio streams in a session with f0_track=F0Track() (the frames launch makes candidates, one more
launch runs the fixed-lag Viterbi tracker, stream_f0_track_kernel; the windows run 8 frames later) against the same streams
with f0_track=None - the path as it was - on the same ppg and audio, 1, 8 and 32 streams at core 32 in both storages.
Reported, not gated.  Its figures go to profiles/decode_stream_f0_track.txt.

    python tools/stream_latency.py [--norm [--horizon H] | --audio | --f0 | --f0-stats | --f0-track | --checked]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import synth as S, decode as Dc
from svcc23_fastsvc_amd.engine import window_assemble, window_stitch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dev = torch.device("cuda:0")
cfg = S.FULL_CONFIG
hop, C, SR, FADE = cfg.hop, cfg.in_channels, 24000, 8
reps = max(int(os.environ.get("STREAM_REPS", "5")), 1)
pushes = max(int(os.environ.get("STREAM_PUSHES", "20")), 1)
ctx = -(-Dc.receptive_field_frames(cfg) // 4) * 4
sg = A.SignalGenerator(sample_rate=SR, hop_size=hop, noise_amp=0.0, signal_types=["sine"])
rng = np.random.default_rng(11)
emb = rng.standard_normal(cfg.spk_emb_size).astype(np.float32)


def build_model(storage):
    m = A.FastSVCGenerator(in_channels=cfg.in_channels, mid_channels=list(cfg.mid_channels), upsampling_scales=list(cfg.upsampling_scales),
                           out_channels=cfg.out_channels, spk_emb_size=cfg.spk_emb_size, use_spk_emb=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synth_state_dict(cfg, 1).items()})
    m.remove_weight_norm()
    m.activation_storage = storage
    return m.eval().to(dev)


def features(F):
    f0 = np.where(rng.random((F, 1)) < 0.3, 0.0, rng.uniform(80, 400, (F, 1)))
    return {"ppg": rng.standard_normal((F, C), dtype=np.float32), "f0": f0, "lft": rng.uniform(-9, 1, (F * hop, 1)).astype(np.float32)}


def spread(name, seconds, audio):
    v = np.array(seconds) * 1e3
    med = float(np.median(v))
    return med, f"{name:44s} median {med:8.3f} ms  (min {v.min():8.3f}, max {v.max():8.3f})  {audio / (med / 1e3):8.1f} x real time"


class Yardstick:
    """N utterances resident as packed device buffers (ppg time-major, lft, excitation); batch k is window k of every one."""

    def __init__(self, model, N, core, K):
        self.model, self.N, self.core = model, N, core
        F = (K + 3) * core                           # (window K still has its whole right context)
        self.rows = Dc.window_plan([F] * N, core, ctx)
        per = -(-F // core)
        self.batches = [[u * per + k for u in range(N)] for k in range(per)]
        self.layout, stage_elems = Dc.stitch_layout(self.rows, self.batches, hop, FADE)
        feats = [features(F) for _ in range(N)]
        self.ppg = torch.from_numpy(np.concatenate([f["ppg"].reshape(-1) for f in feats])).to(dev)
        self.lft = torch.from_numpy(np.concatenate([f["lft"].reshape(-1) for f in feats])).to(dev)
        f0 = torch.from_numpy(np.stack([Dc.F0Statistics().convert(f["f0"].reshape(-1), [5.0, 1.0], [5.3, 1.0]) for f in feats])
                              .astype(np.float32)).to(dev)
        self.sine = sg(f0.view(N, 1, F)).reshape(-1).contiguous()
        self.F = F
        self.stage = torch.empty(max(stage_elems, 1), dtype=torch.float32, device=dev)
        self.emb = torch.from_numpy(np.tile(emb, (N, 1))).to(dev)
        self.host = torch.empty(N * (core + FADE) * hop + 8 * N, dtype=torch.int16, pin_memory=True)
        self.K = K

    @torch.no_grad()
    def batch(self, k):
        """Window k (1 <= k <= K: full context on both sides) of every utterance."""
        chunk, lay = self.batches[k], self.layout[k]
        rows = [self.rows[r] for r in chunk]
        lens = [r[2] - r[1] for r in rows]
        width = max(lens)
        ppg, lft, sine = window_assemble(self.ppg, self.lft, self.sine, [(u * self.F + r[1]) * C for u, r in enumerate(rows)],
                                         [(u * self.F + r[1]) * hop for u, r in enumerate(rows)], lens, C, hop, width)
        y = self.model(ppg, sine, lft, self.emb, lengths=lens).to(torch.float32)
        packed = torch.empty(max(lay["total"], 1), dtype=torch.int16, device=dev)
        window_stitch(y.view(len(rows), width * hop), lay["n_samples"], lay["core_lo"], lay["core_hi"], lay["half"], lay["left_mode"],
                      lay["right_mode"], lay["left_src"], lay["right_src"], lay["dst_off"], stage=self.stage, out_pcm=packed)
        self.host[: lay["total"]].copy_(packed[: lay["total"]], non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        return lens


def main():
    out = [f"stream latency: one StreamSession.push that completes one window per stream (every stream delivers `core` frames), "
           f"host to host, against one batch of the same rows through window_assemble + forward + window_stitch + download with "
           f"the features and the excitation already resident (the yardstick); context {ctx}, fade {FADE}, speaker embedding, F0 "
           f"shift on, int16 out; {pushes} pushes / batches per repetition, {reps} repetitions, legs alternated, median of the "
           f"repetitions' means (min, max); {torch.cuda.get_device_name(0)}"]
    print(out[0], flush=True)
    K = 8
    for storage in ("float32", "bfloat16"):
        m = build_model(storage)
        out.append(f"--- activation storage {storage}")
        for core in (32, 100):
            for N in (1, 8, 32):
                src = [features(core * 8) for _ in range(N)]
                yard = Yardstick(m, N, core, K)
                with Dc.StreamSession(m, sg, dev, n_streams=N, core=core, fade=FADE, max_push=core) as s:
                    ids = [s.open(emb, [5.0, 1.0], [5.3, 1.0], seed=i) for i in range(N)]
                    step = [0]

                    def push():
                        a = (step[0] % 8) * core
                        step[0] += 1
                        return s.push({i: dict(ppg=f["ppg"][a: a + core], f0=f["f0"][a: a + core], lft=f["lft"][a * hop: (a + core) * hop])
                                       for i, f in zip(ids, src)})
                    for _ in range(6):                   # (fill the context, warm every shape)
                        got = push()
                    before = s.forwards
                    got = push()
                    assert s.forwards == before + 1 and all(v.size == core * hop for v in got.values())
                    for k in range(1, 4):
                        lens = yard.batch(k)
                    assert lens == [core + 2 * ctx] * N
                    t = {"push": [], "yard": []}
                    for _ in range(reps):
                        t0 = time.perf_counter()
                        for _ in range(pushes):
                            push()
                        t["push"].append((time.perf_counter() - t0) / pushes)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for j in range(pushes):
                            yard.batch(1 + j % K)
                        t["yard"].append((time.perf_counter() - t0) / pushes)
                    s.end(ids)
                audio = N * core * hop / SR
                mp, line_p = spread(f"{N:2d} streams, core {core:3d}: push", t["push"], audio)
                my, line_y = spread(f"{N:2d} streams, core {core:3d}: resident batch", t["yard"], audio)
                out += [line_p, line_y, f"    push / resident batch {mp / my:.3f}; a push delivers {audio * 1e3:.1f} ms of audio "
                                        f"({core * hop / SR * 1e3:.1f} ms per stream)"]
                print("\n".join(out[-3:]), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "decode_stream.txt"), "w") as f:
        f.write("\n".join(out) + "\n")


def main_norm(horizon=None):
    # the two legs: (its name in the report, StreamSession's arguments), the yardstick first
    if horizon is None:
        pair = [("norm=window", dict(norm="window")), ("norm=running", dict(norm="running"))]
    else:
        pair = [("norm=running", dict(norm="running")), (f"horizon={horizon:g}", dict(norm="running", horizon=horizon))]
    (base, _), (other, _) = pair
    out = [f"stream norm: one StreamSession.push that completes one window per stream (every stream delivers `core` frames), host "
           f"to host, {other}{'' if horizon is None else ' (at least the core)'} against {base} on the same chunks, two sessions in "
           f"one process; context {ctx}, fade "
           f"{FADE}, speaker embedding, F0 shift on, int16 out; {pushes} pushes per repetition, {reps} repetitions, legs alternated, "
           f"median of the repetitions' means (min, max); {torch.cuda.get_device_name(0)}"]
    print(out[0], flush=True)
    for storage in ("float32", "bfloat16"):
        m = build_model(storage)
        out.append(f"--- activation storage {storage}")
        for core in (32, 100):
            for N in (1, 8, 32):
                src = [features(core * 8) for _ in range(N)]
                legs = {}
                for name, kw in pair:
                    if kw.get("horizon") is not None and kw["horizon"] < core:
                        kw = dict(kw, horizon=float(core))           # (a horizon is at least the core)
                    s = Dc.StreamSession(m, sg, dev, n_streams=N, core=core, fade=FADE, max_push=core, **kw)
                    legs[name] = dict(s=s, ids=[s.open(emb, [5.0, 1.0], [5.3, 1.0], seed=i) for i in range(N)], step=0, t=[])

                def push(leg):
                    a = (leg["step"] % 8) * core
                    leg["step"] += 1
                    return leg["s"].push({i: dict(ppg=f["ppg"][a: a + core], f0=f["f0"][a: a + core], lft=f["lft"][a * hop: (a + core) * hop])
                                          for i, f in zip(leg["ids"], src)})
                for leg in legs.values():
                    for _ in range(6):                   # (fill the context, warm every shape)
                        push(leg)
                    before = leg["s"].forwards
                    got = push(leg)
                    assert leg["s"].forwards == before + 1 and all(v.size == core * hop for v in got.values())
                for _ in range(reps):
                    for leg in legs.values():
                        t0 = time.perf_counter()
                        for _ in range(pushes):
                            push(leg)
                        leg["t"].append((time.perf_counter() - t0) / pushes)
                for leg in legs.values():
                    leg["s"].end(leg["ids"])
                    leg["s"].close()
                audio = N * core * hop / SR
                mw, line_w = spread(f"{N:2d} streams, core {core:3d}: push, {base}", legs[base]["t"], audio)
                mr, line_r = spread(f"{N:2d} streams, core {core:3d}: push, {other}", legs[other]["t"], audio)
                tail = "" if horizon is None else f"; spread of the {base} leg {(max(legs[base]['t']) - min(legs[base]['t'])) * 1e6:.0f} us"
                out += [line_w, line_r, f"    {other.split('=')[0] if horizon is not None else 'running'} / "
                                        f"{base.split('=')[1]} {mr / mw:.3f} ({(mr - mw) * 1e3:+.0f} us a push{tail})"]
                print("\n".join(out[-3:]), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "decode_stream_norm.txt" if horizon is None else "decode_stream_horizon.txt"), "w") as f:
        f.write("\n".join(out) + "\n")


def main_audio():
    core = 32
    lag = Dc.stream_loudness_lag(hop)
    out = [f"stream loudness: one StreamSession.push that completes one window per stream (every stream delivers {core} frames), host "
           f"to host, loudness=audio (the chunk carries {core} x {hop} samples of audio; the push finalises {core} frames of loudness "
           f"per stream on the device, {lag} frames behind the audio: two more launches) against loudness=given (the chunk carries "
           f"the loudness) on the same ppg and f0, two sessions in one process; context {ctx}, fade {FADE}, speaker embedding, F0 "
           f"shift on, int16 out; {pushes} pushes per repetition, {reps} repetitions, legs alternated, median of the repetitions' "
           f"means (min, max); {torch.cuda.get_device_name(0)}"]
    print(out[0], flush=True)
    for storage in ("float32", "bfloat16"):
        m = build_model(storage)
        out.append(f"--- activation storage {storage}")
        for N in (1, 8, 32):
            src = [features(core * 8) for _ in range(N)]
            for f in src:
                f["audio"] = (0.1 * rng.standard_normal((core * 8 * hop, 1))).astype(np.float32)
            legs = {}
            for name in ("given", "audio"):
                s = Dc.StreamSession(m, sg, dev, n_streams=N, core=core, fade=FADE, max_push=core, loudness=name)
                legs[name] = dict(s=s, ids=[s.open(emb, [5.0, 1.0], [5.3, 1.0], seed=i) for i in range(N)], step=0, t=[],
                                  key="lft" if name == "given" else "audio")

            def push(leg):
                a = (leg["step"] % 8) * core
                leg["step"] += 1
                k = leg["key"]
                return leg["s"].push({i: {"ppg": f["ppg"][a: a + core], "f0": f["f0"][a: a + core], k: f[k][a * hop: (a + core) * hop]}
                                      for i, f in zip(leg["ids"], src)})
            for leg in legs.values():
                for _ in range(6):                       # (fill the context, warm every shape)
                    push(leg)
                before = leg["s"].forwards
                got = push(leg)
                assert leg["s"].forwards == before + 1 and all(v.size == core * hop for v in got.values())
            for _ in range(reps):
                for leg in legs.values():
                    t0 = time.perf_counter()
                    for _ in range(pushes):
                        push(leg)
                    leg["t"].append((time.perf_counter() - t0) / pushes)
            for leg in legs.values():
                leg["s"].end(leg["ids"])
                leg["s"].close()
            audio = N * core * hop / SR
            mg, line_g = spread(f"{N:2d} streams, core {core:3d}: push, loudness=given", legs["given"]["t"], audio)
            ma, line_a = spread(f"{N:2d} streams, core {core:3d}: push, loudness=audio", legs["audio"]["t"], audio)
            out += [line_g, line_a, f"    audio / given {ma / mg:.3f} ({(ma - mg) * 1e3:+.0f} us a push; spread of the given leg "
                                    f"{(max(legs['given']['t']) - min(legs['given']['t'])) * 1e6:.0f} us)"]
            print("\n".join(out[-3:]), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "decode_stream_loudness.txt"), "w") as f:
        f.write("\n".join(out) + "\n")


def main_f0():
    core = 32
    lag = Dc.stream_loudness_lag(hop)
    out = [f"stream F0: one StreamSession.push that completes one window per stream (every stream delivers {core} frames), host to "
           f"host, f0=audio (the chunk carries ppg and {core} x {hop} samples of audio; the push finalises {core} frames of F0 by YIN, "
           f"their F0 shift and their excitation per stream on the device, {lag} frames behind the audio: two more launches, "
           f"csrc/fastsvc_stream_f0.hip) against f0=given (the chunk carries the F0, shifted on the host; the push synthesises the "
           f"excitation), both with loudness=audio on the same ppg and audio, two sessions in one process; context {ctx}, fade "
           f"{FADE}, speaker embedding, F0 shift on, int16 out; {pushes} pushes per repetition, {reps} repetitions, legs alternated, "
           f"median of the repetitions' means (min, max); {torch.cuda.get_device_name(0)}"]
    print(out[0], flush=True)
    t = np.arange(core * 8 * hop) / SR
    for storage in ("float32", "bfloat16"):
        m = build_model(storage)
        out.append(f"--- activation storage {storage}")
        for N in (1, 8, 32):
            src = [features(core * 8) for _ in range(N)]
            for i, f in enumerate(src):                  # (a voiced tone per stream over a little noise)
                ph = 2.0 * np.pi * (110.0 + 7.0 * i) * t
                f["audio"] = (0.3 * np.sin(ph) + 0.1 * np.sin(2.0 * ph) + 0.01 * rng.standard_normal(t.size)).astype(np.float32)[:, None]
            legs = {}
            for name in ("given", "audio"):
                s = Dc.StreamSession(m, sg, dev, n_streams=N, core=core, fade=FADE, max_push=core, loudness="audio", f0=name)
                legs[name] = dict(s=s, ids=[s.open(emb, [5.0, 1.0], [5.3, 1.0], seed=i) for i in range(N)], step=0, t=[])

            def push(leg, name):
                a = (leg["step"] % 8) * core
                leg["step"] += 1
                chunks = {}
                for i, f in zip(leg["ids"], src):
                    chunks[i] = {"ppg": f["ppg"][a: a + core], "audio": f["audio"][a * hop: (a + core) * hop]}
                    if name == "given":
                        chunks[i]["f0"] = f["f0"][a: a + core]
                return leg["s"].push(chunks)
            for name, leg in legs.items():
                for _ in range(6):                       # (fill the context, warm every shape)
                    push(leg, name)
                before = leg["s"].forwards
                got = push(leg, name)
                assert leg["s"].forwards == before + 1 and all(v.size == core * hop for v in got.values())
            for _ in range(reps):
                for name, leg in legs.items():
                    t0 = time.perf_counter()
                    for _ in range(pushes):
                        push(leg, name)
                    leg["t"].append((time.perf_counter() - t0) / pushes)
            for leg in legs.values():
                leg["s"].end(leg["ids"])
                leg["s"].close()
            audio = N * core * hop / SR
            mg, line_g = spread(f"{N:2d} streams, core {core:3d}: push, f0=given", legs["given"]["t"], audio)
            ma, line_a = spread(f"{N:2d} streams, core {core:3d}: push, f0=audio", legs["audio"]["t"], audio)
            out += [line_g, line_a, f"    audio / given {ma / mg:.3f} ({(ma - mg) * 1e3:+.0f} us a push; spread of the given leg "
                                    f"{(max(legs['given']['t']) - min(legs['given']['t'])) * 1e6:.0f} us)"]
            print("\n".join(out[-3:]), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "decode_stream_f0.txt"), "w") as f:
        f.write("\n".join(out) + "\n")


def main_f0_stats():
    core = 32
    lag = Dc.stream_loudness_lag(hop)
    trg = [5.3, 1.0]
    out = [f"stream F0 statistics: one StreamSession.push that completes one window per stream (every stream delivers {core} "
           f"frames), host to host, streams opened with RunningF0Stats() (the push finalises {core} frames per stream, {lag} frames "
           f"behind the audio: F0 by YIN, the running source statistics and their shift - one more launch, "
           f"stream_f0_running_kernel - and the excitation) against the same streams opened with list statistics (the shift inside "
           f"the F0 launch), both loudness=audio, f0=audio on the same ppg and audio, two sessions in one process; context {ctx}, "
           f"fade {FADE}, speaker embedding, int16 out; {pushes} pushes per repetition, {reps} repetitions, legs alternated, median "
           f"of the repetitions' means (min, max); {torch.cuda.get_device_name(0)}"]
    print(out[0], flush=True)
    t = np.arange(core * 8 * hop) / SR
    for storage in ("float32", "bfloat16"):
        m = build_model(storage)
        out.append(f"--- activation storage {storage}")
        for N in (1, 8, 32):
            src = [features(core * 8) for _ in range(N)]
            for i, f in enumerate(src):                  # (a voiced tone per stream over a little noise)
                ph = 2.0 * np.pi * (110.0 + 7.0 * i) * t
                f["audio"] = (0.3 * np.sin(ph) + 0.1 * np.sin(2.0 * ph) + 0.01 * rng.standard_normal(t.size)).astype(np.float32)[:, None]
            legs = {}
            for name, stats in (("list", [5.0, 1.0]), ("running", Dc.RunningF0Stats())):
                s = Dc.StreamSession(m, sg, dev, n_streams=N, core=core, fade=FADE, max_push=core, loudness="audio", f0="audio")
                legs[name] = dict(s=s, ids=[s.open(emb, stats, trg, seed=i) for i in range(N)], step=0, t=[])

            def push(leg):
                a = (leg["step"] % 8) * core
                leg["step"] += 1
                return leg["s"].push({i: {"ppg": f["ppg"][a: a + core], "audio": f["audio"][a * hop: (a + core) * hop]}
                                      for i, f in zip(leg["ids"], src)})
            for leg in legs.values():
                for _ in range(6):                       # (fill the context, warm every shape)
                    push(leg)
                before = leg["s"].forwards
                got = push(leg)
                assert leg["s"].forwards == before + 1 and all(v.size == core * hop for v in got.values())
            for _ in range(reps):
                for leg in legs.values():
                    t0 = time.perf_counter()
                    for _ in range(pushes):
                        push(leg)
                    leg["t"].append((time.perf_counter() - t0) / pushes)
            voiced = legs["running"]["s"].f0_stats(legs["running"]["ids"][0])["voiced_frames"]
            for leg in legs.values():
                leg["s"].end(leg["ids"])
                leg["s"].close()
            audio = N * core * hop / SR
            ml, line_l = spread(f"{N:2d} streams, core {core:3d}: push, list statistics", legs["list"]["t"], audio)
            mr, line_r = spread(f"{N:2d} streams, core {core:3d}: push, RunningF0Stats()", legs["running"]["t"], audio)
            out += [line_l, line_r, f"    running / list {mr / ml:.3f} ({(mr - ml) * 1e3:+.0f} us a push; spread of the list leg "
                                    f"{(max(legs['list']['t']) - min(legs['list']['t'])) * 1e6:.0f} us; stream 0 counted {voiced} "
                                    f"voiced frames)"]
            print("\n".join(out[-3:]), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "decode_stream_f0_stats.txt"), "w") as f:
        f.write("\n".join(out) + "\n")


def main_f0_track():
    core = 32
    lag = Dc.stream_loudness_lag(hop)
    track = Dc.F0Track()
    out = [f"stream F0 tracking: one StreamSession.push that completes one window per stream (every stream delivers {core} "
           f"frames), host to host, f0_track=F0Track() (the push finalises {core} frames per stream, {lag} frames behind the audio: "
           f"their YIN candidates, the Viterbi recurrence over them and the trace of the frames {track.lag} behind - one more "
           f"launch, stream_f0_track_kernel - their shift and the excitation) against f0_track=None (the per-frame pick inside the "
           f"frames launch), both loudness=audio, f0=audio on the same ppg and audio, two sessions in one process; context {ctx}, "
           f"fade {FADE}, speaker embedding, F0 shift on, int16 out; {pushes} pushes per repetition, {reps} repetitions, legs "
           f"alternated, median of the repetitions' means (min, max); {torch.cuda.get_device_name(0)}"]
    print(out[0], flush=True)
    t = np.arange(core * 8 * hop) / SR
    for storage in ("float32", "bfloat16"):
        m = build_model(storage)
        out.append(f"--- activation storage {storage}")
        for N in (1, 8, 32):
            src = [features(core * 8) for _ in range(N)]
            for i, f in enumerate(src):                  # (a voiced tone per stream over a little noise)
                ph = 2.0 * np.pi * (110.0 + 7.0 * i) * t
                f["audio"] = (0.3 * np.sin(ph) + 0.1 * np.sin(2.0 * ph) + 0.01 * rng.standard_normal(t.size)).astype(np.float32)[:, None]
            legs = {}
            for name, tk in (("untracked", None), ("tracked", track)):
                s = Dc.StreamSession(m, sg, dev, n_streams=N, core=core, fade=FADE, max_push=core, loudness="audio", f0="audio",
                                     f0_track=tk)
                legs[name] = dict(s=s, ids=[s.open(emb, [5.0, 1.0], [5.3, 1.0], seed=i) for i in range(N)], step=0, t=[])

            def push(leg):
                a = (leg["step"] % 8) * core
                leg["step"] += 1
                return leg["s"].push({i: {"ppg": f["ppg"][a: a + core], "audio": f["audio"][a * hop: (a + core) * hop]}
                                      for i, f in zip(leg["ids"], src)})
            for leg in legs.values():
                for _ in range(6):                       # (fill the context, warm every shape)
                    push(leg)
                before = leg["s"].forwards
                got = push(leg)
                assert leg["s"].forwards == before + 1 and all(v.size == core * hop for v in got.values())
            for _ in range(reps):
                for leg in legs.values():
                    t0 = time.perf_counter()
                    for _ in range(pushes):
                        push(leg)
                    leg["t"].append((time.perf_counter() - t0) / pushes)
            latency = [legs[k]["s"].latency_frames for k in ("untracked", "tracked")]
            for leg in legs.values():
                leg["s"].end(leg["ids"])
                leg["s"].close()
            audio = N * core * hop / SR
            mu, line_u = spread(f"{N:2d} streams, core {core:3d}: push, f0_track=None", legs["untracked"]["t"], audio)
            mt, line_t = spread(f"{N:2d} streams, core {core:3d}: push, f0_track=F0Track()", legs["tracked"]["t"], audio)
            out += [line_u, line_t, f"    tracked / untracked {mt / mu:.3f} ({(mt - mu) * 1e3:+.0f} us a push; spread of the untracked leg "
                                    f"{(max(legs['untracked']['t']) - min(legs['untracked']['t'])) * 1e6:.0f} us; latency "
                                    f"{latency[0]} -> {latency[1]} frames)"]
            print("\n".join(out[-3:]), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "decode_stream_f0_track.txt"), "w") as f:
        f.write("\n".join(out) + "\n")


def main_checked():
    core, storage = 32, "float16"
    out = [f"checked streams: one StreamSession.push that completes one window per stream (every stream delivers {core} frames), "
           f"host to host, checked=True (one stream_check launch, 16 bytes a row copied into page-locked memory and one wait per "
           f"forward; no window falls back) against checked=False on the same chunks, two sessions in one process, activation "
           f"storage {storage}; context {ctx}, fade {FADE}, speaker embedding, F0 shift on, int16 out; {pushes} pushes per "
           f"repetition, {reps} repetitions, legs alternated, median of the repetitions' means (min, max); "
           f"{torch.cuda.get_device_name(0)}"]
    print(out[0], flush=True)
    m = build_model(storage)
    for norm in ("window", "running"):
        out.append(f"--- norm={norm}")
        for N in (1, 8, 32):
            src = [features(core * 8) for _ in range(N)]
            legs = {}
            for name in ("unchecked", "checked"):
                s = Dc.StreamSession(m, sg, dev, n_streams=N, core=core, fade=FADE, max_push=core, norm=norm, checked=name == "checked")
                legs[name] = dict(s=s, ids=[s.open(emb, [5.0, 1.0], [5.3, 1.0], seed=i) for i in range(N)], step=0, t=[])

            def push(leg):
                a = (leg["step"] % 8) * core
                leg["step"] += 1
                return leg["s"].push({i: dict(ppg=f["ppg"][a: a + core], f0=f["f0"][a: a + core], lft=f["lft"][a * hop: (a + core) * hop])
                                      for i, f in zip(leg["ids"], src)})
            for leg in legs.values():
                for _ in range(6):                       # (fill the context, warm every shape)
                    push(leg)
                before = leg["s"].forwards
                got = push(leg)
                assert leg["s"].forwards == before + 1 and all(v.size == core * hop for v in got.values())
            for _ in range(reps):
                for leg in legs.values():
                    t0 = time.perf_counter()
                    for _ in range(pushes):
                        push(leg)
                    leg["t"].append((time.perf_counter() - t0) / pushes)
            fell = sum(legs["checked"]["s"].totals(i)["fell_back"] for i in legs["checked"]["ids"])
            for leg in legs.values():
                leg["s"].end(leg["ids"])
                leg["s"].close()
            audio = N * core * hop / SR
            mu, line_u = spread(f"{N:2d} streams, core {core:3d}: push, unchecked", legs["unchecked"]["t"], audio)
            mc, line_c = spread(f"{N:2d} streams, core {core:3d}: push, checked", legs["checked"]["t"], audio)
            out += [line_u, line_c, f"    checked / unchecked {mc / mu:.3f} ({(mc - mu) * 1e3:+.0f} us a push; spread of the unchecked leg "
                                    f"{(max(legs['unchecked']['t']) - min(legs['unchecked']['t'])) * 1e6:.0f} us; {fell} windows fell back)"]
            print("\n".join(out[-3:]), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "decode_stream_checked.txt"), "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    argv = sys.argv[1:]
    if "--checked" in argv:
        main_checked()
    elif "--f0-track" in argv:
        main_f0_track()
    elif "--f0-stats" in argv:
        main_f0_stats()
    elif "--f0" in argv:
        main_f0()
    elif "--audio" in argv:
        main_audio()
    elif "--horizon" in argv:
        if "--norm" not in argv or argv.index("--horizon") + 1 >= len(argv):
            sys.exit("--horizon H goes with --norm")
        main_norm(float(argv[argv.index("--horizon") + 1]))
    else:
        main_norm() if "--norm" in argv else main()
