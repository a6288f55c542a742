"""Throughput of the decode harness from HOST-resident features - what `python -m svcc23_fastsvc_amd.decode` does after
reading the dumps: 512 utterances of 2 - 10 s (SURVEY 8d's variant of cfg4), time-major numpy features, F0 shift on.

Four legs, for activation storage float32 and bfloat16, alternated within the one run and repeated (DECODE_REPS, default
5; spread printed), every timed region ending in a device synchronise:

    floats      decode_utterances: float32 waveforms back as numpy arrays (the leg this tool has always had)
    (a) pcm     the same followed by to_pcm16 of every utterance - what the CLI does per target speaker
    (b) first   DecodeSession(...) + its first convert(): packing, the one upload, int16 back
    (c) next    the same session's second convert(), for another speaker: F0 shift + f0 upload only

Before timing, (b) and (c) are checked to equal (a) sample for sample.  The figures go to profiles/decode_session.txt.

The checked legs (profiles/decode_checked.txt), in float16 activation storage on the same utterances:

    unchecked   a resident session's convert()                      } two sessions alive side by side, their converts
    checked     DecodeSession(checked=True)'s convert()             } alternated, DECODE_REPS each
    pack alone  pcm16_pack and pcm16_pack(report=) on 32 rows of 160000 samples, alternated, device time per call

The checked median is compared with the min - max spread of the unchecked repetitions of the same run; no threshold.

The fan-out leg (DECODE_LEGS=fanout only; profiles/decode_fanout.txt), float32 and bfloat16 storage, one resident session:

    sequential  S convert() calls, one per target speaker           } alternated, DECODE_REPS each, median
    fan-out     one convert_many() of the S speakers                }

for the first U in {1, 8, 64} utterances with S = 16 speakers, and for U = 512 with S = 2 (the large-corpus case).
The windowed leg (DECODE_LEGS=windowed only; profiles/decode_windowed.txt), float32 and bfloat16 storage, one resident session:

    whole       convert()                                            } alternated, DECODE_REPS each, median
    windowed    convert_windowed(core=400): windows of 400 + 2 x 36  }

on the 512 utterances, and on ONE utterance of 30 000 frames (200 s).  The recomputed context makes (core + 2 context) /
core the expected ratio for utterances much longer than a window.
The window-norm leg (DECODE_LEGS=window_norm only; profiles/decode_window_norm.txt), float32 and bfloat16 storage, one
resident session, max_batch 64, speaker embedding:

    whole       convert()                                                } alternated, DECODE_REPS each, median
    window      convert_windowed(core=400)                    per-window  }
    utterance   convert_windowed(core=400, norm="utterance")  pooled      }

on 64 utterances of 2 000 frames and on ONE utterance of 24 000 frames (60 windows: one batch).
    python tools/decode_throughput.py                  (DECODE_LEGS=session or =checked: one of the two parts only;
                                                        DECODE_LEGS=fanout: the fan-out leg; =windowed: the windowed leg;
                                                        =window_norm: the window-norm leg)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import synth as S, decode as Dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dev = torch.device("cuda:0")
cfg = S.FULL_CONFIG
frames = S.workload_frames("cfg4var")
n = int(os.environ.get("DECODE_UTTS", "512"))
reps = max(int(os.environ.get("DECODE_REPS", "5")), 1)
frames = frames[:n]
rng = np.random.default_rng(3)
feats = []
for f in frames:
    f0 = np.where(rng.random((f, 1)) < 0.3, 0.0, rng.uniform(80, 400, (f, 1)))
    feats.append({"ppg": rng.standard_normal((f, cfg.in_channels), dtype=np.float32), "f0": f0,
                  "lft": rng.uniform(-9, 1, (f * cfg.hop, 1)).astype(np.float32)})
sg = A.SignalGenerator(sample_rate=24000, hop_size=cfg.hop, noise_amp=0.0, signal_types=["sine"])
emb = rng.standard_normal(cfg.spk_emb_size).astype(np.float32)
emb2 = rng.standard_normal(cfg.spk_emb_size).astype(np.float32)
src = [[5.0, 1.0]] * len(feats)
trg, trg2 = [5.3, 1.0], [4.8, 1.0]
samples = sum(frames) * cfg.hop
MB = 64
lines = [f"decode_throughput: {len(feats)} utterances (cfg4var), {samples} samples = {samples / 24000:.0f} s of audio, "
         f"max_batch {MB}, {reps} repetitions, legs alternated; {torch.cuda.get_device_name(0)}",
         f"feature bytes (ppg + lft, unpadded): {4 * sum(frames) * (cfg.in_channels + cfg.hop) / 1e6:.1f} MB; "
         f"int16 waveforms: {2 * samples / 1e6:.1f} MB; float32 waveforms: {4 * samples / 1e6:.1f} MB"]
print("\n".join(lines), flush=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def build_model(storage):
    m = A.FastSVCGenerator(in_channels=cfg.in_channels, mid_channels=list(cfg.mid_channels), upsampling_scales=list(cfg.upsampling_scales),
                           out_channels=cfg.out_channels, spk_emb_size=cfg.spk_emb_size, use_spk_emb=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synth_state_dict(cfg, 1).items()})
    m.remove_weight_norm()
    m.activation_storage = storage
    return m.eval().to(dev)


def spread(name, seconds, unit_samples=None):
    v = np.array(seconds) * 1e3
    med = float(np.median(v))
    tail = "" if unit_samples is None else f"  {unit_samples / med / 1e3:7.1f} M samples/s"
    return med, f"{name:42s} median {med:9.3f} ms  (min {v.min():9.3f}, max {v.max():9.3f}){tail}"


def checked_legs():
    """float16 storage: unchecked against checked resident sessions, and the two pack entry points alone."""
    out = [lines[0], "--- activation storage float16, resident sessions: convert() of an unchecked and of a checked session, alternated"]
    m = build_model("float16")
    with Dc.DecodeSession(m, feats, sg, dev, src, max_batch=MB) as plain, \
            Dc.DecodeSession(m, feats, sg, dev, src, max_batch=MB, checked=True) as chk:
        want, got = plain.convert(emb, trg), chk.convert(emb, trg)               # (warm: first converts wait for the uploads)
        same = all(np.array_equal(a, b) for a, b in zip(got, want))
        fell = sum(1 for r in chk.last_report if r["tried"])
        clipped = sum(1 for r in chk.last_report if r["clipped"])
        out.append(f"checked output equals unchecked sample for sample: {same}; forwards {chk.forwards} for {len(chk.batches)} batches; "
                   f"{fell} utterances fell back, {clipped} have clipped samples, largest max_abs "
                   f"{max(r['max_abs'] for r in chk.last_report):.3f}; report download {16 * len(feats)} bytes per convert")
        del want, got
        t = {"u": [], "c": []}
        for _ in range(reps):
            t["u"].append(timed(lambda: plain.convert(emb2, trg2))[0])
            t["c"].append(timed(lambda: chk.convert(emb2, trg2))[0])
    mu, line_u = spread("unchecked convert, per speaker", t["u"], samples)
    mc, line_c = spread("checked convert, per speaker", t["c"], samples)
    inside = min(t["u"]) * 1e3 <= mc <= max(t["u"]) * 1e3
    out += [line_u, line_c, f"checked median - unchecked median: {mc - mu:+.3f} ms ({(mc / mu - 1) * 100:+.2f} %); checked median "
            f"{'inside' if inside else 'OUTSIDE'} the unchecked min - max spread"]
    # the two entry points alone
    B, W, calls = 32, 160000, 50
    y = (torch.randn(B, W, device=dev) * 0.35).contiguous()
    lens = [W] * B
    dst = torch.empty(B * W, dtype=torch.int16, device=dev)
    report = torch.empty((B, 4), dtype=torch.int32, device=dev)

    def device_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls * 1e-3

    legs = {"p": lambda: A.pcm16_pack(y, lens, out=dst), "c": lambda: A.pcm16_pack(y, lens, out=dst, report=report)}
    for fn in legs.values():
        device_ms(fn)
    tp = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            tp[k].append(device_ms(fn))
    out.append(f"--- pack entry points alone: {B} rows of {W} samples ({6 * B * W / 1e6:.1f} MB read + written by the packs), "
               f"{calls} calls per repetition, device time per call")
    mp, line_p = spread("pcm16_pack", tp["p"])
    mk, line_k = spread("pcm16_pack(report=)  [memset + launch]", tp["c"])
    out += [line_p + f"  {6 * B * W / mp / 1e6:7.1f} GB/s", line_k + f"  {6 * B * W / mk / 1e6:7.1f} GB/s",
            f"checked pack - unchecked pack: {(mk - mp) * 1e3:+.1f} us per call ({(mk / mp - 1) * 100:+.1f} %)"]
    print("\n".join(out[1:]), flush=True)
    assert same, "the checked session differs from the unchecked one"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "decode_checked.txt"), "w") as f:
        f.write("\n".join(out) + "\n")


def fanout_legs():
    """Sequential converts against one convert_many, same session, same process."""
    out = [f"decode fan-out: S sequential DecodeSession.convert() calls against one convert_many() of the same S speakers; "
           f"utterances of 2 - 10 s (cfg4var), max_batch {MB}, F0 shift on, int16 out, {reps} repetitions, legs alternated, "
           f"median (min, max); {torch.cuda.get_device_name(0)}"]
    for storage in ("float32", "bfloat16"):
        m = build_model(storage)
        out.append(f"--- activation storage {storage}")
        for U, n_spk in ((1, 16), (8, 16), (64, 16), (512, 2)):
            if U > len(feats):
                continue
            sub, fr = feats[:U], frames[:U]
            r = np.random.default_rng(100 + U)
            speakers = [(r.standard_normal(cfg.spk_emb_size).astype(np.float32), [4.6 + 0.05 * k, 1.0]) for k in range(n_spk)]
            unit = sum(fr) * cfg.hop * n_spk
            with Dc.DecodeSession(m, sub, sg, dev, src[:U], max_batch=MB) as s:
                seq = lambda: [s.convert(e, t) for e, t in speakers]                         # noqa: E731
                fan = lambda: s.convert_many(speakers)                                       # noqa: E731
                want, got = seq(), fan()                                                     # (warm both; compare)
                diff = max(int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max()) for ws, gs in zip(want, got) for a, b in zip(ws, gs))
                n_seq, n_fan = len(s.batches) * n_spk, len(Dc.fanout_batches(fr, n_spk, MB, s.pad_tolerance))
                up = s.uploaded_bytes
                up_seq, up_fan, up_init = sum(up["convert"]) / n_spk, up["convert_many"][0], up["fanout_init"]
                del want, got
                t = {"seq": [], "fan": []}
                for _ in range(reps):
                    t["seq"].append(timed(seq)[0])
                    t["fan"].append(timed(fan)[0])
            ms, line_s = spread(f"U {U:3d} S {n_spk:2d} sequential ({n_seq} forwards)", t["seq"], unit)
            mf, line_f = spread(f"U {U:3d} S {n_spk:2d} fan-out    ({n_fan} forwards)", t["fan"], unit)
            out += [line_s, line_f,
                    f"    fan-out / sequential time {mf / ms:.3f} (speed-up {ms / mf:.2f} x); largest PCM-16 difference {diff}; "
                    f"uploads: {up_seq:.0f} B per convert, {up_fan} B per convert_many, {up_init} B once"]
            print("\n".join(out[-3:]), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "decode_fanout.txt"), "w") as f:
        f.write("\n".join(out) + "\n")


def windowed_legs():
    """convert against convert_windowed(core=400), same session, same process."""
    CORE = 400
    ctx = -(-Dc.receptive_field_frames(cfg) // 4) * 4
    out = [f"windowed decode: DecodeSession.convert() against convert_windowed(core={CORE}) (context {ctx}, fade 8: "
           f"(core + 2 context) / core = {(CORE + 2 * ctx) / CORE:.3f}); max_batch {MB}, F0 shift on, speaker embedding, int16 out, "
           f"{reps} repetitions, legs alternated, median (min, max); {torch.cuda.get_device_name(0)}"]
    r = np.random.default_rng(5)
    F_long = 30000
    long = [{"ppg": r.standard_normal((F_long, cfg.in_channels), dtype=np.float32),
             "f0": np.where(r.random((F_long, 1)) < 0.3, 0.0, r.uniform(80, 400, (F_long, 1))),
             "lft": r.uniform(-9, 1, (F_long * cfg.hop, 1)).astype(np.float32)}]
    for storage in ("float32", "bfloat16"):
        m = build_model(storage)
        out.append(f"--- activation storage {storage}")
        for name, sub, fr in ((f"{len(feats)} utterances of 2 - 10 s", feats, frames), ("1 utterance of 30000 frames", long, [F_long])):
            unit = sum(fr) * cfg.hop
            rows = Dc.window_plan(fr, CORE, ctx)
            with Dc.DecodeSession(m, sub, sg, dev, src[:len(sub)], max_batch=MB) as s:
                whole = lambda: s.convert(emb, trg)                                          # noqa: E731
                wind = lambda: s.convert_windowed(emb, trg, core=CORE)                       # noqa: E731
                torch.cuda.reset_peak_memory_stats(dev)
                want = whole()
                torch.cuda.synchronize()
                peak_w = torch.cuda.max_memory_allocated(dev)
                torch.cuda.reset_peak_memory_stats(dev)
                got = wind()                                                                 # (warm both; compare)
                torch.cuda.synchronize()
                peak_g = torch.cuda.max_memory_allocated(dev)
                diff = max(int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max()) for a, b in zip(want, got))
                n_whole, n_wind = len(s.batches), s.forwards
                work = sum(b - a for _, a, b, _, _ in rows) / sum(fr)
                del want, got
                t = {"whole": [], "wind": []}
                for _ in range(reps):
                    t["whole"].append(timed(whole)[0])
                    t["wind"].append(timed(wind)[0])
            mw, line_w = spread(f"{name}: whole    ({n_whole} forwards)", t["whole"], unit)
            mg, line_g = spread(f"{name}: windowed ({n_wind} forwards)", t["wind"], unit)
            out += [line_w, line_g,
                    f"    windowed / whole time {mg / mw:.3f}; frames computed / frames of audio {work:.3f}; {len(rows)} windows; "
                    f"largest PCM-16 difference to the whole-utterance result {diff} (per-window InstanceNorm statistics); peak "
                    f"device memory whole {peak_w / 2 ** 20:.0f} MiB, windowed {peak_g / 2 ** 20:.0f} MiB"]
            print("\n".join(out[-3:]), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "decode_windowed.txt"), "w") as f:
        f.write("\n".join(out) + "\n")


def window_norm_legs():
    """convert, convert_windowed(core=400) and convert_windowed(core=400, norm="utterance"), same session, same process."""
    CORE, mb = 400, 64
    out = [f"window-norm decode: DecodeSession.convert() against convert_windowed(core={CORE}) with norm=\"window\" and "
           f"norm=\"utterance\"; max_batch {mb}, F0 shift on, speaker embedding, int16 out, {reps} repetitions, legs alternated, "
           f"median (min, max); {torch.cuda.get_device_name(0)}"]
    r = np.random.default_rng(7)

    def utt(F):
        return {"ppg": r.standard_normal((F, cfg.in_channels), dtype=np.float32),
                "f0": np.where(r.random((F, 1)) < 0.3, 0.0, r.uniform(80, 400, (F, 1))),
                "lft": r.uniform(-9, 1, (F * cfg.hop, 1)).astype(np.float32)}
    sets = (("64 utterances of 2000 frames", [utt(2000) for _ in range(64)]), ("1 utterance of 24000 frames", [utt(24000)]))
    for storage in ("float32", "bfloat16"):
        m = build_model(storage)
        out.append(f"--- activation storage {storage}")
        for name, sub in sets:
            unit = sum(len(f["ppg"]) for f in sub) * cfg.hop
            with Dc.DecodeSession(m, sub, sg, dev, [[5.0, 1.0]] * len(sub), max_batch=mb) as s:
                legs = {"whole": lambda: s.convert(emb, trg),
                        "window": lambda: s.convert_windowed(emb, trg, core=CORE),
                        "utterance": lambda: s.convert_windowed(emb, trg, core=CORE, norm="utterance")}
                res, nfw = {}, {}
                for k, fn in legs.items():                                                   # (warm all three; compare)
                    res[k] = fn()
                    nfw[k] = len(s.batches) if k == "whole" else s.forwards
                diff = {k: max(int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max()) for a, b in zip(res["whole"], res[k]))
                        for k in ("window", "utterance")}
                del res
                t = {k: [] for k in legs}
                for _ in range(reps):
                    for k, fn in legs.items():
                        t[k].append(timed(fn)[0])
            med = {}
            for k in legs:
                med[k], line = spread(f"{name}: {k:9s} ({nfw[k]} forwards)", t[k], unit)
                out.append(line)
            out.append(f"    norm=utterance / norm=window time {med['utterance'] / med['window']:.3f}; largest PCM-16 difference to "
                       f"convert(): norm=window {diff['window']}, norm=utterance {diff['utterance']}")
            print("\n".join(out[-4:]), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "decode_window_norm.txt"), "w") as f:
        f.write("\n".join(out) + "\n")


LEGS = os.environ.get("DECODE_LEGS", "all")
for storage in (("float32", "bfloat16") if LEGS in ("all", "session") else ()):
    m = build_model(storage)

    def floats(e=emb, t=trg):
        return Dc.decode_utterances(m, feats, sg, dev, trg_emb=e, src_f0_stats=src, trg_f0_stats=t, max_batch=MB)

    def with_pcm(e=emb, t=trg):
        return [Dc.to_pcm16(y) for y in floats(e, t)]

    # warm every shape (packs, code objects, page-locked pools) and check the session against the existing path
    want, want2 = with_pcm(), with_pcm(emb2, trg2)
    assert all(y.shape == (f * cfg.hop,) for y, f in zip(want, frames))
    with Dc.DecodeSession(m, feats, sg, dev, src, max_batch=MB) as s:
        got, got2 = s.convert(emb, trg), s.convert(emb2, trg2)
        same = all(np.array_equal(a, b) for a, b in zip(got, want)) and all(np.array_equal(a, b) for a, b in zip(got2, want2))
        up = dict(s.uploaded_bytes)
    del want, want2, got, got2
    t = {"floats": [], "a": [], "b": [], "c": []}
    for _ in range(reps):
        t["floats"].append(timed(floats)[0])
        t["a"].append(timed(with_pcm)[0])
        box = {}

        def first():
            box["s"] = Dc.DecodeSession(m, feats, sg, dev, src, max_batch=MB)
            return box["s"].convert(emb, trg)
        t["b"].append(timed(first)[0])
        t["c"].append(timed(lambda: box["s"].convert(emb2, trg2))[0])
        box["s"].close()
    names = {"floats": "decode_utterances (float32 waveforms)", "a": "(a) decode_utterances + to_pcm16",
             "b": "(b) DecodeSession + first convert", "c": "(c) second convert, another speaker"}
    out = [f"--- activation storage {storage}: session output equals (a) sample for sample: {same}; uploaded by the "
           f"constructor {up['init'] / 1e6:.1f} MB, by each convert {up['convert'][0] / 1e6:.2f} MB"]
    for key, name in names.items():
        v = np.array(t[key]) * 1e3
        med = float(np.median(v))
        out.append(f"{name:42s} median {med:8.1f} ms  (min {v.min():8.1f}, max {v.max():8.1f})  "
                   f"{samples / med / 1e3:7.1f} M samples/s  {samples / 24000 / med * 1e3:6.0f} x real time")
    print("\n".join(out), flush=True)
    lines += out
    assert same, "DecodeSession differs from decode_utterances + to_pcm16"
if LEGS in ("all", "session"):
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "decode_session.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
if LEGS in ("all", "checked"):
    checked_legs()
if LEGS == "fanout":
    fanout_legs()
if LEGS == "windowed":
    windowed_legs()
if LEGS == "window_norm":
    window_norm_legs()
