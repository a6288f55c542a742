#!/usr/bin/env python
"""Where the cycles of a STEP of the conditioning pipelines go inside a wave (diagnostic).

Needs the stamped build:  python -m svcc23_fastsvc_amd.build --timeline   (-> libfastsvc_hip_timeline.so; the
product library is never stamped).  2-byte storage only.

    FASTSVC_TIMELINE_STORAGE=bfloat16 python tools/cond_timeline.py cfg3

In that build one c1 wave (0), one layer wave (4: c3) and one heads wave (8) of workgroup (1, 0) of
cond_stage0_pipe_kernel / cond_stage1_pipe_kernel - the three share a SIMD - stamp the cycle counter at five points of
256 consecutive steps (csrc/fastsvc_cond.hip, CsTl):
  0 step start (past the barrier)    1 every fragment of the step arrived     2 last product issued
  3 first accumulator read by the epilogue                                    4 last LDS store done
The stamps are scheduling fences: hipcc moves no work across them, and `arrived` is an explicit wait the product
build does not have - the table shows the order of the SOURCE, run as written.  Stage 0's c1 runs on the VALU:
its stamps 1, 2, 3 coincide.
"""
import os
import struct
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("FASTSVC_HIP_LIB", os.path.join(ROOT, "svcc23_fastsvc_amd", "libfastsvc_hip_timeline.so"))

ROLES = ("c1", "layer (c3)", "heads")
PHASES = ("wait for fragments", "products", "products -> epilogue", "epilogue + stores", "barrier / idle")


def analyse(path, layer):
    raw = open(path, "rb").read()
    roles, steps, words, tpw, B, T = struct.unpack("8q", raw[:64])[:6]
    tl = np.frombuffer(raw[64:], dtype=np.uint64).reshape(roles, steps, words).astype(np.int64)
    print(f"== {layer}: B {B}, T {T}, {tpw} chunks per workgroup, {steps} steps of workgroup (1, 0); median cycles (p10 - p90)")
    print(f"{'role':12s} " + " ".join(f"{p:>22s}" for p in PHASES) + f" {'step':>8s} {'epilogue starts at':>19s}")
    for r in range(roles):
        t = tl[r, :, :5]
        ok = (t[:, 0] > 0) & (np.diff(t, axis=1) >= 0).all(axis=1)
        ok[-1] = False
        nxt = np.roll(t[:, 0], -1)
        ok &= nxt > t[:, 4]
        if ok.sum() < 8:
            print(f"{ROLES[r]:12s} no stamps ({int(ok.sum())} usable steps)")
            continue
        seg = np.concatenate([np.diff(t, axis=1), (nxt - t[:, 4])[:, None]], axis=1)[ok]
        step = (nxt - t[:, 0])[ok]
        cells = [f"{int(np.median(seg[:, i])):8d} ({int(np.percentile(seg[:, i], 10)):5d}-{int(np.percentile(seg[:, i], 90)):5d})"
                 for i in range(5)]
        # how far into the product phase (stamp 1 .. stamp 2) the wave is when its epilogue reads the first accumulator
        prod = np.maximum(seg[:, 1], 1)
        frac = np.median((seg[:, 1] + seg[:, 2]) / prod)
        print(f"{ROLES[r]:12s} " + " ".join(f"{c:>22s}" for c in cells) + f" {int(np.median(step)):8d} {100 * frac:17.0f} %")


def main():
    import torch
    import svcc23_fastsvc_amd as A
    from svcc23_fastsvc_amd import synth as S
    wl = S.WORKLOADS[sys.argv[1] if len(sys.argv) > 1 else "cfg3"]
    cfg = S.FULL_CONFIG
    dev = torch.device("cuda:0")
    storage = os.environ.get("FASTSVC_TIMELINE_STORAGE", "bfloat16")
    plan = A.Plan(cfg, storage=storage, compact_workspace=True)
    blob = plan.pack(S.synth_state_dict(cfg, 201)).to(dev)
    if wl["B"] * wl["F"] > 20000:
        ins = list(S.device_batch(cfg, wl["B"], wl["F"], wl["seed"], dev))
    else:
        b = S.synth_batch(cfg, wl["B"], wl["F"], wl["seed"])
        ins = [torch.from_numpy(a).to(dev) for a in (b.ppg, b.sine, b.lft, b.spk_emb)]
    ws = torch.empty(plan.workspace_bytes(wl["B"], wl["F"]), dtype=torch.uint8, device=dev)
    tmp = tempfile.mkdtemp(prefix="cond_timeline_")
    for _ in range(3):
        plan.forward(blob, *ins, workspace=ws)
    torch.cuda.synchronize()
    print(f"# {os.path.basename(os.environ['FASTSVC_HIP_LIB'])}, {sys.argv[1] if len(sys.argv) > 1 else 'cfg3'} {storage}")
    for layer in ("cond.0", "cond.1"):
        out = os.path.join(tmp, f"{layer}.bin")
        os.environ["FASTSVC_TIMELINE_LAYER"] = layer
        os.environ["FASTSVC_TIMELINE_OUT"] = out
        plan.forward(blob, *ins, workspace=ws)
        torch.cuda.synchronize()
        if not os.path.exists(out):
            print(f"{layer}: the layer pipeline did not run (or not a --timeline build)")
            continue
        analyse(out, layer)
        os.remove(out)
    os.environ.pop("FASTSVC_TIMELINE_LAYER", None)
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
