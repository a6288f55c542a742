#!/usr/bin/env python
"""What every launch route of the forward chose, as one JSON object on stdout (developer tool; the guard of
tests/test_launch_routes_gpu.py, whose fixture tests/golden/launch_routes.json is this tool's output):

    python tools/dump_routes.py > tests/golden/launch_routes.json

{case: [[layer, kernel, tpw], ...]} in launch order - the kernel as in the profile record, the whole-stage
conditioning launches with a fourth entry `small` -, read back from the FASTSVC_VERBOSE_SHAPES lines of profiled
forwards.  Routes follow from shapes, storage, speaker mode and the launch table, never from the data.

Cases:
  matrix/<config>/<storage>/<spk|nospk>/<full|ragged>[/compact]   tests/config_matrix.py on an EMPTY table (cost model
        and gates): B = 2, F = 24 and lengths 28/25/22/23/7/1 padded to 28, the seeds of tests/test_config_matrix_gpu.py
  default/<storage>/<spk|nospk>/<B>x<F>     the default configuration on the SHIPPED table (compact workspace): 1 x 152 exact
        entries, 2 x 24 nearest-entry priors, 1 x 3 the exact-float32 route (2-byte storage: 1 x 4 with one utterance of 3
        frames, which is how the engine runs 3 frames there)
  hand/<storage>[/cond45|/plain]      a hand-made table at 2 x 24 (hand_table below; /cond45: the other
        conditioning kernel under each cond key; /plain: default workspace layout, where stages 0 and 1 run as chains)
  tune/<storage>     autotune=True at 2 x 24 on an empty table: {"keys": sorted keys the pass wrote, "trials": count}
        (not the winners: they depend on timing)
"""
import json
import os
import re
import sys
import tempfile

os.environ["FASTSVC_VERBOSE_SHAPES"] = "1"          # read once, when the library first launches: before it loads
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import config_matrix as CM
import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import synth as S

STORAGES = ("float32", "bfloat16", "float16")
B_FULL, F_FULL = 2, 24
LENS, F_PAD = [28, 25, 22, 23, 7, 1], 28
SEED_X_FULL, SEED_X_RAGGED = 621, 622
LINE = re.compile(r"^\[fastsvc\] (\S+) (\S+) tpw (\d+)(?: small (\d+))?$")
dev = torch.device("cuda:0")


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def routes(plan, blob, b, spk, lengths=None):
    """one profiled forward with file descriptor 2 in a temporary file; the choices it printed"""
    ins = [_t(b.ppg), _t(b.sine), _t(b.lft), _t(b.spk_emb) if spk else None]
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            recs = []
            plan.forward(blob, *ins, profile=recs, lengths=lengths)
            torch.cuda.synchronize()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    out = []
    for line in text.splitlines():
        m = LINE.match(line)
        if m:
            out.append([m.group(1), m.group(2), int(m.group(3))] + ([int(m.group(4))] if m.group(4) is not None else []))
        else:
            sys.stderr.write(line + "\n")              # (whatever else was said on stderr goes where it was meant to)
    return out


def hand_table(storage, cond):
    """Default configuration, 2 x 24 (T = 3840; rows of 48 / 192 / 768 / 3840 columns).  `cond`: (algorithm under cond.0,
    under cond.1)."""
    s = {"float32": "", "bfloat16": "|b", "float16": "|h"}[storage]
    b_only = "|b" if storage == "float16" else s                # a "|b" entry without its "|h" twin: float16 falls back to it
    return {
        f"up.2.conv_first|2|192{s}": [2, 1, 4, 2, 0],           # run_conv, one entry per algorithm: 0 ...
        f"up.1.conv_first|2|48{s}": [1, 1, 4, 1, 1],            # ... 1 (Winograd, the layer's grouping)
        f"down.2.c2_d2|2|192{s}": [1, 1, 4, 1, 2],              # ... 2 (Winograd, 32-channel groups)
        f"up.3.d9|2|3840{s}": [2, 1, 4, 3, 3],                  # ... 3 (half-precision MFMA)
        f"up.0.d27|2|48{s}": [6, 4, 2, 2, 6],                   # ... 6 (the wide layers' kernel: 2-byte storage only)
        f"down.1.c23|2|768{s}": [2, 1, 4, 2, 3],                # chain: fused, with a shape
        f"down.2.c23|2|192{s}": [3, 1, 4, 1, 0],                # chain: two launches
        f"up.1.d3x|2|192{s}": [4, 2, 2, 2, 0],                  # d3x: algorithm 0 that still carries a valid shape
        "up.0.head|2|24": [2, 1, 4, 1, 3],                      # fused head (float32 storage only; no suffix)
        f"cond.0|2|3840{s}": [1, 1, 1, 1, cond[0]],
        f"cond.1|2|768{s}": [1, 1, 1, 1, cond[1]],
        f"up.3.d27|2|3840{s}": [4, 4, 1, 2, 3],                 # stale: WM = 4 needs 4 channel groups, C = 24 has one
        f"up.2.d9|2|768{b_only}": [2, 1, 4, 2, 3],
    }


def main():
    out = {}
    # 1. the configuration matrix on an empty table
    for name in CM.NAMES:
        cfg = CM.config(name)
        sd = S.synth_state_dict(cfg, CM.SEED_W)
        full = S.synth_batch(cfg, B_FULL, F_FULL, SEED_X_FULL)
        ragged = S.synth_batch(cfg, len(LENS), F_PAD, SEED_X_RAGGED)
        for st in STORAGES:
            blob = None
            for compact in (False, True):
                plan = A.Plan(cfg, storage=st, load_shipped_table=False, compact_workspace=compact)
                if blob is None:
                    blob = plan.pack(sd).to(dev)
                for spk in CM.speaker_modes(name):
                    tag = f"matrix/{name}/{st}/{'spk' if spk else 'nospk'}"
                    sfx = "/compact" if compact else ""
                    out[f"{tag}/full{sfx}"] = routes(plan, blob, full, spk)
                    out[f"{tag}/ragged{sfx}"] = routes(plan, blob, ragged, spk, lengths=LENS)
    # 2. - 4. the default configuration
    cfg = S.FULL_CONFIG
    sd = S.synth_state_dict(cfg, CM.SEED_W)
    batches = {(B, F): S.synth_batch(cfg, B, F, SEED_X_FULL) for B, F in ((1, 152), (2, 24), (1, 3), (1, 4))}
    for st in STORAGES:
        plan = A.Plan(cfg, storage=st, compact_workspace=True)
        blob = plan.pack(sd).to(dev)
        for spk in (True, False):
            tag = f"default/{st}/{'spk' if spk else 'nospk'}"
            out[f"{tag}/1x152"] = routes(plan, blob, batches[(1, 152)], spk)
            out[f"{tag}/2x24"] = routes(plan, blob, batches[(2, 24)], spk)
            if st == "float32":
                out[f"{tag}/1x3"] = routes(plan, blob, batches[(1, 3)], spk)
            else:
                out[f"{tag}/1x4of3"] = routes(plan, blob, batches[(1, 4)], spk, lengths=[3])
        for case, compact, cond in (("", True, (5, 4)), ("/cond45", True, (4, 5)), ("/plain", False, (5, 4))):
            plan = A.Plan(cfg, storage=st, load_shipped_table=False, compact_workspace=compact)
            plan.load_tuned(hand_table(st, cond))
            out[f"hand/{st}{case}"] = routes(plan, blob, batches[(2, 24)], True)
        if st != "float16":
            plan = A.Plan(cfg, storage=st, load_shipped_table=False)
            b = batches[(2, 24)]
            plan.forward(blob, _t(b.ppg), _t(b.sine), _t(b.lft), _t(b.spk_emb), autotune=True)
            torch.cuda.synchronize()
            out[f"tune/{st}"] = {"keys": sorted(plan.tuned_shapes()), "trials": plan.last_autotune_trials}
    # one case per line: the fixture diffs case by case
    print("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(out[k])}" for k in sorted(out)) + "\n}")


if __name__ == "__main__":
    main()
