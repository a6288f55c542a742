#!/usr/bin/env python
"""Randomised parity sweep on the GPU (developer tool): random (B, F), ragged or not, with / without
speaker embedding, table / cost-model / forced-Winograd launch choices, vs the CPU oracle.
STRESS_STORAGE=bfloat16 sweeps the bfloat16-storage path (mean-abs error relative to the rms: 3e-2; utterances of
1-2 frames, whose InstanceNorm statistics are over 4-8 samples in stage 0, sit at 3.3-3.7e-2 and get 5e-2);
STRESS_STORAGE=float16 the float16-storage path, held to the same bounds (its error is several times smaller).
FASTSVC_COND_PIPE=2 forces the layer pipelines of conditioning stages 0 / 1 at every size."""
import os, sys, random
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import synth as S
from oracle import fastsvc_oracle as O

STORAGE = os.environ.get("STRESS_STORAGE", "float32")
TWO_BYTE = STORAGE in ("bfloat16", "float16")        # 2-byte storage: the relative error measure and its bounds
seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
n = int(sys.argv[2]) if len(sys.argv) > 2 else 12
rng = random.Random(seed)
cfg = S.FULL_CONFIG
dev = torch.device("cuda:0")
sd = S.synth_state_dict(cfg, 900 + seed)
wf = S.fold_weight_norm(sd)
worst = 0.0
for it in range(n):
    table = rng.random() < 0.5
    compact = rng.random() < 0.5
    plan = A.Plan(cfg, load_shipped_table=table, storage=STORAGE, compact_workspace=compact)
    blob = plan.pack(sd).to(dev)
    B = rng.choice([1, 1, 2, 3, 5, 8])
    F = rng.choice([1, 2, 3, 4, 6, 9, 17, 32, 45, 63, 64, 100, 131, 150, 257])
    spk = rng.random() < 0.8
    ragged = B > 1 and rng.random() < 0.4
    lens = [rng.randint(1, F) for _ in range(B)] if ragged else None
    if lens: lens[rng.randrange(B)] = F
    b = S.synth_batch(cfg, B, F, 5000 + it + 100 * seed)
    ins = [torch.from_numpy(a).to(dev) for a in (b.ppg, b.sine, b.lft)]
    emb = torch.from_numpy(b.spk_emb).to(dev) if spk else None
    # a DIRTY workspace: the forward allocates its workspace from the caching allocator, which hands back this block
    need = plan.workspace_bytes(B, plan.padded_frames(F))
    junk = torch.full((need // 4 + 16,), rng.choice([1e30, float("nan"), -3e38, 1000.0, float("inf")]), dtype=torch.float32, device=dev)
    del junk
    y = plan.forward(blob, *ins, emb, lengths=lens).cpu()
    err = 0.0
    if lens is None:
        ref = O.forward_dedup(wf, cfg.upsampling_scales, b.ppg, b.sine, b.lft, b.spk_emb if spk else None)
        err = float((y - ref).abs().max()) / max(1.0, float(ref.abs().max()))
        if TWO_BYTE: err = float((y - ref).abs().mean()) / max(1e-6, float(ref.pow(2).mean().sqrt()))     # relative to the rms
    else:
        for i, m in enumerate(lens):
            ref = O.forward_dedup(wf, cfg.upsampling_scales, b.ppg[i:i+1, :, :m], b.sine[i:i+1, :, :m*160],
                                  b.lft[i:i+1, :, :m*160], b.spk_emb[i:i+1] if spk else None)
            e = float((y[i:i+1, :, :m*160] - ref).abs().max()) / max(1.0, float(ref.abs().max()))
            if TWO_BYTE: e = float((y[i:i+1, :, :m*160] - ref).abs().mean()) / max(1e-6, float(ref.pow(2).mean().sqrt()))
            err = max(err, e)
            assert float(y[i, :, m*160:].abs().max()) == 0.0 if m < F else True
    if err > (5e-2 if TWO_BYTE else 1e-4) and os.environ.get("STRESS_DEBUG"):
        def one(pl, **kw):
            yy = pl.forward(blob, *ins, emb, lengths=lens, **kw).cpu()
            if lens is None:
                return float((yy - ref).abs().max())
            return max(float((yy[i:i+1, :, :m*160] - O.forward_dedup(wf, cfg.upsampling_scales, b.ppg[i:i+1, :, :m], b.sine[i:i+1, :, :m*160], b.lft[i:i+1, :, :m*160], b.spk_emb[i:i+1] if spk else None)).abs().max()) for i, m in enumerate(lens))
        print("   again, same plan:", [round(one(plan), 6) for _ in range(3)])
        p2 = A.Plan(cfg, load_shipped_table=table, storage=STORAGE, compact_workspace=compact)
        print("   fresh plan:", [round(one(p2), 6) for _ in range(2)])
        p3 = A.Plan(cfg, load_shipped_table=table, storage=STORAGE, compact_workspace=compact); p3.pad_odd_lengths = False
        print("   fresh plan, no padding:", [round(one(p3), 6) for _ in range(2)])
        wsz = torch.zeros(plan.workspace_bytes(B, plan.padded_frames(F)), dtype=torch.uint8, device=dev)
        print("   zeroed workspace:", [round(one(p2, workspace=wsz), 6) for _ in range(2)])
        for v in (1e30, float("nan"), -3e38, 1000.0, float("inf")):
            junk = torch.full((need // 4 + 16,), v, dtype=torch.float32, device=dev); del junk
            print(f"   allocator block poisoned with {v}:", round(one(p2), 6))
        torch.cuda.synchronize()
    worst = max(worst, err)
    tol = (5e-2 if min(lens or [F]) <= 2 else 3e-2) if TWO_BYTE else 1e-4
    flag = "" if err <= tol else "   <-- ABOVE TOLERANCE"
    print(f"B={B} F={F} spk={spk} lens={lens} table={table} compact={compact}: rel err {err:.2e}{flag}", flush=True)
print(f"worst {worst:.3e}")
