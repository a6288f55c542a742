#!/usr/bin/env python
"""What re-packing the generator's weights costs a training step, host route against device route (developer tool;
its output is profiles/pack_device.txt).  Yaml generator, one process, after warm-up, the two routes ALTERNATING so that
clock and thermal drift land on both:

  (a) the existing route as the train step runs it - gather the 251 parameters, device-to-host copy, fastsvc_pack_weights
      on the host pool, upload of the 65 MB blob - by a host clock that ends in a stream synchronise; and the upload
      alone, by events (the part of that route no host-side work can remove);
  (b) Plan.pack_device by events (GPU time) and by the host clock of its call (what the step's issue path pays), and its
      launch count.

Then TrainStep at the recipe batch (32 x 16000 samples) with `pack_on_device` false / true, alternating, float32 and
bfloat16 storage.  Medians, with the spread (min .. max) of the repetitions."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import synth as S
from svcc23_fastsvc_amd import training as TR

REPS = int(os.environ.get("PACK_TIME_REPS", "15"))
STEP_REPS = int(os.environ.get("PACK_TIME_STEP_REPS", "5"))       # blocks of STEP_BLOCK steps per setting
STEP_BLOCK = 6
cfg = S.FULL_CONFIG
dev = torch.device("cuda:0")


def stat(xs):
    return f"median {statistics.median(xs):8.3f} ms   (min {min(xs):.3f} .. max {max(xs):.3f}, n = {len(xs)})"


def new_generator(storage="float32"):
    torch.manual_seed(1234)
    gen = A.FastSVCGenerator(in_channels=cfg.in_channels, mid_channels=list(cfg.mid_channels),
                             upsampling_scales=list(cfg.upsampling_scales), out_channels=1,
                             spk_emb_size=cfg.spk_emb_size, use_spk_emb=True)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in S.synth_state_dict(cfg, 201).items()})
    gen.activation_storage = storage
    return gen.to(dev).train()


def pack_routes():
    gen = new_generator()
    plan = gen.plan
    params = dict(gen.named_parameters())
    print(f"yaml generator: {len(params)} tensors, {sum(p.numel() for p in params.values())} floats; blob {plan.blob_bytes} bytes; "
          f"fastsvc_pack_device_scratch_bytes {plan.pack_device_scratch_bytes}; launches per pack_device {plan.pack_device_launches} "
          f"(kernels + 1 table copy + 1 memset)")
    dev_blob = torch.empty(plan.blob_bytes // 4, dtype=torch.float32, device=dev)
    up_blob = torch.empty_like(dev_blob)
    host_ms, upload_ms, dev_gpu_ms, dev_call_ms = [], [], [], []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for it in range(REPS + 3):
        # (a) host route, as FastSVCGenerator.packed_weights runs it behind prefetch_packed_weights
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pre = plan.pack_prefetch(gen.state_dict())
        host = plan.pack(gen.state_dict(), reuse_pinned=True, prefetched=pre)
        up_blob.copy_(host, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ev[0].record()
        up_blob.copy_(host, non_blocking=True)              # the upload alone (page-locked source)
        ev[1].record()
        # (b) device route
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ev[2].record()
        plan.pack_device(params, out=dev_blob)
        ev[3].record()
        t3 = time.perf_counter()
        torch.cuda.synchronize()
        if it >= 3:
            host_ms.append((t1 - t0) * 1e3)
            upload_ms.append(ev[0].elapsed_time(ev[1]))
            dev_gpu_ms.append(ev[2].elapsed_time(ev[3]))
            dev_call_ms.append((t3 - t2) * 1e3)
    assert torch.equal(dev_blob.view(torch.uint8), up_blob.view(torch.uint8)), "the two routes disagree"
    print("the two routes' blobs are byte-identical")
    print(f"(a) host route, gather + download + fastsvc_pack_weights + upload   {stat(host_ms)}")
    print(f"(a) the upload alone (events)                                       {stat(upload_ms)}")
    print(f"(b) pack_device, GPU time (events)                                  {stat(dev_gpu_ms)}")
    print(f"(b) pack_device, host time of the call                              {stat(dev_call_ms)}")
    ok = statistics.median(dev_gpu_ms) < statistics.median(upload_ms)
    print(f"pack_device takes {'LESS' if ok else 'NOT less'} time than the upload alone: "
          f"{statistics.median(dev_gpu_ms):.3f} ms against {statistics.median(upload_ms):.3f} ms")


def train_steps(storage):
    B, F = TR.RECIPE["batch_size"], TR.RECIPE["batch_length"] // cfg.hop
    T = F * cfg.hop
    ins = S.device_batch(cfg, B, F, 5000, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(77)
    batch = (ins, torch.randn((B, 1, T), generator=g, device=dev) * 0.3)
    steps = {}
    for on in (False, True):
        gen = new_generator(storage)
        disc = TR.MelGANMultiScaleDiscriminator(**TR.RECIPE["discriminator_params"]).to(dev).train()
        steps[on] = TR.TrainStep(gen, disc, dict(discriminator_train_start_steps=0, pack_on_device=on,
                                                 autocast_dtype="bfloat16" if storage == "bfloat16" else None), steps=1)
        for _ in range(6):
            steps[on].step(batch, log=False)
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(STEP_REPS):
        for on in (False, True):
            t0 = time.perf_counter()
            for _ in range(STEP_BLOCK):
                steps[on].step(batch, log=False)
            torch.cuda.synchronize()
            ms[on].append((time.perf_counter() - t0) / STEP_BLOCK * 1e3)
    print(f"train step, batch {B} x {T}, {storage} storage, pack_on_device False   {stat(ms[False])}")
    print(f"train step, batch {B} x {T}, {storage} storage, pack_on_device True    {stat(ms[True])}")


if __name__ == "__main__":
    print(f"{torch.cuda.get_device_name(0)}; torch {torch.__version__}; {os.cpu_count()} host CPUs visible, "
          f"FASTSVC_PACK_THREADS={os.environ.get('FASTSVC_PACK_THREADS', 'unset')}")
    pack_routes()
    for storage in ("float32", "bfloat16"):
        train_steps(storage)
