"""Single-process training driver: ``TrainSession`` batches into ``TrainStep`` (cf. ``harana/bin/train_fastsvc.py``).

    python -m svcc23_fastsvc_amd.train --train-dumpdir dump/train --dev-dumpdir dump/dev --config conf.yaml --outdir exp/

What the reference's ``Trainer.run`` does per step (train_fastsvc.py:76-103, 240-256, 313-356), without its DataLoader:
both dump directories are uploaded once (``TrainSession``), every step is one batch cut out on the device and one
``TrainStep.step``; every ``eval_interval_steps`` the mean of ``TrainStep.eval_step`` over the development set (file
order, fixed crops), every ``save_interval_steps`` a checkpoint in the reference's schema, until ``train_max_steps``.
The sampler is a pure function of (seed, epoch, index), so ``--resume`` needs nothing but the step count the checkpoint
holds.  One GPU; a data-parallel caller builds its own loop from ``TrainSession(rank=, world=)`` and ``TrainStep(group=)``.
"""
from __future__ import annotations

import argparse
import glob
import os
from typing import Dict, List, Optional

import torch

from .training import RECIPE

DEFAULTS = {
    # egs/svcc23/fastsvc1/conf/fastsvc.yaml: what RECIPE does not hold
    "sampling_rate": 16000, "hop_size": 160, "aux_context_window": 0,
    "generator_type": "FastSVCGenerator",
    "generator_params": dict(in_channels=144, out_channels=1, mid_channels=[192, 96, 48, 24],
                             upsampling_scales=[2, 4, 4, 5], spk_emb_size=512, use_spk_emb=True),
    "discriminator_type": "MelGANMultiScaleDiscriminator",
    "signal_generator": dict(sine_amp=0.1, noise_amp=0.003, signal_types=["sine"]),
    "train_max_steps": 600000, "save_interval_steps": 50000, "eval_interval_steps": 5000, "log_interval_steps": 5000,
    "seed": 0,
}


def load_dumpdir(path: str) -> List[dict]:
    from .decode import load_features
    files = sorted(glob.glob(os.path.join(path, "*.npz")) + glob.glob(os.path.join(path, "*.h5")))
    if not files:
        raise ValueError(f"no .npz / .h5 dumps in {path}")
    return [load_features(p) for p in files]


def evaluate(step, session) -> Dict[str, float]:
    """Mean of ``eval_step`` over one pass of ``session`` (train_fastsvc.py:313-340)."""
    total: Dict[str, float] = {}
    n = 0
    for batch in session.batches(0):
        for k, v in step.eval_step(batch).items():
            total[k] = total.get(k, 0.0) + v
        n += 1
    return {k: v / max(n, 1) for k, v in total.items()}


def main(argv=None) -> int:                                   # pragma: no cover - exercised on a GPU box
    import yaml
    from . import FastSVCGenerator
    from . import training as TR
    from .checkpoint import load_checkpoint, save_checkpoint
    from .train_session import TrainSession
    ap = argparse.ArgumentParser(description="FastSVC training on one GPU (cf. harana-train-fastsvc)")
    ap.add_argument("--train-dumpdir", required=True, help="directory of per-utterance training dumps (.npz / .h5)")
    ap.add_argument("--dev-dumpdir", required=True, help="directory of development dumps")
    ap.add_argument("--config", default=None, help="recipe yaml; missing keys take the recipe's values")
    ap.add_argument("--outdir", required=True, help="checkpoints and config.yml go here")
    ap.add_argument("--resume", default="", nargs="?", help="checkpoint to continue from")
    ap.add_argument("--storage", default="float32", choices=["float32", "bfloat16", "float16"],
                    help="activation storage of the generator's forward")
    args = ap.parse_args(argv)
    config = dict(DEFAULTS)
    config.update(RECIPE)
    if args.config:
        with open(args.config) as f:
            config.update(yaml.safe_load(f) or {})
    os.makedirs(args.outdir, exist_ok=True)
    device = torch.device("cuda")
    if config["generator_type"] != "FastSVCGenerator":
        raise ValueError(f"generator_type {config['generator_type']!r}: only FastSVCGenerator is implemented here")
    generator = FastSVCGenerator(**config["generator_params"])
    generator.activation_storage = args.storage
    discriminator = getattr(TR, config["discriminator_type"])(**config["discriminator_params"])
    generator, discriminator = generator.to(device).train(), discriminator.to(device).train()
    step = TR.TrainStep(generator, discriminator, config, steps=0)
    optimizer = {"generator": step.opt_g, "discriminator": step.opt_d}
    scheduler = {"generator": step.sched_g, "discriminator": step.sched_d}
    if args.resume:
        info = load_checkpoint(args.resume, generator, discriminator, optimizer, scheduler)
        step.steps = int(info["steps"])
        print(f"resumed {args.resume} at {step.steps} steps")
    common = dict(batch_size=config["batch_size"], batch_length=config["batch_length"], hop_size=config["hop_size"],
                  sample_rate=config["sampling_rate"], aux_context_window=config.get("aux_context_window", 0),
                  signal_generator_params=config.get("signal_generator"),
                  use_spk_emb=bool(config["generator_params"].get("use_spk_emb", False)))
    train = TrainSession(load_dumpdir(args.train_dumpdir), device, seed=int(config.get("seed", 0)), shuffle=True, **common)
    dev = TrainSession(load_dumpdir(args.dev_dumpdir), device, seed=1, shuffle=False, **common)
    print(f"{len(train.sampler.eligible)} training / {len(dev.sampler.eligible)} development utterances resident "
          f"({train.resident_bytes + dev.resident_bytes} bytes)")
    per_epoch = len(train.sampler.global_indices())
    max_steps = int(config["train_max_steps"])
    log_every, eval_every, save_every = (int(config[k]) for k in ("log_interval_steps", "eval_interval_steps", "save_interval_steps"))

    def save() -> None:
        path = os.path.join(args.outdir, f"checkpoint-{step.steps}steps.pkl")
        save_checkpoint(path, generator, discriminator, optimizer, scheduler, steps=step.steps,
                        epochs=step.steps // per_epoch, config=config)
        print(f"saved {path}")

    saved_at: Optional[int] = None
    while step.steps < max_steps:
        # `steps` batches have been drawn so far: the next one is batch steps % per_epoch of epoch steps // per_epoch
        epoch, first = divmod(step.steps, per_epoch)
        for batch in train.batches(epoch, first):
            logging = (step.steps + 1) % log_every == 0
            log = step.step(batch, log=logging)
            if logging:
                print(f"(steps {step.steps}) " + ", ".join(f"{k} = {v:.4f}" for k, v in log.items()))
            if step.steps % eval_every == 0:
                ev = evaluate(step, dev)
                print(f"(steps {step.steps}) " + ", ".join(f"eval/{k} = {v:.4f}" for k, v in ev.items()))
            if step.steps % save_every == 0:
                save()
                saved_at = step.steps
            if step.steps >= max_steps:
                break
    if saved_at != step.steps:
        save()
    return step.steps


if __name__ == "__main__":                                    # pragma: no cover
    main()
