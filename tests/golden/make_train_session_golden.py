#!/usr/bin/env python
"""Generate tests/golden/train_session.npz from the LIVE reference (build container only; CPU).

    python tests/golden/make_train_session_golden.py

Two parts, data only (inputs regenerated from the integer-hash generator where they are large):

  Collater cases   the reference's own ``Collater`` (harana/bin/train_fastsvc.py:437-557; noise_amp = 0,
                   use_spk_emb = True) for aux_context_window 0 and 2 on four tiny utterances (hop 4, D 5, S 3,
                   6 frames per crop; utterance lengths frames + 2 ctx + 1, + 2, 9 + 2 ctx and 70 frames), two draws
                   each: the utterances, the start frames it drew (``np.random.randint`` wrapped) and its five outputs.
                   Checked while generating: the four sliced outputs equal plain numpy slicing at those start frames
                   bit for bit.
  Eval case        one ``Trainer._eval_step`` (:266-311) on the tiny-width generator and a small MelGAN multi-scale
                   discriminator, the ``Trainer`` constructed as make_golden.py's `train` case constructs it; weights,
                   inputs and target come from the hash generator on both sides; the seven ``eval/*`` values.
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.refimport import import_reference, _placeholder  # noqa: E402
from oracle.refimport import REFERENCE_ROOT as ROOT_REF  # noqa: E402
from svcc23_fastsvc_amd import synth as S  # noqa: E402

warnings.filterwarnings("ignore")
torch.set_num_threads(8)

HOP, D, EMB, FRAMES = 4, 5, 3, 6


def import_trainer():
    # (the trainer module imports two off-path packages that are not installed here: placeholders, test tooling only)
    for name in ("tensorboardX", "soundfile"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                _placeholder(name)
    if not hasattr(sys.modules["tensorboardX"], "SummaryWriter"):
        sys.modules["tensorboardX"].SummaryWriter = lambda *a, **k: None
    from harana.bin import train_fastsvc as TR
    return TR


def utterance(seed: int, n: int) -> dict:
    """n frames in the dump's layout (audio_feats_dataset.py:30-34): time-major, trailing singleton axes."""
    u = lambda name, k: S.hash_uniform(seed, S.stream_id("train_session." + name), k)      # noqa: E731
    f0 = 80.0 + 320.0 * u("f0", n)
    f0[u("uv", n) < 0.25] = 0.0                                          # unvoiced frames
    return {"wave": (0.6 * u("wave", n * HOP) - 0.3).astype(np.float32),
            "f0": f0.astype(np.float32).reshape(n, 1),
            "ppg": (u("ppg", n * D) - 0.5).astype(np.float32).reshape(n, D),
            "lft": u("lft", n * HOP).astype(np.float32).reshape(n * HOP, 1),
            "spk_emb": (u("emb", EMB) - 0.5).astype(np.float32).reshape(EMB, 1)}


def collater_cases(TR, out: dict) -> None:
    for ctx in (0, 2):
        lengths = [FRAMES + 2 * ctx + 1, FRAMES + 2 * ctx + 2, 9 + 2 * ctx, 70]
        utts = [utterance(500 + 10 * ctx + i, n) for i, n in enumerate(lengths)]
        for i, u in enumerate(utts):
            for k, v in u.items():
                out[f"c{ctx}/utt{i}/{k}"] = v
        col = TR.Collater(batch_length=FRAMES * HOP, sample_rate=16000, hop_size=HOP, aux_context_window=ctx,
                          sine_amp=0.1, noise_amp=0.0, signal_types=["sine"], use_spk_emb=True)
        items = [(u["wave"], u["f0"], u["ppg"], u["lft"], u["spk_emb"]) for u in utts]
        drawn = []
        real = np.random.randint

        def recording(*a, **k):
            v = real(*a, **k)
            drawn.append(int(v))
            return v

        np.random.seed(1234 + ctx)
        np.random.randint = recording
        try:
            for draw in range(2):
                del drawn[:]
                (ppg, sine, lft, emb), y = col(items)
                starts = list(drawn)
                assert len(starts) == len(utts)
                for i, (u, s) in enumerate(zip(utts, starts)):
                    assert ctx <= s < lengths[i] - FRAMES - ctx
                    assert np.array_equal(y[i, 0].numpy(), u["wave"][s * HOP: (s + FRAMES) * HOP])
                    assert np.array_equal(lft[i, 0].numpy(), u["lft"][s * HOP: (s + FRAMES) * HOP, 0])
                    assert np.array_equal(ppg[i].numpy(), u["ppg"][s - ctx: s + FRAMES + ctx].T)
                    assert np.array_equal(emb[i].numpy(), u["spk_emb"][:, 0])
                out[f"c{ctx}/draw{draw}/starts"] = np.array(starts, dtype=np.int64)
                for k, v in (("ppg", ppg), ("sine", sine), ("lft", lft), ("emb", emb), ("y", y)):
                    out[f"c{ctx}/draw{draw}/{k}"] = v.numpy().copy()
        finally:
            np.random.randint = real
    out["collater/meta"] = np.array([HOP, D, EMB, FRAMES, 16000], dtype=np.int64)


def eval_case(M, TR, out: dict) -> None:
    from harana.losses import MultiResolutionSTFTLoss, GeneratorAdversarialLoss, DiscriminatorAdversarialLoss
    from harana.optimizers import RAdam
    import yaml
    with open(os.path.join(ROOT_REF, "egs/svcc23/fastsvc1/conf/fastsvc.yaml")) as f:
        recipe = yaml.safe_load(f)
    cfg = S.TINY_CONFIG
    B, F = 2, 25
    T = F * cfg.hop
    seed_w, seed_x, seed_d, seed_t = 411, 412, 413, 414
    g = M.FastSVCGenerator(in_channels=cfg.in_channels, mid_channels=list(cfg.mid_channels),
                           upsampling_scales=list(cfg.upsampling_scales), out_channels=cfg.out_channels,
                           spk_emb_size=cfg.spk_emb_size, use_spk_emb=cfg.use_spk_emb)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in S.synth_state_dict(cfg, seed_w).items()}, strict=True)
    dparams = dict(recipe["discriminator_params"])
    dparams.update(scales=2, channels=4, max_downsample_channels=32, downsample_scales=[4, 4])
    Dm = M.MelGANMultiScaleDiscriminator(**dparams)
    S.fill_module_from_hash(Dm, seed_d)
    conf = dict(recipe)
    conf.update(discriminator_train_start_steps=0, use_stft_loss=True, lambda_aux=1.0, outdir="/tmp",
                train_max_steps=10 ** 9, log_interval_steps=10 ** 9, eval_interval_steps=10 ** 9, save_interval_steps=10 ** 9)
    crit = {"gen_adv": GeneratorAdversarialLoss(), "dis_adv": DiscriminatorAdversarialLoss(),
            "stft": MultiResolutionSTFTLoss(**recipe["stft_loss_params"])}
    opt = {"generator": RAdam(g.parameters(), **recipe["generator_optimizer_params"]),
           "discriminator": RAdam(Dm.parameters(), **recipe["discriminator_optimizer_params"])}
    sch = {k: torch.optim.lr_scheduler.StepLR(opt[k], **recipe[k + "_scheduler_params"]) for k in opt}
    tr = TR.Trainer(steps=1, epochs=0, data_loader={}, sampler={"train": None}, model={"generator": g, "discriminator": Dm},
                    criterion=crit, optimizer=opt, scheduler=sch, config=conf, device=torch.device("cpu"))
    tr.tqdm = types.SimpleNamespace(update=lambda n: None)
    b = S.synth_batch(cfg, B, F, seed_x)
    target = torch.from_numpy((0.3 * S.hash_normalish(seed_t, S.stream_id("train.target"), B * T)).reshape(B, 1, T).astype(np.float32))
    x = tuple(torch.from_numpy(a) for a in (b.ppg, b.sine, b.lft, b.spk_emb))
    for m in (g, Dm):                                        # _eval_epoch's switch (train_fastsvc.py:318-320)
        m.eval()
    tr.total_eval_loss.clear()
    tr._eval_step((x, target))
    for k, v in tr.total_eval_loss.items():
        assert k.startswith("eval/")
        out["eval/" + k.split("/")[-1]] = np.float64(v)
    assert len([k for k in out if k.startswith("eval/")]) == 7
    out["eval/meta"] = np.array([seed_w, seed_x, seed_d, seed_t, B, F], dtype=np.int64)
    out["eval/dparams"] = np.array([dparams["scales"], dparams["channels"], dparams["max_downsample_channels"],
                                    len(dparams["downsample_scales"])], dtype=np.int64)


def main():
    M = import_reference()
    TR = import_trainer()
    out = {}
    collater_cases(TR, out)
    eval_case(M, TR, out)
    path = os.path.join(HERE, "train_session.npz")
    np.savez_compressed(path, **out)
    print("train_session.npz:", len(out), "arrays,", os.path.getsize(path), "bytes",
          {k: float(v) for k, v in out.items() if k.startswith("eval/") and np.ndim(v) == 0})


if __name__ == "__main__":
    main()
