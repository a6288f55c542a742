#!/usr/bin/env python
"""Generate golden vectors from the LIVE reference generator (build container only).

    python tests/golden/make_golden.py          # rewrites tests/golden/*.npz

The reference (`/root/reference`, `harana.models.FastSVCGenerator`, fastsvc.py:235-383) holds no
known-answer tests for this path, so parity is pinned by vectors produced here by
importing and running the reference itself.  Only DATA is stored: inputs, expected outputs and
intermediate taps.  Weights and large inputs are regenerated on every machine from the integer-hash
generator in ``svcc23_fastsvc_amd/synth.py`` (bit-identical everywhere), so the fixtures stay small.

Fixtures written:
  tiny_forward.npz      tiny-width generator (8 -> [16,8,8,4]), B=2, F=24: state dict, inputs, output
                        with / without speaker embedding, per-stage taps (down nets, FiLM, up blocks)
  full_forward_f7.npz   yaml-width generator, B=2, F=7  (shorter than the d=27 receptive field)
  full_forward_f300.npz yaml-width generator, B=1, F=300 (BASELINE cfg1): full output
  full_forward_cfg2.npz yaml-width generator, B=8, F=600 (BASELINE cfg2): 16 slices + checksums
  inference_f40.npz     ``inference()`` call sequence with the reference SignalGenerator, noise_amp=0
  weight_norm_fold.npz  torch ``remove_weight_norm`` result for three layers (g, v -> w)
  tiny_grads.npz        autograd of the reference generator in train() mode (tiny width): d sum(r*y) / d every
                        parameter (weight_g / weight_v / bias) and input, with / without speaker embedding
  train_recipe.npz      one Trainer._train_step at the recipe's own size (yaml-width generator + the yaml's discriminator,
                        batch 32 x 16000): loss values, per-parameter step norms and 4-element slices (`train_recipe`, ~2 min
                        of CPU; not in the default list)
  train_step.npz        MR-STFT / adversarial loss values, a small MelGAN multi-scale discriminator's outputs, eight
                        RAdam steps, and two full Trainer._train_step calls (train_fastsvc.py:157-240): every
                        generator / discriminator parameter after each step
  stft_loss.npz         the reference MultiResolutionSTFTLoss (stft_loss.py:131-180) on three small cases - the recipe's six
                        resolutions, the class defaults (window shorter than the frame, hop not dividing it) and a batch
                        with a silent and a very quiet prediction (bins at the 1e-7 floor): sc, mag and autograd's
                        d sc / dx, d mag / dx
  hifigan_disc.npz      the HiFiGAN multi-scale + multi-period discriminator (fastsvc.py:631-1143; BASELINE config 5): key CRCs and
                        shapes of the default-width module tree, outputs / feature-map means / adversarial losses of a
                        reduced-width instance on hash inputs, one Trainer._train_step against it
  decode_chain.npz      decode_fastsvc.py:160-189 per utterance for three utterances of different
                        length: F0Statistics.estimate / .convert (features.py:41-108, std forced to 1),
                        then ``inference()`` with the converted F0 (noise_amp=0)
  live_tiny.npz         tiny-width generator, B=3, F=31: the output the oracle's ``forward_as_executed`` must reproduce
  live_configs.npz      every generator of tests/config_matrix.py, B=2, F=9: the reference's output with a speaker
                        embedding (`<name>/y`) and, where the generator has one, without (`<name>/y_nospk`)
  ref_checkpoint.npz    a reference generator's own initialisation (reduced width) as its checkpoint stores it, and its
                        state dict after ``remove_weight_norm`` (the checkpoint-loading test of test_boundary.py)

    python tests/golden/make_golden.py decode_chain     # only that fixture
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.refimport import import_reference, import_reference_signal_generator  # noqa: E402
from oracle.refimport import REFERENCE_ROOT as ROOT_REF  # noqa: E402
from svcc23_fastsvc_amd import synth as S  # noqa: E402

warnings.filterwarnings("ignore")
torch.set_num_threads(8)


def build_reference(M, cfg: S.GeneratorConfig, seed: int):
    g = M.FastSVCGenerator(
        in_channels=cfg.in_channels, mid_channels=list(cfg.mid_channels),
        upsampling_scales=list(cfg.upsampling_scales), out_channels=cfg.out_channels,
        spk_emb_size=cfg.spk_emb_size, use_spk_emb=cfg.use_spk_emb)
    sd = S.synth_state_dict(cfg, seed)
    assert list(g.state_dict().keys()) == S.state_dict_keys(cfg)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return g.eval(), sd


def run(g, b: S.SynthBatch, with_spk=True):
    with torch.no_grad():
        return g(torch.from_numpy(b.ppg), torch.from_numpy(b.sine), torch.from_numpy(b.lft),
                 torch.from_numpy(b.spk_emb) if with_spk else None).numpy()


def tiny(M):
    cfg, seed_w, seed_x, B, F = S.TINY_CONFIG, 101, 102, 2, 24
    g, sd = build_reference(M, cfg, seed_w)
    b = S.synth_batch(cfg, B, F, seed_x)
    taps = {}

    def hook(name):
        def fn(mod, inp, out):
            if isinstance(out, tuple):
                taps[name + ".scale"] = out[0].detach().numpy().copy()
                taps[name + ".shift"] = out[1].detach().numpy().copy()
            else:
                taps[name] = out.detach().numpy().copy()
        return fn

    hs = []
    for k in range(cfg.n_stages):
        hs.append(g.downsampling_lft[k].register_forward_hook(hook(f"down_lft.{k}")))
        hs.append(g.downsampling_sine[k].register_forward_hook(hook(f"down_sine.{k}")))
        hs.append(g.film_lft[k].register_forward_hook(hook(f"film_lft.{k}")))
        hs.append(g.film_sine[k].register_forward_hook(hook(f"film_sine.{k}")))
        hs.append(g.upsampling_nets[k].register_forward_hook(hook(f"up.{k}.out")))
    y = run(g, b, True)
    for h in hs:
        h.remove()
    y_nospk = run(g, b, False)
    out = {"y": y, "y_nospk": y_nospk, "ppg": b.ppg, "sine": b.sine, "lft": b.lft,
           "spk_emb": b.spk_emb, "meta": np.array([seed_w, seed_x, B, F])}
    out.update({"tap/" + k: v for k, v in taps.items()})
    out.update({"sd/" + k: v for k, v in sd.items()})
    np.savez_compressed(os.path.join(HERE, "tiny_forward.npz"), **out)
    print("tiny", y.shape, float(np.abs(y).max()), len(taps), "taps")


def full(M):
    cfg, seed_w = S.FULL_CONFIG, 201
    g, _ = build_reference(M, cfg, seed_w)
    # F = 7: every stage shorter than the dilation-27 receptive field
    b = S.synth_batch(cfg, 2, 7, 202)
    np.savez_compressed(os.path.join(HERE, "full_forward_f7.npz"), y=run(g, b, True),
                        y_nospk=run(g, b, False), meta=np.array([seed_w, 202, 2, 7]))
    # cfg1
    w = S.WORKLOADS["cfg1"]
    b = S.synth_batch(cfg, w["B"], w["F"], w["seed"])
    y = run(g, b, True)
    np.savez_compressed(os.path.join(HERE, "full_forward_f300.npz"), y=y.astype(np.float32),
                        meta=np.array([seed_w, w["seed"], w["B"], w["F"]]))
    print("cfg1", y.shape, float(y.std()), float(np.abs(y).max()))
    # cfg2: slices + checksums
    w = S.WORKLOADS["cfg2"]
    b = S.synth_batch(cfg, w["B"], w["F"], w["seed"])
    y = run(g, b, True)
    T = y.shape[-1]
    starts = np.array([0, 17, 4093, 11111, 23999, 31337, 40000, 47999, 48000, 60001,
                       70707, 80000, 88888, 95000, 95700, T - 256])
    slices = np.stack([y[i % w["B"], 0, st:st + 256] for i, st in enumerate(starts)])
    np.savez_compressed(os.path.join(HERE, "full_forward_cfg2.npz"), starts=starts, slices=slices,
                        sum=y.astype(np.float64).sum(axis=-1), sumsq=(y.astype(np.float64) ** 2).sum(axis=-1),
                        absmax=np.abs(y).max(axis=-1), meta=np.array([seed_w, w["seed"], w["B"], w["F"]]))
    print("cfg2", y.shape, float(y.std()), float(np.abs(y).max()))


def inference(M):
    """decode_fastsvc.py:187-189 call sequence: time-major inputs, reference SignalGenerator
    with noise_amp=0 (deterministic), pad_fn = ReplicationPad1d(0)."""
    SignalGenerator = import_reference_signal_generator()
    cfg, seed_w, F = S.FULL_CONFIG, 201, 40
    g, _ = build_reference(M, cfg, seed_w)
    g.remove_weight_norm()                       # decode_fastsvc.py:142
    b = S.synth_batch(cfg, 1, F, 301)
    sg = SignalGenerator(sample_rate=24000, hop_size=cfg.hop, sine_amp=0.1, noise_amp=0.0,
                         signal_types=["sine"])
    pad_fn = torch.nn.ReplicationPad1d(0)
    ppg_tm = torch.from_numpy(b.ppg[0].T.copy())          # (F, 144)
    f0_tm = torch.from_numpy(b.f0[0].T.copy())            # (F, 1)
    lft_tm = torch.from_numpy(b.lft[0].T.copy())          # (T, 1)
    emb = torch.from_numpy(b.spk_emb)                     # (1, 512)
    with torch.no_grad():
        y = g.inference(ppg_tm, f0_tm, lft_tm, sg, pad_fn, emb).numpy()
        sine = sg(f0_tm.transpose(1, 0).unsqueeze(0)).numpy()
    np.savez_compressed(os.path.join(HERE, "inference_f40.npz"), y=y, sine=sine, f0=b.f0,
                        meta=np.array([seed_w, 301, 1, F]))
    print("inference", y.shape, sine.shape)


def decode_chain(M):
    """The caller on the other side of the boundary, decode_fastsvc.py:160-189."""
    from harana.utils.features import F0Statistics
    SignalGenerator = import_reference_signal_generator()
    cfg, seed_w = S.FULL_CONFIG, 201
    g, _ = build_reference(M, cfg, seed_w)
    g.remove_weight_norm()
    sg = SignalGenerator(sample_rate=24000, hop_size=cfg.hop, sine_amp=0.1, noise_amp=0.0, signal_types=["sine"])
    pad_fn = torch.nn.ReplicationPad1d(0)
    fs = F0Statistics()
    frames = [37, 64, 50]
    batches = [S.synth_batch(cfg, 1, F, 400 + i) for i, F in enumerate(frames)]
    f0s = [b.f0[0, 0].astype(np.float64) for b in batches]               # (F,) Hz, 0 = unvoiced
    src_stats = fs.estimate(f0s)                                          # [mean, std] of log f0
    srcstats = np.array([src_stats[0], 1])                                # decode_fastsvc.py:165,176
    trgstats = np.array([np.log(330.0), 1])
    emb = torch.from_numpy(batches[0].spk_emb)                            # one target speaker
    out = {"frames": np.array(frames), "src_stats": src_stats, "srcstats": srcstats, "trgstats": trgstats,
           "meta": np.array([seed_w, 400])}
    for i, b in enumerate(batches):
        cv = fs.convert(f0s[i], srcstats, trgstats)                        # (F,)
        f0_tm = torch.FloatTensor(np.expand_dims(cv, 1))
        with torch.no_grad():
            y = g.inference(torch.from_numpy(b.ppg[0].T.copy()), f0_tm, torch.from_numpy(b.lft[0].T.copy()),
                            sg, pad_fn, emb).view(-1).numpy()
        out[f"cvf0.{i}"] = cv
        out[f"y.{i}"] = y
    np.savez_compressed(os.path.join(HERE, "decode_chain.npz"), **out)
    print("decode_chain", [out[f"y.{i}"].shape for i in range(3)], src_stats)


def grads(M):
    """Gradients of the LIVE reference generator under autograd (train_fastsvc.py:157-240 calls it that way):
    L = sum(r * y) for a fixed r, tiny-width generator in train() mode with weight-norm parametrisation;
    d L / d every parameter and every input, with and without the speaker embedding."""
    cfg, seed_w, seed_x, B, F = S.TINY_CONFIG, 111, 112, 2, 12
    out = {}
    b = S.synth_batch(cfg, B, F, seed_x)
    r = S.hash_normalish(77, S.stream_id("grad.r"), B * F * cfg.hop).reshape(B, 1, F * cfg.hop).astype(np.float32)
    out["meta"] = np.array([seed_w, seed_x, B, F])
    out["r"] = r
    for tag, with_spk in (("spk", True), ("nospk", False)):
        g, sd = build_reference(M, cfg, seed_w)
        g.train()
        ins = [torch.from_numpy(a).clone().requires_grad_(True) for a in (b.ppg, b.sine, b.lft, b.spk_emb)]
        y = g(ins[0], ins[1], ins[2], ins[3] if with_spk else None)
        (y * torch.from_numpy(r)).sum().backward()
        out[f"{tag}/y"] = y.detach().numpy()
        for name, t in zip(("ppg", "sine", "lft", "spk_emb"), ins):
            if t.grad is not None:
                out[f"{tag}/in/{name}"] = t.grad.numpy()
        for name, p in g.named_parameters():
            if p.grad is not None:
                out[f"{tag}/p/{name}"] = p.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "tiny_grads.npz"), **out)
    print("tiny_grads.npz:", len(out), "arrays")


def train(M):
    """train_step.npz: the reference's losses, discriminator, RAdam and two full `_train_step`s (train_fastsvc.py:157-240)
    on the tiny-width generator and a small MelGAN multi-scale discriminator, both sub-networks training from the
    first step (discriminator_train_start_steps = 0, steps start at 1)."""
    import types
    from harana.losses import MultiResolutionSTFTLoss, GeneratorAdversarialLoss, DiscriminatorAdversarialLoss
    from harana.optimizers import RAdam
    import yaml
    with open(os.path.join(ROOT_REF, "egs/svcc23/fastsvc1/conf/fastsvc.yaml")) as f:
        recipe = yaml.safe_load(f)
    out = {}
    cfg = S.TINY_CONFIG
    B, F = 2, 25
    T = F * cfg.hop
    # (1) losses on fixed signals
    gsig = torch.Generator().manual_seed(11)
    y = torch.randn((B, 1, T), generator=gsig) * 0.3
    y_hat = y + torch.randn((B, 1, T), generator=gsig) * 0.1
    stft = MultiResolutionSTFTLoss(**recipe["stft_loss_params"])
    sc, mag = stft(y_hat, y)
    out.update({"loss/y": y.numpy(), "loss/y_hat": y_hat.numpy(), "loss/sc": np.float64(sc), "loss/mag": np.float64(mag)})
    # (2) small discriminator: state dict, final outputs, adversarial losses
    dparams = dict(recipe["discriminator_params"])
    dparams.update(scales=2, channels=4, max_downsample_channels=32, downsample_scales=[4, 4])
    torch.manual_seed(12)
    D = M.MelGANMultiScaleDiscriminator(**dparams)
    for k, v in D.state_dict().items():
        out["dsd/" + k] = v.numpy().copy()
    outs, outs_hat = D(y), D(y_hat)
    for i, (o, oh) in enumerate(zip(outs, outs_hat)):
        out[f"d/real.{i}"] = o[-1].detach().numpy()
        out[f"d/fake.{i}"] = oh[-1].detach().numpy()
        out[f"d/nlayers.{i}"] = np.int64(len(o))
    out["loss/gen_adv"] = np.float64(GeneratorAdversarialLoss()(outs_hat))
    real, fake = DiscriminatorAdversarialLoss()(outs_hat, outs)
    out["loss/dis_real"], out["loss/dis_fake"] = np.float64(real), np.float64(fake)
    # (3) RAdam: 8 steps on two tensors with given gradients (rectification switches on at step 6)
    gr = torch.Generator().manual_seed(13)
    ps = [torch.nn.Parameter(torch.randn((5, 3), generator=gr)), torch.nn.Parameter(torch.randn((7,), generator=gr))]
    opt = RAdam(ps, lr=1e-2, eps=1e-6, weight_decay=1e-3)
    out["radam/p0.0"], out["radam/p1.0"] = ps[0].detach().numpy().copy(), ps[1].detach().numpy().copy()
    for t in range(1, 9):
        for i, p_ in enumerate(ps):
            p_.grad = torch.randn(p_.shape, generator=gr)
            out[f"radam/g{i}.{t}"] = p_.grad.numpy().copy()
        opt.step()
        for i, p_ in enumerate(ps):
            out[f"radam/p{i}.{t}"] = p_.detach().numpy().copy()
    # (4) two full train steps through the reference Trainer's _train_step
    # (the trainer module imports two off-path packages that are not installed here: placeholders, test tooling only)
    from oracle.refimport import _placeholder
    for name in ("tensorboardX", "soundfile"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                _placeholder(name)
    if not hasattr(sys.modules["tensorboardX"], "SummaryWriter"):
        sys.modules["tensorboardX"].SummaryWriter = lambda *a, **k: None
    from harana.bin import train_fastsvc as TR
    g, sd = build_reference(M, cfg, 21)
    g.train()
    torch.manual_seed(14)
    D2 = M.MelGANMultiScaleDiscriminator(**dparams)
    for k, v in D2.state_dict().items():
        out["step/dsd0/" + k] = v.numpy().copy()
    conf = dict(recipe)
    conf.update(discriminator_train_start_steps=0, use_stft_loss=True, lambda_aux=1.0, outdir="/tmp",
                train_max_steps=10 ** 9, log_interval_steps=10 ** 9, eval_interval_steps=10 ** 9, save_interval_steps=10 ** 9)
    crit = {"gen_adv": GeneratorAdversarialLoss(), "dis_adv": DiscriminatorAdversarialLoss(),
            "stft": MultiResolutionSTFTLoss(**recipe["stft_loss_params"])}
    opt = {"generator": RAdam(g.parameters(), **recipe["generator_optimizer_params"]),
           "discriminator": RAdam(D2.parameters(), **recipe["discriminator_optimizer_params"])}
    sch = {k: torch.optim.lr_scheduler.StepLR(opt[k], **recipe[k + "_scheduler_params"]) for k in opt}
    tr = TR.Trainer(steps=1, epochs=0, data_loader={}, sampler={"train": None}, model={"generator": g, "discriminator": D2},
                    criterion=crit, optimizer=opt, scheduler=sch, config=conf, device=torch.device("cpu"))
    tr.tqdm = types.SimpleNamespace(update=lambda n: None)
    tr._check_train_finish = lambda: None
    b = S.synth_batch(cfg, B, F, 22)
    gy = torch.Generator().manual_seed(15)
    target = torch.randn((B, 1, T), generator=gy) * 0.3
    out["step/target"] = target.numpy()
    x = tuple(torch.from_numpy(a) for a in (b.ppg, b.sine, b.lft, b.spk_emb))
    for it in (1, 2):
        tr.total_train_loss.clear()
        tr._train_step((x, target))
        for k, v in tr.total_train_loss.items():
            out[f"step/loss{it}/{k.split('/')[-1]}"] = np.float64(v)
        for k, v in g.state_dict().items():
            out[f"step/g{it}/{k}"] = v.numpy().copy()
        for k, v in D2.state_dict().items():
            out[f"step/d{it}/{k}"] = v.numpy().copy()
    out["meta"] = np.array([21, 22, B, F], dtype=np.int64)
    out["dparams"] = np.array([dparams["scales"], dparams["channels"], dparams["max_downsample_channels"],
                               len(dparams["downsample_scales"])], dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "train_step.npz"), **out)
    print("train_step.npz:", len(out), "arrays")


def train_recipe(M):
    """train_recipe.npz: ONE full `Trainer._train_step` of the reference (train_fastsvc.py:157-240) at the RECIPE's size -
    yaml-width generator, the yaml's MelGAN multi-scale discriminator (4.35 M parameters), batch 32 x 16000 samples
    (fastsvc.yaml:71-72), both sub-networks training - BASELINE config 5 at its own size.  Weights, inputs and target are
    regenerated on both sides from the integer-hash generator; the fixture holds the loss values, and per generator /
    discriminator parameter the norm of the step it took plus a 4-element slice of the stepped tensor."""
    import types
    from harana.losses import MultiResolutionSTFTLoss, GeneratorAdversarialLoss, DiscriminatorAdversarialLoss
    from harana.optimizers import RAdam
    import yaml
    with open(os.path.join(ROOT_REF, "egs/svcc23/fastsvc1/conf/fastsvc.yaml")) as f:
        recipe = yaml.safe_load(f)
    from oracle.refimport import _placeholder
    for name in ("tensorboardX", "soundfile"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                _placeholder(name)
    if not hasattr(sys.modules["tensorboardX"], "SummaryWriter"):
        sys.modules["tensorboardX"].SummaryWriter = lambda *a, **k: None
    from harana.bin import train_fastsvc as TR
    cfg = S.FULL_CONFIG
    B, F = int(recipe["batch_size"]), int(recipe["batch_length"]) // cfg.hop
    T = F * cfg.hop
    seed_w, seed_x, seed_d, seed_t = 301, 302, 303, 304
    g, sd = build_reference(M, cfg, seed_w)
    g.train()
    D = M.MelGANMultiScaleDiscriminator(**recipe["discriminator_params"])
    S.fill_module_from_hash(D, seed_d)
    D.train()
    conf = dict(recipe)
    conf.update(discriminator_train_start_steps=0, use_stft_loss=True, lambda_aux=1.0, outdir="/tmp",
                train_max_steps=10 ** 9, log_interval_steps=10 ** 9, eval_interval_steps=10 ** 9, save_interval_steps=10 ** 9)
    crit = {"gen_adv": GeneratorAdversarialLoss(), "dis_adv": DiscriminatorAdversarialLoss(),
            "stft": MultiResolutionSTFTLoss(**recipe["stft_loss_params"])}
    opt = {"generator": RAdam(g.parameters(), **recipe["generator_optimizer_params"]),
           "discriminator": RAdam(D.parameters(), **recipe["discriminator_optimizer_params"])}
    sch = {k: torch.optim.lr_scheduler.StepLR(opt[k], **recipe[k + "_scheduler_params"]) for k in opt}
    tr = TR.Trainer(steps=1, epochs=0, data_loader={}, sampler={"train": None}, model={"generator": g, "discriminator": D},
                    criterion=crit, optimizer=opt, scheduler=sch, config=conf, device=torch.device("cpu"))
    tr.tqdm = types.SimpleNamespace(update=lambda n: None)
    tr._check_train_finish = lambda: None
    b = S.synth_batch(cfg, B, F, seed_x)
    target = torch.from_numpy((0.3 * S.hash_normalish(seed_t, S.stream_id("train.target"), B * T)).reshape(B, 1, T).astype(np.float32))
    x = tuple(torch.from_numpy(a) for a in (b.ppg, b.sine, b.lft, b.spk_emb))
    before = {"g": {k: v.detach().clone() for k, v in g.state_dict().items()},
              "d": {k: v.detach().clone() for k, v in D.state_dict().items()}}
    out = {"meta": np.array([seed_w, seed_x, seed_d, seed_t, B, F], dtype=np.int64)}
    tr.total_train_loss.clear()
    tr._train_step((x, target))
    for k, v in tr.total_train_loss.items():
        out[f"loss/{k.split('/')[-1]}"] = np.float64(v)
    for tag, module in (("g", g), ("d", D)):
        for k, v in module.state_dict().items():
            out[f"{tag}/step_norm/{k}"] = np.float64((v.detach() - before[tag][k]).double().norm())
            out[f"{tag}/head/{k}"] = v.detach().flatten()[:4].numpy().copy()
    np.savez_compressed(os.path.join(HERE, "train_recipe.npz"), **out)
    print("train_recipe.npz:", len(out), "arrays", {k: float(v) for k, v in out.items() if k.startswith("loss/")})


def hifigan(M):
    """hifigan_disc.npz: the HiFiGAN multi-scale + multi-period discriminator BASELINE config 5 names (fastsvc.py:631-1143).
    (1) default-width module tree: CRC32 of every state-dict key, every shape (70.7 M parameters - incl. the reference's
    quirk that its scale discriminators carry NO weight / spectral norm); (2) reduced widths (synth.HIFIGAN_FIXTURE_PARAMS),
    parameters from the integer-hash generator: the eight outputs and every hidden feature map's mean |.| on a hash input,
    the adversarial losses, d gen_adv / d input; (3) one `Trainer._train_step` (train_fastsvc.py:157-240) of the tiny-width
    generator against this discriminator, both sub-networks training: losses, per-parameter step norms and 4-element slices."""
    import copy
    import types
    from harana.losses import MultiResolutionSTFTLoss, GeneratorAdversarialLoss, DiscriminatorAdversarialLoss
    from harana.optimizers import RAdam
    import yaml
    with open(os.path.join(ROOT_REF, "egs/svcc23/fastsvc1/conf/fastsvc.yaml")) as f:
        recipe = yaml.safe_load(f)
    out = {}
    Dfull = M.HiFiGANMultiScaleMultiPeriodDiscriminator()
    sdf = Dfull.state_dict()
    out["full/key_crc"] = S.key_hashes(sdf.keys())
    out["full/shapes"] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sdf.values()], dtype=np.int64)
    out["full/numel"] = np.int64(sum(p.numel() for p in Dfull.parameters()))
    del Dfull, sdf
    seed_d, seed_x = 501, 502
    D = M.HiFiGANMultiScaleMultiPeriodDiscriminator(**copy.deepcopy(S.HIFIGAN_FIXTURE_PARAMS))
    S.fill_module_from_hash(D, seed_d)
    D.train()
    out["small/key_crc"] = S.key_hashes(D.state_dict().keys())
    B, _, T = S.HIFIGAN_FIXTURE_INPUT
    x = torch.from_numpy((0.3 * S.hash_normalish(seed_x, S.stream_id("hifigan.x"), B * T)).reshape(B, 1, T).astype(np.float32))
    x_hat = torch.from_numpy((0.3 * S.hash_normalish(seed_x, S.stream_id("hifigan.x_hat"), B * T)).reshape(B, 1, T).astype(np.float32))
    x_hat.requires_grad_(True)
    outs, fmaps = D(x, return_fmaps=True)
    outs_hat = D(x_hat)
    for i, o in enumerate(outs):
        out[f"small/real.{i}"] = o.detach().numpy()
        out[f"small/fake.{i}"] = outs_hat[i].detach().numpy()
    out["small/fmap_mean_abs"] = np.array([float(f.detach().abs().mean()) for f in fmaps], dtype=np.float64)
    out["small/fmap_numel"] = np.array([f.numel() for f in fmaps], dtype=np.int64)
    adv = GeneratorAdversarialLoss()(outs_hat)
    adv.backward()
    out["small/gen_adv"] = np.float64(adv)
    out["small/d_gen_adv_d_x"] = x_hat.grad.numpy().copy()
    real, fake = DiscriminatorAdversarialLoss()(outs_hat, outs)
    out["small/dis_real"], out["small/dis_fake"] = np.float64(real), np.float64(fake)
    # (3) one full train step, tiny generator + this discriminator
    from oracle.refimport import _placeholder
    for name in ("tensorboardX", "soundfile"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                _placeholder(name)
    if not hasattr(sys.modules["tensorboardX"], "SummaryWriter"):
        sys.modules["tensorboardX"].SummaryWriter = lambda *a, **k: None
    from harana.bin import train_fastsvc as TR
    cfg = S.TINY_CONFIG
    seed_w, seed_b, seed_t, seed_d2 = 511, 512, 513, 514
    Bt, F = 2, 25
    Tt = F * cfg.hop
    g, _ = build_reference(M, cfg, seed_w)
    g.train()
    D2 = M.HiFiGANMultiScaleMultiPeriodDiscriminator(**copy.deepcopy(S.HIFIGAN_FIXTURE_PARAMS))
    S.fill_module_from_hash(D2, seed_d2)
    D2.train()
    conf = dict(recipe)
    conf.update(discriminator_train_start_steps=0, use_stft_loss=True, lambda_aux=1.0, outdir="/tmp",
                train_max_steps=10 ** 9, log_interval_steps=10 ** 9, eval_interval_steps=10 ** 9, save_interval_steps=10 ** 9)
    crit = {"gen_adv": GeneratorAdversarialLoss(), "dis_adv": DiscriminatorAdversarialLoss(),
            "stft": MultiResolutionSTFTLoss(**recipe["stft_loss_params"])}
    opt = {"generator": RAdam(g.parameters(), **recipe["generator_optimizer_params"]),
           "discriminator": RAdam(D2.parameters(), **recipe["discriminator_optimizer_params"])}
    sch = {k: torch.optim.lr_scheduler.StepLR(opt[k], **recipe[k + "_scheduler_params"]) for k in opt}
    tr = TR.Trainer(steps=1, epochs=0, data_loader={}, sampler={"train": None}, model={"generator": g, "discriminator": D2},
                    criterion=crit, optimizer=opt, scheduler=sch, config=conf, device=torch.device("cpu"))
    tr.tqdm = types.SimpleNamespace(update=lambda n: None)
    tr._check_train_finish = lambda: None
    b = S.synth_batch(cfg, Bt, F, seed_b)
    target = torch.from_numpy((0.3 * S.hash_normalish(seed_t, S.stream_id("train.target"), Bt * Tt)).reshape(Bt, 1, Tt).astype(np.float32))
    xs = tuple(torch.from_numpy(a) for a in (b.ppg, b.sine, b.lft, b.spk_emb))
    before = {"g": {k: v.detach().clone() for k, v in g.state_dict().items()},
              "d": {k: v.detach().clone() for k, v in D2.state_dict().items()}}
    tr.total_train_loss.clear()
    tr._train_step((xs, target))
    for k, v in tr.total_train_loss.items():
        out[f"step/loss/{k.split('/')[-1]}"] = np.float64(v)
    for tag, module in (("g", g), ("d", D2)):
        for k, v in module.state_dict().items():
            out[f"step/{tag}/step_norm/{k}"] = np.float64((v.detach() - before[tag][k]).double().norm())
            out[f"step/{tag}/head/{k}"] = v.detach().flatten()[:4].numpy().copy()
    out["meta"] = np.array([seed_d, seed_x, seed_w, seed_b, seed_t, seed_d2, Bt, F], dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "hifigan_disc.npz"), **out)
    print("hifigan_disc.npz:", len(out), "arrays", {k: float(v) for k, v in out.items() if k.startswith("step/loss/")})


def fold(M):
    cfg = S.TINY_CONFIG
    g, sd = build_reference(M, cfg, 101)
    g.remove_weight_norm()
    sd2 = g.state_dict()
    names = ["upsampling_nets.0.conv_first", "downsampling_sine.1.downsample_block.4", "conv_last"]
    out = {}
    for n in names:
        out[n + ".weight"] = sd2[n + ".weight"].numpy()
        out[n + ".weight_g"] = sd[n + ".weight_g"]
        out[n + ".weight_v"] = sd[n + ".weight_v"]
    np.savez_compressed(os.path.join(HERE, "weight_norm_fold.npz"), **out)


def live_tiny(M):
    """live_tiny.npz: the reference generator's output (eval, weight norm on) for the tiny width, B=3, F=31."""
    cfg = S.TINY_CONFIG
    g, _ = build_reference(M, cfg, 555)
    b = S.synth_batch(cfg, 3, 31, 556)
    np.savez_compressed(os.path.join(HERE, "live_tiny.npz"), y=run(g, b, True),
                        meta=np.array([555, 556, 3, 31], np.int64))


def live_configs(M):
    """live_configs.npz: the reference generator's output (eval, weight norm on) for every configuration of
    tests/config_matrix.py, B=2, F=9, with and (where use_spk_emb) without a speaker embedding."""
    sys.path.insert(0, os.path.dirname(HERE))
    import config_matrix as CM
    out = {"meta": np.array([CM.SEED_W, CM.SEED_X, CM.B, CM.F], np.int64)}
    for name in CM.NAMES:
        cfg = CM.config(name)
        g, _ = build_reference(M, cfg, CM.SEED_W)
        b = S.synth_batch(cfg, CM.B, CM.F, CM.SEED_X)
        for spk in CM.speaker_modes(name):
            out[f"{name}/y" if spk else f"{name}/y_nospk"] = run(g, b, spk)
    np.savez_compressed(os.path.join(HERE, "live_configs.npz"), **out)


def ref_checkpoint(M):
    """ref_checkpoint.npz: a reference generator's own initialisation (torch.manual_seed(3), reduced width) as the
    checkpoint's ["model"]["generator"] stores it (`ckpt/<key>`), and its state dict after ``remove_weight_norm``
    (`folded/<key>`)."""
    params = dict(in_channels=8, mid_channels=[16, 8, 8, 4], upsampling_scales=[2, 4, 4, 5], out_channels=1,
                  spk_emb_size=16, use_spk_emb=True)
    torch.manual_seed(3)
    g = M.FastSVCGenerator(**params)
    out = {f"ckpt/{k}": v.numpy().copy() for k, v in g.state_dict().items()}
    g.remove_weight_norm()
    out.update({f"folded/{k}": v.numpy().copy() for k, v in g.state_dict().items()})
    np.savez_compressed(os.path.join(HERE, "ref_checkpoint.npz"), **out)


def stft_loss(M):
    """stft_loss.npz: inputs are regenerated from seeds (numpy default_rng) by the tests; expected values stored."""
    from harana.losses import MultiResolutionSTFTLoss
    import yaml
    with open(os.path.join(ROOT_REF, "egs/svcc23/fastsvc1/conf/fastsvc.yaml")) as f:
        recipe = yaml.safe_load(f)
    out = {}
    for tag, x, y, params in S.stft_loss_cases(recipe["stft_loss_params"]):
        crit = MultiResolutionSTFTLoss(**params)
        for which in (0, 1):
            xt = torch.from_numpy(x).clone().requires_grad_(True)
            losses = crit(xt, torch.from_numpy(y))
            losses[which].backward()
            out[f"{tag}/grad_{('sc', 'mag')[which]}"] = xt.grad.numpy().copy()
        out[f"{tag}/sc"], out[f"{tag}/mag"] = np.float64(losses[0]), np.float64(losses[1])
        for k, v in params.items():
            if k != "window":
                out[f"{tag}/{k}"] = np.asarray(v, np.int64)
    np.savez_compressed(os.path.join(HERE, "stft_loss.npz"), **out)
    print("stft_loss.npz:", len(out), "arrays")


if __name__ == "__main__":
    M = import_reference()
    todo = sys.argv[1:] or ["tiny", "full", "inference", "fold", "decode_chain", "grads", "train", "stft_loss", "hifigan",
                            "live_tiny", "live_configs", "ref_checkpoint"]
    for name in todo:
        {"tiny": tiny, "full": full, "inference": inference, "fold": fold, "decode_chain": decode_chain, "grads": grads,
         "train": train, "train_recipe": train_recipe, "stft_loss": stft_loss, "hifigan": hifigan,
         "live_tiny": live_tiny, "live_configs": live_configs, "ref_checkpoint": ref_checkpoint}[name](M)
    for f in sorted(os.listdir(HERE)):
        if f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(HERE, f)))
