"""The training data path on the GPU (train_session.py, csrc/fastsvc_collate.hip, TrainStep.eval_step, train.main):
crops against numpy slicing bit for bit with canaries around every output, invalid requests, the reference Collater's
recorded batches and `_eval_step` values (tests/golden/train_session.npz, made by make_train_session_golden.py from the
live reference), excitation determinism, buffer reuse, and the driver end to end with a resume."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import synth as S
from svcc23_fastsvc_amd import train_session as TS
from svcc23_fastsvc_amd import training as TR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _corpus(lens, hop, D, S_emb, seed):
    """Utterances of `lens` frames packed back to back (no alignment: odd lengths leave the later blocks unaligned)."""
    rng = np.random.default_rng(seed)
    offs, total = TS.store_layout(lens)
    store = {"wave": rng.standard_normal(total * hop).astype(np.float32), "lft": rng.standard_normal(total * hop).astype(np.float32),
             "ppg": rng.standard_normal(total * D).astype(np.float32), "f0": rng.uniform(60, 500, total).astype(np.float32),
             "emb": rng.standard_normal((len(lens), S_emb)).astype(np.float32)}
    return offs, store


def _expected(store, offs, utt, start, hop, D, frames, ctx):
    """The Collater's slices (train_fastsvc.py:500-543) in plain numpy."""
    T, W = frames * hop, frames + 2 * ctx
    y = np.stack([store["wave"][(offs[u] + s) * hop: (offs[u] + s) * hop + T] for u, s in zip(utt, start)])[:, None]
    lft = np.stack([store["lft"][(offs[u] + s) * hop: (offs[u] + s) * hop + T] for u, s in zip(utt, start)])[:, None]
    f0 = np.stack([store["f0"][offs[u] + s: offs[u] + s + frames] for u, s in zip(utt, start)])[:, None]
    ppg = np.stack([store["ppg"][(offs[u] + s - ctx) * D: (offs[u] + s - ctx + W) * D].reshape(W, D).T for u, s in zip(utt, start)])
    emb = store["emb"][list(utt)]
    return y, lft, ppg, f0, emb


def _guarded(shapes, guard, dev):
    """NaN-filled buffers with `guard` elements in front of and behind each output; -> (buffers, views)."""
    bufs = [torch.full((2 * guard + int(np.prod(s)),), float("nan"), dtype=torch.float32, device=dev) for s in shapes]
    views = [b[guard: b.numel() - guard].view(*s) for b, s in zip(bufs, shapes)]
    return bufs, views


def _rows(lens, frames, ctx, B):
    """First legal start, the last start np.random.randint can draw, and the closed end n - frames - ctx, utterance by
    utterance; row 0 is the closed end of the LAST utterance: its ppg block (its wave block too when ctx = 0) ends at the
    store's last element."""
    rows = [(len(lens) - 1, lens[-1] - frames - ctx)]
    for u, n in enumerate(lens):
        last = n - frames - ctx
        rows += [(u, ctx), (u, last), (u, max(ctx, last - 1)), (u, (ctx + last) // 2)]
    rows = (rows * (B // len(rows) + 1))[:B]
    return [r[0] for r in rows], [r[1] for r in rows]


# hop, D, frames, ctx, B, S: every value of the issue's matrix, odd hop with D % 4 != 0 together, the recipe's shape,
# two channel tiles (68, 144) and two time tiles (70, 100), one row, several rows, more rows than one launch holds
CASES = [(4, 5, 6, 0, 1, 3), (5, 5, 6, 2, 4, 3), (4, 8, 70, 2, 4, 3), (4, 68, 70, 0, 65, 3), (5, 68, 6, 2, 65, 512),
         (160, 144, 100, 0, 4, 512), (5, 144, 100, 2, 4, 512), (4, 8, 6, 0, 65, 512)]


@pytest.mark.parametrize("hop,D,frames,ctx,B,S_emb", CASES)
def test_crops_equal_numpy_slicing_and_leave_the_guards_alone(dev, hop, D, frames, ctx, B, S_emb):
    need = frames + 2 * ctx
    lens = [need + 1, need + 2, need + 9, need + 3, 2 * need + 5]            # odd lengths: unaligned blocks behind them
    offs, store = _corpus(lens, hop, D, S_emb, seed=hop * 1000 + D)
    utt, start = _rows(lens, frames, ctx, B)
    assert (offs[-1] + start[0] + frames + ctx) == offs[-1] + lens[-1]        # row 0 ends at the store's last frame
    want = _expected(store, offs, utt, start, hop, D, frames, ctx)
    d = {k: torch.from_numpy(v).to(dev) for k, v in store.items()}
    T, W = frames * hop, need
    shapes = [(B, 1, T), (B, 1, T), (B, D, W), (B, 1, frames), (B, S_emb)]
    for guard in (64, 37):                                                    # 16-byte aligned outputs, and unaligned ones
        bufs, views = _guarded(shapes, guard, dev)
        got = A.collate_crops(d["wave"], d["lft"], d["ppg"], d["f0"], d["emb"], offs, lens, utt, start, D, hop, frames, ctx, out=views)
        torch.cuda.synchronize()
        for name, g, w, buf in zip(("y", "lft", "ppg", "f0", "emb"), got, want, bufs):
            assert np.array_equal(g.cpu().numpy(), w), (name, guard)          # every element, bit for bit
            assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[-guard:]).all()), (name, guard)
    # without out=, and without speaker embeddings (emb_out is not written)
    got = A.collate_crops(d["wave"], d["lft"], d["ppg"], d["f0"], None, offs, lens, utt, start, D, hop, frames, ctx)
    assert got[4] is None and all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got[:4], want[:4]))


def test_invalid_requests_are_refused_before_anything_is_launched(dev):
    hop, D, frames, ctx, S_emb = 4, 8, 6, 2, 3
    lens = [15, 22]
    offs, store = _corpus(lens, hop, D, S_emb, seed=9)
    d = {k: torch.from_numpy(v).to(dev) for k, v in store.items()}
    shapes = [(2, 1, frames * hop), (2, 1, frames * hop), (2, D, frames + 2 * ctx), (2, 1, frames), (2, S_emb)]
    bufs, views = _guarded(shapes, 16, dev)
    call = lambda offs_, lens_, utt, start: A.collate_crops(d["wave"], d["lft"], d["ppg"], d["f0"], d["emb"], offs_, lens_,     # noqa: E731
                                                            utt, start, D, hop, frames, ctx, out=views)
    bad = [(offs, lens, [0, 2], [2, 2]),                                      # utt out of range
           (offs, lens, [0, -1], [2, 2]),
           (offs, lens, [0, 1], [2, 1]),                                      # start below ctx
           (offs, lens, [0, 1], [15 - 6 - 2 + 1, 2]),                         # start past the closed end
           ([0, 16], lens, [0, 1], [2, 2]),                                   # utterance 1's block leaves the buffers
           (offs, [15, 23], [0, 1], [2, 2])]
    for args in bad:
        with pytest.raises(ValueError, match="fastsvc_collate_crops: "):      # FASTSVC_E_INVALID (-1) with the library's text
            call(*args)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(b).all()) for b in bufs), args            # nothing ran: no output element was written
    call(offs, lens, [0, 1], [15 - 6 - 2, 2])                                 # the closed end itself is legal
    torch.cuda.synchronize()
    assert not bool(torch.isnan(views[0]).any())


def test_launch_count():
    from svcc23_fastsvc_amd.engine import collate_launch_count
    assert [collate_launch_count(b) for b in (1, 4, 64)] == [1, 1, 1] and collate_launch_count(65) == 2


def _golden_utts(g, ctx):
    return [{k: g[f"c{ctx}/utt{i}/{k}"] for k in ("wave", "f0", "ppg", "lft", "spk_emb")} for i in range(4)]


def test_reference_collater_batches_through_the_session(dev):
    """The reference Collater's own batches (start frames recorded from its np.random.randint): ppg, lft, emb and y bit
    for bit; the sine within the device generator's bound against the reference's sine (test_parity_gpu.py:703-712:
    1e-3 on an amplitude-0.1 signal - the reference accumulates the phase in float32)."""
    g = load_golden("train_session.npz")
    hop, D, S_emb, frames, rate = (int(v) for v in g["collater/meta"])
    for ctx in (0, 2):
        s = TS.TrainSession(_golden_utts(g, ctx), dev, batch_size=4, batch_length=frames * hop, hop_size=hop, sample_rate=rate,
                            aux_context_window=ctx, signal_generator_params=dict(sine_amp=0.1, noise_amp=0.0, signal_types=["sine"]))
        assert s.omitted == [] and s.resident_bytes > 0
        for draw in (0, 1):
            (ppg, sine, lft, emb), y = s.batch(range(4), g[f"c{ctx}/draw{draw}/starts"])
            for name, t in (("ppg", ppg), ("lft", lft), ("emb", emb), ("y", y)):
                assert np.array_equal(t.cpu().numpy(), g[f"c{ctx}/draw{draw}/{name}"]), (ctx, draw, name)
            err = float(np.abs(sine.cpu().numpy() - g[f"c{ctx}/draw{draw}/sine"]).max())
            print(f"ctx {ctx} draw {draw}: max |sine - reference| = {err:.3e}")
            assert sine.shape == y.shape and err <= 1e-3, (ctx, draw, err)


def _session(dev, noise_amp, seed=5, n=9, **kw):
    hop, D, S_emb = 4, 8, 3
    rng = np.random.default_rng(77)
    feats = []
    for i in range(n):
        f = 20 + 3 * i
        feats.append({"wave": rng.standard_normal(f * hop).astype(np.float32), "f0": rng.uniform(80, 400, (f, 1)).astype(np.float32),
                      "ppg": rng.standard_normal((f, D)).astype(np.float32), "lft": rng.standard_normal((f * hop, 1)).astype(np.float32),
                      "spk_emb": rng.standard_normal((S_emb, 1)).astype(np.float32)})
    return TS.TrainSession(feats, dev, batch_size=4, batch_length=12 * hop, hop_size=hop, seed=seed,
                           signal_generator_params=dict(sine_amp=0.1, noise_amp=noise_amp, signal_types=["sine"]), **kw)


def _host(batch):
    x, y = batch
    return [t.cpu().numpy().copy() for t in x] + [y.cpu().numpy().copy()]


def test_sine_is_the_existing_generator_and_noise_depends_on_the_batch_number_only(dev):
    s = _session(dev, noise_amp=0.0)
    utts, starts = s.epoch_batches(0)[0]
    (ppg, sine, lft, emb), y = s.batch(utts, starts)
    sg = A.SignalGenerator(sample_rate=16000, hop_size=4, sine_amp=0.1, noise_amp=0.0, signal_types=["sine"])
    assert torch.equal(sine, sg(s.last_f0))                                   # no new excitation arithmetic
    # with noise: batch k is the same whether or not batches 0 .. k-1 were drawn
    a, b = _session(dev, noise_amp=0.003), _session(dev, noise_amp=0.003)
    drawn = [_host(bt) for bt in a.batches(1)]
    k = 2
    only = [_host(bt) for bt in b.batches(1, first=k)]
    assert len(drawn) == 3 and len(only) == 1
    assert all(np.array_equal(p, q) for p, q in zip(drawn[k], only[0]))
    # the same crops under two batch numbers: everything but the noise agrees
    p, q = _host(a.batch(utts, starts, step=7)), _host(a.batch(utts, starts, step=8))
    assert np.array_equal(p[0], q[0]) and np.array_equal(p[4], q[4]) and not np.array_equal(p[1], q[1])
    assert not np.array_equal(drawn[0][1][:1], drawn[1][1][:1])
    assert all(np.array_equal(u, v) for u, v in zip(p, _host(b.batch(utts, starts, step=7))))


def test_a_batch_survives_the_assembly_of_the_next_one(dev):
    s = _session(dev, noise_amp=0.003)
    batches = s.epoch_batches(0)
    b0 = s.batch(*batches[0], step=0)
    keep = _host(b0)
    b1 = s.batch(*batches[1], step=1)
    torch.cuda.synchronize()
    assert all(np.array_equal(u, v) for u, v in zip(keep, _host(b0)))
    assert {t.data_ptr() for t in b0[0] + (b0[1],)}.isdisjoint({t.data_ptr() for t in b1[0] + (b1[1],)})
    assert not np.array_equal(keep[-1], _host(b1)[-1])
    b2 = s.batch(*batches[0], step=2)                                         # the next-but-one reuses batch 0's set
    assert b2[1].data_ptr() == b0[1].data_ptr()


def test_budget_is_enforced_and_omitted_utterances_cannot_be_asked_for(dev):
    with pytest.raises(ValueError, match="budget"):
        _session(dev, 0.0, budget_bytes=1000)
    s = _session(dev, 0.0, budget_bytes=1 << 20)
    assert 0 < s.resident_bytes <= 1 << 20
    rng = np.random.default_rng(3)
    short = {"wave": rng.standard_normal(12 * 4).astype(np.float32), "f0": np.zeros((12, 1), np.float32),
             "ppg": np.zeros((12, 8), np.float32), "lft": np.zeros((48, 1), np.float32), "spk_emb": np.zeros((3, 1), np.float32)}
    long_ = {k: np.concatenate([v, v]) if k != "spk_emb" else v for k, v in short.items()}
    s = TS.TrainSession([short, long_], dev, batch_size=2, batch_length=48, hop_size=4)
    assert s.omitted == [0] and s.epoch_batches(0)[0][0] == [1]
    with pytest.raises(ValueError, match="not in the store"):
        s.batch([0], [0])


def _small_discriminator(dparams):
    scales, channels, maxc, nds = (int(v) for v in dparams)
    p = dict(TR.RECIPE["discriminator_params"])
    p.update(scales=scales, channels=channels, max_downsample_channels=maxc, downsample_scales=[4] * nds)
    return TR.MelGANMultiScaleDiscriminator(**p)


def _opt_tensors(step):
    out = []
    for opt in (step.opt_g, step.opt_d):
        for st in opt.state.values():
            out += [v for v in st.values() if isinstance(v, torch.Tensor)]
    return out


def test_eval_step_matches_the_reference_and_changes_nothing(dev):
    """`Trainer._eval_step` of the reference (train_fastsvc.py:266-311) on hash-generated weights and inputs: the seven
    values within 1e-3 * max(1, |want|), the bound test_training.py:269 holds a step's loss values to."""
    g = load_golden("train_session.npz")
    cfg = S.TINY_CONFIG
    seed_w, seed_x, seed_d, seed_t, B, F = (int(v) for v in g["eval/meta"])
    T = F * cfg.hop
    gen = A.FastSVCGenerator(in_channels=cfg.in_channels, mid_channels=list(cfg.mid_channels),
                             upsampling_scales=list(cfg.upsampling_scales), out_channels=cfg.out_channels,
                             spk_emb_size=cfg.spk_emb_size, use_spk_emb=cfg.use_spk_emb)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in S.synth_state_dict(cfg, seed_w).items()})
    gen = gen.to(dev).train()
    disc = _small_discriminator(g["eval/dparams"])
    S.fill_module_from_hash(disc, seed_d)
    disc = disc.to(dev).train()
    # (far above the step count: the reference's _eval_step computes every term whatever the start step says)
    step = TR.TrainStep(gen, disc, dict(discriminator_train_start_steps=10 ** 6), steps=1)
    b = S.synth_batch(cfg, B, F, seed_x)
    x = tuple(torch.from_numpy(a).to(dev) for a in (b.ppg, b.sine, b.lft, b.spk_emb))
    target = torch.from_numpy((0.3 * S.hash_normalish(seed_t, S.stream_id("train.target"), B * T)).reshape(B, 1, T).astype(np.float32)).to(dev)
    names = ["spectral_convergence_loss", "log_stft_magnitude_loss", "adversarial_loss", "generator_loss", "real_loss",
             "fake_loss", "discriminator_loss"]

    def check(tag):
        params = {k: v.detach().clone() for m in (gen, disc) for k, v in m.state_dict().items()}
        grads = [None if p.grad is None else p.grad.clone() for m in (gen, disc) for p in m.parameters()]
        opt = [t.clone() for t in _opt_tensors(step)]
        steps, lrs = step.steps, (step.sched_g.get_last_lr(), step.sched_d.get_last_lr())
        log = step.eval_step((x, target))
        assert sorted(log) == sorted(names)
        assert step.steps == steps and (step.sched_g.get_last_lr(), step.sched_d.get_last_lr()) == lrs
        assert gen.training and disc.training
        now = {k: v for m in (gen, disc) for k, v in m.state_dict().items()}
        assert all(torch.equal(params[k], now[k]) for k in params), tag
        for before, p in zip(grads, [p for m in (gen, disc) for p in m.parameters()]):
            assert (p.grad is None) if before is None else torch.equal(before, p.grad), tag
        assert len(opt) == len(_opt_tensors(step)) and all(torch.equal(u, v) for u, v in zip(opt, _opt_tensors(step))), tag
        return log

    log = check("fresh")
    assert all(p.grad is None for m in (gen, disc) for p in m.parameters())   # no .grad was created
    for k in names:
        want = float(g["eval/" + k])
        print(f"eval/{k}: {log[k]:.6f} (reference {want:.6f})")
    for k in names:
        want = float(g["eval/" + k])
        assert abs(log[k] - want) <= 1e-3 * max(1.0, abs(want)), (k, log[k], want)
    # with optimizer state and gradients in place (after a real step of both networks), and from eval mode
    step.config["discriminator_train_start_steps"] = 0
    step.step((x, target), log=False)
    assert len(_opt_tensors(step)) > 0
    check("after a step")
    gen.eval()
    step.eval_step((x, target))
    assert not gen.training and disc.training                                  # previous modes, whatever they were
    gen.train()


def _write_dumps(path, lens, seed, hop, D, S_emb):
    os.makedirs(path)
    rng = np.random.default_rng(seed)
    for i, f in enumerate(lens):
        np.savez(os.path.join(path, f"utt{i:02d}.npz"),
                 wave=(0.3 * rng.standard_normal(f * hop)).astype(np.float32), f0=rng.uniform(80, 400, (f, 1)).astype(np.float32),
                 ppg=rng.standard_normal((f, D)).astype(np.float32), lft=rng.uniform(0, 1, (f * hop, 1)).astype(np.float32),
                 spk_emb=rng.standard_normal((S_emb, 1)).astype(np.float32))


def test_driver_end_to_end_and_resume_continues_bit_for_bit(dev, tmp_path):
    """train.main on tiny dumps: 3 steps with an evaluation and a checkpoint, then --resume for 2 more, against an
    uninterrupted 5-step run.  The sampler is stateless, the excitation noise is seeded by the batch number and the
    checkpoint holds both networks, optimizers and schedulers, so the resumed run continues bit for bit.  MIOpen's default
    choice for the last convolution of each MelGAN scale is not reproducible run to run (tests/test_pack_device_gpu.py
    measured that: the step does not reproduce ITSELF), so the convolutions are pinned to its deterministic algorithms for
    all three runs, as that test pins them."""
    import yaml
    from svcc23_fastsvc_amd import checkpoint as C
    from svcc23_fastsvc_amd import train
    cfg = S.TINY_CONFIG
    gparams = dict(in_channels=cfg.in_channels, mid_channels=list(cfg.mid_channels), upsampling_scales=list(cfg.upsampling_scales),
                   out_channels=cfg.out_channels, spk_emb_size=cfg.spk_emb_size, use_spk_emb=True)
    dparams = dict(TR.RECIPE["discriminator_params"])
    dparams.update(scales=2, channels=4, max_downsample_channels=32, downsample_scales=[4, 4])
    conf = dict(generator_params=gparams, discriminator_params=dparams, hop_size=cfg.hop, sampling_rate=16000,
                # (the recipe's six STFT resolutions: the 2048-point frame's reflect padding needs more than 1024 samples,
                # and 25 frames x 160 = 4000 is the crop the tiny generator and this discriminator already train on in
                # tests/test_training.py's two-step test)
                batch_size=2, batch_length=25 * cfg.hop,
                discriminator_train_start_steps=0, log_interval_steps=1, eval_interval_steps=2, save_interval_steps=3, seed=4)
    _write_dumps(str(tmp_path / "train"), [27, 33, 29, 40, 31, 28, 36, 35], 1, cfg.hop, cfg.in_channels, cfg.spk_emb_size)
    _write_dumps(str(tmp_path / "dev"), [30, 28, 34], 2, cfg.hop, cfg.in_channels, cfg.spk_emb_size)

    def run(outdir, max_steps, resume=None):
        path = str(tmp_path / f"conf{max_steps}.yaml")
        with open(path, "w") as f:
            yaml.safe_dump(dict(conf, train_max_steps=max_steps), f)
        torch.manual_seed(123)                                                 # the modules' own initialisation
        argv = ["--train-dumpdir", str(tmp_path / "train"), "--dev-dumpdir", str(tmp_path / "dev"), "--config", path,
                "--outdir", str(tmp_path / outdir)] + (["--resume", resume] if resume else [])
        return train.main(argv)

    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        assert run("a", 3) == 3
        ckpt3 = str(tmp_path / "a" / "checkpoint-3steps.pkl")
        assert os.path.exists(ckpt3) and os.path.exists(str(tmp_path / "a" / "config.yml"))
        gen, disc = A.FastSVCGenerator(**gparams), TR.MelGANMultiScaleDiscriminator(**dparams)
        assert C.load_checkpoint(ckpt3, gen, disc)["steps"] == 3
        assert run("a", 5, resume=ckpt3) == 5
        assert run("b", 5) == 5
    finally:
        torch.backends.cudnn.deterministic = was
    resumed = torch.load(str(tmp_path / "a" / "checkpoint-5steps.pkl"), map_location="cpu")
    straight = torch.load(str(tmp_path / "b" / "checkpoint-5steps.pkl"), map_location="cpu")
    assert resumed["steps"] == straight["steps"] == 5
    start = torch.load(ckpt3, map_location="cpu")
    worst = 0.0
    for net in ("generator", "discriminator"):
        for k, v in straight["model"][net].items():
            worst = max(worst, float((resumed["model"][net][k] - v).abs().max()))
    print(f"resume: max |resumed - uninterrupted| over all parameters = {worst:.3e}")
    moved = max(float((straight["model"]["generator"][k] - v).abs().max()) for k, v in start["model"]["generator"].items())
    assert moved > 0.0                                                         # steps 4 and 5 really trained
    for net in ("generator", "discriminator"):
        for k, v in straight["model"][net].items():
            assert torch.equal(resumed["model"][net][k], v), (net, k)
