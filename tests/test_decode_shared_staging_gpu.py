"""convert, convert_many and convert_windowed of one DecodeSession download through the SAME two page-locked sets, grown on
demand and reused by batch parity.  What every one of them returns must be the caller's own memory: it keeps its values
through later converts of every kind (which overwrite and may reallocate the sets) and through close()."""
import numpy as np
import pytest
import torch

import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import decode as Dc, synth as S
from test_decode_session_gpu import _invariance_set, _module, _same

pytestmark = pytest.mark.gpu


def test_results_survive_later_converts_of_every_kind_and_close():
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    dev = torch.device("cuda:0")
    cfg = S.FULL_CONFIG
    frames, feats, emb_a = _invariance_set(cfg)
    emb_b = np.random.default_rng(5).standard_normal(cfg.spk_emb_size).astype(np.float32)
    a, b = (emb_a, [5.2, 1.0]), (emb_b, [4.7, 1.0])
    m = _module(cfg, S.synth_state_dict(cfg, 12), dev)
    sg = A.SignalGenerator(sample_rate=24000, hop_size=cfg.hop, sine_amp=0.1, noise_amp=0.0, signal_types=["sine"])
    kept = []
    with Dc.DecodeSession(m, feats, sg, dev, [[5.0, 1.0]] * len(feats), max_batch=4, pad_tolerance=0.9) as s:
        assert len(s.batches) >= 3                           # (both sets are reused within a pass)
        for pcm16 in (True, False):
            kinds = {"convert": lambda spk: s.convert(*spk, pcm16=pcm16),
                     "many": lambda spk: [y for ys in s.convert_many([spk, a], pcm16=pcm16) for y in ys],
                     "windowed": lambda spk: s.convert_windowed(*spk, core=16, pcm16=pcm16)}
            for name, fn in kinds.items():
                out = fn(a)
                assert all(y.dtype == (np.int16 if pcm16 else np.float32) for y in out)
                kept.append((name, pcm16, out, [y.copy() for y in out]))
            first = {name: out for name, _, out, _ in kept[-3:]}
            for name in ("windowed", "many", "convert"):         # another speaker through every path: other bytes in the sets
                assert not _same(kinds[name](b)[: len(feats)], first[name][: len(feats)])
            for name, p, out, snap in kept:
                assert _same(out, snap), (name, p)
    for name, p, out, snap in kept:                              # and after close()
        assert _same(out, snap), (name, p)
