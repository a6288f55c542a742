"""Host side of the training data path (train_session.py; no GPU): the store layout, the construction checks, the
stateless crop sampler's properties, the refusal of CPU tensors, and the two new ABI symbols."""
import ctypes

import numpy as np
import pytest
import torch

import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import train_session as TS

HOP, D, S_EMB = 4, 5, 3


@pytest.fixture(scope="module", autouse=True)
def _built():
    from svcc23_fastsvc_amd.build import build
    build()


def _utt(n, seed=0, hop=HOP, d=D, s=S_EMB):
    rng = np.random.default_rng(seed)
    return {"wave": rng.standard_normal(n * hop).astype(np.float32), "f0": rng.uniform(80, 400, (n, 1)).astype(np.float32),
            "ppg": rng.standard_normal((n, d)).astype(np.float32), "lft": rng.standard_normal((n * hop, 1)).astype(np.float32),
            "spk_emb": rng.standard_normal((s, 1)).astype(np.float32)}


def test_store_layout_blocks_are_contiguous_and_aligned_ones_do_not_overlap():
    counts = [7, 1, 12, 5, 70, 3]
    offs, total = TS.store_layout(counts)
    assert offs == [0, 7, 8, 20, 25, 95] and total == 98                  # back to back, in order
    for o, n, nxt in zip(offs, counts, offs[1:] + [total]):
        assert o + n == nxt
    offs4, total4 = TS.store_layout(counts, align_frames=4)
    assert offs4 == [0, 8, 12, 24, 32, 104] and total4 == 107
    for o, n, nxt in zip(offs4, counts, offs4[1:] + [total4]):
        assert o % 4 == 0 and 0 <= nxt - (o + n) < 4                       # 16-byte starts, gaps below one alignment unit
    assert TS.store_layout([]) == ([], 0)


def test_batch_length_is_rounded_down_to_a_multiple_of_the_hop():
    assert TS.round_batch_length(16000, 160) == 16000
    assert TS.round_batch_length(16100, 160) == 16000                      # train_fastsvc.py:461-465
    assert TS.round_batch_length(27, 4) == 24
    with pytest.raises(ValueError):
        TS.round_batch_length(3, 4)
    plan = TS.corpus_plan([_utt(20)], batch_length=27, hop_size=HOP)
    assert plan["batch_length"] == 24 and plan["frames"] == 6 and plan["D"] == D and plan["S"] == S_EMB


def test_length_check_violations_raise_and_name_the_utterance():
    for key, cut in (("wave", 1), ("lft", 2), ("f0", 1), ("ppg", 1)):
        feats = [_utt(20, 1), _utt(20, 2), _utt(20, 3)]
        feats[2][key] = feats[2][key][:-cut]
        with pytest.raises(ValueError, match="utterance 2"):
            TS.corpus_plan(feats, 24, HOP)
        with pytest.raises(ValueError, match="utterance 2"):               # the constructor checks before it wants a device
            TS.TrainSession(feats, "cpu", batch_size=2, batch_length=24, hop_size=HOP)
    feats = [_utt(20, 1), _utt(20, 2, d=D + 1)]
    with pytest.raises(ValueError, match="utterance 1"):
        TS.corpus_plan(feats, 24, HOP)


def test_short_utterances_land_in_omitted():
    frames = 6
    for ctx in (0, 2):
        lens = [frames + 2 * ctx, frames + 2 * ctx + 1, 3, 40, frames + 2 * ctx - 1]
        plan = TS.corpus_plan([_utt(n, i) for i, n in enumerate(lens)], frames * HOP, HOP, aux_context_window=ctx)
        assert plan["omitted"] == [0, 2, 4] and plan["eligible"] == [1, 3]   # n - 2 ctx <= frames cannot be cropped (:501, :522-527)
        assert plan["n_frames"] == lens


def _sampler(lens, frames=6, ctx=0, bs=4, **kw):
    eligible = [i for i, n in enumerate(lens) if n - 2 * ctx > frames]
    return TS.CropSampler(lens, eligible, frames, bs, ctx, **kw), eligible


LENS = [7, 8, 30, 6, 70, 9, 11, 7, 25, 5, 13, 40, 8, 19]


def test_sampler_starts_lie_in_the_half_open_range_and_every_utterance_is_visited_once():
    for ctx in (0, 2):
        lens = [n + 2 * ctx for n in LENS]
        for seed in range(6):
            sm, eligible = _sampler(lens, ctx=ctx, seed=seed)
            for epoch in range(40):
                batches = sm.epoch_batches(epoch)
                seen = [u for us, _ in batches for u in us]
                assert sorted(seen) == eligible                            # each eligible utterance exactly once
                assert [len(us) for us, _ in batches] == [4] * (len(eligible) // 4) + ([len(eligible) % 4] if len(eligible) % 4 else [])
                for us, ss in batches:
                    assert len(us) == len(ss)
                    for u, s in zip(us, ss):
                        assert ctx <= s < lens[u] - 6 - ctx, (u, s)
                        if lens[u] - 2 * ctx == 7:                         # exactly one legal start
                            assert s == ctx


def test_sampler_covers_the_range_and_is_a_pure_function_of_seed_and_epoch():
    sm, _ = _sampler(LENS, seed=3)
    first = sm.epoch_batches(5)
    assert sm.epoch_batches(5) == first                                    # no hidden state
    assert _sampler(LENS, seed=3)[0].epoch_batches(5) == first
    sm.epoch_batches(9)
    assert sm.epoch_batches(5) == first
    assert sm.epoch_batches(6) != first and _sampler(LENS, seed=4)[0].epoch_batches(5) != first
    # utterance 5 (9 frames, crops of 6): starts 0, 1, 2 all occur, 3 (the closed end) never does
    got = set()
    for epoch in range(200):
        for us, ss in sm.epoch_batches(epoch):
            got.update(s for u, s in zip(us, ss) if u == 5)
    assert got == {0, 1, 2}
    orders = {tuple(u for us, _ in sm.epoch_batches(e) for u in us) for e in range(20)}
    assert len(orders) > 15                                                # a new permutation per epoch


def test_sampler_without_shuffle_reproduces_file_order():
    sm, eligible = _sampler(LENS, bs=3, shuffle=False, seed=7)
    for epoch in (0, 1, 17):
        batches = sm.epoch_batches(epoch)
        assert [u for us, _ in batches for u in us] == eligible
        assert [us for us, _ in batches] == [eligible[k: k + 3] for k in range(0, len(eligible), 3)]   # last group kept short
    assert sm.epoch_batches(0) != sm.epoch_batches(1)                       # the crops still move


def test_ranks_take_disjoint_batches_whose_union_is_the_global_list():
    for world in (2, 3, 5):
        for epoch in (0, 3):
            whole = _sampler(LENS, bs=2, seed=11)[0].epoch_batches(epoch)
            parts = [_sampler(LENS, bs=2, seed=11, rank=r, world=world)[0] for r in range(world)]
            merged = {}
            for r, sm in enumerate(parts):
                ks, bs = sm.global_indices(), sm.epoch_batches(epoch)
                assert len(ks) == len(bs) and all(k % world == r for k in ks)
                for k, b in zip(ks, bs):
                    assert k not in merged
                    merged[k] = b
            assert [merged[k] for k in sorted(merged)] == whole and sorted(merged) == list(range(len(whole)))


def test_cpu_devices_and_cpu_tensors_are_refused():
    feats = [_utt(20, 1), _utt(30, 2)]
    with pytest.raises(A.FastSVCError):
        TS.TrainSession(feats, "cpu", batch_size=2, batch_length=24, hop_size=HOP)
    n = 20
    wave, lft, ppg, f0, emb = (torch.zeros(n * HOP), torch.zeros(n * HOP), torch.zeros(n * D), torch.zeros(n), torch.zeros(1, S_EMB))
    with pytest.raises(A.FastSVCError):
        A.collate_crops(wave, lft, ppg, f0, emb, [0], [n], [0], [0], D, HOP, 6)


def test_library_exports_the_collate_symbols_at_abi_version_1():
    lib = ctypes.CDLL(A.library_path())
    assert hasattr(lib, "fastsvc_collate_launch_count") and hasattr(lib, "fastsvc_collate_crops")
    assert lib.fastsvc_abi_version() == 1
    lib = A.load_library()
    assert [lib.fastsvc_collate_launch_count(b) for b in (1, 32, 64, 65, 128, 129)] == [1, 1, 1, 2, 2, 3]
    # the checks come before any launch, so they can be seen without a device: null pointers, then (with dummy non-null
    # pointers that are never dereferenced on this path) a row outside the store
    assert lib.fastsvc_collate_crops(None, None, 0, None, 0, None, 0, None, 1, None, None, None, None,
                                     None, None, None, None, None, 1, D, S_EMB, HOP, 6, 0, None) == -1
    assert b"null" in lib.fastsvc_last_error()
