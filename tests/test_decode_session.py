"""CPU-side tests of the resident decode path (decode.DecodeSession): the packing layout, the int16 wav writer, the
CLI's grouping, and the two new entry points' refusal of CPU tensors.  No kernel is launched here; the kernels and the
session itself are checked on the GPU in tests/test_decode_session_gpu.py."""
import wave

import numpy as np
import pytest
import torch

import svcc23_fastsvc_amd as A
from svcc23_fastsvc_amd import decode as Dc


@pytest.fixture(scope="module", autouse=True)
def _built():
    from svcc23_fastsvc_amd.build import build
    build()


class _Hop:
    hop_size = 160


def test_pack_layout_and_blocks_are_contiguous_in_batch_order():
    """Blocks lie back to back in the order given (the session's: batch by batch, longest first), offsets are indexed
    by utterance, totals add up, and a time-major (F, C) array is copied as it is - no transpose."""
    frames = [5, 0, 9, 1, 7]
    C = 3
    rng = np.random.default_rng(0)
    ppg = [rng.standard_normal((f, C)).astype(np.float32) for f in frames]
    order = [2, 4, 0, 3, 1]
    counts = [f * C for f in frames]
    offsets, total = Dc.pack_layout(counts, order)
    assert total == sum(counts)
    pos = 0
    for i in order:                                        # contiguity, in order
        assert offsets[i] == pos
        pos += counts[i]
    assert pos == total
    dst = np.full(total, np.nan, dtype=np.float32)
    Dc.pack_blocks(ppg, counts, offsets, dst)
    for i, a in enumerate(ppg):
        assert np.array_equal(dst[offsets[i]: offsets[i] + counts[i]].reshape(frames[i], C), a)
    assert not np.isnan(dst).any()
    # a subset (one batch) fills only its own blocks; float64 input is converted; an (n, 1) column is flattened; a longer
    # array is cut to its count (lft beyond F * hop samples), a shorter one is an error
    dst[:] = np.nan
    Dc.pack_blocks(ppg, counts, offsets, dst, [2, 4])
    assert not np.isnan(dst[: counts[2] + counts[4]]).any() and np.isnan(dst[counts[2] + counts[4]:]).all()
    lft = [np.arange(8, dtype=np.float64).reshape(8, 1)]
    d2 = np.zeros(6, dtype=np.float32)
    Dc.pack_blocks(lft, [6], [0], d2)
    assert d2.dtype == np.float32 and list(d2) == [0, 1, 2, 3, 4, 5]
    with pytest.raises(ValueError):
        Dc.pack_blocks(lft, [9], [0], np.zeros(9, dtype=np.float32))
    assert Dc.pack_layout([], []) == ([], 0)


def test_empty_session_converts_to_nothing():
    with Dc.DecodeSession(None, [], _Hop(), "cpu") as s:
        assert s.batches == [] and s.uploaded_bytes == {"init": 0, "convert": []}
        assert s.convert() == []
        assert s.convert(np.zeros(4, np.float32), [5.0, 1.0], pcm16=False) == []
    with pytest.raises(RuntimeError):
        s.convert()
    s.close()                                              # idempotent


def test_session_needs_a_gpu_and_one_output_channel():
    class M:
        out_channels = 1
    feats = [dict(f0=np.zeros((4, 1)), ppg=np.zeros((4, 8), np.float32), lft=np.zeros((640, 1), np.float32))]
    with pytest.raises(A.FastSVCError):
        Dc.DecodeSession(M(), feats, _Hop(), "cpu")
    M.out_channels = 2
    with pytest.raises(ValueError):
        Dc.DecodeSession(M(), feats, _Hop(), "cpu")


def test_write_wav_int16_equals_write_wav_float(tmp_path):
    rng = np.random.default_rng(1)
    y = np.concatenate([rng.normal(0, 0.7, 4000).astype(np.float32),
                        np.array([0.0, 0.5, -0.5, 1.0, -1.0, 1.7, -3.0, 1e-5], dtype=np.float32)])
    pa, pb = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    Dc.write_wav(pa, y, 24000)
    Dc.write_wav(pb, Dc.to_pcm16(y), 24000)
    assert open(pa, "rb").read() == open(pb, "rb").read()
    with wave.open(pb, "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 24000, len(y))
        assert np.array_equal(np.frombuffer(w.readframes(len(y)), dtype=np.int16), Dc.to_pcm16(y))
    # a non-contiguous int16 view (every other sample) is written as its values
    pc = str(tmp_path / "c.wav")
    Dc.write_wav(pc, Dc.to_pcm16(y)[::2], 24000)
    with wave.open(pc, "rb") as w:
        assert np.array_equal(np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16), Dc.to_pcm16(y)[::2])


def test_resident_groups_respect_the_budget_and_keep_order():
    frames = {"a": 10, "b": 20, "c": 5, "d": 100, "e": 1}
    C, hop = 4, 16

    def load(p):
        return {"ppg": np.zeros((frames[p], C), np.float32)}
    per = {p: 4 * f * (C + hop) for p, f in frames.items()}
    groups = list(Dc.resident_groups(list(frames), per["a"] + per["b"] + per["c"], hop, load))
    assert [g[0] for g in groups] == [["a", "b", "c"], ["d"], ["e"]]       # "d" alone exceeds the budget: its own group
    assert all(len(g[0]) == len(g[1]) for g in groups)
    assert [g[0] for g in Dc.resident_groups(list(frames), 1 << 40, hop, load)] == [list(frames)]
    assert list(Dc.resident_groups([], 1 << 20, hop, load)) == []


def test_new_entry_points_refuse_cpu_tensors():
    """Like every entry point of the package: no CPU fallback (the library loads without a device)."""
    with pytest.raises(A.FastSVCError):
        A.gather_time_major(torch.zeros(12), [0], [3], 4, 8)
    with pytest.raises(A.FastSVCError):
        A.pcm16_pack(torch.zeros(2, 8), [8, 8])
    with pytest.raises(A.FastSVCError):
        A.pcm16_pack(np.zeros((2, 8), np.float32), [8, 8])
