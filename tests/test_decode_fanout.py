"""CPU-side tests of the speaker fan-out of the resident decode path: the batch planning (decode.fanout_batches), the empty
session, the CLI's argument check and grouping, and the binding's refusal of CPU tensors.  No kernel is launched here; the
kernel and DecodeSession.convert_many are checked on the GPU in tests/test_decode_fanout_gpu.py."""
import ctypes

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


FRAME_SETS = [[31, 7, 25, 26, 18, 40, 12, 33, 9, 21, 38], [12], [5, 5, 5], [100, 1, 99, 2, 50, 50, 51]]


@pytest.mark.parametrize("frames", FRAME_SETS)
@pytest.mark.parametrize("S", [1, 2, 3, 16])
@pytest.mark.parametrize("max_batch,tol", [(1, 0.125), (2, 0.125), (3, 0.9), (8, 0.0), (16, 0.9), (64, 0.125)])
def test_fanout_batches_cover_every_pair_once_within_the_limits(frames, S, max_batch, tol):
    batches = Dc.fanout_batches(frames, S, max_batch, tol)
    rows = [pair for chunk in batches for pair in chunk]
    assert sorted(rows) == [(u, s) for u in range(len(frames)) for s in range(S)]          # every pair, exactly once
    for chunk in batches:
        assert 1 <= len(chunk) <= max_batch
        longest = frames[chunk[0][0]]
        assert all(frames[u] <= longest for u, _ in chunk)                                   # longest first
        assert all(frames[u] >= (1.0 - tol) * longest for u, _ in chunk)                     # bounded padding
    # longest first over the whole pass, and an utterance's speakers adjacent and ascending
    assert [frames[u] for u, _ in rows] == sorted((frames[u] for u, _ in rows), reverse=True)
    for u in range(len(frames)):
        at = [k for k, (v, _) in enumerate(rows) if v == u]
        assert at == list(range(at[0], at[0] + S)) and [rows[k][1] for k in at] == list(range(S))
    # it IS bucket_ragged over the expanded row list
    n = len(frames) * S
    want = Dc.bucket_ragged(range(n), [frames[r // S] for r in range(n)], max_batch, tol)
    assert batches == [[(r // S, r % S) for r in chunk] for chunk in want]


@pytest.mark.parametrize("frames", FRAME_SETS)
def test_fanout_batches_of_one_speaker_are_the_sessions_batches(frames):
    for max_batch, tol in ((2, 0.125), (3, 0.9), (32, 0.125)):
        want = Dc.bucket_ragged(range(len(frames)), frames, max_batch, tol)
        assert Dc.fanout_batches(frames, 1, max_batch, tol) == [[(i, 0) for i in chunk] for chunk in want]
    with pytest.raises(ValueError):
        Dc.fanout_batches(frames, 0)
    assert Dc.fanout_batches([], 3) == []


@pytest.mark.parametrize("frames", FRAME_SETS)
@pytest.mark.parametrize("S,max_batch", [(1, 3), (3, 4), (16, 5), (2, 64)])
def test_fanout_layout_puts_every_row_where_the_speakers_result_expects_it(frames, S, max_batch):
    """The per-speaker runs of every batch, copied as wholes, put each row's samples at the place the per-row layout
    names: result[speaker][pack offset of the utterance]."""
    hop = 4
    counts = [f * hop for f in frames]
    order = [i for chunk in Dc.bucket_ragged(range(len(frames)), frames, max_batch, 0.9) for i in chunk]
    offsets, total = Dc.pack_layout(counts, order)
    result = np.full((S, total), -1, dtype=np.int64)
    for chunk in Dc.fanout_batches(frames, S, max_batch, 0.9):
        offs, runs, n = Dc.fanout_layout(chunk, counts, offsets)
        packed = np.full(n, -1, dtype=np.int64)
        for j, (u, sp) in enumerate(chunk):                                   # what the pack kernel writes: row j at offs[j]
            assert np.all(packed[offs[j]: offs[j] + counts[u]] == -1)         # rows do not overlap
            packed[offs[j]: offs[j] + counts[u]] = (u * S + sp) * 100000 + np.arange(counts[u])
        assert n == sum(counts[u] for u, _ in chunk) and np.all(packed >= 0)
        assert [r[0] for r in runs] == sorted({sp for _, sp in chunk})
        for sp, first, start, count in runs:
            assert np.all(result[sp, first: first + count] == -1)
            result[sp, first: first + count] = packed[start: start + count]
    for u in range(len(frames)):
        for sp in range(S):
            assert np.array_equal(result[sp, offsets[u]: offsets[u] + counts[u]], (u * S + sp) * 100000 + np.arange(counts[u]))


def test_empty_session_fans_out_to_the_empty_shape():
    with Dc.DecodeSession(None, [], _Hop(), "cpu") as s:
        assert s.convert_many([]) == []
        assert s.convert_many([(None, None)]) == [[]]
        assert s.convert_many([(np.zeros(4, np.float32), [5.0, 1.0])] * 3, pcm16=False) == [[], [], []]
        assert s.uploaded_bytes == {"init": 0, "convert": []}             # nothing was made resident for it
    with pytest.raises(RuntimeError):
        s.convert_many([(None, None)])


def test_fanout_without_resident_is_an_argument_error(capsys):
    base = ["--dumpdir", "d", "--checkpoint", "c", "--config", "y", "--outdir", "o"]
    with pytest.raises(SystemExit) as e:
        Dc.main(base + ["--fanout", "4"])
    assert e.value.code == 2 and "--fanout" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        Dc.main(base + ["--resident", "--fanout", "0"])
    assert e.value.code == 2


def test_speaker_groups_keep_order_size_and_kind():
    assert Dc.speaker_groups(list("abcdefg"), 3) == [["a", "b", "c"], ["d", "e", "f"], ["g"]]
    assert Dc.speaker_groups(list("abc"), 1) == [["a"], ["b"], ["c"]]
    assert Dc.speaker_groups([], 4) == []
    # a speaker of another kind (no embedding, no statistics) never shares a call
    assert Dc.speaker_groups(["a", "b", None, "c", "d"], 4, lambda s: s is None) == [["a", "b"], [None], ["c", "d"]]


def test_fanout_binding_refuses_cpu_tensors():
    """Like every entry point of the package: no CPU fallback (the library loads without a device)."""
    ppg, lft, f0 = torch.zeros(12), torch.zeros(6), torch.zeros(3)
    with pytest.raises(A.FastSVCError):
        A.fanout_assemble(ppg, lft, f0, [0], [0], [0], [3], [0], [0], 4, 2, 8)
    with pytest.raises(A.FastSVCError):
        A.fanout_assemble(np.zeros(12, np.float32), lft, f0, [0], [0], [0], [3], [0], [0], 4, 2, 8)
    assert A.fanout_launch_count(0) == 0 and A.fanout_launch_count(1) == 1
    assert A.fanout_launch_count(64) == 1 and A.fanout_launch_count(65) == 2 and A.fanout_launch_count(130) == 3


def test_fanout_assemble_validates_on_the_host_before_any_launch():
    """The C entry point itself, with host memory behind every pointer: each bad argument is FASTSVC_E_INVALID with the
    row and the reason in fastsvc_last_error(), decided before anything touches a device (there is none here)."""
    lib = A.load_library()
    C, hop, width, E = 4, 2, 8, 3
    bufs = [np.zeros(n, np.float32) for n in (13 * C, 13 * hop, 13)]
    emb, outs = np.zeros((2, E), np.float32), [np.full(n, 7.0, np.float32) for n in (2 * C * width, 2 * width * hop, 2 * width, 2 * E)]
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)                                          # noqa: E731

    def call(ppg_off=(0, 5 * C), lft_off=(0, 5 * hop), f0_off=(0, 5), n_frames=(5, 8), utt=(0, 1), spk=(0, 1), w=width,
             first=None, R=2):
        i64, i32 = (lambda v: (ctypes.c_int64 * len(v))(*v)), (lambda v: (ctypes.c_int32 * len(v))(*v))
        rc = lib.fastsvc_fanout_assemble(first if first is not None else vp(bufs[0]), bufs[0].size, vp(bufs[1]), bufs[1].size,
                                         vp(bufs[2]), bufs[2].size, 2, i64(ppg_off), i64(lft_off), i64(f0_off), i32(n_frames),
                                         None, None, vp(emb), 2, i32(utt), i32(spk), *[vp(o) for o in outs],
                                         R, C, E, hop, w, None)
        return rc, lib.fastsvc_last_error().decode()

    INVALID = -1                                               # FASTSVC_E_INVALID
    for kw, text in ((dict(ppg_off=(0, 6 * C)), "row 1: ppg block of utterance 1"),
                     (dict(lft_off=(0, 6 * hop)), "row 1: lft block of utterance 1"),
                     (dict(f0_off=(0, 6)), "row 1: f0 block of utterance 1"),
                     (dict(f0_off=(-1, 5)), "row 0: f0 block of utterance 0"),
                     (dict(utt=(0, 2)), "row 1: utterance 2 outside [0, 2)"),
                     (dict(utt=(-1, 1)), "row 0: utterance -1 outside"),
                     (dict(spk=(0, 2)), "row 1: speaker 2 outside [0, 2)"),
                     (dict(n_frames=(5, 9), ppg_off=(0, 0), lft_off=(0, 0), f0_off=(0, 0)), "row 1: utterance 1 has 9 frames"),
                     (dict(first=ctypes.c_void_p(0)), "null pointer"),
                     (dict(w=0), "size out of range"),
                     (dict(R=0), "size out of range")):
        rc, msg = call(**kw)
        assert rc == INVALID and text in msg, (kw, rc, msg)
    assert all(np.all(o == 7.0) for o in outs)
