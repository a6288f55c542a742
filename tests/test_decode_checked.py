"""CPU-side tests of the checked decode path: the host reference of the per-row output report (decode.output_report),
the choice of the batches a checked session runs again (decode.flagged_batches), and the refusal of CPU devices.  No
kernel is launched here; the kernels and the session are checked on the GPU in tests/test_decode_checked_gpu.py."""
from fractions import Fraction

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


F32 = np.float32
NAN, INF = F32(np.nan), F32(np.inf)


def _saturates(v) -> bool:
    """The header's definition in exact rational arithmetic: round-half-to-even of y * 32767 outside [-32768, 32767]."""
    return not -32768 <= round(Fraction(float(F32(v))) * 32767) <= 32767       # (round() of a Fraction: half to even)


def _one(values, n=None):
    row = np.asarray(values, dtype=F32)[None]
    nf, cl, mx = Dc.output_report(row, [row.shape[1] if n is None else n])
    assert nf.dtype == np.int32 and cl.dtype == np.int32 and mx.dtype == np.float32
    return int(nf[0]), int(cl[0]), mx[0]


def test_output_report_counts_nonfinite_apart_from_clipped_and_keeps_them_out_of_the_maximum():
    assert _one([0.25, NAN, INF, -INF, -0.5]) == (3, 0, F32(0.5))
    assert _one([INF]) == (1, 0, F32(0))
    assert _one([NAN] * 5) == (5, 0, F32(0))                       # an all-NaN row: no finite sample, max_abs is 0
    assert _one([3.0, NAN, -7.5]) == (1, 2, F32(7.5))


def test_output_report_stops_at_len():
    """lens shorter than the row: a NaN (and a clipping sample) just past len are not counted; len 0 reads nothing."""
    row = [0.5, -0.75, 0.1, NAN, 9.0]
    assert _one(row, 3) == (0, 0, F32(0.75))
    assert _one(row, 4) == (1, 0, F32(0.75))
    assert _one(row, 5) == (1, 1, F32(9.0))
    assert _one(row, 0) == (0, 0, F32(0))
    assert _one([NAN, NAN], 0) == (0, 0, F32(0))
    nf, cl, mx = Dc.output_report(np.zeros((0, 4), F32), [])
    assert nf.shape == cl.shape == mx.shape == (0,)
    with pytest.raises(ValueError):
        Dc.output_report(np.zeros((1, 4), F32), [5])
    with pytest.raises(ValueError):
        Dc.output_report(np.zeros((2, 4), F32), [4])


def test_output_report_edges_of_the_int16_range():
    """`clipped` is the header's formula with to_pcm16's float64 arithmetic: rint(float64(y) * 32767.0) outside
    [-32768, 32767].  +-1.0 give +-32767 and are not clipped; 1 + 2^-14 rounds to 32769 and is.  -1 - 2^-15 gives
    -32767.99997 -> -32768, which IS an int16 value: by the formula it does not saturate (the int16 range is one step
    longer on the negative side); -1 - 2^-14 (-> -32769) is the first power-of-two step below -1 that does.  The float32
    nearest the tie 32767.5 / 32767, and its neighbours, go by exact rational arithmetic, as does every case above."""
    stated = [(1.0, False), (-1.0, False), (1 + 2.0 ** -14, True), (-1 - 2.0 ** -15, False), (-1 - 2.0 ** -14, True),
              (1 + 2.0 ** -15, True), (1.0001, True), (-1.0001, True)]
    tie, ntie = F32(32767.5) / F32(32767.0), F32(-32768.5) / F32(32767.0)
    derived = [tie, np.nextafter(tie, F32(0)), np.nextafter(tie, F32(2)), ntie, np.nextafter(ntie, F32(0)),
               np.nextafter(ntie, F32(-2)), np.nextafter(F32(1), F32(2)), np.nextafter(F32(-1), F32(-2))]
    assert {_saturates(v) for v in derived[:3]} == {False, True}               # (the tie's neighbourhood has both sides)
    assert {_saturates(v) for v in derived[3:6]} == {False, True}
    for v, want in stated + [(v, _saturates(v)) for v in derived]:
        assert _saturates(v) == want, v
        nf, cl, mx = _one([0.0, v, 0.0])
        assert (nf, cl) == (0, int(want)), v
        assert mx == abs(F32(v))
        # and it is what to_pcm16 does: a clipped sample is one whose unsaturated value is not what comes out
        exact = round(Fraction(float(F32(v))) * 32767)
        assert (int(Dc.to_pcm16(np.array([v], F32))[0]) != exact) == want, v


def test_output_report_takes_a_list_of_waveforms_and_tensors():
    ys = [np.array([0.5, 2.0, NAN], F32), np.array([-3.0], F32), np.zeros(0, F32)]
    nf, cl, mx = Dc.output_report(ys)
    assert list(nf) == [1, 0, 0] and list(cl) == [1, 1, 0] and list(mx) == [2.0, 3.0, 0.0]
    t = torch.tensor([[[0.5, -2.0, float("inf")]]])                            # (B, 1, width), as the generator returns it
    nf, cl, mx = Dc.output_report(t, [3])
    assert (int(nf[0]), int(cl[0]), float(mx[0])) == (1, 1, 2.0)


def test_flagged_batches_picks_whole_batches():
    batches = [[4, 2], [0, 5], [1], [3, 6]]
    assert Dc.flagged_batches(batches, []) == []                               # none flagged
    assert Dc.flagged_batches(batches, [5]) == [1]                             # one row flagged in one batch
    assert Dc.flagged_batches(batches, {5, 0}) == [1]                          # two rows of one batch: the batch once
    assert Dc.flagged_batches(batches, [6, 1, 2, 0]) == [0, 1, 2, 3]           # every batch flagged
    # a second round: of the batches run again, only those that still hold a flagged utterance
    first = Dc.flagged_batches(batches, [2, 1, 6])
    assert first == [0, 2, 3]
    assert Dc.flagged_batches(batches, [6], first) == [3]
    assert Dc.flagged_batches(batches, [6, 0], first) == [3]                   # (batch 1 was not among the first round's)
    assert Dc.flagged_batches(batches, [], first) == []
    assert Dc.flagged_batches([], [1]) == []


def test_checked_session_needs_a_gpu_like_the_unchecked_one():
    class M:
        out_channels = 1
    feats = [dict(f0=np.zeros((4, 1)), ppg=np.zeros((4, 8), np.float32), lft=np.zeros((640, 1), np.float32))]
    with pytest.raises(A.FastSVCError):
        Dc.DecodeSession(M(), feats, _Hop(), "cpu", checked=True)
    with pytest.raises(A.FastSVCError):
        Dc.DecodeSession(M(), feats, _Hop(), "cpu", checked=True, fallback=("bfloat16", "float32"), strict=True)
    with pytest.raises(ValueError):
        Dc.DecodeSession(M(), feats, _Hop(), "cpu", checked=True, fallback=("float8",))
    with Dc.DecodeSession(None, [], _Hop(), "cpu", checked=True) as s:         # an empty session converts to nothing
        assert s.convert() == [] and s.last_report == [] and s.forwards == 0


def test_checked_entry_points_refuse_cpu_tensors():
    """Like every entry point of the package: no CPU fallback (the library loads without a device)."""
    with pytest.raises(A.FastSVCError):
        A.output_check(torch.zeros(2, 8), [8, 8])
    nf, cl, mx = A.report_arrays(np.array([[1, 2, np.float32(1.5).view(np.int32), 0]], dtype=np.int32))
    assert (list(nf), list(cl), list(mx)) == ([1], [2], [1.5]) and mx.dtype == np.float32


def test_closing_line_counts_fallbacks_clipping_and_the_largest_magnitude():
    reports = [dict(storage="bfloat16", tried=["float16"], nonfinite=0, clipped=3, max_abs=1.5),
               dict(storage="float16", tried=[], nonfinite=0, clipped=0, max_abs=0.5),
               dict(storage="float32", tried=["float16", "bfloat16"], nonfinite=2, clipped=1, max_abs=7.25)]
    text = Dc.summarize_reports(reports, "float16")
    assert "3 utterances" in text and "2 fell back (1 to bfloat16, 1 to float32)" in text
    assert "1 STILL NON-FINITE" in text and "2 have clipped samples" in text and "max_abs 7.25" in text
    assert "0 fell back;" in Dc.summarize_reports(reports[1:2], "float16")
