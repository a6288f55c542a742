"""CPU-side tests of the checked decode path: the host reference of the per-row output report (decode.output_report),
the choice of the batches a checked session runs again (decode.flagged_batches), the storage fallback every checked
convert drives (decode.storage_fallback, with a fake model and scripted flags), and the refusal of CPU devices.  No
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


class _FakeModel:
    """What ``storage_fallback`` needs of a model: the attribute, and a switch that records its calls."""

    def __init__(self, storage="float16"):
        self.activation_storage = storage
        self.calls = []

    def use_activation_storage(self, name):
        self.calls.append(name)
        self.activation_storage = name


def _scripted(model, clears):
    """``is_flagged`` / ``rerun`` over scripted flags: ``clears[unit]`` is the storage that clears the unit (None: none
    does; a unit that is not in it was never flagged).  ``rerun`` records ``(name, the model's storage, flagged)``."""
    flagged, rounds = set(clears), []

    def rerun(name, units):
        rounds.append((name, getattr(model, "activation_storage", None), list(units)))
        for i in units:
            if clears[i] == name:
                flagged.discard(i)
    return (lambda i: i in flagged), rerun, rounds


def test_fallback_driver_leaves_a_clean_pass_alone():
    m = _FakeModel()
    is_flagged, rerun, rounds = _scripted(m, {})
    storage, tried, still = Dc.storage_fallback(m, ("bfloat16", "float32"), 4, is_flagged, rerun)
    assert storage == ["float16"] * 4 and tried == [[], [], [], []] and still == []
    assert m.calls == [] and rounds == []                                       # no switch, no rerun, no restore


def test_fallback_driver_walks_the_storages_with_the_units_still_flagged():
    m = _FakeModel()
    is_flagged, rerun, rounds = _scripted(m, {1: "bfloat16", 3: "float32", 4: "bfloat16", 5: "float32"})
    storage, tried, still = Dc.storage_fallback(m, ("bfloat16", "float32"), 6, is_flagged, rerun)
    assert rounds == [("bfloat16", "bfloat16", [1, 3, 4, 5]), ("float32", "float32", [3, 5])]     # exactly the still-flagged units
    assert storage == ["float16", "bfloat16", "float16", "float32", "bfloat16", "float32"]
    assert tried == [[], ["float16"], [], ["float16", "bfloat16"], ["float16"], ["float16", "bfloat16"]]
    assert still == []
    assert m.calls == ["bfloat16", "float32", "float16"] and m.activation_storage == "float16"    # restored, once, at the end
    # everything cleared by the first fallback: the second is never switched to
    m = _FakeModel()
    is_flagged, rerun, rounds = _scripted(m, {0: "bfloat16"})
    assert Dc.storage_fallback(m, ("bfloat16", "float32"), 2, is_flagged, rerun) == (["bfloat16", "float16"], [["float16"], []], [])
    assert m.calls == ["bfloat16", "float16"] and len(rounds) == 1


def test_fallback_driver_names_what_the_last_storage_left_flagged():
    m = _FakeModel()
    is_flagged, rerun, rounds = _scripted(m, {0: None, 2: "float32", 3: None})
    storage, tried, still = Dc.storage_fallback(m, ("bfloat16", "float32"), 4, is_flagged, rerun)
    assert still == [0, 3]
    assert [storage[i] for i in still] == ["float32", "float32"]                # the last name tried
    assert [tried[i] for i in still] == [["float16", "bfloat16"]] * 2
    assert storage[1] == "float16" and storage[2] == "float32" and tried[1] == []
    assert [r[2] for r in rounds] == [[0, 2, 3], [0, 2, 3]]
    assert m.activation_storage == "float16"


def test_fallback_driver_without_fallbacks_only_reports():
    class Bare:                                                                 # (no switch at all: it must not be needed)
        activation_storage = "float16"
    is_flagged, rerun, rounds = _scripted(Bare(), {1: None})
    assert Dc.storage_fallback(Bare(), (), 3, is_flagged, rerun) == (["float16"] * 3, [[], [], []], [1])
    assert rounds == []


def test_fallback_driver_restores_the_storage_when_a_rerun_raises():
    m = _FakeModel()
    is_flagged, rerun, rounds = _scripted(m, {0: None})

    def failing(name, units):
        rerun(name, units)
        if len(rounds) == 2:
            raise RuntimeError("the forward failed")
    with pytest.raises(RuntimeError, match="the forward failed"):
        Dc.storage_fallback(m, ("bfloat16", "float32"), 1, is_flagged, failing)
    assert m.calls == ["bfloat16", "float32", "float16"] and m.activation_storage == "float16"


def test_fallback_driver_takes_a_model_without_the_attribute_for_float32():
    class M:
        def __init__(self):
            self.calls = []

        def use_activation_storage(self, name):
            self.calls.append(name)
    m = M()
    is_flagged, rerun, _ = _scripted(m, {1: "bfloat16"})
    assert Dc.storage_fallback(m, ("bfloat16",), 2, is_flagged, rerun) == (["float32", "bfloat16"], [[], ["float32"]], [])
    assert m.calls == ["bfloat16"]                  # (nothing says that the storage changed: nothing to restore)
    assert Dc.storage_fallback(M(), ("bfloat16",), 2, lambda i: False, rerun)[0] == ["float32", "float32"]


def test_batch_narrowing_reruns_every_flagged_unit_in_every_round():
    """The ``rerun`` of the batch methods, as ``convert`` builds it: whole batches, chosen by ``flagged_batches`` among
    those of the round before.  Whatever clears when, each round's batches hold every unit still flagged (a unit flagged
    now was flagged in every earlier round, so its batch was run in every earlier round), hold nothing but batches
    with a flagged unit, and name exactly the flagged units' positions."""
    batches = [[4, 2], [0, 5], [1], [3, 6, 7]]
    for clears in ({2: "bfloat16", 6: "float32", 7: None}, {0: None, 1: None}, {i: "float32" for i in range(8)},
                   {5: "bfloat16"}, {4: "float32", 3: "bfloat16", 7: "float32", 1: "bfloat16"}):
        m = _FakeModel()
        is_flagged, mark, rounds = _scripted(m, clears)
        runs = []

        def run(work, mark=mark, runs=runs, m=m):
            runs.append(work)
            mark(m.activation_storage, [batches[k][j] for k, js in work for j in js])
        storage, tried, still = Dc.storage_fallback(m, ("bfloat16", "float32"), 8, is_flagged, Dc._rerun_in_batches(batches, run))
        expect = sorted(clears)                                                 # (the units flagged before each round)
        for name, work in zip(("bfloat16", "float32"), runs):
            assert [k for k, _ in work] == Dc.flagged_batches(batches, expect)
            assert sorted(batches[k][j] for k, js in work for j in js) == expect
            assert all(js for _, js in work)
            expect = [i for i in expect if clears[i] != name]
        assert len(runs) == (0 if not clears else 1 if all(v == "bfloat16" for v in clears.values()) else 2)
        assert still == sorted(i for i, v in clears.items() if v is None)
        for i in range(8):
            assert storage[i] == ("float16" if i not in clears else clears[i] or "float32")


def test_report_dicts_and_the_strict_error():
    rep = np.array([[0, 2, np.float32(1.5).view(np.int32), 0], [3, 0, np.float32(0.25).view(np.int32), 0]], dtype=np.int32)
    assert Dc._report_dicts(rep, ["float16", "bfloat16"], [[], ["float16"]]) == [
        dict(storage="float16", nonfinite=0, clipped=2, max_abs=1.5, tried=[]),
        dict(storage="bfloat16", nonfinite=3, clipped=0, max_abs=0.25, tried=["float16"])]
    with pytest.raises(A.FastSVCError) as e:
        Dc._raise_still_nonfinite(_FakeModel(), ("bfloat16",), "utterances", [1])
    assert str(e.value) == "utterances [1] still have non-finite samples after storages ['float16', 'bfloat16'] (strict=True)"


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
