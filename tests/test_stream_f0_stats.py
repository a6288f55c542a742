"""CPU tests of the running source F0 statistics of live streams (decode.RunningF0Stats, decode.running_f0_convert; DESIGN.md
4.10) against the float64 reference tests/stream_f0_stats_ref.py, which is written from the rule alone: the loop against the
cumsum closed form, the host function against the loop bit for bit, the variance bound, unvoiced frames, the heavy prior
against F0Statistics.convert, convergence to the whole-track statistics, and the constructor's refusals."""
import math

import numpy as np
import pytest

import stream_f0_stats_ref as R
from svcc23_fastsvc_amd import decode as Dc

TRG = [5.45, 0.33]
# (prior, prior_frames, horizon): the default, a prior of its own with little weight, a horizon short enough to matter
SETTINGS = ((None, 100.0, None), ([5.1, 0.21], 10.0, None), (None, 100.0, 8.0), ([5.0, 0.3], 1.0, 200.0))

# Convergence, measured here (wandering_track(3000, 0): 2552 voiced frames, estimate = [5.0452, 0.1275], target TRG, prior =
# target): the largest relative difference over the last fifth against F0Statistics.convert with the whole track's estimate.
# The gates are twice these; the margin is for another libm, nothing else.
MEASURED = {1.0: 9.03e-3, 100.0: 1.564e-1}
MEASURED_HORIZON_200 = {1.0: 8.97e-2, 100.0: 4.055e-1}      # (reported in the documents, not gated)


@pytest.fixture(scope="module")
def tracks():
    return {F: R.wandering_track(F, seed) for F, seed in ((60, 1), (300, 2), (3000, 0))}


def _running(prior, frames, horizon):
    return Dc.RunningF0Stats(prior, frames, horizon)


def test_the_loop_equals_the_closed_form(tracks):
    """Without a horizon the sums are running sums: at most a few hundred float64 terms of size ~1, so the sequential loop
    and np.cumsum agree to 1e-12 relative on the mean, the variance and the output."""
    for F in (60, 300):
        f0 = tracks[F]
        for prior, frames, horizon in SETTINGS:
            if horizon is not None:
                continue
            c = R.constants(TRG, prior, frames)
            a, b = R.running_loop(f0, c), R.running_closed(f0, c)
            assert a.mean.size == (f0 > 0).sum() >= 20
            for name in ("mean", "var", "out"):
                x, y = getattr(a, name), getattr(b, name)
                ok = y != 0
                assert np.array_equal(x == 0, y == 0) and np.abs(x[ok] / y[ok] - 1.0).max() <= 1e-12, (F, name)


def test_the_host_function_is_the_reference_bit_for_bit(tracks):
    for F, f0 in tracks.items():
        for prior, frames, horizon in SETTINGS:
            got = Dc.running_f0_convert(f0, _running(prior, frames, horizon), TRG)
            want = R.running_loop(f0, R.constants(TRG, prior, frames, horizon)).out
            assert got.dtype == np.float64 and got.shape == (F,)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (F, prior, frames, horizon)
    assert _running(None, 100.0, None).decay == 1.0 and _running(None, 100.0, 8.0).decay == math.exp(-1.0 / 8.0)
    assert _running([5.1, 0.21], 10.0, None).constants(TRG) == R.constants(TRG, [5.1, 0.21], 10.0)
    assert _running(None, 3.0, 50.0).constants(TRG) == R.constants(TRG, None, 3.0, 50.0)


def test_the_variance_stays_above_the_priors_share(tracks):
    """Cauchy-Schwarz: var N >= n0 s_p^2 on every frame, so nothing is divided by zero and nothing is NaN."""
    for F, f0 in tracks.items():
        for prior, frames, horizon in SETTINGS + ((None, 1.0, None), (None, 25.0, 200.0)):
            c = R.constants(TRG, prior, frames, horizon)
            t = R.running_loop(f0, c)
            assert (t.var * (c[2] + t.w) >= c[2] * c[1] * c[1]).all(), (F, prior, frames, horizon)
            assert np.isfinite(t.out).all() and (t.out[f0 > 0] > 0).all()


def test_unvoiced_frames_are_zero_and_leave_the_state_alone(tracks):
    """The voiced frames of a track are shifted as if the unvoiced ones were not there - silence neither counts nor forgets,
    with a horizon too - and the unvoiced ones come out as exactly 0."""
    f0 = tracks[300]
    voiced = f0 > 0
    assert voiced.sum() >= 20 and (~voiced).sum() >= 20
    for prior, frames, horizon in SETTINGS:
        r = _running(prior, frames, horizon)
        whole, dense = Dc.running_f0_convert(f0, r, TRG), Dc.running_f0_convert(f0[voiced], r, TRG)
        assert not whole[~voiced].any()
        assert np.array_equal(whole[voiced].view(np.uint64), dense.view(np.uint64))
    assert not Dc.running_f0_convert(np.zeros(7, np.float32), _running(None, 100.0, None), TRG).any()
    assert Dc.running_f0_convert(np.zeros(0, np.float32), _running(None, 100.0, None), TRG).shape == (0,)


def test_a_heavy_prior_is_the_fixed_shift(tracks):
    """prior = src with 1e15 frames: the evidence of 3000 frames moves mu and var by ~1e-12 relative to s_p, and the result is
    F0Statistics.convert(f0, src, trg) to 1e-12 relative."""
    f0 = tracks[3000]
    src = [5.1, 0.21]
    got = Dc.running_f0_convert(f0, _running(src, 1e15, None), TRG)
    want = Dc.F0Statistics().convert(f0.astype(np.float64), src, TRG)
    voiced = f0 > 0
    assert not got[~voiced].any() and not want[~voiced].any()
    worst = np.abs(got[voiced] / want[voiced] - 1.0).max()
    print(f"heavy prior against the fixed shift: {worst:.3e} relative")
    assert worst <= 1e-12
    assert np.array_equal(want, R.fixed_convert(f0, src, TRG))


@pytest.mark.parametrize("n0", [1.0, 100.0])
def test_without_a_horizon_the_shift_converges_to_the_whole_tracks(tracks, n0):
    """3000 frames, no horizon, prior = target: over the last fifth the output is within 2 x MEASURED[n0] of
    F0Statistics.convert with estimate() of the whole track - the prior's n0 frames against ~2500 voiced ones."""
    f0 = tracks[3000]
    src = Dc.F0Statistics().estimate([f0.astype(np.float64)])
    assert np.allclose(src, R.estimate(f0), rtol=1e-12, atol=0)
    want = Dc.F0Statistics().convert(f0.astype(np.float64), src, TRG)
    last = np.arange(f0.size) >= f0.size - f0.size // 5
    sel = last & (f0 > 0)
    assert sel.sum() >= 400
    worst = {}
    for horizon in (None, 200.0):
        got = Dc.running_f0_convert(f0, _running(None, n0, horizon), TRG)
        worst[horizon] = float(np.abs(got[sel] / want[sel] - 1.0).max())
    print(f"n0 {n0:g}: last fifth against the whole track's statistics {worst[None]:.3e} relative (gate {2 * MEASURED[n0]:.3e}); "
          f"with horizon 200 {worst[200.0]:.3e} (recorded {MEASURED_HORIZON_200[n0]:.3e})")
    assert worst[None] <= 2.0 * MEASURED[n0]
    assert worst[200.0] > worst[None]                   # (a horizon forgets: it does not converge to the whole track)


def test_running_f0_stats_refuses_what_it_cannot_use():
    for kw in (dict(prior=[5.0, 0.0]), dict(prior=[5.0, -0.1]), dict(prior=[float("nan"), 0.2]), dict(prior=[5.0]),
               dict(prior_frames=0.0), dict(prior_frames=float("inf")), dict(prior_frames=-3.0), dict(horizon=0.5),
               dict(horizon=float("nan")), dict(horizon=float("inf"))):
        with pytest.raises(ValueError):
            Dc.RunningF0Stats(**kw)
    r = Dc.RunningF0Stats([5.0, 0.2], 30, 1)
    assert r.prior == (5.0, 0.2) and r.prior_frames == 30.0 and r.horizon == 1.0
    with pytest.raises(Exception):                       # (immutable)
        r.prior_frames = 1.0
    with pytest.raises(ValueError):                      # (no prior: the target's std is the prior's)
        Dc.running_f0_convert(np.ones(3, np.float32), Dc.RunningF0Stats(), [5.0, 0.0])
