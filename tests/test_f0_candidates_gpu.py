"""GPU test (-m gpu) of the tracker's candidates (f0.f0_candidates; csrc/fastsvc_f0.inc: f0_frame_candidates) against the
float64 reference (tests/stream_f0_track_ref.py) on the tracker's signals and stream_f0_ref.f0_signals() at hop 160 and 256 -
where a frame never has more than four local minima, so all are kept - and on the WIDE cases, the same kernel searched down
to f0_floor = 24 Hz (tau_max 1000), where a 339 Hz tone has up to 14 minima a frame, the glide 8 and a 220 Hz tone in noise 9:
there the four smallest d' must be chosen, and the margin against the fifth-best is finite.

Measured on the CPU with the float32 model of the kernel's arithmetic (stream_f0_ref.yin_frame_f32, its d' given to the
reference's candidate rule in float32) against float64, over every frame of stream_f0_track_ref.measured_cases() - every
signal below and the ones left out, both hops, narrow and wide; `python tests/stream_f0_track_ref.py` repeats it (minutes),
tests/test_stream_f0_track.py holds the model to the figures on a sample of the frames:
                                                  f0_floor 70   f0_floor 24
    largest |d'_32 - d'_64|                       4.56e-6       2.68e-6    a decision compares two d' (or one with the threshold):
                                                                           it cannot flip at a margin above 9.12e-6; twice that:
                                                                           MARGIN = 1.84e-5
    candidates the model lost or gained           none          none
    largest |s_32 - s_64| of a candidate          5.42e-7       3.47e-7    twice the larger: S_BOUND = 1.09e-6
    largest |tau_hat_32 - tau_hat_64|             7.36e-4       1.76e-4    (lags; the parabola divides small differences) twice
                                                                           the larger: TAU_BOUND = 1.48e-3
A reference candidate's margin is the smallest distance of d'(t) from cand_threshold, from its two neighbours and from the
fifth-best local minimum.  Frames with a candidate under MARGIN, narrow: none on the tones, the burst, the modulations, the
noise and the silence, 1 of 61 on `gap` at hop 160 - within 2 % - and 2 of 61 / 1 of 38 on `glide` and 1 of 38 on `gap` at hop
256, which are left out for it (a glide's minima wander through ties between neighbouring lags).  Wide: none on tone339, glide
and tone220n at hop 256 and 1 of 61 on glide at hop 160; tone339 (1 of 31) and tone220n (2 of 31) at hop 160 exceed 2 % - the
dips of a steady tone at multiples of its period are nearly equal - and are left out there."""
import numpy as np
import pytest
import torch

import stream_f0_ref as R
import stream_f0_track_ref as Q
import svcc23_fastsvc_amd as A

pytestmark = pytest.mark.gpu

MARGIN = 4 * 4.6e-6
S_BOUND = 2 * 5.42e-7
TAU_BOUND = 2 * 7.36e-4
LEFT_OUT = {160: ("glide",), 256: ("glide", "gap")}
WIDE = {160: ("glide",), 256: ("tone339", "glide", "tone220n")}
CAND_THRESHOLD = 0.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (and fail loudly without one)"
    A.load_library()
    return torch.device("cuda:0")


def _compare(dev, hop, signals, f0_floor):
    """f0_candidates against the reference on ``signals`` (name -> audio) -> (candidates compared, frames with more than four
    reference minima among the compared frames)."""
    tau_min, tau_max = R.lags(R.SR, f0_floor, R.F0_CEIL)
    lo = max(tau_min, 2)
    seen = crowded = 0
    for name, y in signals.items():
        _, ref, dns = Q.audio_candidates(y, hop, CAND_THRESHOLD, f0_floor=f0_floor)
        got = A.f0_candidates(torch.from_numpy(y).to(dev), R.SR, hop, f0_floor=f0_floor, cand_threshold=CAND_THRESHOLD).cpu().numpy()
        assert got.shape == (len(ref), 4, 2) and got.dtype == np.float32
        crowded += sum(1 for c in ref if len(c.minima) > 4 and all(m >= MARGIN for m in c.margin))
        for f, (c, dn) in enumerate(zip(ref, dns)):
            g = got[f]
            on = np.isfinite(g[:, 1])
            assert np.array_equal(on, g[:, 0] > 0) and on[:int(on.sum())].all(), (name, f)      # the absent ones last, (0, inf)
            assert np.all(np.diff(g[on, 0]) > 0), (name, f)          # ascending lag
            # every reference candidate whose decisions have margin MARGIN is there, with its tau_hat and s
            for k, t in enumerate(c.lags):
                if c.margin[k] < MARGIN:
                    continue
                near = np.nonzero(on & (np.abs(g[:, 0] - c.pairs[k, 0]) <= TAU_BOUND))[0]
                assert near.size == 1, (name, f, t, g)
                assert abs(float(g[near[0], 1]) - c.pairs[k, 1]) <= S_BOUND, (name, f, t)
                seen += 1
            # every candidate of the GPU is a local minimum of the reference under the threshold, to MARGIN
            for tau_hat, s in g[on].astype(np.float64):
                ok = False
                for t in {int(np.floor(tau_hat)), int(np.ceil(tau_hat))}:
                    if lo <= t <= tau_max and abs(dn[t] - s) <= S_BOUND:
                        right = dn[t + 1] if t < tau_max else np.inf
                        ok = ok or (dn[t] < CAND_THRESHOLD + MARGIN and dn[t] < dn[t - 1] + MARGIN and dn[t] <= right + MARGIN)
                assert ok, (name, f, tau_hat, s)
        frames_out = sum(1 for c in ref if any(m < MARGIN for m in c.margin))
        assert frames_out <= 0.02 * len(ref), (name, frames_out, len(ref))
        if name in ("noise", "zeros"):
            assert not np.isfinite(got[..., 1]).any() and not got[..., 0].any()
    return seen, crowded


@pytest.mark.parametrize("hop", [160, 256])
def test_candidates_against_the_reference(dev, hop):
    seen, _ = _compare(dev, hop, {k: y for k, (y, _) in Q.track_signals().items() if k not in LEFT_OUT[hop]}, R.F0_FLOOR)
    assert seen >= 700                                             # (the tones alone offer several candidates a frame)


@pytest.mark.parametrize("hop", [160, 256])
def test_the_four_smallest_are_chosen_among_more(dev, hop):
    """The wide cases: frames with up to 14 local minima under the threshold.  The kernel's four rounds of a block-wide
    minimum over (bits of d', lag) must keep the reference's four - a key ordered by lag alone, by the largest d' or with
    the bits the wrong way round keeps others, which the reference's kept ones, all with margin, then miss."""
    seen, crowded = _compare(dev, hop, {k: y for k, y in Q.wide_signals().items() if k in WIDE[hop]}, Q.WIDE_FLOOR)
    assert crowded >= 25 and seen >= 4 * crowded, (seen, crowded)
