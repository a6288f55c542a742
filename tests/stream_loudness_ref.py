"""Float64 reference of the loudness of a live stream (decode.StreamSession(loudness="audio")), over
oracle.loudness_oracle: the whole-file function's first F = T // hop frames, each floored 80 dB below the RUNNING maximum of
the power up to and including it.  Plus the test signals the stream-loudness tests share."""
import numpy as np

from oracle import loudness_oracle as LO

SR = 24000


def stream_loudness_frames(audio, sampling_rate: int, hop: int) -> np.ndarray:
    """(F,) float64: one value per frame, F = len(audio) // hop."""
    F = len(audio) // hop
    P = LO.stft_power(np.asarray(audio)[: F * hop], hop)[:, :F]
    floor = 10.0 * np.log10(np.maximum(1e-10, np.maximum.accumulate(P.max(axis=0)))) - 80.0
    db = np.maximum(10.0 * np.log10(np.maximum(1e-10, P)), floor[None, :])
    db = db + LO.a_weighting(np.linspace(0.0, sampling_rate / 2.0, LO.N_FFT // 2 + 1))[:, None]
    return np.log(np.mean(10.0 ** (db / 20.0), axis=0) + 1e-5)


def stream_loudness(audio, sampling_rate: int, hop: int) -> np.ndarray:
    """(F hop,) float64: every frame's value repeated hop times."""
    return np.repeat(stream_loudness_frames(audio, sampling_rate, hop), hop)


def rising_signal(F: int, hop: int, seed: int = 0) -> np.ndarray:
    """A 0.9 sine at 1 kHz, 100 times louder from the middle on, over 1e-6 noise: the running maximum keeps changing."""
    T = F * hop
    y = 0.9 * np.sin(2.0 * np.pi * 1000.0 * np.arange(T) / SR)
    y[: T // 2] *= 0.01
    return (y + 1e-6 * np.random.default_rng(seed).standard_normal(T)).astype(np.float32)


def peak_first_signal(F: int, hop: int, seed: int = 0) -> np.ndarray:
    """A 0.9 sine at 1 kHz in the first 128 samples over a 0.05 sine at 440 Hz, plus 1e-6 noise: frame 0 holds the peak."""
    T = F * hop
    t = np.arange(T) / SR
    y = 0.05 * np.sin(2.0 * np.pi * 440.0 * t)
    y[:128] += 0.9 * np.sin(2.0 * np.pi * 1000.0 * t[:128])
    return (y + 1e-6 * np.random.default_rng(seed).standard_normal(T)).astype(np.float32)
