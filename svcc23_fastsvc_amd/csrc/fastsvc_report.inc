// fastsvc_report.inc - the per-sample half of a fastsvc_row_report, shared by the kernels that fill one from float32
// samples (fastsvc_decodeio.hip: pcm16_check_kernel; fastsvc_stream_check.hip): one definition of "non-finite", "clipped"
// and "max_abs", so that two reports of the same samples cannot disagree.  Include inside the unit's anonymous namespace.
#pragma once

// What pcm16_of hides, for one sample: counts in one word (non-finite in the low half, saturating in the high half: a block
// sees at most 2048 of either) and the largest finite magnitude as the bit pattern of |y| (non-negative floats order like
// their bits).  No float64 here: double(y) * 32767.0 is exact and rint is monotonic, so "rint(...) outside [-32768, 32767]"
// is a comparison of y itself with two float32 constants - the product reaches 32767.5 (the tie rounds to the even 32768)
// from the smallest float32 >= 32767.5 / 32767 on, and falls below -32768.5 (that tie rounds to -32768, a value) from the
// largest float32 < -32768.5 / 32767 down.  (A second rint next to pcm16_of's is not merged by the compiler: each sinks
// into its own branch.)
constexpr float PCM16_CLIPS_FROM = 0x1.000102p+0f;             // bits 0x3f800081
constexpr float PCM16_CLIPS_DOWN_FROM = -0x1.000302p+0f;       // bits 0xbf800181

__device__ __forceinline__ void pcm16_tally(float y, unsigned& counts, unsigned& maxbits) {
    const unsigned mag = __float_as_uint(y) & 0x7fffffffu;
    const bool finite = mag < 0x7f800000u;
    const bool clips = y >= PCM16_CLIPS_FROM || y <= PCM16_CLIPS_DOWN_FROM;        // (false for a NaN)
    counts += finite ? (clips ? 0x10000u : 0u) : 1u;
    maxbits = (finite && mag > maxbits) ? mag : maxbits;
}
