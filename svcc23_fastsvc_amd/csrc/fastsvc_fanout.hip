// fastsvc_fanout.hip - one launch assembles a decode batch whose rows are (utterance, target speaker) pairs, out of the
// buffers a resident decode session holds on gfx950 (decode.DecodeSession.convert_many; the decode-side counterpart of
// fastsvc_collate.hip).
//
// The reference converts one utterance to one speaker at a time on the host (decode_fastsvc.py:150-200: F0Statistics.convert
// in float64 numpy, a numpy transpose, the speaker's embedding repeated).  A session keeps ppg and lft packed on the device
// (fastsvc_decodeio.hip); with f0 packed next to them, batch row r = (utt[r], spk[r]) becomes
//     ppg_out[r, :, :]   utterance's time-major (frames, C) block transposed to channel-major, columns >= frames zero
//                        (gather_time_major's bits)
//     lft_out[r, 0, :]   utterance's frames * hop samples, then zeros                     (gather_padded's bits)
//     f0_out[r, 0, :]    utterance's f0 moved to the speaker's log-F0 statistics, then zeros
//     emb_out[r, :]      row spk[r] of the speaker table
// so a batch can hold one utterance for many speakers, and what depends on the speaker - the F0 shift and the embedding -
// is made here instead of once per (utterance, speaker) on the host.  Apart from the F0 transform this is data movement;
// what a small batch costs is launches, and this is ONE launch per 64 rows where the session's own path needs two
// assembly launches, a host loop over the utterances and an f0 upload per batch.
//
// F0 transform (F0Statistics.convert, features.py:88-108): a voiced frame (f > 0) becomes
//     (float) exp((s1 / s0) * (log((double) f) - m0) + m1)
// with (m0, s0) the utterance's source statistics and (m1, s1) the speaker's - every operation a separately rounded IEEE
// double operation in that order: this unit is compiled with -ffp-contract=off, so the multiply and the add are not
// fused.  Unvoiced frames (f <= 0 or NaN) and the padding are exactly 0.  log and exp are the device library's
// double-precision ones (not correctly rounded, like the host's); the float32 result is within one ulp of the host's.
//
// Block roles, by blockIdx.x range (uniform per block):
//     [0, n_lft)            padded row copies of lft   (1024 destination elements per block)
//     [.., + n_tile)        64 x 64 ppg transpose tiles through LDS
//     [.., + n_f0)          padded row copies of f0, transformed
//     [.., + n_emb)         row copies of emb          (absent when the speaker table is null)
// Row descriptors (the three block offsets, the frame count, utterance and speaker) travel IN the kernel arguments, 64
// rows per launch, like CollateArgs: 36 bytes a row, 2.3 KB of the 4 KB argument segment.  The statistics are two small
// device tables of doubles, (n_utts, 2) and (n_spk, 2), indexed by the row's utterance and speaker.
//
// Requests.  A row copy gives every lane one 16-byte ALIGNED piece of the destination row (the pieces before the first and
// after the last boundary inside the row are clipped and go out element by element: no byte outside the row is written);
// a piece that lies inside the source block loads its four elements as one 16-byte request when their address is a
// multiple of 16 too, else as four 4-byte ones; a piece that straddles the block's end loads only the elements inside
// it, and a piece past it loads nothing - no load leaves the row's own source block.  The transpose is
// gather_time_major's (fastsvc_decodeio.hip:30-46): 16 bytes per lane along C when C % 4 == 0 and the block is 16-byte
// aligned, else 4; 16 bytes per lane along time where the destination allows; LDS pitch 65 dwords (bank of (c, t) =
// (c + t) % 32: both 16-byte phases 2-way, the element-wise fill conflict-free).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "fastsvc_hip.h"

namespace fastsvc {
int set_last_error(int code, const char* msg);      // fastsvc_plan.cpp: the text fastsvc_last_error() returns
}

namespace {

constexpr int FO_MAX = 64;                          // rows per launch (the arguments hold their descriptors)
constexpr int FO_TILE = 64;
constexpr int FO_PITCH = 65;
constexpr int FO_CHUNK = 1024;                      // elements of a row one copy block covers (256 lanes x 16 bytes)

struct FanoutArgs {
    long ppg_off[FO_MAX];                           // first element of the row's (frames, C) block in `ppg`
    long lft_off[FO_MAX];                           // first of its frames * hop samples in `lft`
    long f0_off[FO_MAX];                            // first of its frames values in `f0`
    int frames[FO_MAX];
    int utt[FO_MAX];                                // row of `src_stats`
    int spk[FO_MAX];                                // row of `spk_stats` and of `spk_emb`
};

struct FanoutDims {
    int nb, C, E, hop, width;
    int lft_chunks, f0_chunks, emb_chunks;          // copy blocks per row
    int tiles_t, tiles_c;                           // ppg tiles per row
    unsigned n_lft, n_tile, n_f0;                   // blocks of the first three roles
};

inline int row_chunks(long len) { return (int)((len + 3 + FO_CHUNK - 1) / FO_CHUNK); }

struct Identity {
    __device__ __forceinline__ float operator()(float f) const { return f; }
};

// F0Statistics.convert for one frame; `ratio` = s1 / s0 (one double division, the same in every lane).
struct ShiftF0 {
    double m0, ratio, m1;
    __device__ __forceinline__ float operator()(float f) const {
        if (!(f > 0.f)) return 0.f;
        const double l = log((double)f);
        const double d = l - m0;
        const double p = ratio * d;
        const double s = p + m1;
        return (float)exp(s);
    }
};

// Lane `tid` of copy block `chunk` owns one 16-byte aligned piece of dst[0, width): with s = elements between the
// previous 16-byte boundary and dst, piece g = chunk * 256 + tid holds elements [4 g - s, 4 g - s + 4) clipped to
// [0, width).  Element k is op(src[k]) for k < len and 0 from len on; src is read at [0, len) only.
template <class Op>
__device__ __forceinline__ void padded_piece(const float* __restrict__ src, float* __restrict__ dst, int len, int width,
                                             int chunk, int tid, Op op) {
    const int s = (int)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3);
    const long k0 = ((long)chunk * 256 + tid) * 4 - s;
    if (k0 >= width) return;
    if (k0 >= 0 && k0 + 4 <= width) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k0 + 4 <= len) {
            if ((reinterpret_cast<uintptr_t>(src + k0) & 15) == 0) {
                v = *reinterpret_cast<const float4*>(src + k0);
            } else {
                v.x = src[k0]; v.y = src[k0 + 1]; v.z = src[k0 + 2]; v.w = src[k0 + 3];
            }
            v.x = op(v.x); v.y = op(v.y); v.z = op(v.z); v.w = op(v.w);
        } else if (k0 < len) {                      // (the piece that holds the block's end: 1 - 3 elements of it)
            v.x = op(src[k0]);
            if (k0 + 1 < len) v.y = op(src[k0 + 1]);
            if (k0 + 2 < len) v.z = op(src[k0 + 2]);
        }
        *reinterpret_cast<float4*>(dst + k0) = v;
    } else {
        #pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long k = k0 + e;
            if (k >= 0 && k < width) dst[k] = k < len ? op(src[k]) : 0.f;
        }
    }
}

__global__ __launch_bounds__(256)
void fanout_assemble_kernel(FanoutArgs a, FanoutDims d, const float* __restrict__ ppg, const float* __restrict__ lft,
                            const float* __restrict__ f0, const double* __restrict__ src_stats,
                            const double* __restrict__ spk_stats, const float* __restrict__ spk_emb,
                            float* __restrict__ ppg_out, float* __restrict__ lft_out, float* __restrict__ f0_out,
                            float* __restrict__ emb_out) {
    __shared__ float tile[FO_TILE * FO_PITCH];
    const int tid = threadIdx.x;
    unsigned blk = blockIdx.x;
    if (blk < d.n_lft) {                            // ---- lft: row b, chunk
        const int chunk = (int)(blk % (unsigned)d.lft_chunks), b = (int)(blk / (unsigned)d.lft_chunks);
        const int W = d.width * d.hop;
        padded_piece(lft + a.lft_off[b], lft_out + (long)b * W, a.frames[b] * d.hop, W, chunk, tid, Identity());
        return;
    }
    blk -= d.n_lft;
    if (blk < d.n_tile) {                           // ---- ppg: a 64 (time) x 64 (channel) tile of row b
        const int C = d.C, width = d.width;
        const int per_row = d.tiles_t * d.tiles_c;
        const int b = (int)(blk / (unsigned)per_row), q = (int)(blk % (unsigned)per_row);
        const int c0 = (q / d.tiles_t) * FO_TILE, t0 = (q % d.tiles_t) * FO_TILE;
        const int len = a.frames[b];
        const bool live = t0 < len;                 // (uniform per block) a tile past the utterance's end is all padding
        if (live) {
            const float* s = ppg + a.ppg_off[b];
            if ((C & 3) == 0 && (reinterpret_cast<uintptr_t>(s) & 15) == 0) {
                const int cl = tid & 15, tl = tid >> 4;
                const int c = c0 + 4 * cl;
                #pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int tt = tl + 16 * p, t = t0 + tt;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (t < len && c < C) v = *reinterpret_cast<const float4*>(s + (long)t * C + c);   // (C % 4 == 0: c + 3 < C)
                    float* w = tile + (4 * cl) * FO_PITCH + tt;
                    w[0] = v.x; w[FO_PITCH] = v.y; w[2 * FO_PITCH] = v.z; w[3 * FO_PITCH] = v.w;
                }
            } else {
                const int cc = tid & 63, tl = tid >> 6;
                const int c = c0 + cc;
                #pragma unroll 4
                for (int p = 0; p < 16; ++p) {
                    const int tt = tl + 4 * p, t = t0 + tt;
                    tile[cc * FO_PITCH + tt] = (t < len && c < C) ? s[(long)t * C + c] : 0.f;
                }
            }
            __syncthreads();
        }
        const int tq = tid & 15, cr = tid >> 4;
        const int t = t0 + 4 * tq;
        if (t >= width) return;
        #pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int cc = cr + 16 * p, c = c0 + cc;
            if (c >= C) break;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (live) {
                const float* r = tile + cc * FO_PITCH + 4 * tq;         // (the fill wrote zeros at t >= len)
                #pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = r[e];
            }
            float* o = ppg_out + ((long)b * C + c) * width + t;
            if (t + 3 < width && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
                *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                #pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (t + e < width) o[e] = v[e];
            }
        }
        return;
    }
    blk -= d.n_tile;
    if (blk < d.n_f0) {                             // ---- f0
        const int chunk = (int)(blk % (unsigned)d.f0_chunks), b = (int)(blk / (unsigned)d.f0_chunks);
        const float* s = f0 + a.f0_off[b];
        float* o = f0_out + (long)b * d.width;
        if (src_stats && spk_stats) {               // (uniform: both tables or a plain copy)
            const double* s0 = src_stats + 2 * (long)a.utt[b];
            const double* s1 = spk_stats + 2 * (long)a.spk[b];
            ShiftF0 op;
            op.m0 = s0[0];
            op.ratio = s1[1] / s0[1];
            op.m1 = s1[0];
            padded_piece(s, o, a.frames[b], d.width, chunk, tid, op);
        } else {
            padded_piece(s, o, a.frames[b], d.width, chunk, tid, Identity());
        }
        return;
    }
    blk -= d.n_f0;                                  // ---- emb (these blocks exist only when the table is given)
    const int chunk = (int)(blk % (unsigned)d.emb_chunks), b = (int)(blk / (unsigned)d.emb_chunks);
    if (b < d.nb) padded_piece(spk_emb + (long)a.spk[b] * d.E, emb_out + (long)b * d.E, d.E, d.E, chunk, tid, Identity());
}

int invalid(const char* fmt, long a = 0, long b = 0, long c = 0, long e = 0) {
    char buf[200];
    snprintf(buf, sizeof buf, fmt, a, b, c, e);
    return fastsvc::set_last_error(FASTSVC_E_INVALID, buf);
}

}  // namespace

extern "C" {

int fastsvc_fanout_launch_count(int32_t R) { return R < 1 ? 0 : (R + FO_MAX - 1) / FO_MAX; }

int fastsvc_fanout_assemble(const float* ppg, int64_t ppg_elems, const float* lft, int64_t lft_elems,
                            const float* f0, int64_t f0_elems, int32_t n_utts,
                            const int64_t* ppg_off, const int64_t* lft_off, const int64_t* f0_off, const int32_t* n_frames,
                            const double* src_stats, const double* spk_stats, const float* spk_emb, int32_t n_spk,
                            const int32_t* utt, const int32_t* spk,
                            float* ppg_out, float* lft_out, float* f0_out, float* emb_out,
                            int32_t R, int32_t C, int32_t E, int32_t hop, int32_t width, void* stream_) {
    if (!ppg || !lft || !f0 || !ppg_off || !lft_off || !f0_off || !n_frames || !utt || !spk || !ppg_out || !lft_out || !f0_out)
        return invalid("fastsvc_fanout_assemble: null pointer");
    if (spk_emb && !emb_out) return invalid("fastsvc_fanout_assemble: spk_emb given without emb_out");
    if (R < 1 || C < 1 || hop < 1 || width < 1 || n_utts < 1 || n_spk < 1 || (spk_emb && E < 1) || ppg_elems < 0 ||
            lft_elems < 0 || f0_elems < 0)
        return invalid("fastsvc_fanout_assemble: size out of range (R %ld, C %ld, hop %ld, width %ld)", R, C, hop, width);
    if ((int64_t)width * hop > INT32_MAX || (int64_t)width * C > INT32_MAX)
        return invalid("fastsvc_fanout_assemble: row too large (width %ld, hop %ld, C %ld)", width, hop, C);
    const void* ptrs[] = {ppg, lft, f0, spk_emb, ppg_out, lft_out, f0_out, emb_out};
    for (const void* p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) & 3) return invalid("fastsvc_fanout_assemble: pointers must be 4-byte aligned");
    if ((reinterpret_cast<uintptr_t>(src_stats) | reinterpret_cast<uintptr_t>(spk_stats)) & 7)
        return invalid("fastsvc_fanout_assemble: statistics tables must be 8-byte aligned");
    for (int r = 0; r < R; ++r) {
        const int u = utt[r], s = spk[r];
        if (u < 0 || u >= n_utts) return invalid("fastsvc_fanout_assemble: row %ld: utterance %ld outside [0, %ld)", r, u, n_utts);
        if (s < 0 || s >= n_spk) return invalid("fastsvc_fanout_assemble: row %ld: speaker %ld outside [0, %ld)", r, s, n_spk);
        const int64_t n = n_frames[u];
        if (n < 0 || n > width)
            return invalid("fastsvc_fanout_assemble: row %ld: utterance %ld has %ld frames, outside [0, width %ld]", r, u, n, width);
        if (ppg_off[u] < 0 || n * C > ppg_elems - ppg_off[u] || ppg_off[u] > ppg_elems)
            return invalid("fastsvc_fanout_assemble: row %ld: ppg block of utterance %ld ([%ld, +%ld)) leaves its buffer", r, u, ppg_off[u], n * C);
        if (lft_off[u] < 0 || n * hop > lft_elems - lft_off[u] || lft_off[u] > lft_elems)
            return invalid("fastsvc_fanout_assemble: row %ld: lft block of utterance %ld ([%ld, +%ld)) leaves its buffer", r, u, lft_off[u], n * hop);
        if (f0_off[u] < 0 || n > f0_elems - f0_off[u] || f0_off[u] > f0_elems)
            return invalid("fastsvc_fanout_assemble: row %ld: f0 block of utterance %ld ([%ld, +%ld)) leaves its buffer", r, u, f0_off[u], n);
    }
    const int64_t W = (int64_t)width * hop;
    FanoutDims d;
    d.C = C; d.E = E; d.hop = hop; d.width = width;
    d.lft_chunks = row_chunks(W);
    d.f0_chunks = row_chunks(width);
    d.emb_chunks = spk_emb ? row_chunks(E) : 1;
    d.tiles_t = (width + FO_TILE - 1) / FO_TILE;
    d.tiles_c = (C + FO_TILE - 1) / FO_TILE;
    const int64_t per_row = (int64_t)d.lft_chunks + (int64_t)d.tiles_t * d.tiles_c + d.f0_chunks + (spk_emb ? d.emb_chunks : 0);
    if (per_row * (R < FO_MAX ? R : FO_MAX) > INT32_MAX) return invalid("fastsvc_fanout_assemble: grid too large");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    for (int b0 = 0; b0 < R; b0 += FO_MAX) {
        const int nb = R - b0 < FO_MAX ? R - b0 : FO_MAX;
        FanoutArgs a;
        for (int i = 0; i < FO_MAX; ++i) {
            const bool on = i < nb;
            const int u = on ? utt[b0 + i] : 0;
            a.utt[i] = u;
            a.spk[i] = on ? spk[b0 + i] : 0;
            a.frames[i] = on ? n_frames[u] : 0;
            a.ppg_off[i] = on ? (long)ppg_off[u] : 0;
            a.lft_off[i] = on ? (long)lft_off[u] : 0;
            a.f0_off[i] = on ? (long)f0_off[u] : 0;
        }
        d.nb = nb;
        d.n_lft = (unsigned)nb * (unsigned)d.lft_chunks;
        d.n_tile = (unsigned)nb * (unsigned)(d.tiles_t * d.tiles_c);
        d.n_f0 = (unsigned)nb * (unsigned)d.f0_chunks;
        hipLaunchKernelGGL(fanout_assemble_kernel, dim3((unsigned)(per_row * nb)), dim3(256), 0, stream,
                           a, d, ppg, lft, f0, src_stats, spk_stats, spk_emb, ppg_out + (long)b0 * C * width,
                           lft_out + (long)b0 * W, f0_out + (long)b0 * width, spk_emb ? emb_out + (long)b0 * E : nullptr);
    }
    return hipGetLastError() == hipSuccess ? FASTSVC_OK
                                           : fastsvc::set_last_error(FASTSVC_E_HIP, "fastsvc_fanout_assemble: launch failed");
}

}  // extern "C"
