// fastsvc_collate.hip - one launch cuts a whole training batch out of a resident corpus on gfx950
// (train_session.TrainSession; the counterpart of fastsvc_decodeio.hip on the training side).
//
// The reference makes a batch on the host, in DataLoader workers (Collater.__call__, train_fastsvc.py:484-551): per
// utterance one random start frame, four numpy slices (wave, lft at the sample rate; f0, ppg at the frame rate), then
// np.array + transpose.  Here the corpus is uploaded once as five packed float32 buffers - utterance u has n_u frames and
// starts at frame frame_off[u]:
//     f0    [frame_off[u], +n_u)
//     ppg   time-major (n_u, D) at element frame_off[u] * D        (the dump's own layout, as in DecodeSession)
//     wave, lft   n_u * hop samples at frame_off[u] * hop
//     emb   (U, S)
// and batch row b = (utt[b], start[b]) becomes, with T = frames * hop and W = frames + 2 ctx,
//     y[b, 0, :]       wave_u[start * hop, +T)
//     lft_out[b, 0, :] lft_u [start * hop, +T)
//     f0_out[b, 0, :]  f0_u  [start, +frames)
//     ppg_out[b, :, :] ppg_u [start - ctx, +W) transposed to channel-major (D, W)
//     emb_out[b, :]    emb[u, :]
// Pure data movement: bit-identical to the numpy slices.  A recipe-size batch is tiny (32 x 16000 samples twice, 32 x 100 x
// 144 ppg values: 6 MB), so what it costs is launches, not bytes - stock tensor ops need four slice copies per row plus a
// transpose, more than 128 launches for a batch of 32; this is ONE launch per 64 rows.
//
// Block roles, by blockIdx.x range (uniform per block):
//     [0, n_wave)           row copies of y and lft   (1024 elements per block)
//     [.., + n_tile)        64 x 64 ppg transpose tiles through LDS
//     [.., + n_f0)          row copies of f0
//     [.., + n_emb)         row copies of emb          (absent when emb is null: use_spk_emb False)
// Row descriptors (frame offset, start frame, utterance) travel IN the kernel arguments, 64 rows per launch, like
// TimeMajorArgs in fastsvc_decodeio.hip: a device table would be one more small upload per batch.
//
// Requests.  A row copy gives every lane one 16-byte ALIGNED piece of the destination row (the pieces before the first
// and after the last boundary inside the row are clipped and go out element by element, so no byte outside the row is
// written); the piece's four source elements are one 16-byte load when their address is a multiple of 16 too, else four
// 4-byte loads - of the same four elements, so no load leaves the crop's own source range either (a crop that ends at
// the store's last element reads nothing behind it).  Source and destination agree mod 16 whenever hop % 4 == 0 and
// the utterance's block starts on a 16-byte boundary (the session aligns blocks to 4 frames); odd hops, T % 4 != 0 and
// unaligned blocks take the element loads and stay exact.  The transpose reads 16 bytes per lane along D when
// D % 4 == 0 and the crop's first ppg element is 16-byte aligned (then c + 3 < D for every piece it reads), else 4
// bytes per lane, and writes 16 bytes per lane along time where the destination row allows - the fill / drain pattern
// and the 65-dword pitch of fastsvc_decodeio.hip:30-46 (bank of (c, t) = (c + t) % 32: both 16-byte phases 2-way, the
// element-wise fill conflict-free; an even pitch would be 4-way or worse).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "fastsvc_hip.h"

namespace fastsvc {
int set_last_error(int code, const char* msg);      // fastsvc_plan.cpp: the text fastsvc_last_error() returns
}

namespace {

constexpr int CL_MAX = 64;                          // rows per launch (the arguments hold their descriptors)
constexpr int CL_TILE = 64;
constexpr int CL_PITCH = 65;
constexpr int CL_CHUNK = 1024;                      // elements of a row one copy block covers (256 lanes x 16 bytes)

struct CollateArgs {
    long foff[CL_MAX];                              // frame_off[utt[b]]
    int start[CL_MAX];                              // start frame of row b inside its utterance
    int utt[CL_MAX];                                // row of `emb`
};

struct CollateDims {
    int nb, D, S, hop, frames, ctx;
    int wave_chunks, f0_chunks, emb_chunks;         // copy blocks per row
    int tiles_t, tiles_c;                           // ppg tiles per row
    unsigned n_wave, n_tile, n_f0;                  // blocks of the first three roles
};

__host__ __device__ inline int row_chunks(long len) { return (int)((len + 3 + CL_CHUNK - 1) / CL_CHUNK); }

// Lane `tid` of copy block `chunk` owns one 16-byte aligned piece of dst[0, len): with s = elements between the previous
// 16-byte boundary and dst, piece g = chunk * 256 + tid holds elements [4 g - s, 4 g - s + 4) clipped to [0, len).
__device__ __forceinline__ void copy_piece(const float* __restrict__ src, float* __restrict__ dst, int len, int chunk, int tid) {
    const int s = (int)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3);
    const long k0 = ((long)chunk * 256 + tid) * 4 - s;
    if (k0 >= len) return;
    if (k0 >= 0 && k0 + 4 <= len) {
        float4 v;
        if ((reinterpret_cast<uintptr_t>(src + k0) & 15) == 0) {
            v = *reinterpret_cast<const float4*>(src + k0);
        } else {
            v.x = src[k0]; v.y = src[k0 + 1]; v.z = src[k0 + 2]; v.w = src[k0 + 3];
        }
        *reinterpret_cast<float4*>(dst + k0) = v;
    } else {
        #pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long k = k0 + e;
            if (k >= 0 && k < len) dst[k] = src[k];
        }
    }
}

__global__ __launch_bounds__(256)
void collate_crops_kernel(CollateArgs a, CollateDims d, const float* __restrict__ wave, const float* __restrict__ lft,
                          const float* __restrict__ ppg, const float* __restrict__ f0, const float* __restrict__ emb,
                          float* __restrict__ y, float* __restrict__ lft_out, float* __restrict__ ppg_out,
                          float* __restrict__ f0_out, float* __restrict__ emb_out) {
    __shared__ float tile[CL_TILE * CL_PITCH];
    const int tid = threadIdx.x;
    unsigned blk = blockIdx.x;
    if (blk < d.n_wave) {                           // ---- y / lft: row b, buffer `which`, chunk
        const int chunk = (int)(blk % (unsigned)d.wave_chunks);
        const unsigned r = blk / (unsigned)d.wave_chunks;
        const int which = (int)(r & 1), b = (int)(r >> 1);
        const int T = d.frames * d.hop;
        const long so = (a.foff[b] + a.start[b]) * (long)d.hop;
        copy_piece((which ? lft : wave) + so, (which ? lft_out : y) + (long)b * T, T, chunk, tid);
        return;
    }
    blk -= d.n_wave;
    if (blk < d.n_tile) {                           // ---- ppg: a 64 (time) x 64 (channel) tile of row b
        const int W = d.frames + 2 * d.ctx, D = d.D;
        const int per_row = d.tiles_t * d.tiles_c;
        const int b = (int)(blk / (unsigned)per_row), q = (int)(blk % (unsigned)per_row);
        const int c0 = (q / d.tiles_t) * CL_TILE, t0 = (q % d.tiles_t) * CL_TILE;
        const float* s = ppg + (a.foff[b] + a.start[b] - d.ctx) * (long)D;
        if ((D & 3) == 0 && (reinterpret_cast<uintptr_t>(s) & 15) == 0) {
            const int cl = tid & 15, tl = tid >> 4;
            const int c = c0 + 4 * cl;
            #pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int tt = tl + 16 * p, t = t0 + tt;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (t < W && c < D) v = *reinterpret_cast<const float4*>(s + (long)t * D + c);    // (D % 4 == 0: c + 3 < D)
                float* w = tile + (4 * cl) * CL_PITCH + tt;
                w[0] = v.x; w[CL_PITCH] = v.y; w[2 * CL_PITCH] = v.z; w[3 * CL_PITCH] = v.w;
            }
        } else {
            const int cc = tid & 63, tl = tid >> 6;
            const int c = c0 + cc;
            #pragma unroll 4
            for (int p = 0; p < 16; ++p) {
                const int tt = tl + 4 * p, t = t0 + tt;
                tile[cc * CL_PITCH + tt] = (t < W && c < D) ? s[(long)t * D + c] : 0.f;
            }
        }
        __syncthreads();
        const int tq = tid & 15, cr = tid >> 4;
        const int t = t0 + 4 * tq;
        if (t >= W) return;
        #pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int cc = cr + 16 * p, c = c0 + cc;
            if (c >= D) break;
            const float* r = tile + cc * CL_PITCH + 4 * tq;
            float v[4];
            #pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = r[e];
            float* o = ppg_out + ((long)b * D + c) * W + t;
            if (t + 3 < W && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
                *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                #pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (t + e < W) o[e] = v[e];
            }
        }
        return;
    }
    blk -= d.n_tile;
    if (blk < d.n_f0) {                             // ---- f0
        const int chunk = (int)(blk % (unsigned)d.f0_chunks), b = (int)(blk / (unsigned)d.f0_chunks);
        copy_piece(f0 + a.foff[b] + a.start[b], f0_out + (long)b * d.frames, d.frames, chunk, tid);
        return;
    }
    blk -= d.n_f0;                                  // ---- emb (these blocks exist only when emb is given)
    const int chunk = (int)(blk % (unsigned)d.emb_chunks), b = (int)(blk / (unsigned)d.emb_chunks);
    if (b < d.nb) copy_piece(emb + (long)a.utt[b] * d.S, emb_out + (long)b * d.S, d.S, chunk, tid);
}

int invalid(const char* fmt, long a = 0, long b = 0, long c = 0, long e = 0) {
    char buf[200];
    snprintf(buf, sizeof buf, fmt, a, b, c, e);
    return fastsvc::set_last_error(FASTSVC_E_INVALID, buf);
}

}  // namespace

extern "C" {

int fastsvc_collate_launch_count(int32_t B) { return B < 1 ? 0 : (B + CL_MAX - 1) / CL_MAX; }

int fastsvc_collate_crops(const float* wave, const float* lft, int64_t wave_elems, const float* ppg, int64_t ppg_elems,
                          const float* f0, int64_t f0_elems, const float* emb, int32_t n_utts,
                          const int64_t* frame_off, const int32_t* n_frames, const int32_t* utt, const int32_t* start,
                          float* y, float* lft_out, float* ppg_out, float* f0_out, float* emb_out,
                          int32_t B, int32_t D, int32_t S, int32_t hop, int32_t frames, int32_t ctx, void* stream_) {
    if (!wave || !lft || !ppg || !f0 || !frame_off || !n_frames || !utt || !start || !y || !lft_out || !ppg_out || !f0_out)
        return invalid("fastsvc_collate_crops: null pointer");
    if (emb && !emb_out) return invalid("fastsvc_collate_crops: emb given without emb_out");
    if (B < 1 || D < 1 || hop < 1 || frames < 1 || ctx < 0 || n_utts < 1 || (emb && S < 1) || wave_elems < 0 || ppg_elems < 0 || f0_elems < 0)
        return invalid("fastsvc_collate_crops: size out of range (B %ld, D %ld, hop %ld, frames %ld)", B, D, hop, frames);
    const int64_t T = (int64_t)frames * hop, W = (int64_t)frames + 2 * (int64_t)ctx;
    if (T > INT32_MAX || W > INT32_MAX || W * D > INT32_MAX) return invalid("fastsvc_collate_crops: crop too large (T %ld, W %ld)", T, W);
    const float* ptrs[] = {wave, lft, ppg, f0, emb, y, lft_out, ppg_out, f0_out, emb_out};
    for (const float* p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) & 3) return invalid("fastsvc_collate_crops: pointers must be 4-byte aligned");
    for (int b = 0; b < B; ++b) {
        const int u = utt[b];
        if (u < 0 || u >= n_utts) return invalid("fastsvc_collate_crops: row %ld: utterance %ld outside [0, %ld)", b, u, n_utts);
        const int64_t off = frame_off[u], n = n_frames[u];
        if (off < 0 || n < 0 || off + n > f0_elems || (off + n) > wave_elems / hop || (off + n) > ppg_elems / D)
            return invalid("fastsvc_collate_crops: row %ld: utterance %ld (frames [%ld, +%ld)) leaves its buffer", b, u, off, n);
        if (start[b] < ctx || (int64_t)start[b] > n - frames - ctx)
            return invalid("fastsvc_collate_crops: row %ld: start %ld outside [ctx, %ld] of utterance %ld", b, start[b], n - frames - ctx, u);
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    for (int b0 = 0; b0 < B; b0 += CL_MAX) {
        const int nb = B - b0 < CL_MAX ? B - b0 : CL_MAX;
        CollateArgs a;
        for (int i = 0; i < CL_MAX; ++i) {
            const bool on = i < nb;
            a.utt[i] = on ? utt[b0 + i] : 0;
            a.foff[i] = on ? (long)frame_off[utt[b0 + i]] : 0;
            a.start[i] = on ? start[b0 + i] : 0;
        }
        CollateDims d;
        d.nb = nb; d.D = D; d.S = S; d.hop = hop; d.frames = frames; d.ctx = ctx;
        d.wave_chunks = row_chunks(T);
        d.f0_chunks = row_chunks(frames);
        d.emb_chunks = emb ? row_chunks(S) : 1;
        d.tiles_t = (int)((W + CL_TILE - 1) / CL_TILE);
        d.tiles_c = (D + CL_TILE - 1) / CL_TILE;
        const int64_t n_wave = 2 * (int64_t)nb * d.wave_chunks, n_tile = (int64_t)nb * d.tiles_t * d.tiles_c;
        const int64_t n_f0 = (int64_t)nb * d.f0_chunks, n_emb = emb ? (int64_t)nb * d.emb_chunks : 0;
        if (n_wave + n_tile + n_f0 + n_emb > INT32_MAX) return invalid("fastsvc_collate_crops: grid too large");
        d.n_wave = (unsigned)n_wave; d.n_tile = (unsigned)n_tile; d.n_f0 = (unsigned)n_f0;
        hipLaunchKernelGGL(collate_crops_kernel, dim3((unsigned)(n_wave + n_tile + n_f0 + n_emb)), dim3(256), 0, stream,
                           a, d, wave, lft, ppg, f0, emb, y + (long)b0 * T, lft_out + (long)b0 * T,
                           ppg_out + (long)b0 * D * W, f0_out + (long)b0 * frames, emb ? emb_out + (long)b0 * S : nullptr);
    }
    return hipGetLastError() == hipSuccess ? FASTSVC_OK : fastsvc::set_last_error(FASTSVC_E_HIP, "fastsvc_collate_crops: launch failed");
}

}  // extern "C"
