// fastsvc_pack.h - the job table of the device-side weight packer (fastsvc_pack.hip), shared by the host code that builds
// it once per plan (fastsvc_plan.cpp: build_pack_table) and the kernels that read it.
//
// The packer's jobs are DATA: what fastsvc_pack_weights walks as lists of lambdas (pack_jobs, chain_jobs, xr_jobs,
// film_chain_jobs, up_head_jobs, cond_bound_jobs, raw_jobs) is flattened into arrays of the records below, one array per
// kernel, so that a pack is one launch per kernel whatever the number of layers.  The table depends on the generator's
// configuration only.  It is copied into the caller's scratch at the start of every pack (the scratch is the caller's and
// may hold anything), from a page-locked copy the plan makes at its first device pack.
//
// All offsets are in FLOATS: `s_*` into the scratch, `d_*` into the blob.  Every record's `work0` is the first work item
// (one thread each) of the job in its kernel's launch; the work of a job is rounded up to a multiple of PK_BLOCK, so a
// block never straddles two jobs.
#ifndef FASTSVC_PACK_H
#define FASTSVC_PACK_H

#include <stddef.h>
#include <stdint.h>

namespace fastsvc_pack {

constexpr int PK_BLOCK = 256;
constexpr uint32_t PK_NONE = 0xffffffffu;
constexpr int PK_PTR_LAYERS = 160;          // layers per launch of the two kernels that read the caller's tensors

// One state-dict layer (fetch_layer): bias (cout), weight or weight_v (cout x per), weight_g (cout) or none.
struct PkLayer {
    uint32_t cout, per;
    uint32_t s_bias;                        // copy of the bias
    uint32_t s_sc;                          // g / ||v|| per output channel (weight-norm layout only)
    uint32_t s_w;                           // the folded dense weight (cout x per), what HostLayer::w is on the host
};

// The tensors of PK_PTR_LAYERS layers, in the kernel arguments: [3 l] bias, [3 l + 1] weight or weight_v, [3 l + 2]
// weight_g or null (null = the state dict holds the folded `.weight`).
struct PkPtrs {
    const float* p[3 * PK_PTR_LAYERS];
};

// A dense matrix W[rows][cin][ntaps] assembled from up to four layers (FiLM heads: four C x C blocks; the block-diagonal
// first conv of the fused FiLM net: two), zero elsewhere.
struct PkVirt {
    uint32_t work0, s_dst, rows, cin, ntaps, npieces;
    struct { uint32_t s_src, co_off, ci_off, rows, cin; } piece[4];
};

// float32 fragments [group][q][lane][m] (pack_fragments, pack_wino, MODE_DEC2)
enum { PK_FRAG_PLAIN = 0, PK_FRAG_POLY = 1, PK_FRAG_WINO = 2, PK_FRAG_DEC2 = 3 };
struct PkFrag {
    uint32_t work0, d_dst, s_src, s_src1;   // s_src1: the 1x1 conv of MODE_DEC2
    uint32_t cout, cin, ntaps, KC, MW, Q, ngroups, kind;
};

// Half-precision fragments (pack_hx): a job's virtual input-channel axis is `nch` units of 32 channels; unit u reads
// channels [cj0, cj0 + 32) of one dense matrix (row pitch ld channels, 3 taps), those >= lim are zero.
enum { PK_HX_PLAIN = 0, PK_HX_POLY = 1, PK_HX_DEC2 = 2 };
struct PkHxUnit {
    uint32_t s_src, s_src1, ld, cj0, lim, kind, table;     // table: which scale table the unit's fragments use (DEC2: + 1 for slot 3)
};
struct PkHx {
    uint32_t work0;                         // fragments kernel: one item per (group, unit, slot, tile, lane)
    uint32_t row0;                          // exponent kernel: one item per (table, channel of n16)
    uint32_t d_off[3];                      // split-binary16 / bfloat16 / binary16 sets (0 = absent)
    uint32_t d_inv;                         // inverse scale tables (0 = none: unscaled)
    uint32_t s_ex;                          // exponents [table][n16], int32
    uint32_t ntables, nslots, MW, ngroups, nch, cout, unit0;
};

// dst[i] = a[i] (mode 0), 0.f + a[i] (mode 1), (0.f + a[i]) + b[i] (mode 2): raw weights, bias rows, the heads' bias sums
struct PkCopy {
    uint32_t work0, d_dst, n, s_a, s_b, mode;
};

// (l1, bmax): largest float64 row sum of |W| and largest |bias| over `rows` rows; bias of row r = a[h][r - h * half]
// (+ b[h][...] unless PK_NONE), h = r >= half.  rows = 0 writes (0, 0).
struct PkBound {
    uint32_t d_dst, s_w, rows, per, half, s_a[2], s_b[2];
};

// per-channel (alpha, beta) recurrences of one conditioning stage and signal (cond_bound_jobs)
struct PkCond {
    uint32_t d_dst, C, Cin, s_tmp;          // s_tmp: 4 C doubles (8-byte aligned)
    uint32_t s_w[5], s_b[5];                // downsample_block.2, residual_block.0, downsample_block.4, .6, film conv
};

struct PkHeader {
    uint32_t n_layers, layers;              // (count, byte offset of the array in the table)
    uint32_t n_virt, virts, virt_work;
    uint32_t n_frag, frags, frag_work;
    uint32_t n_hx, hxs, hx_units, hx_work, hx_rows;
    uint32_t n_copy, copies, copy_work;
    uint32_t n_bound, bounds;
    uint32_t n_cond, conds;
    uint32_t max_rows, max_w;               // largest cout / cout * per of a layer
    uint32_t table_off, table_bytes;        // the table's place in the scratch: behind the arena
};

// Enqueues one pack on `stream` (hipStream_t): table -> scratch, zero the blob, fold, assemble, every format.
// `ptrs`: 3 device pointers per layer (PkPtrs order).  Returns 0 or the hipError_t of the first failed call.
int launch_pack(const PkHeader& h, const void* pinned_table, const float* const* ptrs, void* dev_blob, size_t blob_bytes,
                void* scratch, void* stream, int* n_launches);

}  // namespace fastsvc_pack

#endif
