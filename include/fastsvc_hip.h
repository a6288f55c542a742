/*
 * fastsvc_hip.h - C ABI of the MI355X-native FastSVC generator forward pass (gfx950 / CDNA4).
 *
 * Drop-in boundary for ONE path of lesterphillip/SVCC23_FastSVC (package `harana`):
 *
 *     harana/models/fastsvc.py:305-332   FastSVCGenerator.forward(x, s, l, spk_emb=None)
 *
 * plus the weight preparation that `decode_fastsvc.py:140-143` performs before it
 * (`load_model` -> `remove_weight_norm()` -> `.to(device)`).  The reference is pure Python on
 * PyTorch, so there is no FFI in it today; these entry points are what a ctypes / torch C++
 * binding inside `FastSVCGenerator.forward` binds (see INTEGRATION.md, and the binding shipped in
 * svcc23_fastsvc_amd/engine.py).
 *
 * Conventions
 *   - plain C types only; no torch types.  All tensors are contiguous float32, channel-major
 *     (B, C, T) exactly as the reference passes them (fastsvc.py:305-316).
 *   - device memory is owned by the caller (PyTorch's caching allocator in the shipped host
 *     code): the packed weight blob, the workspace, the inputs and the output.  The plan object
 *     is host-only and immutable after creation, so one plan may serve several devices/streams.
 *   - every launch is ordered with respect to the hipStream_t passed in; no hidden synchronisation - with ONE
 *     exception: large calls (from ~1.5e5 output samples) may fork kernels off the critical path onto a helper
 *     stream, forked from and joined back into that stream with events, and the helper streams / events of a
 *     (device, stream) pair are created, and the cost of a fork + join through them MEASURED (which synchronises
 *     the stream once), by the first such forward on that pair - or ahead of time by fastsvc_stream_prepare(),
 *     e.g. before graph capture (during capture nothing is created or measured: one stream).  Where the fork +
 *     join is slow the forward stays on the one stream.  fastsvc_stream_release() frees the pair's
 *     context (streams handed to forward must outlive it).  Concurrent forwards on DIFFERENT streams are
 *     independent; forwards issued from several host threads on the SAME stream are serialised while they enqueue.
 *   - return value 0 = success; negative = FASTSVC_E_*; fastsvc_last_error() gives the text.
 */
#ifndef FASTSVC_HIP_H
#define FASTSVC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FASTSVC_ABI_VERSION 1
#define FASTSVC_MAX_STAGES 8

enum {
    FASTSVC_OK = 0,
    FASTSVC_E_INVALID = -1,      /* bad argument / shape invariant violated (reference: ValueError / RuntimeError) */
    FASTSVC_E_MISSING = -2,      /* a state-dict tensor is missing or has the wrong element count */
    FASTSVC_E_WORKSPACE = -3,    /* workspace too small */
    FASTSVC_E_HIP = -4,          /* a HIP runtime call or kernel launch failed */
    FASTSVC_E_UNSUPPORTED = -5   /* valid in the reference, not implemented here */
};

/* Constructor kwargs of FastSVCGenerator (fastsvc.py:238-246; egs/svcc23/fastsvc1/conf/fastsvc.yaml:23-29). */
typedef struct fastsvc_config {
    int32_t in_channels;                              /* 144 */
    int32_t n_stages;                                 /* len(mid_channels) == len(upsampling_scales) = 4 */
    int32_t mid_channels[FASTSVC_MAX_STAGES];         /* 192, 96, 48, 24 */
    int32_t upsampling_scales[FASTSVC_MAX_STAGES];    /* 2, 4, 4, 5 */
    int32_t out_channels;                             /* 1 */
    int32_t spk_emb_size;                             /* 512 */
    int32_t use_spk_emb;                              /* 1 */
} fastsvc_config;

/* One entry of the generator's state_dict, host memory, float32.  `name` is the reference key
 * (SURVEY.md 8(b)), e.g. "upsampling_nets.0.conv_first.weight_g". */
typedef struct fastsvc_tensor {
    const char* name;
    const float* data;
    int64_t numel;
} fastsvc_tensor;

typedef struct fastsvc_plan fastsvc_plan;   /* opaque, host-only */

int fastsvc_abi_version(void);
const char* fastsvc_last_error(void);       /* thread-local text of the last failure */

/* Replaces FastSVCGenerator.__init__ (fastsvc.py:238-303): builds the layer table, the packed
 * weight-blob layout and the workspace layout.  No GPU needed. */
int fastsvc_plan_create(const fastsvc_config* cfg, fastsvc_plan** out_plan);
void fastsvc_plan_destroy(fastsvc_plan* plan);

/* Activation storage in the workspace: 0 = float32 (default; the parity path), 1 = bfloat16 - every
 * intermediate tensor (conv outputs, FiLM-affined tensors, scale / shift) is stored as bfloat16, which
 * halves the traffic of the HBM-bound layers and the workspace; arithmetic (fp32 MFMA), weights,
 * InstanceNorm sums, inputs and output stay float32.  Accuracy is that of bf16 activations (about 1e-2
 * of the output range), so this is the mode for BASELINE config 3, not for the 1e-3 parity bar.
 * Set it before fastsvc_workspace_bytes / fastsvc_forward; needs F % 4 == 0 and the yaml channel counts.
 *
 * 2 = float16 (IEEE binary16): the same tensors, the same 2 bytes per element (workspace size, layout, taps and
 * HBM traffic are those of bfloat16 storage) with 11 significand bits instead of 8; one
 * v_mfma_f32_16x16x32_f16 per product on binary16-rounded weights and activations, every store rounds to nearest
 * even.  What stays float32 / float64 is what stays so in bfloat16 storage: accumulators, InstanceNorm sums, FiLM
 * arithmetic, the inputs (ppg is copied to binary16 in the workspace; sine, lft, spk_emb are read as they are) and
 * the output.  Accuracy (measured on an MI355X against the float64 oracle, DESIGN.md "float16 activation storage"):
 * 8 x 600 frames of the yaml generator, mean-abs 8.7e-4 and max-abs 1.3e-2 on a waveform of range 4.1, i.e. 2.1e-4 /
 * 3.1e-3 of the range - 7 to 8 times less than bfloat16 storage on the same inputs (6.8e-3 / 9.0e-2), about 30 PCM-16
 * steps where bfloat16 storage is off by 220; float32 storage stays two orders of magnitude closer still.
 * RANGE CONTRACT: the format is unscaled, so every workspace tensor of the call must stay below 65504 in magnitude,
 * and values under 2^-14 lose relative precision (subnormals, floor 2^-24).  Outside the contract nothing faults and
 * the call still returns FASTSVC_OK: an element past the ceiling is stored as an infinity, and infinities / NaNs
 * propagate to the output; no state survives the call (the next forward on the same workspace is unaffected).
 * The contract covers the WEIGHTS too: this mode multiplies unscaled binary16 copies of the folded weights, so a weight
 * above 65504 in magnitude is packed as an infinity and weights under 2^-14 lose relative precision (float32 storage
 * scales its binary16 weight pieces per output channel, bfloat16 has float32's range: neither has this limit).
 * float32 storage (0) scales its binary16 operands by measured maxima and has no such contract; bfloat16 storage has
 * float32's range.  Same needs as bfloat16 storage (F % 4 == 0, the yaml channel counts). */
int fastsvc_plan_set_storage(fastsvc_plan* plan, int32_t dtype);
int fastsvc_plan_get_storage(const fastsvc_plan* plan);

/* Size in bytes of the packed weight blob (device resident; also what rank 0 broadcasts over RCCL). */
size_t fastsvc_weight_blob_bytes(const fastsvc_plan* plan);

/* Replaces load_state_dict + remove_weight_norm (harana/utils/utils.py:243-280, fastsvc.py:342-352):
 * takes the state dict in EITHER layout - `<layer>.weight_g` + `<layer>.weight_v` (checkpoint
 * layout, folded here as w = g * v / ||v|| per output channel) or `<layer>.weight` (after
 * remove_weight_norm) - plus `<layer>.bias`, and writes the kernel-layout blob (MFMA fragment
 * order, FiLM heads concatenated, zero padded) into `host_blob` (fastsvc_weight_blob_bytes bytes,
 * host memory).  Pure host code; the caller uploads the blob.  strict: every tensor must be present. */
int fastsvc_pack_weights(const fastsvc_plan* plan, const fastsvc_tensor* tensors, int32_t n_tensors,
                         void* host_blob);

/* Device twin of fastsvc_pack_weights (csrc/fastsvc_pack.hip): `tensors[i].data` are DEVICE pointers (float32, contiguous)
 * on the current device; dev_blob receives fastsvc_weight_blob_bytes(plan) bytes, bit for bit what fastsvc_pack_weights
 * writes for the same values (one exception, unreachable from finite parameters: a NaN that the packing arithmetic itself
 * generates - an infinite folded weight, an all-zero weight_v row - has x86's sign bit on the host and none here);
 * scratch >= fastsvc_pack_device_scratch_bytes(plan), device memory, contents irrelevant (FASTSVC_E_WORKSPACE if smaller).
 * Names and element counts are checked on the host before anything is launched (FASTSVC_E_MISSING with the host packer's
 * messages; null arguments FASTSVC_E_INVALID).  Asynchronous on `stream`: no synchronisation and no device allocation;
 * the first call on a plan page-locks a copy of the plan's job table (host memory, freed with the plan), every call
 * copies it into the scratch.  dev_blob may be the blob that earlier forwards on `stream` read (stream order protects
 * them).  The number of launches (kernels, one copy, one memset) is fastsvc_pack_device_launch_count(plan): it depends
 * on the configuration only through ceil(layers / 160), a dozen for every generator that exists. */
size_t fastsvc_pack_device_scratch_bytes(const fastsvc_plan* plan);
int fastsvc_pack_device_launch_count(const fastsvc_plan* plan);
int fastsvc_pack_weights_device(const fastsvc_plan* plan, const fastsvc_tensor* tensors, int32_t n_tensors,
                                void* dev_blob, void* scratch, size_t scratch_bytes, void* stream);

/* Workspace layout of the plan's later fastsvc_workspace_bytes / fastsvc_forward calls: 0 (default) = every
 * intermediate has its own buffer (all fastsvc_workspace_tap tensors stay readable after a forward); 1 = compact,
 * intermediates of different stages whose lifetimes cannot overlap share buffers (about 40 % less at 64 x 10 s;
 * taps of shared buffers then hold the last stage's tensor).  Set it before sizing the workspace. */
int fastsvc_plan_set_workspace_mode(fastsvc_plan* plan, int32_t compact);

/* Device scratch needed by one forward of B utterances of F frames each (T = F * prod(scales)). */
size_t fastsvc_workspace_bytes(const fastsvc_plan* plan, int32_t B, int32_t F);

/* Replaces FastSVCGenerator.forward (fastsvc.py:305-332).
 *   ppg      (B, in_channels, F)   device
 *   sine     (B, 1, T)             device   T = F * prod(upsampling_scales)
 *   lft      (B, 1, T)             device
 *   spk_emb  (B, spk_emb_size)     device, or NULL (reference: spk_emb=None skips InstanceNorm and
 *                                  the speaker bias, fastsvc.py:134-140)
 *   out      (B, out_channels, T)  device, written
 *   lengths  NULL (all utterances F frames) or DEVICE pointer to B int32 frame counts, 1 <= lengths[b] <= F:
 *            a ragged batch.  Inputs and outputs keep the padded shapes above; utterance b is computed
 *            exactly as if it were run alone with lengths[b] frames (zero "same" padding at its own
 *            end, InstanceNorm over its own length); out[b, :, lengths[b]*hop:] is set to zero and the
 *            padding of the inputs is never read.  (The reference batches equal-length crops only.)
 *   dev_blob packed weights on the same device; workspace >= fastsvc_workspace_bytes(B, F)
 *   stream   hipStream_t (void* to keep this header free of HIP includes)
 * Launches are asynchronous on `stream`; the caller synchronises. */
int fastsvc_forward(const fastsvc_plan* plan, const void* dev_blob,
                    const float* ppg, const float* sine, const float* lft, const float* spk_emb,
                    float* out, int32_t B, int32_t F, const int32_t* lengths,
                    void* workspace, size_t workspace_bytes, void* stream);

/* fastsvc_forward with InstanceNorm statistics POOLED over groups of batch rows (csrc/fastsvc_normgroup.hip): what
 * decode.DecodeSession.convert_windowed(norm="utterance") runs the windows of one utterance through.  The reference
 * normalises whole utterances (fastsvc.py:134-139) and has no counterpart.  Arguments as fastsvc_forward, and
 *   group    DEVICE, B int32: the index of the FIRST row of row b's group (group[b] <= b, group[group[b]] == group[b])
 *   own_lo, own_hi   DEVICE, B int32 each, in frames: row b OWNS the frames [own_lo[b], own_hi[b]) of its lengths[b]
 *            (F without lengths) valid ones, 0 <= own_lo < own_hi <= lengths[b]
 *   scratch  DEVICE, >= fastsvc_norm_group_scratch_bytes(plan, B, F) bytes: the partial sums (not part of the workspace)
 * At each of the three norm points of every up block, behind whichever launch produced the tensor, sum u and sum u^2
 * are taken in float64 over the columns each row owns (chunks of 2048 columns from the start of the owned range, so a
 * row's partial sums do not depend on the batch; no floating-point atomics: two runs give the same bits), added over
 * the rows of the group in ascending (row, chunk) order and written to EVERY member row as S * len_b / N - len_b the
 * row's own column count, which the consuming convolution divides by, N the group's owned columns.  Each member is thus
 * normalised by the mean and biased variance of the group's owned columns.  Two extra launches per norm point.
 * A row that is alone in its group and owns all its frames is a PASS-THROUGH row: nothing is read or written for it,
 * and a batch of such rows gives fastsvc_forward's output bit for bit.  float32 storage: the bound the split-binary16
 * staging scale of a normalised row is derived from grows from sqrt(len_b) to sqrt(N) for the member rows.
 * spk_emb == NULL: there is no norm; the four extra arguments are ignored (may be NULL) and the launches and bytes are
 * fastsvc_forward's.  The device arrays cannot be checked here - values out of range are clamped to the row, never
 * followed outside it; the Python layer validates them on the host.  Too little scratch: FASTSVC_E_WORKSPACE. */
size_t fastsvc_norm_group_scratch_bytes(const fastsvc_plan* plan, int32_t B, int32_t F);
int fastsvc_forward_grouped(const fastsvc_plan* plan, const void* dev_blob,
                            const float* ppg, const float* sine, const float* lft, const float* spk_emb,
                            float* out, int32_t B, int32_t F, const int32_t* lengths,
                            const int32_t* group, const int32_t* own_lo, const int32_t* own_hi,
                            void* workspace, size_t workspace_bytes,
                            void* scratch, size_t scratch_bytes, void* stream);

/* The same two launches for ONE tensor u (B, C, ld) of `storage` (0 float32, 1 bfloat16, 2 float16 elements), rows of
 * lengths[b] * len_mul valid columns (lengths NULL: ld; ld a multiple of len_mul), row b owning the columns
 * [own_lo[b], own_hi[b]) * len_mul: stats_out (B, C, 2) float64 DEVICE receives S1 * len_b / N and S2 * len_b / N for
 * every row that is not a pass-through row; those rows' entries are left as they are.  No column at or beyond a row's
 * valid length or outside its owned range is read; no alignment requirement on ld or own_lo * len_mul.
 * scratch: DEVICE, >= B * C * ceil(ld / 2048) * 16 bytes.  All pointers DEVICE; asynchronous on `stream`. */
int fastsvc_norm_group_stats(const void* u, int32_t storage, int32_t B, int32_t C, int32_t ld, const int32_t* lengths,
                             int32_t len_mul, const int32_t* group, const int32_t* own_lo, const int32_t* own_hi,
                             double* stats_out, void* scratch, size_t scratch_bytes, void* stream);

/* fastsvc_forward with RUNNING InstanceNorm statistics, carried on the device from one forward to the next: what
 * decode.StreamSession(norm="running") runs the windows of live streams through.  Row b is a window of the stream in
 * slot[b]; window k of a stream is normalised at every norm point by the mean and biased variance of ALL frames of the
 * stream up to the window's right edge, each counted once.  Arguments as fastsvc_forward, and
 *   slot     DEVICE, B int32: the carry slot of row b's stream.  Rows of one slot are ASCENDING in b (window order).
 *            slot[] is followed, not clamped: 0 <= slot[b] < the number of records `carry` holds is the caller's duty
 *   own_lo, own_hi   DEVICE, B int32 each, in frames: the row's CORE [own_lo[b], own_hi[b]) of its lengths[b] valid
 *            frames, 0 <= own_lo < own_hi <= lengths[b]; the frames [own_hi[b], lengths[b]) are its look-ahead
 *   prior    DEVICE, B int32: frames of the stream in front of the core (all inside earlier cores), own_lo <= prior
 *   reset    DEVICE, B int32: nonzero on the first window a stream runs in this slot - for it and the slot's rows behind
 *            it in the batch the carry is taken as zero and NOT read, so opening a slot needs no memset.  Only on the
 *            first row of a slot in the batch; prior == own_lo
 *   parity   DEVICE, B int32, 0 / 1: which entry of the slot's record holds its carry; the same for all rows of a slot
 *   carry    DEVICE: record s at carry + s * carry_bytes; carry_bytes >= fastsvc_norm_carry_bytes(plan), a multiple of
 *            8.  A record is two ENTRIES (parity 0, 1) of, per up block in order, its three norm points' C x 2 doubles
 *   scratch  DEVICE, >= fastsvc_norm_running_scratch_bytes(plan, B, F) bytes: the partial sums
 * At each norm point, behind the launch that produced the tensor, per (row, channel) and all in float64, in this order:
 * the carry; the core chunks of earlier rows of the slot in this batch, ascending (row, chunk); the row's own core chunks
 * - the slot's new carry; the row's look-ahead chunks - the statistics, written as S * len_b / N with N = (prior[b] +
 * lengths[b] - own_lo[b]) columns' worth of frames.  Chunks are 2048 columns from the start of each range.  The LAST row
 * of a slot in the batch writes the new carry into entry parity ^ 1: a launch reads one entry of a record and writes the
 * other, so its workgroups need no order; the CALLER flips the slot's parity after every call that had a row of it.
 * No floating-point atomics: two runs give the same bits, and a stream's windows give the same carry and statistics
 * bits however they fall into calls.  Two extra launches per norm point.  A reset row with own_lo == 0 (window 0 of a
 * stream, which owns its whole row) is a PASS-THROUGH row: its statistics are left as the producer wrote them and only
 * its carry is written - a batch of such rows gives fastsvc_forward's output bit for bit.  float32 storage: the bound
 * behind the split-binary16 staging scale grows from sqrt(len_b) to sqrt(N), as in fastsvc_forward_grouped.
 * spk_emb == NULL: there is no norm; the extra arguments are ignored (may be NULL), the carry is untouched and the
 * launches and bytes are fastsvc_forward's.  Not together with the grouped route.  The device arrays cannot be checked
 * here; the Python layer validates them on the host (engine.check_norm_running). */
size_t fastsvc_norm_carry_bytes(const fastsvc_plan* plan);
size_t fastsvc_norm_running_scratch_bytes(const fastsvc_plan* plan, int32_t B, int32_t F);
int fastsvc_forward_running(const fastsvc_plan* plan, const void* dev_blob,
                            const float* ppg, const float* sine, const float* lft, const float* spk_emb,
                            float* out, int32_t B, int32_t F, const int32_t* lengths,
                            const int32_t* slot, const int32_t* own_lo, const int32_t* own_hi,
                            const int32_t* prior, const int32_t* reset, const int32_t* parity,
                            void* carry, size_t carry_bytes,
                            void* workspace, size_t workspace_bytes,
                            void* scratch, size_t scratch_bytes, void* stream);

/* The same two launches for ONE tensor u (B, C, ld) of `storage` and one norm point's carry: record s is the 2 x C x 2
 * doubles (entry, channel, sum u / sum u^2) at carry + s * 4 * C.  stats_out (B, C, 2) receives the statistics of every
 * row that is not a pass-through row.  No column at or beyond a row's valid length or in front of own_lo * len_mul is
 * read.  scratch: DEVICE, >= B * C * ceil(ld / 2048) * 32 bytes.  All pointers DEVICE; asynchronous on `stream`. */
int fastsvc_norm_running_stats(const void* u, int32_t storage, int32_t B, int32_t C, int32_t ld, const int32_t* lengths,
                               int32_t len_mul, const int32_t* slot, const int32_t* own_lo, const int32_t* own_hi,
                               const int32_t* prior, const int32_t* reset, const int32_t* parity, double* carry,
                               double* stats_out, void* scratch, size_t scratch_bytes, void* stream);

/* fastsvc_forward_running with a FORGETTING HORIZON: what decode.StreamSession(norm="running", horizon=H) runs its windows
 * through.  The running sums are forgotten exponentially - a frame j cores back counts with the product of the decays of
 * the cores since - so the population a window is normalised by, and with it the float32 headroom the statistics cost,
 * is bounded however long the stream lives.  Arguments as fastsvc_forward_running, and
 *   decay    DEVICE, B doubles, 8-byte aligned, 0 < decay[b] <= 1: what the slot's running sum is multiplied by in front
 *            of row b's core (exp(-core frames / H), computed by the caller; any value on a stream's first window)
 *   weight   DEVICE, B doubles: the weighted frames row b is normalised over - the decayed frame count of the cores up
 *            to its own plus its look-ahead frames, weight[b] >= lengths[b] - own_lo[b]
 *   bound    DEVICE, B doubles, bound[b] >= weight[b]: weight[b] over the smallest weight a column of the row has
 * The fold is fastsvc_forward_running's with ONE multiplication per row at a fixed place: the carry (or zero behind a
 * reset row); then for each row q <= b of the slot, ascending, the sum times decay[q] - rounded once, not fused into the
 * next addition - plus q's core chunks; behind row b's core the slot's new carry; plus b's look-ahead chunks - the
 * statistics, written as S * len_b / N with N = weight[b] * columns per frame, a double.  Carry and statistics are the
 * same bits however a stream's windows fall into calls.  prior[] is validated by the caller but counts nothing here.
 * float32 storage: a column of weight w is bounded by sqrt(N / w), so the staging scale's bound becomes sqrt(bound[b] *
 * columns per frame) where that exceeds sqrt(len_b).  Same launches as fastsvc_forward_running (the pool kernel is
 * norm_running_decay_pool_kernel), same carry record, scratch and pass-through rule.  With every decay 1, weight[b] =
 * prior[b] + lengths[b] - own_lo[b] and bound = weight the statistics and the carry are fastsvc_forward_running's bits.
 * spk_emb == NULL: there is no norm; the extra arguments are ignored (may be NULL), the carry is untouched and the
 * launches and bytes are fastsvc_forward's.  The arrays cannot be checked here; the Python layer validates them on the
 * host (engine.check_norm_decay). */
int fastsvc_forward_running_decay(const fastsvc_plan* plan, const void* dev_blob,
                                  const float* ppg, const float* sine, const float* lft, const float* spk_emb,
                                  float* out, int32_t B, int32_t F, const int32_t* lengths,
                                  const int32_t* slot, const int32_t* own_lo, const int32_t* own_hi,
                                  const int32_t* prior, const int32_t* reset, const int32_t* parity,
                                  const double* decay, const double* weight, const double* bound,
                                  void* carry, size_t carry_bytes,
                                  void* workspace, size_t workspace_bytes,
                                  void* scratch, size_t scratch_bytes, void* stream);

/* The same two launches for ONE tensor and one norm point's carry: fastsvc_norm_running_stats with the three arrays
 * above (bound is read by nobody here: there is no staging scale to raise).  Scratch and carry as there. */
int fastsvc_norm_running_stats_decay(const void* u, int32_t storage, int32_t B, int32_t C, int32_t ld, const int32_t* lengths,
                                     int32_t len_mul, const int32_t* slot, const int32_t* own_lo, const int32_t* own_hi,
                                     const int32_t* prior, const int32_t* reset, const int32_t* parity,
                                     const double* decay, const double* weight, const double* bound, double* carry,
                                     double* stats_out, void* scratch, size_t scratch_bytes, void* stream);

/* Creates (and calibrates, see the conventions above: synchronises `stream`) the helper streams / events
 * fastsvc_forward may use for `stream` on the current device, so that the forward itself allocates nothing and
 * never synchronises (call once per stream, e.g. before graph capture or a latency-critical first call).
 * Idempotent. */
int fastsvc_stream_prepare(void* stream);

/* Frees the helper streams / events held for `stream` on the current device (after waiting for whatever
 * they still run).  Call it BEFORE destroying a stream that forwards were issued on: contexts are keyed by
 * the stream handle, are otherwise kept for the life of the process, and a new stream that reuses the
 * handle value would inherit the old one's.  No forward may be in flight on `stream` from another host
 * thread.  Returns 1 if a context was freed, 0 if there was none. */
int fastsvc_stream_release(void* stream);

/* Host-side number formats of the half-precision-MFMA kernels (csrc/fastsvc_hx.hip), exported so that the
 * packer's conversions can be pinned against an independent implementation (tests/test_boundary.py):
 * for each of n floats x:  f16_hi = binary16(x), f16_lo = binary16(x - f16_hi)  (the split-half pieces:
 * x = hi + lo to 22 significand bits) and bf16 = bfloat16(x); all round-to-nearest-even, raw bit patterns.
 * Any output pointer may be NULL. */
void fastsvc_split_half(const float* x, int64_t n, uint16_t* f16_hi, uint16_t* f16_lo, uint16_t* bf16);

/* Test / profiling support: location of a named intermediate tensor inside the workspace after a
 * forward (names as in oracle/fastsvc_oracle.py taps: "down_lft.0", "scale.2", "up.1.xmid", ...).
 * Returns 0 and fills byte offset / element count / shape (up to 3 dims: B, C, T). */
int fastsvc_workspace_tap(const fastsvc_plan* plan, int32_t B, int32_t F, const char* tap_name,
                          size_t* byte_offset, int64_t* numel, int64_t shape3[3]);

/* Optional device-side autotuning for one problem size (the analogue of the reference's
 * `torch.backends.cudnn.benchmark = True`, train_fastsvc.py:617): runs one forward in which every
 * convolution times its candidate launch shapes (time tile x channel split x tiles per workgroup)
 * on `stream`, keeps the fastest per layer in the plan (thread-safe cache keyed by layer, B, T) and
 * synchronises the stream.  `out` holds a valid forward result afterwards.  Without this call the
 * launch shapes come from a static cost model.  n_trials (nullable) returns the number of timed
 * trial configurations. */
int fastsvc_autotune(const fastsvc_plan* plan, const void* dev_blob,
                     const float* ppg, const float* sine, const float* lft, const float* spk_emb,
                     float* out, int32_t B, int32_t F,
                     void* workspace, size_t workspace_bytes, void* stream, int32_t* n_trials);

/* Launch-shape table.  fastsvc_autotune stores its winners in the plan under keys
 * "<layer>|<B>|<T>" ("<layer>|<B>|<T>|b" while the plan uses bfloat16 activation storage, whose variants
 * compile under different register budgets; "...|h" in float16 storage, whose instances have bfloat16's shapes and
 * budgets: a float16 plan looks "|h" up first and falls back to the "|b" entry); these entry points export them and load them back (a table measured once on an
 * MI355X ships as svcc23_fastsvc_amd/tuned_mi355x.json, so production runs need no trial launches).
 * An entry whose shape is not compiled for that layer is ignored at launch time (cost model instead).
 *   fastsvc_tuned_count: number of entries;
 *   fastsvc_tuned_get:   entry `index` in key order; key_out holds >= 96 bytes; shape = NW, WM, WN,
 *                        tiles per workgroup, algorithm (0 = as launched, 1 = Winograd F(2,3) along time);
 *   fastsvc_tuned_set:   insert / replace one entry. */
int fastsvc_tuned_count(const fastsvc_plan* plan);
int fastsvc_tuned_get(const fastsvc_plan* plan, int32_t index, char* key_out, int32_t shape_out[5]);
int fastsvc_tuned_set(const fastsvc_plan* plan, const char* key, const int32_t shape[5]);

/* Per-launch timing of one forward (bench.py roofline accounting).  Same arguments as
 * fastsvc_forward; brackets every kernel launch with hipEvents on `stream`, synchronises the
 * stream at the end and fills one record per launch: the layer it computes, the kernel symbol
 * (template instance) it ran, its algorithmic FLOPs (2*MAC, padding excluded) and algorithmic HBM
 * bytes (each operand tensor once + packed weights once), and the measured duration.  The profiled
 * forward runs on `stream` ONLY (no helper streams), so every kernel is timed running alone. */
typedef struct fastsvc_launch_record {
    char layer[64];
    char kernel[40];
    double flops;
    double bytes;
    float ms;
    int32_t x2_path;   /* up.<i>.d3x, 2-byte storage, stretch 4 / 5: how the second operand was fetched - 1 element loads,
                          2 through the raw LDS tile; 0 everywhere else.  (Takes the struct's former tail padding.) */
} fastsvc_launch_record;

int fastsvc_forward_profile(const fastsvc_plan* plan, const void* dev_blob,
                            const float* ppg, const float* sine, const float* lft, const float* spk_emb,
                            float* out, int32_t B, int32_t F, const int32_t* lengths,
                            void* workspace, size_t workspace_bytes, void* stream,
                            fastsvc_launch_record* records, int32_t max_records, int32_t* n_records);

/* Number of kernel launches one forward enqueues at most (fused launches of the conditioning chains, chosen per
 * call from its shapes and the launch table, lower it by up to n_stages + 1) and algorithmic FLOPs (2*MAC of every conv /
 * linear, de-duplicated dataflow) per output sample - used by bench.py's roofline accounting. */
int fastsvc_forward_launch_count(const fastsvc_plan* plan, int32_t with_spk_emb);
double fastsvc_flops_per_sample(const fastsvc_plan* plan);

/* ---- the step right before the forward inside `inference()` ----
 * Replaces SignalGenerator.__call__ (harana/utils/features.py:144-213; called at fastsvc.py:381):
 *   f0   (B, 1, F) device, Hz, 0 = unvoiced
 *   out  (B, ntypes, F*hop) device; channel k is signal type types[k]: 0 = "noise", 1 = "sine"
 *        (NSF sine + voiced/unvoiced noise, features.py:177-197), 2 = "uv"
 *   scratch  fastsvc_signal_scratch_bytes(B, F) device bytes (per-frame phase prefix, f64)
 * Deterministic for a given seed (the reference draws torch.randn). Asynchronous on `stream`. */
size_t fastsvc_signal_scratch_bytes(int32_t B, int32_t F);
int fastsvc_signal_generate(const float* f0, float* out, void* scratch, int32_t B, int32_t F, int32_t hop,
                            float sample_rate, float sine_amp, float noise_amp,
                            const int32_t* types, int32_t ntypes, uint64_t seed, void* stream);

/* Batch assembly for ragged batches (csrc/fastsvc_stage.hip; the reference decodes one utterance at a time,
 * decode_fastsvc.py:160-200, and has no counterpart): utterance b's tensor is a (C, lens[b]) float32 block at
 * src[b] ON THE DEVICE whose rows are pitches[b] elements apart; dst (B, C, width) receives them zero-padded to
 * `width` columns (lens[b] <= width).  `src`, `lens`, `pitches` are HOST arrays of B entries, read during the call
 * (their values travel in the kernel arguments: nothing to keep alive, no table upload).  One launch per 64
 * utterances on `stream`. */
int fastsvc_gather_padded(const float* const* src, const int32_t* lens, const int32_t* pitches, float* dst,
                          int32_t B, int32_t C, int32_t width, void* stream);

/* The two ends of a resident decode session (csrc/fastsvc_decodeio.hip; decode.DecodeSession).  The reference does both
 * on the host, one utterance at a time (decode_fastsvc.py:150-200).
 *
 * Time-major batch assembly: utterance b is a contiguous time-major (lens[b], C) float32 block that starts offsets[b]
 * ELEMENTS into `packed`, a device buffer of packed_elems floats (the dump layout, audio_feats_dataset.py:30-34, blocks
 * back to back); dst (B, C, width), device, receives it transposed to channel-major and zero-padded: every column
 * >= lens[b] is written as 0, whatever dst held.  0 <= lens[b] <= width, 1 <= C <= 65535, no alignment or % 4
 * requirement on anything (16-byte accesses are used where the addresses allow).  `offsets` and `lens` are HOST arrays
 * of B entries, read during the call (their values travel in the kernel arguments); a block that does not lie inside
 * [0, packed_elems) is FASTSVC_E_INVALID, as are null pointers and sizes out of range; a failed launch is
 * FASTSVC_E_HIP.  One launch per 64 utterances, asynchronous on `stream`. */
int fastsvc_gather_time_major(const float* packed, int64_t packed_elems, const int64_t* offsets, const int32_t* lens,
                              float* dst, int32_t B, int32_t C, int32_t width, void* stream);

/* PCM-16 packing: row b of y (B, width), device float32, valid for lens[b] samples, goes to int16 at
 * dst + offsets[b] (offsets in int16 ELEMENTS; dst a device buffer of dst_elems int16): a packed, unpadded buffer.
 * Each value is rint of double(y) * 32767.0, computed in float64 (the product is exact there), ties to even,
 * saturated to [-32768, 32767] - bit for bit what decode.to_pcm16 gives on the host.  +inf / -inf saturate to
 * 32767 / -32768; NaN becomes 0 (the host's conversion of a NaN is implementation-defined).  Bytes of dst outside
 * every [offsets[b], offsets[b] + lens[b]) are not touched; rows must not overlap.  Any offsets and lens work; a row
 * whose destination starts on a 16-byte boundary (every row when lens are multiples of 8) is written with 16-byte
 * stores.  `lens` and `offsets` are HOST arrays of B entries, read during the call; 0 <= lens[b] <= width; a row that
 * does not lie inside [0, dst_elems) is FASTSVC_E_INVALID; a failed launch is FASTSVC_E_HIP.  One launch per 64 rows,
 * asynchronous on `stream`. */
int fastsvc_pcm16_pack(const float* y, const int32_t* lens, const int64_t* offsets, int16_t* dst, int64_t dst_elems,
                       int32_t B, int32_t width, void* stream);

/* What the PCM-16 conversion hides, per row: the conversion writes a NaN as 0 and saturates everything beyond the int16
 * range, so a packed buffer looks like audio whatever the waveform held.  One entry per row, 16 bytes. */
typedef struct fastsvc_row_report {
    int32_t nonfinite;   /* NaN / +-inf among the row's first lens[b] samples */
    int32_t clipped;     /* finite samples whose PCM-16 value saturates: rint(double(y) * 32767.0) outside [-32768, 32767] */
    float   max_abs;     /* largest |y| over the row's finite samples, 0 when there is none (exact: a maximum, not a sum) */
    int32_t reserved;    /* written as 0 by every entry point but fastsvc_stream_check, which counts the non-finite doubles
                            of the row's InstanceNorm carry entry here */
} fastsvc_row_report;

/* Checked PCM-16 packing: writes into dst exactly the bytes the unchecked packing writes, and touches exactly the same
 * bytes, in the same single pass over y (the eight samples a lane converts are the eight it reports on), and fills
 * report[b] for every row.  `report` is a DEVICE array of B entries that every call OVERWRITES: one memset on `stream`,
 * then the launches; calls never accumulate.  Samples at or beyond lens[b] are never read into the report.  Blocks reduce
 * in registers and LDS and issue integer atomics only (count sums, a maximum over the bit pattern of |y|), so the report
 * is bit-reproducible.  Arguments, checks and error codes are those of the unchecked packing, and a null `report` is
 * FASTSVC_E_INVALID; on an argument error nothing is enqueued.  One launch per 64 rows (row b's report at report + b),
 * asynchronous on `stream`.
 *
 * What a report tells about float16 activation storage (the RANGE CONTRACT above): an overflow that REACHES the waveform
 * is seen - an infinity survives LeakyReLU, turns a convolution's sum into inf / NaN even through a zero weight and
 * poisons InstanceNorm's mean, so it arrives as inf / NaN samples and `nonfinite` counts them.  Not seen: precision lost
 * below 2^-14, and a tensor past the ceiling whose infinity is never read.  The contract itself is unchanged; this
 * detects its observable violations (decode.DecodeSession(checked=True) acts on them). */
int fastsvc_pcm16_pack_checked(const float* y, const int32_t* lens, const int64_t* offsets, int16_t* dst, int64_t dst_elems,
                               fastsvc_row_report* report, int32_t B, int32_t width, void* stream);

/* The same reduction without a destination (for waveforms that stay float32): report[b] of row b of y (B, width) over its
 * first lens[b] samples.  `lens` a HOST array, `report` a DEVICE array of B entries, overwritten as above. */
int fastsvc_output_check(const float* y, const int32_t* lens, fastsvc_row_report* report,
                         int32_t B, int32_t width, void* stream);

/* Training-batch assembly from a resident corpus (csrc/fastsvc_collate.hip) - what the reference's Collater.__call__
 * (harana/bin/train_fastsvc.py:500-543) slices on the host, cut out of five packed float32 DEVICE buffers by one launch.
 * Stored utterance u has n_frames[u] frames and starts at frame frame_off[u] of the store:
 *   f0          elements [frame_off[u], + n_frames[u])                      (f0_elems floats)
 *   ppg         time-major (n_frames[u], D) at element frame_off[u] * D     (ppg_elems floats; the dump's own layout)
 *   wave, lft   n_frames[u] * hop samples at frame_off[u] * hop             (wave_elems floats each)
 *   emb         (n_utts, S), or NULL (use_spk_emb False: emb_out is then not touched and may be NULL)
 * Batch row b is the crop of utterance utt[b] that starts at frame start[b], ctx <= start[b] <= n_frames - frames - ctx
 * (the closed end; the reference's np.random.randint draws from the half-open range).  With T = frames * hop:
 *   y       (B, 1, T)                 wave[(frame_off + start) * hop, + T)
 *   lft_out (B, 1, T)                 lft, the same samples
 *   f0_out  (B, 1, frames)            f0[frame_off + start, + frames)
 *   ppg_out (B, D, frames + 2 ctx)    ppg frames [start - ctx, start + frames + ctx), transposed to channel-major
 *   emb_out (B, S)                    emb[utt[b], :]
 * all device float32, contiguous; every value is copied bit for bit.  No alignment or % 4 requirement on anything:
 * 16-byte requests are used where source and destination addresses allow (hop % 4 == 0, D % 4 == 0, T % 4 == 0 and
 * blocks that start on 16-byte boundaries make that every request), 4-byte ones elsewhere.  No load touches a byte
 * outside the crop's own source range - a crop may end at the last element of the store - and no store a byte outside
 * the five outputs.  `frame_off`, `n_frames` (n_utts entries) and `utt`, `start` (B entries) are HOST arrays, read during
 * the call (the rows' values travel in the kernel arguments).  Everything is checked on the host BEFORE anything is
 * launched: null pointers, sizes out of range, utt[b] outside [0, n_utts), start[b] outside [ctx, n_frames - frames - ctx],
 * an utterance whose block does not lie inside its buffers - FASTSVC_E_INVALID, with the row and the reason in
 * fastsvc_last_error(); a failed launch is FASTSVC_E_HIP.  One launch per 64 rows (fastsvc_collate_launch_count(B)),
 * asynchronous on `stream`. */
int fastsvc_collate_launch_count(int32_t B);
int fastsvc_collate_crops(const float* wave, const float* lft, int64_t wave_elems, const float* ppg, int64_t ppg_elems,
                          const float* f0, int64_t f0_elems, const float* emb, int32_t n_utts,
                          const int64_t* frame_off, const int32_t* n_frames, const int32_t* utt, const int32_t* start,
                          float* y, float* lft_out, float* ppg_out, float* f0_out, float* emb_out,
                          int32_t B, int32_t D, int32_t S, int32_t hop, int32_t frames, int32_t ctx, void* stream);

/* Speaker fan-out batch assembly for a resident decode session (csrc/fastsvc_fanout.hip;
 * decode.DecodeSession.convert_many) - a decode batch whose rows are (utterance, target speaker) pairs, so that a small
 * source set fills its batches across the speaker axis.  The reference converts one utterance to one speaker at a time on
 * the host (decode_fastsvc.py:150-200).  Three packed float32 DEVICE buffers hold the utterances; utterance u has
 * n_frames[u] frames and
 *   ppg   its time-major (n_frames[u], C) block at element ppg_off[u]           (ppg_elems floats; the dump's own layout)
 *   lft   n_frames[u] * hop samples at element lft_off[u]                       (lft_elems floats)
 *   f0    n_frames[u] values at element f0_off[u]                               (f0_elems floats; the dump's values)
 * and batch row r = (utt[r], spk[r]) becomes, all device float32, contiguous:
 *   ppg_out (R, C, width)        the block transposed to channel-major, every column >= n_frames written as 0 - the bits
 *                                of fastsvc_gather_time_major
 *   lft_out (R, 1, width * hop)  the samples copied bit for bit, the tail written as 0 - the bits of fastsvc_gather_padded
 *   f0_out  (R, 1, width)        voiced frames (f > 0): (float) exp((s1 / s0) * (log((double) f) - m0) + m1) with
 *                                (m0, s0) = src_stats[utt[r]] and (m1, s1) = spk_stats[spk[r]] - F0Statistics.convert
 *                                (features.py:88-108), every operation a separately rounded IEEE double operation in that
 *                                order (no fused multiply-add; log and exp are the device library's double-precision ones,
 *                                so the float32 result is within one ulp of the host's); unvoiced frames and the padding
 *                                are exactly 0.  src_stats (n_utts, 2) and spk_stats (n_spk, 2) are DEVICE tables of
 *                                doubles, [mean, std] of log F0 per row; when either is NULL f0 is copied bit for bit
 *   emb_out (R, E)               row spk[r] of spk_emb (n_spk, E), a DEVICE float32 table; a NULL spk_emb leaves emb_out
 *                                untouched (it may be NULL then)
 * 0 <= n_frames[u] <= width.  No alignment or % 4 requirement on anything (16-byte requests where source and destination
 * addresses agree mod 16, element requests elsewhere); no load touches a byte outside the row's own source block and no
 * store a byte outside the four outputs.  `ppg_off`, `lft_off`, `f0_off`, `n_frames` (n_utts entries) and `utt`, `spk`
 * (R entries) are HOST arrays, read during the call (the rows' values travel in the kernel arguments).  Everything is
 * checked on the host BEFORE anything is enqueued: null pointers, sizes out of range, utt[r] outside [0, n_utts), spk[r]
 * outside [0, n_spk), n_frames > width, a block that does not lie inside its buffer - FASTSVC_E_INVALID, with the row and
 * the reason in fastsvc_last_error(); a failed launch is FASTSVC_E_HIP.  One launch per 64 rows
 * (fastsvc_fanout_launch_count(R)), asynchronous on `stream`. */
int fastsvc_fanout_launch_count(int32_t R);
int fastsvc_fanout_assemble(const float* ppg, int64_t ppg_elems, const float* lft, int64_t lft_elems,
                            const float* f0, int64_t f0_elems, int32_t n_utts,
                            const int64_t* ppg_off, const int64_t* lft_off, const int64_t* f0_off, const int32_t* n_frames,
                            const double* src_stats, const double* spk_stats, const float* spk_emb, int32_t n_spk,
                            const int32_t* utt, const int32_t* spk,
                            float* ppg_out, float* lft_out, float* f0_out, float* emb_out,
                            int32_t R, int32_t C, int32_t E, int32_t hop, int32_t width, void* stream);

/* Windowed decode (csrc/fastsvc_window.hip; decode.DecodeSession.convert_windowed) - a long utterance runs as overlapping
 * windows, rows of ragged batches, and the windows' waveforms are cross-faded back into one.  The reference decodes whole
 * utterances (decode_fastsvc.py:150-200) and has no counterpart.
 *
 * Assembly.  Batch row r is a slice of an utterance held in three packed float32 DEVICE buffers: n_frames[r] frames of the
 * time-major ppg (frames x C) from element ppg_off[r] of `ppg` (ppg_elems floats), and the matching n_frames[r] * hop
 * samples from element sig_off[r] of `lft` and of `sine` (sig_elems floats each: the two share one layout).  It becomes,
 * all device float32, contiguous:
 *   ppg_out (R, C, width)                 the slice transposed to channel-major, every column >= n_frames written as 0
 *   lft_out, sine_out (R, 1, width * hop) the samples copied bit for bit, the tail written as 0
 * 0 <= n_frames[r] <= width.  No alignment or % 4 requirement on any offset (16-byte requests where source and destination
 * addresses allow, element requests elsewhere); no load touches a byte outside the row's own slices and no store a byte
 * outside the three outputs.  `ppg_off`, `sig_off`, `n_frames` are HOST arrays of R entries, read during the call (their
 * values travel in the kernel arguments).  Everything is checked on the host BEFORE anything is enqueued - null pointers,
 * sizes out of range, n_frames > width, a slice that does not lie inside its buffer: FASTSVC_E_INVALID, with the row and
 * the reason in fastsvc_last_error(); a failed launch is FASTSVC_E_HIP.  One launch per 64 rows
 * (fastsvc_window_launch_count(R)), asynchronous on `stream`. */
int fastsvc_window_launch_count(int32_t R);
int fastsvc_window_assemble(const float* ppg, int64_t ppg_elems, const float* lft, const float* sine, int64_t sig_elems,
                            const int64_t* ppg_off, const int64_t* sig_off, const int32_t* n_frames,
                            float* ppg_out, float* lft_out, float* sine_out,
                            int32_t R, int32_t C, int32_t hop, int32_t width, void* stream);

/* Stitch.  y (B, width) device float32: row r holds a window's waveform, valid for n_samples[r] samples; its core - the
 * samples of the utterance the window owns - is [core_lo[r], core_hi[r]) of the row.  A window that has a neighbour on a
 * side shares with it a FADE ZONE of 2 * half samples centred on the boundary: [core_lo - half, core_lo + half) on the
 * left, [core_hi - half, core_hi + half) on the right, clipped to n_samples (an utterance may end inside a zone).  Every
 * sample of the utterance is written once: outside the zones the owning row's sample; sample j of a zone
 *     (1 - w) * y_left + w * y_right,   w = (j + 0.5) / (2 * half),
 * in float64, the two products and the sum rounded separately - decode.stitch_windows' values bit for bit.  The two rows
 * of a zone may be in different calls, so each side of a row has a mode (left_mode[r], right_mode[r]):
 *   0 NONE        no neighbour: the core's edge is the utterance's
 *   1 STAGE       the neighbour runs in a LATER call: the row's zone samples are copied to stage + src and the zone is
 *                 not written
 *   2 FROM_STAGE  the neighbour ran in an EARLIER call on this stream and staged its samples at stage + src: this row
 *                 writes the blended zone
 *   3 FROM_Y      the neighbour is a row of this y: its zone samples start at y + src; this row writes the blended zone
 *   4 SKIP        the neighbour is a row of this y and writes the zone (its side is FROM_Y)
 * (src: left_src[r] / right_src[r], in float ELEMENTS; `stage` a device buffer of stage_elems floats, may be NULL when no
 * mode uses it).  So a row writes ONE contiguous run - its core without the zones it does not resolve, with the ones it
 * does - to element dst_off[r] of dst16 (PCM-16: rint(v * 32767.0) in float64, ties to even, saturated, NaN -> 0; for
 * samples outside the zones exactly fastsvc_pcm16_pack's value) and / or of dstf (the float64 value rounded to float32);
 * either may be NULL, both hold dst_elems elements.  16-byte stores where dst_off[r] % 8 == 0; runs must not overlap.
 * With half == 0 every mode must be NONE and the result is the concatenation of the cores.
 * `report` (may be NULL): a DEVICE array of n_utts entries; the float32 values of the samples row r writes are ADDED to
 * report[utt[r]] (counts summed, the maximum of |y| taken - integer atomics only, so the result is bit-reproducible).
 * Unlike fastsvc_pcm16_pack_checked the entries are NOT cleared: an utterance's windows arrive in several calls; clear
 * them before the first.
 * All row arrays are HOST arrays of B entries, read during the call.  Everything is checked on the host before anything is
 * enqueued: null pointers, sizes, modes, a core or zone outside its row, a slot outside `stage`, neighbour samples outside
 * y, a run outside [0, dst_elems), two runs of the call that overlap, utt[r] outside [0, n_utts) - FASTSVC_E_INVALID with the row and the reason in
 * fastsvc_last_error(); a failed launch is FASTSVC_E_HIP.  One launch per 64 rows, asynchronous on `stream`. */
int fastsvc_window_stitch(const float* y, int32_t B, int32_t width, const int32_t* n_samples,
                          const int32_t* core_lo, const int32_t* core_hi, int32_t half,
                          const int32_t* left_mode, const int32_t* right_mode, const int64_t* left_src, const int64_t* right_src,
                          float* stage, int64_t stage_elems, const int64_t* dst_off, int16_t* dst16, float* dstf,
                          int64_t dst_elems, const int32_t* utt, fastsvc_row_report* report, int32_t n_utts, void* stream);

/* Live streams (csrc/fastsvc_stream.hip; decode.StreamSession) - an utterance whose features arrive a few frames at a time.
 * The reference decodes whole files (decode_fastsvc.py:150-200) and has no counterpart.
 *
 * State, all DEVICE, for n_streams slots; `cap` (a multiple of 4) frames are retained per stream, frame p at index p % cap:
 *   ppg_ring (n_streams, cap, C)   time-major        lft_ring, exc_ring (n_streams, cap * hop)        float32, 16-byte aligned
 *   phase    (n_streams, 2)        float64: the sine phase C_f in cycles, in [0, 1), of the stream's next frame, in the
 *                                  entry the last push WROTE (a push reads entry parity[i] and writes entry parity[i] ^ 1:
 *                                  the caller alternates it per stream and push that appends at least one frame)
 *
 * Push.  Entry i appends n[i] frames (0 <= n[i] <= max_push <= min(cap, 1024); 0 changes nothing) to stream stream[i] (every
 * stream at most once per call), which held pos[i] frames before.  The frames come from the packed float32 DEVICE buffer
 * `upload` (upload_elems floats), from element up_off[i]: the time-major ppg n x C, then f0 n, then lft n x hop.  ppg and
 * lft are copied bit for bit into the rings at frame index pos[i] % cap (a chunk wraps at most once); the excitation of
 * the chunk is synthesised into exc_ring by the same launch: fastsvc_signal_generate's "sine" signal for
 *     C_{f+1} = frac(C_f + hop * rad_f),   rad_f = (f0_f / sample_rate) % 1 in float32,
 * run in float64 by one lane over the chunk, starting from phase[stream][parity] - or from 0 when first[i] is set, which
 * reads nothing: opening a slot needs no clearing - and then the closed form of the whole-utterance synthesis per sample.
 * hop * rad_f is a float32 times a small integer, and while the partial sums stay below 2^16 no float64 add rounds
 * (DESIGN.md 4.10), so with noise_amp == 0 the samples are bit for bit fastsvc_signal_generate's on the whole f0.  Noise is keyed by seed[i] and the ABSOLUTE sample index
 * pos[i] * hop + k: it depends neither on the slot nor on how the stream was cut into pushes.
 * 16-byte requests where source and destination addresses allow (C % 4 == 0, up_off and n multiples of 4), element
 * requests elsewhere; plain vector stores, no atomics; no load outside the entry's slice of `upload` and the phase entry,
 * no store outside the stream's own rings and phase pair.  All per-entry arrays are HOST arrays of S entries, read during
 * the call (their values travel in the kernel arguments).  Everything is checked on the host BEFORE anything is enqueued -
 * null or misaligned pointers, sizes, n[i] > max_push, a stream out of range or pushed twice, a slice that leaves
 * `upload`: FASTSVC_E_INVALID with the stream and the reason in fastsvc_last_error(), and nothing has changed; a failed
 * launch is FASTSVC_E_HIP.  One launch per 64 entries (fastsvc_stream_launch_count(S)), none when every n[i] is 0;
 * asynchronous on `stream_`.
 *
 * Push without f0.  exc_ring == NULL means "no f0 in the slice, no synthesis" (decode.StreamSession(f0="audio")): a slice is
 * the time-major ppg n x C, then n x hop samples for lft_ring - the audio ring of such a session - and the launch only
 * copies (the same 16-byte rule); phase and seed are not read and may be NULL, first and parity are checked and ignored.
 * The excitation of those frames is made when they are final, by fastsvc_stream_f0.  With an exc_ring the launches, kernel
 * arguments, bytes and bits are what they were.
 *
 * Assembly.  fastsvc_window_assemble's outputs for rows cut from the rings: row r is the n_frames[r] frames from frame
 * first_frame[r] of stream stream[r], read modulo cap ->
 *   ppg_out (R, C, width)                 transposed to channel-major, every column >= n_frames written as 0
 *   lft_out, sine_out (R, 1, width * hop) copied bit for bit, the tail written as 0
 * pos[s] (HOST, n_streams entries) is the number of frames stream s holds: a row must lie inside the retained frames
 * [pos[s] - cap, pos[s]) of its stream and 0 <= n_frames[r] <= min(width, cap), else FASTSVC_E_INVALID with the row and the
 * reason, before anything is enqueued.  No load outside the rings, no store outside the three outputs.  One launch per 64
 * rows (fastsvc_stream_launch_count(R)), asynchronous on `stream_`. */
int fastsvc_stream_launch_count(int32_t R);
int fastsvc_stream_push(const float* upload, int64_t upload_elems, int32_t S, const int32_t* stream, const int32_t* n,
                        const int64_t* up_off, const int64_t* pos, const int32_t* first, const int32_t* parity,
                        const uint64_t* seed, float* ppg_ring, float* lft_ring, float* exc_ring, double* phase,
                        int32_t n_streams, int32_t cap, int32_t max_push, int32_t C, int32_t hop,
                        float sample_rate, float sine_amp, float noise_amp, void* stream_);
int fastsvc_stream_assemble(const float* ppg_ring, const float* lft_ring, const float* exc_ring, int32_t n_streams, int32_t cap,
                            const int64_t* pos, const int32_t* stream, const int64_t* first_frame, const int32_t* n_frames,
                            float* ppg_out, float* lft_out, float* sine_out,
                            int32_t R, int32_t C, int32_t hop, int32_t width, void* stream_);

/* Per-window output check of live streams (csrc/fastsvc_stream_check.hip; decode.StreamSession(checked=True)).  A window
 * row of a stream's forward is judged on the samples it CONTRIBUTES, not on its whole length: report[r] describes
 * y[r, span_lo[r] : span_hi[r]) of y (B, width), device float32 - the caller passes the row's emitted run together with the
 * fade zones it stages or that a neighbour row reads (decode.stream_check_spans), so that an overflow confined to context
 * that is never emitted (no InstanceNorm without a speaker embedding) is not reported.  nonfinite, clipped and max_abs
 * follow fastsvc_output_check's rules exactly (one shared definition per sample): the report equals that of the span as a
 * row of its own, bit for bit.  Any 0 <= span_lo <= span_hi <= width works; the span's first byte need not be aligned
 * (16-byte loads over the aligned body, element loads for head and tail), and no sample outside [span_lo, span_hi) is read
 * into the report.
 *
 * The fourth word (`reserved`) receives the number of non-finite doubles in the running InstanceNorm carry entry the
 * forward just wrote for the row's stream: the entry_doubles doubles at
 *     (char*) carry + slot[r] * carry_bytes + entry[r] * entry_doubles * 8
 * (fastsvc_plan_norm_running's records: two entries per slot, carry_bytes >= 2 * entry_doubles * 8 per slot).  Only that
 * entry is read - the other entry and other slots' records are legitimately uninitialised.  entry[r] == -1: no carry, the
 * word is 0 and nothing is read; `slot` and `entry` may both be NULL (every row without a carry) and `carry` may be NULL
 * when no entry is >= 0.  A non-finite carry implies a non-finite row by reasoning (inf sums give a NaN variance); the
 * word makes that a checked invariant.
 *
 * `report` is a DEVICE array of B entries that every call OVERWRITES with plain stores: one workgroup per row reduces in
 * registers (wave shuffles) and LDS and its first lane stores the 16 bytes - no atomics, no memset, and two calls give the
 * same bits.  span_lo, span_hi, slot, entry are HOST arrays of B entries, read during the call (their values travel in the
 * kernel arguments).  Everything is checked on the host BEFORE anything is enqueued: null y or report, B < 1, width < 1,
 * span_lo > span_hi, span_hi > width, a negative value, entry outside {-1, 0, 1}, an entry >= 0 with a null or misaligned
 * carry or a null slot, slot outside [0, n_slots), entry_doubles < 1 or carry_bytes < 2 * entry_doubles * 8 or not a
 * multiple of 8 with an entry >= 0 - FASTSVC_E_INVALID with the row and the reason in fastsvc_last_error(), and nothing is
 * written; a failed launch is FASTSVC_E_HIP.  One launch per 64 rows (row r's report at report + r), asynchronous on
 * `stream_`. */
int fastsvc_stream_check(const float* y, int32_t B, int32_t width, const int32_t* span_lo, const int32_t* span_hi,
                         const void* carry, int64_t carry_bytes, int32_t entry_doubles, int32_t n_slots,
                         const int32_t* slot, const int32_t* entry, fastsvc_row_report* report, void* stream_);

/* Loudness of live streams from their raw audio (csrc/fastsvc_stream_loudness.hip; decode.StreamSession(loudness="audio")).
 * The stream's audio is appended to an AUDIO ring, (n_streams, cap * hop) float32 with sample p at index p % (cap * hop) -
 * fastsvc_stream_push does that when it is handed the audio ring where it takes the lft ring - and this call turns the
 * frames that have become FINAL into fastsvc_loudness_extract's value, hop samples per frame, written into lft_ring at
 * frame index f % cap.  Frame f is the whole-file function's frame f of the stream's audio y[0, T), T = F hop (periodic
 * Hann, 2048 samples centred on f hop, np.pad reflection at 0 and, once the stream has ended, at T), except for ONE
 * thing: its 80 dB floor hangs under the running maximum M_f = max over frames g <= f and all bins of the power, not
 * under the maximum of the whole utterance, which a live stream does not know.  A frame is final once
 * its last sample f hop + 1023 has arrived, or the stream has ended.
 *
 * Entry i finalises the n[i] frames from first_frame[i] of stream stream[i] (every stream at most once per call; 0 <= n[i]
 * <= max_frames <= min(cap, 2048); 0 changes nothing), of which seen[i] frames (seen[i] * hop samples) have arrived; with
 * ended[i] these are the stream's last frames, first_frame[i] + n[i] == seen[i].  A stream's frames must be finalised in
 * order, each once.
 *   peak     (n_streams, 2) float32: the running maximum, in the entry the last call WROTE (a call reads entry parity[i]
 *            and writes entry parity[i] ^ 1: the caller alternates it per stream and call that finalises at least one
 *            frame).  first_frame[i] == 0 starts from 0 and reads nothing: opening a slot needs no clearing.
 *   scratch  fastsvc_stream_loudness_scratch_bytes(n_streams, max_frames) DEVICE bytes: the power rows and maxima of one
 *            call's frames.
 * Two launches per 64 entries - the power rows, then maximum / floor / A-weighting / mean / log - none when every n[i] is
 * 0; plain vector stores, no atomics; no load outside the stream's audio ring, its peak entry and the scratch, no store
 * outside the scratch, the stream's lft ring rows and its peak pair.  Per-entry arrays are HOST arrays of S entries, read
 * during the call.  Everything is checked on the host BEFORE anything is enqueued - null or misaligned pointers, sizes,
 * n[i] > max_frames, a stream out of range or listed twice, frames that are not final or whose samples the ring no longer
 * holds: FASTSVC_E_INVALID with the reason in fastsvc_last_error(); a failed launch is FASTSVC_E_HIP.  Asynchronous on
 * `stream_`. */
size_t fastsvc_stream_loudness_scratch_bytes(int32_t n_streams, int32_t max_frames);
int fastsvc_stream_loudness(const float* audio_ring, float* lft_ring, float* peak, void* scratch, int32_t S,
                            const int32_t* stream, const int64_t* first_frame, const int32_t* n, const int64_t* seen,
                            const int32_t* ended, const int32_t* parity, int32_t n_streams, int32_t cap, int32_t max_frames,
                            int32_t hop, float sample_rate, void* stream_);

/* F0 and excitation of live streams from their raw audio (csrc/fastsvc_stream_f0.hip; decode.StreamSession(f0="audio")).
 * For the frames of a stream that have become FINAL - exactly the frames fastsvc_stream_loudness finalises, with the same
 * first_frame / n / seen / ended - this call computes fastsvc_f0_extract's value from the AUDIO ring (below: YIN, a function
 * of the frame's 2048 samples alone, so a streamed frame has the whole-file bits for every push schedule, slot and ring
 * position, the reflected frames at the end included), shifts it, and synthesises the frames' excitation:
 *   f0_ring   (n_streams, cap) float32: the raw F0 of frame f at index f % cap (0 = unvoiced)
 *   f0s_ring  (n_streams, cap) float32: the F0 the excitation is made from - for a voiced frame of a stream with statistics
 *             (float) exp((s1 / s0) * (log((double) f0) - m0) + m1), every operation a separately rounded double operation
 *             in that order (F0Statistics.convert; within one float32 ulp of the host's, as fastsvc_fanout_assemble's), else
 *             the raw value; unvoiced frames exactly 0
 *   stats     HOST, 4 doubles per entry: m0, s0 (source mean and std of log F0), m1, s1 (target) - finite with s0 > 0 - or
 *             four NaN: no shift
 *   exc_ring  (n_streams, cap * hop), 16-byte aligned: fastsvc_stream_push's excitation of those frames, the same expressions
 *             (csrc/fastsvc_signal.inc): the phase recurrence C_{f+1} = frac(C_f + hop * rad_f) in float64 by one lane from
 *             phase[stream][parity[i]] - or from 0 when first_frame[i] == 0, which reads nothing - writing entry parity[i] ^ 1
 *             (the caller alternates it per stream and call that finalises at least one frame); the noise keyed by seed[i]
 *             and the absolute sample index.  With noise_amp == 0 the samples are bit for bit fastsvc_signal_generate's on
 *             the whole shifted F0.
 * 0 <= n[i] <= max_frames <= min(cap, 2048).  A stream's frames must be finalised in order, each once.  Two launches per 64
 * entries - F0 and shift, one block per frame; then the excitation - none when every n[i] is 0; plain vector stores, no
 * atomics; no load outside the stream's audio ring, its f0s ring and its phase entry, no store outside the stream's rows of
 * the three rings and its phase pair.  Per-entry arrays are HOST arrays of S entries, read during the call.  Everything is
 * checked on the host BEFORE anything is enqueued - null or misaligned pointers, sizes, lags outside [1, 1024]
 * (fastsvc_f0_lags), threshold <= 0, n[i] > max_frames, a stream out of range or listed twice, statistics that are neither,
 * frames that are not final or whose samples the ring no longer holds: FASTSVC_E_INVALID with the reason in
 * fastsvc_last_error(); a failed launch is FASTSVC_E_HIP.  Asynchronous on `stream_`. */
int fastsvc_stream_f0(const float* audio_ring, float* f0_ring, float* f0s_ring, float* exc_ring, double* phase, int32_t S,
                      const int32_t* stream, const int64_t* first_frame, const int32_t* n, const int64_t* seen,
                      const int32_t* ended, const int32_t* parity, const uint64_t* seed, const double* stats,
                      int32_t n_streams, int32_t cap, int32_t max_frames, int32_t hop, float sample_rate, float f0_floor,
                      float f0_ceil, float threshold, float sine_amp, float noise_amp, void* stream_);

/* fastsvc_stream_f0 for calls in which a stream runs SOURCE STATISTICS (decode.RunningF0Stats): a live stream
 * has no corpus to take the source's mean and std of log F0 from, so they are defined causally, per frame, and carried on the
 * device.  Everything is fastsvc_stream_f0's - arguments, rings, phase, checks - plus:
 *   running       HOST, 6 doubles per entry: prior mean m_p, prior std s_p > 0, prior weight n0 > 0 (frames), decay g in
 *                 (0, 1] (exp(-1 / horizon), or exactly 1: nothing is forgotten), target mean m_t, target std s_t - all
 *                 finite - or six NaN: the entry runs none, and `stats` says what it gets, as in fastsvc_stream_f0.  An entry
 *                 with running statistics has four NaN in `stats`.
 *   stats_record  device, (n_streams, 2, 4) doubles, 8-byte aligned: per stream two entries of (w, S1, S2, voiced frames).
 *                 The call reads entry parity[i] - or starts from zeros when first_frame[i] == 0, which reads nothing, so the
 *                 record is never zeroed and a reused slot is fresh - and writes entry parity[i] ^ 1: the phase record's bit.
 * The rule, frame by frame in order, for a final frame with raw F0 v: v <= 0 gives 0 and leaves the state alone; else, every
 * operation a separately rounded double operation,
 *   d = log((double) v) - m_p;   w = w g + 1;   S1 = S1 g + d;   S2 = S2 g + d d;   N = n0 + w;   mu = S1 / N
 *   var = (n0 s_p s_p + S2) / N - mu mu;   f0s = (float) exp((s_t / sqrt(var)) (d - mu) + m_t)
 * so a frame is shifted by the statistics of the voiced frames up to and including itself, blended with a prior that counts as
 * n0 frames; var >= n0 s_p^2 / N > 0 (Cauchy-Schwarz): no NaN, no floor.  The value depends on the stream's frames alone, not
 * on how they fall into calls.  One launch more than fastsvc_stream_f0 per 64 entries, between its two - one block per stream
 * with running statistics and frames in the call: all lanes take d, one lane runs the three sums in frame order, all lanes
 * shift and overwrite f0s_ring, 256 frames a tile - and none more when no entry of the 64 has any; plain vector stores, no
 * atomics; no load or store outside the stream's rows of f0_ring, f0s_ring and its record pair.  Checked on the host before
 * anything is enqueued, in addition: a null or misaligned record, null `running`, constants that are not finite, s_p <= 0,
 * n0 <= 0, g outside (0, 1], an entry with both kinds of statistics: FASTSVC_E_INVALID. */
int fastsvc_stream_f0_running(const float* audio_ring, float* f0_ring, float* f0s_ring, float* exc_ring, double* phase,
                              double* stats_record, int32_t S, const int32_t* stream, const int64_t* first_frame,
                              const int32_t* n, const int64_t* seen, const int32_t* ended, const int32_t* parity,
                              const uint64_t* seed, const double* stats, const double* running, int32_t n_streams, int32_t cap,
                              int32_t max_frames, int32_t hop, float sample_rate, float f0_floor, float f0_ceil, float threshold,
                              float sine_amp, float noise_amp, void* stream_);

/* ---- F0 of whole files by YIN (csrc/fastsvc_f0.hip, csrc/fastsvc_f0.inc; de Cheveigne & Kawahara 2002) ----
 * The recipe's F0 is pyworld.harvest's, a whole-file CPU algorithm; this is a per-frame DEFINITION that
 * a live stream can compute as well.  Frames and conventions are fastsvc_loudness_extract's: audio (B, T) device float32,
 * out (B, frames) float32, frames = 1 + T / hop, frame f the 2048 samples x[k] = y[reflect(f hop - 1024 + k)], no window.
 *   tau_min = floor(sr / f0_ceil), tau_max = ceil(sr / f0_floor), 1 <= tau_min <= tau_max <= 1024 (fastsvc_f0_lags: else
 *   FASTSVC_E_INVALID), W = 2048 - tau_max
 *   d(tau) = sum over 1 <= j < W of (x[j] - x[j + tau])^2 for tau = 1 .. tau_max, computed directly (no FFT: no float32
 *            cancellation); x[0] is never read - frame 0's is sample 1024 by reflection, which a live stream whose hop
 *            divides 1024 has not received when the frame is final
 *   d'(tau) = d(tau) tau / (d(1) + ... + d(tau));  d(1) == 0 (a constant frame: a zero denominator) -> unvoiced, no NaN
 *   tau    = the smallest lag in [tau_min, tau_max] with d'(tau) < threshold, walked right while d'(tau + 1) < d'(tau) and
 *            tau + 1 <= tau_max; none -> f0 = 0
 *   parabolic interpolation of d' over tau - 1, tau, tau + 1, skipped when a neighbour lies outside [1, tau_max] or d'(tau)
 *            is not the smallest of the three;  f0 = sr / tau_hat
 * float32 arithmetic in an order fixed by the code (csrc/fastsvc_f0.inc), not by the launch.  One launch, no scratch, no
 * atomics; asynchronous on `stream`. */
int fastsvc_f0_lags(float sample_rate, float f0_floor, float f0_ceil, int32_t* tau_min, int32_t* tau_max);
int fastsvc_f0_extract(const float* audio, float* out, int32_t B, int32_t T, int32_t hop, float sample_rate, float f0_floor,
                       float f0_ceil, float threshold, void* stream);

/* ---- Fixed-lag Viterbi F0 tracking over YIN candidates (decode.F0Track) ----
 * A DEFINITION like the estimator above: the value of frame f is a function of the audio of the frames <= f + lag alone.
 *
 * fastsvc_f0_candidates: out (B, frames, 4, 2) float32, per frame up to four (tau_hat, s), the rest (0, inf).  With d' as
 * above, a lag t in [max(tau_min, 2), tau_max] is a candidate when d'(t) < cand_threshold, d'(t) < d'(t - 1) and t == tau_max
 * or d'(t) <= d'(t + 1); the four with the smallest d' are kept (ties: the smaller lag), in ascending lag, each with the
 * parabola above under its conditions as tau_hat, and s = d'(t).  A constant frame has none.  One launch, one workgroup per
 * frame: the lanes flag local minima, four rounds of a block-wide minimum over the key (bits of d', lag), one lane refines.
 *
 * fastsvc_f0_track: cands (B, frames, 4, 2) -> out (B, frames) float32; scratch: fastsvc_f0_track_scratch_bytes(B, frames)
 * bytes of device memory (5 backpointers and the best state per frame).  Viterbi over the states {candidate 0..3, unvoiced},
 * all float64, every operation rounded separately:
 *   local cost   c_k = s_k + lag_bias ((tau_hat_k - tau_hat_0) / tau_max); unvoiced: `unvoiced`; an absent state: +inf
 *   transition   unvoiced -> unvoiced 0; voiced <-> unvoiced switch_cost; voiced a -> voiced b jump (|ta - tb| / min(ta, tb))
 *   recurrence   frame 0: C = local; then C'[j] = (min over a of C[a] + tr(a, j)) + local[j], ties to the smallest a, which is
 *                the backpointer; absent states take no part; then min_j C'[j] is subtracted from every state
 *   output       e = min(f + lag, frames - 1); the state at e is the argmin of C_e (ties: the smallest index), followed back
 *                to f; f0 = sample_rate / tau_hat in float32, 0 when unvoiced
 * One launch, one workgroup per row: one lane runs the recurrence, then all lanes trace back at most `lag` steps each.
 * lag in [0, 64], costs finite and >= 0, tau_max in [1, 1024]: else FASTSVC_E_INVALID.  Asynchronous on `stream`. */
int fastsvc_f0_candidates(const float* audio, float* out, int32_t B, int32_t T, int32_t hop, float sample_rate, float f0_floor,
                          float f0_ceil, float cand_threshold, void* stream);
int64_t fastsvc_f0_track_scratch_bytes(int32_t B, int32_t frames);
int fastsvc_f0_track(const float* cands, float* out, void* scratch, int32_t B, int32_t frames, int32_t tau_max, float sample_rate,
                     int32_t lag, double lag_bias, double jump, double switch_cost, double unvoiced, void* stream);

/* fastsvc_stream_f0_running with TRACKING (csrc/fastsvc_stream_f0.hip): the newly final frames [first_frame, + n) get their
 * candidates into cand_ring (n_streams, cap, 4, 2) float32 - frame f at f % cap - the recurrence advances over them from
 * track_record (n_streams, 2, 8) doubles (entry track_parity[i] is read, or nothing when first_frame[i] == 0; the other is
 * written; 5 of the 8 are used) and leaves backpointers and best states in bp_ring (n_streams, cap, 8) bytes; the frames
 * [emit_first, + emit_n) - up to frame max(0, first_frame + n - lag) before the end, first_frame + n at the end, which the call
 * checks - get the tracked raw F0 in f0_ring and its static shift in f0s_ring, and the running shift (`running` and
 * stats_record, both or neither may be null) and the excitation run over THEM: `parity` addresses the phase and the statistics
 * record as before and flips with a call that emits.  An entry may have n[i] == 0 and still emit (a stream that ends in a
 * call that finalises nothing).  Per 64 entries the launches are: the frames launch in candidate mode (when an entry has new
 * frames), the tracker (one block per stream), the running shift (when an entry runs statistics and emits) and the excitation
 * (when an entry emits) - ONE launch more than the untracked call.  Plain vector stores, no atomics. */
int fastsvc_stream_f0_tracked(const float* audio_ring, float* cand_ring, void* bp_ring, float* f0_ring, float* f0s_ring,
                              float* exc_ring, double* phase, double* stats_record, double* track_record, int32_t S,
                              const int32_t* stream, const int64_t* first_frame, const int32_t* n, const int64_t* seen,
                              const int32_t* ended, const int32_t* parity, const int32_t* track_parity, const int64_t* emit_first,
                              const int32_t* emit_n, const uint64_t* seed, const double* stats, const double* running,
                              int32_t n_streams, int32_t cap, int32_t max_frames, int32_t hop, float sample_rate, float f0_floor,
                              float f0_ceil, float cand_threshold, int32_t lag, double lag_bias, double jump, double switch_cost,
                              double unvoiced, float sine_amp, float noise_amp, void* stream_);

/* ---- the producer of the generator's loudness input ----
 * Replaces loudness_extract(audio, sampling_rate, hop_length) (harana/bin/preprocess_fastsvc.py:60-75; librosa
 * 0.8.1 stft n_fft 2048 / periodic Hann / reflect padding, perceptual (A) weighting with the 80 dB floor below
 * the utterance maximum, db_to_amplitude, log(mean over bins + 1e-5), nearest stretch by the hop):
 *   audio (B, T) device float32, one utterance per row;  out (B, frames * hop), frames = 1 + T / hop
 *   scratch  fastsvc_loudness_scratch_bytes(B, T, hop) device bytes (power spectrogram + per-utterance maximum)
 * Asynchronous on `stream`. */
int32_t fastsvc_loudness_frames(int32_t T, int32_t hop);
size_t fastsvc_loudness_scratch_bytes(int32_t B, int32_t T, int32_t hop);
int fastsvc_loudness_extract(const float* audio, float* out, void* scratch, int32_t B, int32_t T, int32_t hop,
                             float sample_rate, void* stream);

/* ---- the multi-resolution STFT loss of the training step, forward and backward ----
 * Replaces MultiResolutionSTFTLoss.forward(x, y) (harana/losses/stft_loss.py:131-180; STFTLoss :100-128, the magnitude
 * stft() :21-51, SpectralConvergenceLoss :54-74, LogSTFTMagnitudeLoss :77-97) and the gradient autograd derives from
 * it for the predicted signal x (the call site: harana/bin/train_fastsvc.py:163-170):
 *   x, y      (B, T) device float32: predicted / ground-truth waveforms, one per row
 *   n_res resolutions: fft_sizes[i] (a power of two in [8, 2048]: anything else FASTSVC_E_UNSUPPORTED), hop_sizes[i],
 *             win_lengths[i] <= fft_sizes[i] (HOST arrays); windows[i] = device pointer to win_lengths[i] window values
 *             (HOST array of pointers: whatever getattr(torch, window)(win_length) gives; centred in the frame)
 *   frames are centred with reflect padding (fft_size / 2 < T, else FASTSVC_E_INVALID - torch raises there too)
 *   loss      device float32 [2]: (spectral convergence, log STFT magnitude), each averaged over the resolutions
 *   scratch   fastsvc_stft_loss_scratch_bytes(...) device bytes; the forward leaves the per-resolution sums there,
 *             the backward of the SAME (x, y) reads them and uses the rest for the frame gradients
 *   grad_loss device float32 [2]: incoming gradients of (sc, mag);  grad_x (B, T): d(grad_loss . loss) / dx
 * No atomics: loss and gradient are bit-reproducible.  Asynchronous on `stream`. */
size_t fastsvc_stft_loss_scratch_bytes(int32_t B, int32_t T, int32_t n_res, const int32_t* fft_sizes, const int32_t* hop_sizes);
int fastsvc_stft_loss_forward(const float* x, const float* y, int32_t B, int32_t T, int32_t n_res, const int32_t* fft_sizes,
                              const int32_t* hop_sizes, const int32_t* win_lengths, const float* const* windows,
                              float* loss, void* scratch, void* stream);
int fastsvc_stft_loss_backward(const float* x, const float* y, int32_t B, int32_t T, int32_t n_res, const int32_t* fft_sizes,
                               const int32_t* hop_sizes, const int32_t* win_lengths, const float* const* windows,
                               const float* grad_loss, float* grad_x, void* scratch, void* stream);

/* ---- the grouped strided convolutions of the recipe's discriminator, forward and backward ----
 * Replaces, for the downsampling layers of MelGANDiscriminator (harana/models/fastsvc.py:386-520: Conv1d(c, min(4c, 512),
 * kernel_size = 41, stride = 4, padding = 20, groups = c / 4) + LeakyReLU; yaml egs/svcc23/fastsvc1/conf/fastsvc.yaml:34-52), what
 * the trainer's discriminator calls and their autograd run (harana/bin/train_fastsvc.py:172-175,207-224):
 *   fastsvc_gconv1d_forward          y = lrelu_slope(bias + grouped_conv(x, w))        x (B, Cin, T), w (Cout, Cin / groups, K),
 *                                    y (B, Cout, Tout), Tout = (T + 2 pad - K) / stride + 1; slope = 1: no activation
 *   fastsvc_gconv1d_backward_data    dx = grouped_conv_transpose(dy * lrelu'(y_act), w)  (y_act = the forward's output, or NULL)
 *   fastsvc_gconv1d_backward_weight  dw[o, i, k] = sum_{b, t} dy'[b, o, t] x[b, g(o) Ig + i, stride t + k - pad], dbias[o] = sum dy'
 *                                    (dbias may be NULL); scratch: fastsvc_gconv1d_backward_weight_scratch_bytes(B, Cout, T)
 *                                    device bytes (per-slab partial sums added in a fixed order: bit-reproducible)
 * Device float32, contiguous.  Supported (fastsvc_gconv1d_supported != 0): Cin / groups = 4, Cout / groups in {8, 16}, K = 41,
 * stride = 4, pad = 20; anything else FASTSVC_E_UNSUPPORTED (the caller keeps its own convolution).  Asynchronous on `stream`. */
int fastsvc_gconv1d_supported(int32_t Cin, int32_t Cout, int32_t groups, int32_t K, int32_t stride, int32_t pad);
int fastsvc_gconv1d_forward(const float* x, const float* w, const float* bias, float* y, int32_t B, int32_t Cin, int32_t Cout,
                            int32_t groups, int32_t T, int32_t K, int32_t stride, int32_t pad, float slope, void* stream);
int fastsvc_gconv1d_backward_data(const float* dy, const float* y_act, const float* w, float* dx, int32_t B, int32_t Cin,
                                  int32_t Cout, int32_t groups, int32_t T, int32_t K, int32_t stride, int32_t pad, float slope,
                                  void* stream);
size_t fastsvc_gconv1d_backward_weight_scratch_bytes(int32_t B, int32_t Cout, int32_t T);
int fastsvc_gconv1d_backward_weight(const float* x, const float* dy, const float* y_act, float* dw, float* dbias, void* scratch,
                                    int32_t B, int32_t Cin, int32_t Cout, int32_t groups, int32_t T, int32_t K, int32_t stride,
                                    int32_t pad, float slope, void* stream);

/* ---- the convolutions of the generator's backward pass (float32 matrix-core kernels) ----
 * What autograd runs for every Conv1d / Conv2d(1 x k) of the generator when the reference trainer calls
 * gen_loss.backward() (harana/bin/train_fastsvc.py:183; the layers: harana/layers/residual_block.py:27-48,
 * harana/models/fastsvc.py:34-232 - all stride 1, "same" zero padding, k = 1 or 3, dilation d with (k / 2) d <= 27):
 *   fastsvc_conv1d_forward   y[b, o, t] = bias[o] + sum_{i, k} w[o, i, k] x[b, i, t + (k - k/2) d]
 *       x (B, Cin, T), y (B, Cout, T), w (Cout, Cin, K), bias (Cout) or NULL - device float32, contiguous.
 *       transposed != 0: w is read as (Cin, Cout, K) with flipped taps - with x = dy and w the forward weight this IS the
 *       backward-data convolution dx = conv_transpose(dy, w) (Cin = the forward's Cout, Cout = the forward's Cin).
 *   fastsvc_conv1d_backward_weight   dw[o, i, k] = sum_{b, t} dy[b, o, t] x[b, i, t + (k - k/2) d],  dbias[o] = sum dy
 *       (dbias may be NULL); both are overwritten.  scratch: fastsvc_conv1d_backward_weight_scratch_bytes(...) device
 *       bytes (per-slab partial sums, added in a fixed order: bit-reproducible).
 * Anything else (even k, k > 3, longer halos): FASTSVC_E_UNSUPPORTED.  Asynchronous on `stream`. */
int fastsvc_conv1d_forward(const float* x, const float* w, const float* bias, float* y, int32_t B, int32_t Cin, int32_t Cout,
                           int32_t T, int32_t K, int32_t dilation, int32_t transposed, void* stream);
size_t fastsvc_conv1d_backward_weight_scratch_bytes(int32_t B, int32_t Cin, int32_t Cout, int32_t T, int32_t K);
int fastsvc_conv1d_backward_weight(const float* x, const float* dy, float* dw, float* dbias, void* scratch, int32_t B, int32_t Cin,
                                   int32_t Cout, int32_t T, int32_t K, int32_t dilation, void* stream);

/* ---- FiLM affine + InstanceNorm + speaker bias + LeakyReLU of the up blocks, forward and backward ----
 * `_feature_affine` with a speaker embedding (harana/models/fastsvc.py:115-139) followed by the LeakyReLU that opens the
 * next conv block (fastsvc.py:60-83), as ONE node of the training graph:
 *   out = lrelu((u - mean_t u) / sqrt(var_t u + eps) + bias[row]),  u = scale * x + shift
 *   x, scale, shift, out (rows, T) device float32 with rows = B * C; bias (rows) = emb_projector(normalize(spk_emb));
 *   mean, rstd (rows) are written by the forward and read by the backward of the same inputs
 *   backward: dx, dscale, dshift (rows, T) and dbias (rows) from dout
 * Asynchronous on `stream`. */
int fastsvc_film_norm_forward(const float* x, const float* scale, const float* shift, const float* bias, float* out, float* mean,
                              float* rstd, int32_t rows, int32_t T, float eps, float slope, void* stream);
int fastsvc_film_norm_backward(const float* dout, const float* x, const float* scale, const float* shift, const float* bias,
                               const float* mean, const float* rstd, float* dx, float* dscale, float* dshift, float* dbias,
                               int32_t rows, int32_t T, float slope, void* stream);

/* ---- weight normalisation w = g * v / ||v|| of up to 56 layers in ONE launch, forward and backward ----
 * torch.nn.utils.weight_norm as the reference applies it to every conv (harana/models/fastsvc.py:354-362; norm over all
 * dims but 0) and what autograd derives from it.  HOST arrays of n device pointers / sizes:
 *   v[i] (rows[i], cols[i]), g[i] (rows[i]);  forward writes w[i] (rows, cols) and norm[i] (rows);
 *   backward reads dw[i], norm[i] and writes dv[i] (rows, cols), dg[i] (rows).   n > 56: FASTSVC_E_UNSUPPORTED (call again for the rest). */
int fastsvc_weight_norm_forward(int32_t n, const float* const* v, const float* const* g, float* const* w, float* const* norm,
                                const int32_t* rows, const int32_t* cols, void* stream);
int fastsvc_weight_norm_backward(int32_t n, const float* const* v, const float* const* g, const float* const* dw,
                                 const float* const* norm, float* const* dv, float* const* dg, const int32_t* rows,
                                 const int32_t* cols, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FASTSVC_HIP_H */
