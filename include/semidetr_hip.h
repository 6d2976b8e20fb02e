/*
 * semidetr_hip.h -- C ABI of libsemidetr_hip.so: the MI355X (gfx950) native hot path of Semi-DETR.
 *
 * Drop-in boundary: plain pointers + sizes, no torch types.  All pointers are DEVICE pointers unless
 * the parameter is documented as host.  `stream` is a hipStream_t passed as void* (NULL = the null
 * stream).  Every call is asynchronous on `stream`, keeps no global state between calls (apart from a
 * thread-local last-error string and the per-(device, call site) forward-kernel choice documented at
 * semidetr_msda_set_forward_policy, which also lists the one-time allocation it makes) and is re-entrant.  Return value: 0 on success, otherwise a
 * SEMIDETR_E_* code (negative: argument/precondition error detected on the host; positive: the
 * hipError_t returned by the launch).  semidetr_last_error() gives the message for the calling thread.
 *
 * Each entry point names the reference interface it replaces (paths relative to the Semi-DETR tree).
 */
#ifndef SEMIDETR_HIP_H
#define SEMIDETR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEMIDETR_OK 0
#define SEMIDETR_E_BADARG (-1)      /* null pointer / non-positive size / unsupported combination   */
#define SEMIDETR_E_TOOLARGE (-2)    /* an index would overflow the 32-bit arithmetic used on device  */
#define SEMIDETR_E_NODEVICE (-3)    /* no HIP device available                                        */

#define SEMIDETR_ABI_VERSION 7

int semidetr_abi_version(void);
const char *semidetr_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Multi-scale deformable attention (MSDA).
 *
 * Replaces  ms_deformable_im2col_cuda   detr_od/models/utils/ops/src/cuda/ms_deform_im2col_cuda.cuh:923-954
 *           ms_deformable_col2im_cuda   detr_od/models/utils/ops/src/cuda/ms_deform_im2col_cuda.cuh:956-1327
 * i.e. the launchers behind ms_deform_attn_cuda_forward/backward (ms_deform_attn_cuda.cu:20-153), which
 * the pybind module MultiScaleDeformableAttention exports (src/vision.cpp:13-16).
 *
 * Layouts (contiguous, row-major), exactly the reference's:
 *   value          (batch, spatial_size, num_heads, channels)
 *   spatial_shapes (num_levels, 2) int64  [(H_l, W_l)]          -- device memory, read by the kernel
 *   level_start    (num_levels,)   int64                         -- device memory, read by the kernel
 *   sampling_loc   (batch, num_query, num_heads, num_levels, num_point, 2)   (x, y) in [0,1] coords
 *   attn_weight    (batch, num_query, num_heads, num_levels, num_point)
 *   out / grad_out (batch, num_query, num_heads * channels)
 * Semantics: bilinear sampling with align_corners=False pixel mapping (h = y*H - 0.5), zero padding,
 * a sample contributes only if -1 < h < H and -1 < w < W.  forward writes every element of `out`.
 * backward zero-fills grad_value itself (on `stream`: hipMemsetAsync, or as a side job of its first kernel),
 * accumulates into it with fp atomics, and writes every element of grad_sampling_loc / grad_attn_weight.
 * The whole batch is one launch (the reference's im2col_step chunking does not change results).
 * f32: fast path for channels == 32, generic path otherwise.  f64: generic path (gradcheck parity).
 *
 * `flags` (f32 entry points): SEMIDETR_MSDA_QUERIES_ARE_PIXELS tells the library that this is encoder
 * self-attention -- num_query == spatial_size, query i IS pixel i of the pyramid, and spatial_shapes /
 * level_start tile [0, spatial_size) exactly (level_start[l+1] == level_start[l] + H_l*W_l, sum H_l*W_l ==
 * spatial_size), with every H_l, W_l <= 32766.  The level table lives in device memory, so the library cannot verify this without a
 * host synchronisation: the CALLER vouches for it (the Python / pybind layer checks it once per
 * spatial_shapes tensor).  With the flag the forward / gather kernels take 2-D pixel patches and
 * grad_value is produced by the region-owned scatter kernel; without it every query set takes the strip
 * kernels, which make no assumption (the reference op has no such coupling).  Results are identical
 * either way (up to fp32 summation order); the flag only selects faster kernels.  With the flag the backward clears
 * grad_value inside its first kernel; grad_value of the encoder path is produced by the region-owned scatter.
 * ------------------------------------------------------------------------------------------- */
#define SEMIDETR_MSDA_QUERIES_ARE_PIXELS 1
/* Bits 8..15 of `flags`: the call site's slot of the forward-kernel choice (semidetr_msda_set_forward_policy below), 0..255.
 * The reference builds twelve MSDeformAttn instances per model (transformer.py:609,760); give each its own slot and its
 * encoder forward is chosen from ITS launches' sample spread.  Slot 0 (no bits set) is shared by every caller that names none. */
#define SEMIDETR_MSDA_POLICY_SLOT(s) (((s) & 0xff) << 8)
/* The forward kernel is to be a function of the arguments alone: with the adaptive policy WHICH of the two encoder forward
 * kernels runs depends on when earlier launches' counts reached the host, and the two sum a row's samples in different orders
 * (results agree to ~2e-6 absolute, not bit for bit) -- two passes over identical inputs may then differ in the last bits,
 * which the reference's single kernel never does.  With this flag the patch kernel runs, and the backward's small-gradient half is
 * the patch gather whatever the slot's counts say (the compiled front end sets it while
 * torch.use_deterministic_algorithms(True) is in force).  grad_value is accumulated with fp32 atomics either way, exactly as in
 * the reference (ms_deform_im2col_cuda.cuh:87-159): the BACKWARD's summation order is run-dependent there and here. */
#define SEMIDETR_MSDA_FIXED_FORWARD 2
/* Backward only (ABI 7): WHICH kernel computes grad_sampling_loc / grad_attn_weight of an encoder backward, stated by the caller instead of
 * read from the slot's live counts.  The two gathers agree to fp32 rounding, not bit for bit, and in the reference these two gradients
 * are deterministic (no atomics: ms_deform_im2col_cuda.cuh:301-403) -- so a caller that wants the backward to follow what was known when the
 * matching FORWARD ran (the autograd functions do: they ask semidetr_msda_gather_choice right after the forward launch and hand the answer
 * back here) sets one of the two.  Neither bit: the slot's state at the time of the backward decides (ABI <= 6 behaviour).
 * SEMIDETR_MSDA_FIXED_FORWARD still wins (patch gather). */
#define SEMIDETR_MSDA_GATHER_WINDOW (1 << 16)
#define SEMIDETR_MSDA_GATHER_PATCH (1 << 17)
/* The paragraph above stays true of every entry point declared before this one.  The EXACT backward (additive, ABI 7; fp32,
 * channels == 32) is the opt-in exception: semidetr_msda_backward_exact_f32 takes the arguments of semidetr_msda_backward_f32 plus a
 * workspace and returns
 *   grad_value[n, row, m, d] = the EXACT sum of its fp32 contributions, rounded once to nearest even,
 * where, for a valid corner k of a sample with attention weight a, w = fl(a * c_k) with c_k the fp32 product of the corner's two
 * bilinear factors, and contribution[d] = fl(w * grad_out[n, q, m, d]) (each a single individually rounded operation).  The bits of
 * grad_value are therefore a function of the SET of contributions: the same on every run, for every launch order, independent of the
 * image's position in the batch, of the order in which queries or points are listed and of `flags`.  A sum that exceeds fp32's range
 * is +-inf exactly when the exact sum rounds there; non-finite contributions give what IEEE addition gives in every order (NaN if a
 * NaN or both infinities occur, otherwise the infinity).  Every element of grad_value is written exactly once (rows nobody samples
 * are stored as zeros): the buffer needs no fill.  No float atomic is used: contributions are counted and bucketed per destination
 * row with integer atomics into the workspace (8 bytes per (query, head, level, point, corner)), then each row is summed in a long
 * fixed-point accumulator.  grad_sampling_loc / grad_attn_weight come from the gather kernels of the default route, which never used
 * atomics (with SEMIDETR_MSDA_QUERIES_ARE_PIXELS: the patch gather, as under SEMIDETR_MSDA_FIXED_FORWARD); all three results are
 * bitwise reproducible.  The price is time: the route is for runs that must be reproducible, not for speed.
 *   workspace: device memory, 16-byte aligned, at least semidetr_msda_exact_workspace_bytes(...) bytes (0: the sizes are not
 *   supported); contents need no initialisation and mean nothing afterwards.  No host synchronisation, no allocation: legal inside a
 *   stream capture.  SEMIDETR_E_BADARG (reason in semidetr_last_error) for channels != 32, num_levels * num_point > 62 (the gather
 *   kernel's LDS), more than 32 heads, pointers not 16-byte aligned, a workspace too small or misaligned, and
 *   num_query * num_levels * num_point * 4 >= 2^32.  Bits 8..17 of `flags` are accepted and ignored. */
size_t semidetr_msda_exact_workspace_bytes(int batch, int spatial_size, int num_heads, int num_levels, int num_query, int num_point);
int semidetr_msda_backward_exact_f32(void *stream, const float *grad_out, const float *value, const int64_t *spatial_shapes,
                                     const int64_t *level_start, const float *sampling_loc, const float *attn_weight, int batch,
                                     int spatial_size, int num_heads, int channels, int num_levels, int num_query, int num_point,
                                     int flags, void *workspace, size_t workspace_bytes, float *grad_value,
                                     float *grad_sampling_loc, float *grad_attn_weight);
int semidetr_msda_forward_f32(void *stream, const float *value, const int64_t *spatial_shapes,
                              const int64_t *level_start, const float *sampling_loc,
                              const float *attn_weight, int batch, int spatial_size, int num_heads,
                              int channels, int num_levels, int num_query, int num_point, int flags, float *out);
int semidetr_msda_forward_f64(void *stream, const double *value, const int64_t *spatial_shapes,
                              const int64_t *level_start, const double *sampling_loc,
                              const double *attn_weight, int batch, int spatial_size, int num_heads,
                              int channels, int num_levels, int num_query, int num_point, double *out);
int semidetr_msda_backward_f32(void *stream, const float *grad_out, const float *value,
                               const int64_t *spatial_shapes, const int64_t *level_start,
                               const float *sampling_loc, const float *attn_weight, int batch,
                               int spatial_size, int num_heads, int channels, int num_levels,
                               int num_query, int num_point, int flags, float *grad_value,
                               float *grad_sampling_loc, float *grad_attn_weight);
int semidetr_msda_backward_f64(void *stream, const double *grad_out, const double *value,
                               const int64_t *spatial_shapes, const int64_t *level_start,
                               const double *sampling_loc, const double *attn_weight, int batch,
                               int spatial_size, int num_heads, int channels, int num_levels,
                               int num_query, int num_point, double *grad_value,
                               double *grad_sampling_loc, double *grad_attn_weight);

/* ---------------------------------------------------------------------------------------------
 * MSDA with the MSDeformAttn prologue / epilogue fused in (fp32, channels == 32).
 *
 * Replaces  MSDeformAttn.forward lines between the Linear layers
 *           detr_od/models/utils/ops/modules/ms_deform_attn.py:99-111  (softmax over L*P, sampling_locations =
 *           reference_points + offsets / (W_l, H_l)   [ref_dim 2]   or
 *           reference_points[:2] + offsets / P * reference_points[2:] * 0.5   [ref_dim 4])
 *           together with MSDeformAttnFunction.apply (:121-123) and their autograd backward.
 * The kernels read the RAW outputs of the two Linear layers, so the (N,Lq,M,L,P,2) locations tensor, the
 * softmaxed weights and their gradients never exist in HBM.
 *   reference_points  (batch, num_query, num_levels, ref_dim)       ref_dim 2 or 4; 16-byte aligned, < 4 GB (read with
 *                     one bounded 16-byte buffer load per (query, level))
 *   sampling_offsets  (batch, num_query, num_heads, num_levels, num_point, 2)   raw Linear output
 *   attn_logits       (batch, num_query, num_heads, num_levels * num_point)     raw Linear output (pre-softmax)
 *   padding_mask      (batch, spatial_size) bytes, nonzero = padded pixel, or NULL: `value.masked_fill(mask[..., None], 0)`
 *                     (ms_deform_attn.py:95-96) folded in -- a corner on a padded pixel reads as zero and receives no
 *                     gradient, so `value` is passed UNMASKED and grad_value comes back with zero rows there.
 *   mask_extents      (batch, num_levels) int32 words vh | vw << 16 written by semidetr_msda_mask_extents for THIS padding_mask
 *                     and level table, or NULL.  DETR's masks mark the band below / right of each image inside the batch canvas
 *                     (transformer.py:1268-1288), so "pixel (y, x) of level l is padding iff y >= vh or x >= vw" describes them
 *                     exactly; with it the kernels test a corner with two compares instead of a dependent byte load (which
 *                     cost +15 % on every kernel).  A level whose mask is not of that form carries -1 and its corners read
 *                     their bytes, as all corners do when mask_extents is NULL: the results are the mask's either way.
 *   grad_sampling_offsets / grad_attn_logits: same shapes, every element written.
 * (The gradient w.r.t. reference_points, when a caller needs it, follows from grad_sampling_offsets on the
 *  host side; the reference detaches reference points between decoder layers, transformer.py:1033.)
 * ------------------------------------------------------------------------------------------- */
int semidetr_msda_fused_forward_f32(void *stream, const float *value, const int64_t *spatial_shapes,
                                    const int64_t *level_start, const float *reference_points, int ref_dim,
                                    const float *sampling_offsets, const float *attn_logits,
                                    const unsigned char *padding_mask, const int *mask_extents, int batch,
                                    int spatial_size, int num_heads, int channels, int num_levels,
                                    int num_query, int num_point, int flags, float *out);
int semidetr_msda_fused_backward_f32(void *stream, const float *grad_out, const float *value,
                                     const int64_t *spatial_shapes, const int64_t *level_start,
                                     const float *reference_points, int ref_dim,
                                     const float *sampling_offsets, const float *attn_logits,
                                     const unsigned char *padding_mask, const int *mask_extents, int batch,
                                     int spatial_size, int num_heads, int channels, int num_levels,
                                     int num_query, int num_point, int flags, float *grad_value,
                                     float *grad_sampling_offsets, float *grad_attn_logits);
/* ---------------------------------------------------------------------------------------------
 * The f32 entry points with the level table on the host as well (ABI 7, additive).  `host_spatial_shapes`: a HOST copy of
 * spatial_shapes (num_levels x {H, W}, int64) that the caller already holds, or NULL; everything else as in the call of the same name
 * without `_v2`, which is this call with NULL.  The encoder kernels (SEMIDETR_MSDA_QUERIES_ARE_PIXELS) cut the finest level into regions,
 * one workgroup per (image, region, head); with the table on the host the library picks the region grid per launch so that the
 * workgroups fill whole waves of the device's compute units, and launches exactly batch x regions x num_heads of them (see
 * semidetr_msda_set_region_grid below).  The device table stays what the kernels read: a host copy that disagrees with it costs speed,
 * never correctness (a kernel takes no grid coarser than its windows allow, and walks whatever regions the grid size leaves over).
 * Results are the same either way up to fp32 summation order.  NULL, more than 8 levels, or a level of more than 32766 rows or
 * columns: the launch is exactly that of the call without `_v2`.
 * ------------------------------------------------------------------------------------------- */
int semidetr_msda_forward_f32_v2(void *stream, const float *value, const int64_t *spatial_shapes,
                                 const int64_t *level_start, const float *sampling_loc,
                                 const float *attn_weight, int batch, int spatial_size, int num_heads,
                                 int channels, int num_levels, int num_query, int num_point, int flags, float *out,
                                 const int64_t *host_spatial_shapes);
int semidetr_msda_backward_f32_v2(void *stream, const float *grad_out, const float *value,
                                  const int64_t *spatial_shapes, const int64_t *level_start,
                                  const float *sampling_loc, const float *attn_weight, int batch,
                                  int spatial_size, int num_heads, int channels, int num_levels,
                                  int num_query, int num_point, int flags, float *grad_value,
                                  float *grad_sampling_loc, float *grad_attn_weight, const int64_t *host_spatial_shapes);
int semidetr_msda_fused_forward_f32_v2(void *stream, const float *value, const int64_t *spatial_shapes,
                                       const int64_t *level_start, const float *reference_points, int ref_dim,
                                       const float *sampling_offsets, const float *attn_logits,
                                       const unsigned char *padding_mask, const int *mask_extents, int batch,
                                       int spatial_size, int num_heads, int channels, int num_levels,
                                       int num_query, int num_point, int flags, float *out,
                                       const int64_t *host_spatial_shapes);
int semidetr_msda_fused_backward_f32_v2(void *stream, const float *grad_out, const float *value,
                                        const int64_t *spatial_shapes, const int64_t *level_start,
                                        const float *reference_points, int ref_dim,
                                        const float *sampling_offsets, const float *attn_logits,
                                        const unsigned char *padding_mask, const int *mask_extents, int batch,
                                        int spatial_size, int num_heads, int channels, int num_levels,
                                        int num_query, int num_point, int flags, float *grad_value,
                                        float *grad_sampling_offsets, float *grad_attn_logits,
                                        const int64_t *host_spatial_shapes);
/* Summarise a padding mask for the two calls above: one small launch (batch x num_levels workgroups, reads the mask once).
 *   extents (batch, num_levels) int32: vh | vw << 16 when level l of image n is padded exactly on rows >= vh and columns >= vw
 *   (no padding: H_l | W_l << 16; everything padded: 0), -1 otherwise (and for levels of more than 32767 rows / columns).  Valid for as long as the mask bytes and the
 *   level table do not change; the reference builds one mask per batch and hands it to all twelve layers
 *   (transformer.py:1309,1380), so one call per batch serves 12 forward + 12 backward launches. */
int semidetr_msda_mask_extents(void *stream, const unsigned char *padding_mask, const int64_t *spatial_shapes,
                               const int64_t *level_start, int batch, int spatial_size, int num_levels, int *extents);

/* ---------------------------------------------------------------------------------------------
 * Which kernel runs the encoder self-attention FORWARD (SEMIDETR_MSDA_QUERIES_ARE_PIXELS, num_point == 4, four or five levels;
 * with or without a padding mask).  The reference has one kernel for everything (ms_deform_im2col_cuda.cuh:237-299); here two
 * produce the same results at different speeds depending on how far the learned offsets reach:
 *   patch kernel   -- 4 x 8 query patches, every corner row through the vector-memory path; insensitive to the offsets
 *   window kernel  -- regions of up to 25 x 16 pixels, the coarse levels' corner rows from LDS windows +- 5 px (five levels: +- 4 px) around
 *                     the region; ~35 % faster while most samples stay inside (sigma <= 2 px), level with the patch kernel when
 *                     ~85 % of them are more than 4 px away (sigma ~8 px at four images, ~6 px for one)
 * policy 0 (default, adaptive): both kernels count, in a few workgroups, the share of samples further than 4 px from their
 *   query's pixel centre; launch k's count reaches the host through mapped pinned memory when launch k + 1 OF THE SAME SLOT starts
 *   (no copy command, no synchronisation) and the NEXT dispatch of that slot moves between the kernels with hysteresis (to the
 *   window kernel below 78 %, back above 86 %; five levels 82 % / 90 %).  State is per (device, slot) -- see
 *   SEMIDETR_MSDA_POLICY_SLOT; launches inside a stream capture keep their slot's kernel of the moment and count nothing.  The
 *   first adaptive dispatch on a device allocates the counters (64 KB of device memory, 4 KB of pinned host memory; the two
 *   allocation calls may synchronise that device once).  Launches of ONE slot on two streams of a device at the same time share
 *   its counter pair: the counts may mix, the results do not depend on them.  The choice makes the forward's last bits depend on
 *   timing: SEMIDETR_MSDA_FIXED_FORWARD (or policy 1) for bitwise reproducible forwards.
 *   LIFETIME of that state: the counters (64 KB of device memory + 4 KB of mapped pinned host memory per device) and the per-slot host words are
 *   allocated at a device's first adaptive dispatch and live until the process ends -- launches in flight reference them, so no call
 *   releases them (semidetr_msda_set_forward_policy only changes how dispatches READ them; a device reset invalidates them like any allocation).
 * policy 1: always the patch kernel.   policy 2: the window kernel whenever it applies.   (Process-wide.)
 * The encoder BACKWARD (four levels) reads the same slot: its small-gradient half runs as the lane-per-sample region-window gather
 *   (msda_gw_d32; whole backward 572 / 635 / 796 us against 659 / 707 / 834 us at sigma 1 / 2 / 3 px, bs 4) while the slot's last
 *   count has fewer than 55 % of the samples further than 4 px away (policy 2: always; policy 1 or no count yet: the patch gather) --
 *   or as SEMIDETR_MSDA_GATHER_WINDOW / _PATCH in the backward's `flags` say (the caller's record of the choice at forward time).
 *   grad_value's summation order is run-dependent either way (fp32 atomics); the two gathers agree to fp32 rounding.
 * If the device does not grant the window kernel its LDS (~150 KB per workgroup) the patch kernel runs instead.
 * semidetr_msda_forward_policy_state[_slot]: for the calling thread's current device and slot (0 without _slot) -- the policy,
 *   the kernel the adaptive policy stands on (0 patch, 1 window), the last far-sample fraction received (-1: none yet), the
 *   number of counts received.
 * ------------------------------------------------------------------------------------------- */
int semidetr_msda_set_forward_policy(int policy);
int semidetr_msda_forward_policy_state(int *policy, int *mode, float *far_fraction, unsigned *updates);
int semidetr_msda_forward_policy_state_slot(int slot, int *policy, int *mode, float *far_fraction, unsigned *updates);
/* What an encoder backward of `slot` issued NOW would pick for its small-gradient half, as the flag to pass later:
 * SEMIDETR_MSDA_GATHER_WINDOW or SEMIDETR_MSDA_GATHER_PATCH (never 0, never an error: an unknown slot / device answers PATCH). */
int semidetr_msda_gather_choice(int slot);

/* ---------------------------------------------------------------------------------------------
 * The REGION GRID of the three encoder window kernels (ABI 7, additive): SEMIDETR_MSDA_GRID_FORWARD the window forward (msda_rw_d32),
 * _GATHER the window gather (msda_gw_d32), _SCATTER the region scatter of grad_value (msda_bwd_scatter_d32_reg).  Each cuts the finest
 * level into nry x nrx regions; ceil(H / RTH) x ceil(W / RTW) -- RTH x RTW the largest region the kernel's windows are sized for -- is the
 * coarsest grid, any finer one gives the same results.
 * semidetr_msda_set_region_grid(kernel, nry, nrx): pin the grid of `kernel` (process-wide; tests, A/B timing); 0, 0: automatic (default).
 *   A pinned count below the coarsest one is raised to it; one above the level's pixels is legal (regions without a level-0 pixel).
 *   Counts up to 32767 each, 2^22 regions at most.
 *   Automatic: with a host table (the `_v2` calls) the grid that minimises ceil(batch x regions x num_heads / slots) x (set-up +
 *   rounds of the largest region), ties to the coarsest; without one the coarsest.
 * semidetr_msda_region_grid_query: what a launch of `kernel` with this host table (or NULL), batch, num_heads on a device of num_cus
 *   compute units takes, pins included; needs no device.  grid6 = {nry, nrx (0, 0: the kernel's own coarsest grid), regions (0: table
 *   unknown -- the grid size is a hint), workgroups = batch x regions x num_heads, 1 if the forward adds its tail-split helpers (one
 *   per compute unit), queries of the largest region}.
 * ------------------------------------------------------------------------------------------- */
#define SEMIDETR_MSDA_GRID_FORWARD 0
#define SEMIDETR_MSDA_GRID_GATHER 1
#define SEMIDETR_MSDA_GRID_SCATTER 2
int semidetr_msda_set_region_grid(int kernel, int nry, int nrx);
int semidetr_msda_region_grid_query(int kernel, const int64_t *host_spatial_shapes, int num_levels, int batch, int num_heads,
                                    int num_cus, int *grid6);

/* Names of the device kernels the LAST semidetr_msda_* call of the calling thread launched ("+"-separated, as the
 * profiler prints their base names), so that a benchmark reports what actually ran instead of a hand-kept table. */
const char *semidetr_msda_last_kernels(void);

/* ---------------------------------------------------------------------------------------------
 * MSDA on fp16 / bf16 value maps (ABI 7, additive): what torch.autocast hands MSDeformAttn
 * (detr_od/models/utils/ops/modules/ms_deform_attn.py:113-120, the "for amp" branch) without the fp32 copies of that branch.
 *
 * value, out, grad_out and grad_value hold `dtype` elements (SEMIDETR_H16_FP16: IEEE binary16, SEMIDETR_H16_BF16: bfloat16),
 * 2-byte aligned; sampling_loc, attn_weight and their gradients are fp32 as above; layouts as above.
 * Contract: every result is the fp32 op applied to the EXACTLY up-cast value / grad_out; out and grad_value are then rounded
 * ONCE, to nearest even, into `dtype` (fp16 overflows to inf as the conversion does); grad_sampling_loc / grad_attn_weight are
 * returned in fp32, unrounded.  Nothing is accumulated in 16 bits, locations and weights are never narrowed, the pixel mapping
 * rounds exactly as in the fp32 op, corners outside a level are never loaded.  forward writes every element of `out`.
 * backward: `workspace` = semidetr_msda_backward_h16_workspace_bytes(batch, spatial_size, num_heads, channels) bytes of device
 *   memory (batch * spatial_size * num_heads * channels floats, 4-byte aligned; 16-byte aligned for the fastest conversion) that
 *   the CALLER has zero-filled on `stream`: grad_value is accumulated there with fp32 atomics and converted by a last kernel,
 *   which writes every element of grad_value.
 * channels == 32, num_heads <= 32, 8-byte aligned value / out / grad_out: the fast kernels (any query set); everything else the
 *   reference accepts under AMP (any channels, any head count, value on any 2-byte boundary): one wavefront per (n, q, m) row.
 * semidetr_msda_h16_last_kernels: as semidetr_msda_last_kernels, for the last semidetr_msda_*_h16 call of the calling thread.
 * ------------------------------------------------------------------------------------------- */
#define SEMIDETR_H16_FP16 0
#define SEMIDETR_H16_BF16 1
int semidetr_msda_forward_h16(void *stream, int dtype, const void *value, const int64_t *spatial_shapes,
                              const int64_t *level_start, const float *sampling_loc, const float *attn_weight,
                              int batch, int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                              int num_point, void *out);
size_t semidetr_msda_backward_h16_workspace_bytes(int batch, int spatial_size, int num_heads, int channels);
int semidetr_msda_backward_h16(void *stream, int dtype, const void *grad_out, const void *value,
                               const int64_t *spatial_shapes, const int64_t *level_start, const float *sampling_loc,
                               const float *attn_weight, int batch, int spatial_size, int num_heads, int channels,
                               int num_levels, int num_query, int num_point, void *workspace, void *grad_value,
                               float *grad_sampling_loc, float *grad_attn_weight);
/* The fused MSDeformAttn prologue / epilogue (semidetr_msda_fused_forward_f32 / _backward_f32 above) on a 16-bit value map (ABI 7,
 * additive): softmax over num_levels * num_point, location arithmetic and the padding mask inside the 16-bit kernels, so that a
 * call under torch.autocast (or of a .half() module) reads the Linear layers' raw 16-bit outputs and no fp32 locations / weights
 * ever exist in memory.
 *   value, out, grad_out, grad_value            `dtype` elements (SEMIDETR_H16_FP16 / _BF16), 8-byte aligned (grad_value: 2-byte)
 *   sampling_offsets, attn_logits and their two gradients   `prologue_type` elements: SEMIDETR_ROW_F32 (below), or the 16-bit type of
 *                                               `dtype` (SEMIDETR_ROW_FP16 with _H16_FP16, SEMIDETR_ROW_BF16 with _H16_BF16); the other
 *                                               16-bit type and any other code: SEMIDETR_E_BADARG.  Offsets 8-byte, logits 4-byte aligned.
 *   reference_points                            fp32 ALWAYS, 8-byte aligned: locations are never narrowed (bf16-rounded points alone
 *                                               leave the fp32 error bound); a 16-bit caller up-casts them, exactly
 *   padding_mask                                (batch, spatial_size) bytes or NULL, as above; every corner tests its byte while the
 *                                               sample records are built -- no mask_extents
 * Contract: every result is the fp32 fused op applied to the EXACTLY up-cast operands: the softmax is computed in fp32, the location is
 * ref + off * scale with the fp32 kernels' own code, the pixel mapping rounds as everywhere.  out, grad_value and 16-bit
 * grad_sampling_offsets / grad_attn_logits are each rounded ONCE to nearest even from the unrounded fp32 value (an fp32 prologue_type
 * returns the two gradients unrounded); nothing is accumulated in 16 bits.  A corner on a padded pixel is never loaded, reads as zero
 * and receives no gradient.  `workspace`: as semidetr_msda_backward_h16 (same size function, zero-filled by the caller).
 * Only the fast kernels exist: channels == 32, num_heads <= 32, num_levels * num_point <= 64 and the alignments above; anything else
 * is SEMIDETR_E_BADARG (there is no generic fused kernel).  No gradient with respect to reference_points.  Both set
 * semidetr_msda_h16_last_kernels. */
int semidetr_msda_fused_forward_h16(void *stream, int dtype, const void *value, const int64_t *spatial_shapes,
                                    const int64_t *level_start, const float *reference_points, int ref_dim,
                                    const void *sampling_offsets, const void *attn_logits, int prologue_type,
                                    const unsigned char *padding_mask, int batch, int spatial_size, int num_heads,
                                    int channels, int num_levels, int num_query, int num_point, void *out);
int semidetr_msda_fused_backward_h16(void *stream, int dtype, const void *grad_out, const void *value,
                                     const int64_t *spatial_shapes, const int64_t *level_start,
                                     const float *reference_points, int ref_dim, const void *sampling_offsets,
                                     const void *attn_logits, int prologue_type, const unsigned char *padding_mask,
                                     int batch, int spatial_size, int num_heads, int channels, int num_levels,
                                     int num_query, int num_point, void *workspace, void *grad_value,
                                     void *grad_sampling_offsets, void *grad_attn_logits);
const char *semidetr_msda_h16_last_kernels(void);

/* ---------------------------------------------------------------------------------------------
 * Hungarian matcher: cost matrix + linear sum assignment + assignment scatter, batched and
 * device-resident (no host round trip inside).
 *
 * Replaces  HungarianAssigner.assign   thirdparty/mmdetection/mmdet/core/bbox/assigners/hungarian_assigner.py:55-188
 *           FocalLossCost/BBoxL1Cost/IoUCost.__call__  .../match_costs/match_cost.py:33-50,83-99,169-185
 *           bbox_overlaps(giou|iou)    .../iou_calculators/iou2d_calculator.py:200-261
 *           scipy.optimize.linear_sum_assignment (call sites hungarian_assigner.py:136,
 *           detr_ssod/models/dino_detr_ssod.py:279) -- third-party scipy, pinned at 1.15.3
 *           the inline twin of the above in DinoDetrSSOD.unsup_loss  detr_ssod/models/dino_detr_ssod.py:248-293
 *
 * A batch holds B independent problems; problem b has Q predictions (same Q for all) and
 * G_b = gt_offsets[b+1] - gt_offsets[b] ground truths (ragged, G_b may be 0).
 *   bbox_pred  (B, Q, 4) fp32  cx,cy,w,h normalised
 *   cls_pred   (B, Q, C) fp32  logits
 *   gt_bboxes  (sumG, 4) fp32  x1,y1,x2,y2 pixels ; gt_labels (sumG,) int64
 *   gt_offsets (B+1,) int32 DEVICE ; img_wh (B, 2) fp32 DEVICE (img_w, img_h)
 *   cost       (Q * sumG) fp32: problem b's matrix is TRANSPOSED-CONTIGUOUS, i.e. element (q, g) lives at
 *              cost[Q*gt_offsets[b] + g*Q + q]  (a (G_b, Q) row-major block; the (Q, G_b) matrix the
 *              reference builds is its transpose view).
 * ------------------------------------------------------------------------------------------- */
typedef struct semidetr_cost_params {
    float cls_weight;   /* FocalLossCost.weight  (DINO config: 2.0)  */
    float alpha;        /* 0.25 */
    float gamma;        /* 2.0  */
    float eps;          /* 1e-12 */
    float reg_weight;   /* BBoxL1Cost.weight (5.0) */
    int   reg_xywh;     /* 1: box_format='xywh', 0: 'xyxy' */
    float iou_weight;   /* IoUCost.weight (2.0) */
    int   iou_giou;     /* 1: 'giou', 0: 'iou' */
    int   pred_xyxy;    /* 0: bbox_pred is cx,cy,w,h (HungarianAssigner.assign); 1: it already is x1,y1,x2,y2
                           (the stand-alone IoUCost.__call__ contract, match_cost.py:169-185) */
} semidetr_cost_params;

int semidetr_match_cost_f32(void *stream, const float *bbox_pred, const float *cls_pred,
                            const float *gt_bboxes, const int64_t *gt_labels,
                            const int32_t *gt_offsets, const float *img_wh, int num_problems,
                            int num_query, int num_classes, int total_gt,
                            const semidetr_cost_params *params /* host */, float *cost);

/* Solve all B assignment problems on the device (one wavefront per problem), bit-exact with
 * scipy.optimize.linear_sum_assignment on the same fp32 matrix (up-cast to fp64 as scipy does).
 *   cost as laid out above.
 *   match_row / match_col (sumK,) int64 with K_b = min(Q, G_b) pairs for problem b stored at
 *       pair_offsets[b] = sum_{b'<b} min(Q, G_b')  -- because Q is shared this is computed on device
 *       from gt_offsets; rows ascending (scipy's output order), cols = matched gt index in the problem.
 *       Either may be NULL.
 *   assigned_gt_inds / assigned_labels (B, Q) int64: hungarian_assigner.py:142-147 scatter
 *       (0 / -1 for unmatched; when G_b == 0: gt_inds = 0, labels = -1). Either may be NULL.
 *   status (B,) int32: 0 ok, 1 infeasible, 2 invalid numeric entries (NaN / -inf) -- scipy raises
 *       ValueError for those; the host wrapper turns them into the same exception.
 *   workspace: device scratch of semidetr_lsap_workspace_bytes(B, Q, maxG) bytes.
 */
int64_t semidetr_lsap_workspace_bytes(int num_problems, int num_query, int max_gt);
int semidetr_lsap_solve(void *stream, const float *cost, const int32_t *gt_offsets,
                        const int64_t *gt_labels, int num_problems, int num_query, int total_gt,
                        int max_gt, int64_t *match_row, int64_t *match_col,
                        int64_t *assigned_gt_inds, int64_t *assigned_labels, int32_t *status,
                        void *workspace);

/* Training targets of all problems from their assignment, one launch.
 * Replaces the tail of  _get_target_single   detr_od/models/dense_heads/dino_detr_ssod_head.py:1170-1205,
 *                                            detr_od/models/dense_heads/dino_detr_head.py:937-980
 *           with PseudoSampler               thirdparty/mmdetection/mmdet/core/bbox/samplers/pseudo_sampler.py:35-41
 *   assigned_gt_inds (B,Q) int64 from semidetr_lsap_solve; gt_bboxes / gt_labels / gt_offsets / img_wh as above.
 *   labels (B,Q) int64 = num_classes for background else the gt label; label_weights (B,Q) = 1;
 *   bbox_targets (B,Q,4) = cxcywh(gt / (w,h,w,h)) for positives else 0; bbox_weights (B,Q,4) = 1 / 0;
 *   num_pos (B,) int32 (zeroed inside the call). */
int semidetr_build_targets(void *stream, const int64_t *assigned_gt_inds, const float *gt_bboxes,
                           const int64_t *gt_labels, const int32_t *gt_offsets, const float *img_wh,
                           int num_problems, int num_query, int64_t num_classes, int64_t *labels,
                           float *label_weights, float *bbox_targets, float *bbox_weights, int32_t *num_pos);

/* The three calls above as ONE call that needs no staging: cost, then assignment, then (where asked) the training targets, back
 * to back on `stream`.  The ground truths stay where the caller has them: problem b reads boxes[b] ((count[b], 4) fp32
 * contiguous, 16-byte aligned) and labels[b] ((count[b],) int64) through the table below, which travels BY VALUE in the kernel
 * arguments together with the exclusive offsets and the image sizes -- no device allocation, no copy command, and the launch has
 * copied the block when the call returns (nothing has to outlive it but the tensors the pointers name, until the kernels ran).
 * Same kernels, same arithmetic and same outputs as the three calls on the concatenated ground truths.
 *   SEMIDETR_MATCH_TABLE = 64 problems: sizeof(semidetr_match_table) = 2056 bytes, and the largest argument block of the three
 *   kernels (the assignment's) is 2136 bytes of the 4096 the HIP runtime accepts for one launch.  (A loss() call of the benchmark
 *   has 28 problems, one of the warm-up stage 35; callers with more take the three calls above.)
 *   table (host): num_problems in [1, SEMIDETR_MATCH_TABLE]; offsets[b] = sum of count[:b], offsets[num_problems] = total;
 *       img_wh[b] = (img_w, img_h); entries past num_problems are ignored; boxes[b] / labels[b] may be NULL where count[b] == 0.
 *   cost (Q * total) fp32 as laid out above; match_row .. workspace as semidetr_lsap_solve takes them.
 *   target_labels NULL: no targets.  Otherwise target_labels .. num_pos as semidetr_build_targets' labels .. num_pos, and
 *   assigned_gt_inds is required. */
#define SEMIDETR_MATCH_TABLE 64
typedef struct semidetr_match_table {
    int num_problems;
    int32_t count[SEMIDETR_MATCH_TABLE];
    int32_t offsets[SEMIDETR_MATCH_TABLE + 1];
    float img_wh[SEMIDETR_MATCH_TABLE][2];
    const float *boxes[SEMIDETR_MATCH_TABLE];
    const int64_t *labels[SEMIDETR_MATCH_TABLE];
} semidetr_match_table;
int semidetr_hungarian_assign_f32(void *stream, const float *bbox_pred, const float *cls_pred,
                                  const semidetr_match_table *table /* host */, int num_query, int num_classes,
                                  const semidetr_cost_params *params /* host */, float *cost, int64_t *match_row,
                                  int64_t *match_col, int64_t *assigned_gt_inds, int64_t *assigned_labels, int32_t *status,
                                  void *workspace, int64_t target_num_classes, int64_t *target_labels, float *label_weights,
                                  float *bbox_targets, float *bbox_weights, int32_t *num_pos);

/* ---------------------------------------------------------------------------------------------
 * Mean-teacher EMA, one launch for the whole parameter list.
 *
 * Replaces  MeanTeacher.momentum_update   detr_ssod/utils/hooks/mean_teacher.py:60-64
 *           (tgt.mul_(m).add_(src, alpha=1-m) per parameter => ~1000 launches per step).
 *   teacher_ptrs / student_ptrs (T,) device arrays of device pointers (float*), numels (T,) int64
 *   device array, block_starts (T+1,) int32 device array = exclusive prefix sum of
 *   ceil(numel / SEMIDETR_EMA_CHUNK) -- one workgroup processes one chunk.
 *   Arithmetic per element: t = rn(t * (float)m); t = fma(s, (float)(1-m), t)   (torch's rounding).
 * ------------------------------------------------------------------------------------------- */
#define SEMIDETR_EMA_CHUNK 8192
int semidetr_ema_multi_f32(void *stream, float *const *teacher_ptrs, const float *const *student_ptrs,
                           const int64_t *numels, const int32_t *block_starts, int num_tensors,
                           int total_blocks, double momentum);
/* Same arithmetic on one flat arena (parameters laid out contiguously in HBM). */
int semidetr_ema_flat_f32(void *stream, float *teacher, const float *student, int64_t numel,
                          double momentum);

/* ---------------------------------------------------------------------------------------------
 * Pseudo-label filter: per image mean+std score threshold, then drop empty boxes; one launch for
 * the batch.
 *
 * Replaces  the per-image loop in DinoDetrSSOD.extract_teacher_info  detr_ssod/models/dino_detr_ssod.py:918-939
 *   proposals (sumK, 5) fp32 x1,y1,x2,y2,score ; labels (sumK,) int64 ; prop_offsets (B+1,) int32 DEVICE:
 *   image b's proposals are rows [prop_offsets[b], prop_offsets[b+1]); with prop_counts (B,) int32 DEVICE
 *   (nullable) only the first prop_counts[b] of them exist -- the padded layout semidetr_pseudo_nms_f32 emits.
 *   out_boxes (sumK,4), out_labels (sumK,), out_scores (sumK,): image b's kept entries are written
 *   compacted, in the original order, starting at prop_offsets[b]; out_count (B,) int32 kept per image;
 *   out_thr (B,) fp32 the threshold used (NaN for <2 proposals, as torch.std gives).
 * ------------------------------------------------------------------------------------------- */
int semidetr_pseudo_label_filter_f32(void *stream, const float *proposals, const int64_t *labels,
                                     const int32_t *prop_offsets, const int32_t *prop_counts,
                                     int num_images, float *out_boxes,
                                     int64_t *out_labels, float *out_scores, int32_t *out_keep_idx,
                                     int32_t *out_count, float *out_thr);

/* ---------------------------------------------------------------------------------------------
 * Teacher test-time box decoding for pseudo labels, whole batch, no host
 * round trip: sigmoid, cxcywh -> clamped pixel xyxy, score threshold, class-aware greedy NMS, the
 * max_per_img best by score.
 *
 * Replaces  DINODETRSSODHead._get_bboxes_single(for_pseudo_label=True)
 *               detr_od/models/dense_heads/dino_detr_ssod_head.py:1364-1395 (called per image from :1320-1331)
 *           multiclass_nms  thirdparty/mmdetection/mmdet/core/post_processing/bbox_nms.py:8-95
 *           mmcv.ops.batched_nms / nms (mmcv-full 1.3.16, un-vendored: README.md:11,30)
 *   cls_logits (B,Q,C) fp32 raw logits of the last decoder layer; bbox_pred (B,Q,4) fp32 normalised cxcywh;
 *   img_hw (B,2) fp32 DEVICE = img_meta['img_shape'][:2] (height, width); Q <= 2048; 1 <= max_per_img <= 2048.
 *   workspace: semidetr_nms_workspace_bytes(B,Q,C) bytes of device memory, 16-byte aligned.
 *   out_dets (B,max_per_img,5) x1,y1,x2,y2,score; out_labels (B,max_per_img) int64; out_count (B,) int32:
 *   image b's detections are the first out_count[b] rows of its slice, by descending score (equal logits:
 *   ascending query*C + class; the reference's order of exact ties is unspecified).
 * ------------------------------------------------------------------------------------------- */
size_t semidetr_nms_workspace_bytes(int batch, int num_query, int num_classes);
int semidetr_pseudo_nms_f32(void *stream, const float *cls_logits, const float *bbox_pred, const float *img_hw,
                            int batch, int num_query, int num_classes, float score_thr, float iou_thr,
                            int max_per_img, void *workspace, size_t workspace_bytes, float *out_dets,
                            int64_t *out_labels, int32_t *out_count);

/* ---------------------------------------------------------------------------------------------
 * Weak -> strong augmentation warp of the pseudo boxes, one launch for the batch.
 *
 * Replaces  Transform2D.transform_bboxes  detr_ssod/models/utils/bbox_utils.py:167-192 (bbox2points :18-25,
 *           points2bbox :28-41), called through DinoDetrSSOD._transform_bbox  detr_ssod/models/dino_detr_ssod.py:804-807
 *   boxes: rows of box_stride (>= 4) floats, x1,y1,x2,y2 first; image b owns rows [box_offsets[b], +n_b) with
 *   n_b = box_counts[b] if box_counts else box_offsets[b+1] - box_offsets[b] (both int32 DEVICE arrays);
 *   max_boxes_per_image >= every n_b (grid sizing); matrices (B,3,3) row major fp32; out_hw (B,2) fp32 (h, w)
 *   of the target image; out_boxes rows of 4 floats at the same row indices.
 * ------------------------------------------------------------------------------------------- */
int semidetr_transform_bboxes_f32(void *stream, const float *boxes, int box_stride, const int32_t *box_offsets,
                                  const int32_t *box_counts, int num_images, int max_boxes_per_image,
                                  const float *matrices, const float *out_hw, float *out_boxes);

/* The teacher's chain semidetr_pseudo_nms_f32 -> semidetr_pseudo_label_filter_f32 as ONE call, and the warp in a form that reads
 * every image's boxes where they are; the small per-image arguments travel BY VALUE in the kernel arguments (no device
 * allocation, no copy command; the launch has copied the block when the call returns).  Same kernels and same bits as the calls
 * above.  SEMIDETR_IMAGE_TABLE = 64 images: sizeof(semidetr_image_sizes) = 516 and sizeof(semidetr_box_table) = 2312 bytes of the
 * 4096 bytes of kernel arguments the HIP runtime accepts for one launch; callers with more images take the calls above.
 *   semidetr_teacher_pseudo_labels_f32: img_hw (host) holds num_images in [1, SEMIDETR_IMAGE_TABLE] and (height, width) per image.
 *       The filter reads the NMS's padded output (image b's rows start at b * max_per_img).  counts (2, B) int32: row 0 the NMS's
 *       out_count, row 1 the filter's -- one buffer for the one read-back.  out_dets / out_det_labels as semidetr_pseudo_nms_f32's
 *       out_dets / out_labels; out_boxes (B * max_per_img, 4), out_labels, out_scores (B * max_per_img,), out_thr (B,) as the
 *       filter's.
 *   semidetr_transform_bboxes_table_f32: table (host): image b has count[b] boxes, rows of box_stride[b] (>= 4) floats at boxes[b]
 *       (x1,y1,x2,y2 first), its (3,3) row-major fp32 matrix at matrix[b] (DEVICE pointers), out_hw[b] = (h, w) of the target
 *       image, and its warped boxes go to rows [out_offset[b], +count[b]) of out_boxes (rows of 4 floats).  boxes[b] / matrix[b] may
 *       be NULL where count[b] == 0. */
#define SEMIDETR_IMAGE_TABLE 64
typedef struct semidetr_image_sizes {
    int num_images;
    float hw[SEMIDETR_IMAGE_TABLE][2];
} semidetr_image_sizes;
typedef struct semidetr_box_table {
    int num_images;
    int32_t count[SEMIDETR_IMAGE_TABLE];
    int32_t box_stride[SEMIDETR_IMAGE_TABLE];
    int32_t out_offset[SEMIDETR_IMAGE_TABLE];
    float out_hw[SEMIDETR_IMAGE_TABLE][2];
    const float *boxes[SEMIDETR_IMAGE_TABLE];
    const float *matrix[SEMIDETR_IMAGE_TABLE];
} semidetr_box_table;
int semidetr_teacher_pseudo_labels_f32(void *stream, const float *cls_logits, const float *bbox_pred,
                                       const semidetr_image_sizes *img_hw /* host */, int num_query, int num_classes,
                                       float score_thr, float iou_thr, int max_per_img, void *workspace, size_t workspace_bytes,
                                       float *out_dets, int64_t *out_det_labels, float *out_boxes, int64_t *out_labels,
                                       float *out_scores, int32_t *counts, float *out_thr);
int semidetr_transform_bboxes_table_f32(void *stream, const semidetr_box_table *table /* host */, float *out_boxes);

/* ---------------------------------------------------------------------------------------------
 * One-to-many (task-aligned) assigner of the warm-up stage + its training targets (SURVEY.md section 8(f)
 * row 4), all (layer, image) problems of a loss() call in one launch.
 *
 * Replaces  O2MAssigner.assign  detr_od/core/bbox/assigners/o2m_assigner.py:50-170 (teacher_assign=False, or
 *           teacher_assign=True with multiple_pos=False via candidate_topk = 1)
 *           the in_warm_up branch of DINODETRSSODHead._get_target_single
 *               detr_od/models/dense_heads/dino_detr_ssod_head.py:1108-1165
 * Batch layout as semidetr_match_cost_f32 (gt_offsets (B+1,) int32 DEVICE, img_wh (B,2) fp32 DEVICE = (w, h)),
 * but cls_prob (B,Q,C) holds PROBABILITIES (the call site passes cls_score.sigmoid(), head.py:1111).
 * max_gt_per_problem >= every G_b (<= 1024); Q <= 2048; candidate_topk <= Q unless total_gt == 0.
 * dynamic_k != 0 = the `teacher_assign and multiple_pos` option (o2m_assigner.py:125-133): per ground truth the first k_g of its
 * top-candidate_topk candidates are positive whatever their metric, k_g = max(1, int(sum of its candidate_topk largest IoUs)).
 * Outputs, all (B,Q[,4]):
 *   gt_inds int64 (0 background, g+1 positive), labels int64 (class of the gt or -1),
 *   max_overlaps fp32 (IoU with the assigned gt; -1e8 when unassigned; 0 for a problem without gts),
 *   assign_metrics fp32 (score^alpha * IoU^beta of the assigned pair, else 0),
 *   labels_full int64 (class or num_classes), bbox_targets fp32 (gt as normalised cx,cy,w,h, else 0),
 *   norm_metrics fp32 = metric / (max metric of the gt's positives + 10e-8) * max IoU of the gt's positives.
 * ------------------------------------------------------------------------------------------- */
int semidetr_o2m_assign_f32(void *stream, const float *bbox_pred, const float *cls_prob, const float *gt_bboxes,
                            const int64_t *gt_labels, const int32_t *gt_offsets, const float *img_wh,
                            int num_problems, int num_query, int num_classes, int total_gt,
                            int max_gt_per_problem, int candidate_topk, int dynamic_k, float alpha, float beta,
                            int64_t *gt_inds, int64_t *labels, float *max_overlaps, float *assign_metrics,
                            int64_t *labels_full, float *bbox_targets, float *norm_metrics);

/* ---------------------------------------------------------------------------------------------
 * Task-aligned focal loss of the warm-up stage, fused with the sigmoid in front of it; loss sum and (optionally)
 * its gradient w.r.t. the logits in one streaming pass, deterministic summation.
 *
 * Replaces  task_aigned_focal_loss / TaskAlignedFocalLoss  detr_od/models/losses/task_aligned_focal_loss.py:35-66,:166-200
 *           as called at  detr_od/models/dense_heads/dino_detr_ssod_head.py:693-694  (prob = cls_scores.sigmoid())
 *   logits (N,C) fp32 (input_is_prob != 0: they already are probabilities, the reference module's contract, and the
 *   gradient is d/d prob); labels (N,) int64 in [0, C] (C = background); metrics (N,) fp32 normalised alignment metrics;
 *   workspace: semidetr_tal_loss_workspace_bytes() bytes of device memory;
 *   loss_sum (1,) fp32 = sum_ic |s - p|^gamma * BCE(p, s)  (the caller divides by avg_factor / applies loss_weight);
 *   grad_logits (N,C) fp32 or NULL = d loss_sum / d logits.
 * ------------------------------------------------------------------------------------------- */
size_t semidetr_tal_loss_workspace_bytes(void);
int semidetr_tal_loss_f32(void *stream, const float *logits, const int64_t *labels, const float *metrics,
                          int64_t num_rows, int num_classes, float gamma, int input_is_prob, void *workspace,
                          float *loss_sum, float *grad_logits);

/* ---------------------------------------------------------------------------------------------
 * Cost-GMM double filter of the unsupervised loss (ABI 7, additive): matched costs at the LSAP pairs, a two-component
 * one-feature Gaussian-mixture threshold over them (one rank or all ranks), then the two pseudo-label index sets.
 *
 * Replaces  the per-image loop + concat_all_gather + _fit_gmm + the per-image filter of DinoDetrSSOD.unsup_loss
 *               detr_ssod/models/dino_detr_ssod.py:243-353, DinoDetrSSOD._fit_gmm :832-890 (sklearn GaussianMixture,
 *               covariance_type 'diag', weights_init [.5,.5], means_init [min,max], precisions_init [[1],[1]])
 *
 * semidetr_gmm_match_costs_f32: cost (match_cost layout of semidetr_match_cost_f32), gt_offsets (B+1,) int32, pair_offsets
 *   (B+1,) int32 DEVICE (image b's LSAP pairs are rows/cols [pair_offsets[b], pair_offsets[b+1]) of semidetr_lsap_solve);
 *   num_pairs (host) = pair_offsets[B] <= capacity.  out_seg[k] = cost[rows[k], cols[k]] of problem b, out_count (1,)
 *   int32 = num_pairs: one segment of the padded buffer semidetr_gmm_fit_f64 reads.
 * semidetr_gmm_fit_f64: num_segments segments, segment s = values[s * value_stride + j], j < counts[s * count_stride]
 *   (DEVICE int32, each in [0, capacity]); the fit runs over their concatenation in segment order.  covariance_type must be
 *   SEMIDETR_GMM_COVARIANCE_DIAG.  One workgroup, fp64, scikit-learn 1.7.2's EM step for step.  out_thr (1,) fp32: 0 for no
 *   point, the point for one, otherwise the cost of the best-scoring component-0 point (component 1 if component 0 is
 *   empty; equal scores -> the smaller cost).  out_labels (n,) int32 / out_scores (n,) fp64 (nullable) = predict /
 *   score_samples in the concatenated order (NaN scores for n < 2).  out_info (4,) int32 = n_iter, converged, error
 *   (0 ok, 1 a covariance <= 0 -- sklearn raises there --, 2 a count outside [0, capacity]; out_thr is NaN on error), n.
 * semidetr_gmm_double_filter_f32: per image b (gt rows [gt_offsets[b], gt_offsets[b+1]), at most max_gt <= slot and
 *   <= 8192 of them): keep_base = {g : gt_scores[g] >= base_thr}, keep_gmm = {cols[k] : seg_costs[k] <= *thr} over the
 *   image's pairs; boxes (sumG,4) fp32.  Ascending indices, written from b * slot: out_base_* = gt_* at keep_base,
 *   out_gmm_* = gt_* and out_det_* = det_* at keep_base | keep_gmm; out_counts (2,B) int32 = (|keep_base|, |union|).
 * ------------------------------------------------------------------------------------------- */
#define SEMIDETR_GMM_COVARIANCE_DIAG 1
int semidetr_gmm_match_costs_f32(void *stream, const float *cost, const int32_t *gt_offsets, const int32_t *pair_offsets,
                                 const int64_t *rows, const int64_t *cols, int num_images, int num_query, int num_pairs,
                                 int capacity, float *out_seg, int32_t *out_count);
int semidetr_gmm_fit_f64(void *stream, const float *values, int64_t value_stride, const int32_t *counts,
                         int64_t count_stride, int num_segments, int capacity, int covariance_type, double reg_covar,
                         double tol, int max_iter, float *out_thr, int32_t *out_labels, double *out_scores,
                         int32_t *out_info);
int semidetr_gmm_double_filter_f32(void *stream, const float *seg_costs, const int32_t *pair_offsets, const int64_t *cols,
                                   const float *thr, const float *gt_bboxes, const int64_t *gt_labels,
                                   const float *gt_scores, const float *det_bboxes, const int64_t *det_labels,
                                   const float *det_scores, const int32_t *gt_offsets, int num_images, int max_gt,
                                   float base_thr, int slot, float *out_base_boxes, int64_t *out_base_labels,
                                   float *out_base_scores, float *out_gmm_boxes, int64_t *out_gmm_labels,
                                   float *out_gmm_scores, float *out_det_boxes, int64_t *out_det_labels,
                                   float *out_det_scores, int32_t *out_counts);

/* ---------------------------------------------------------------------------------------------
 * Set-prediction losses of the SSOD head (ABI 7, additive): sigmoid focal (task-aligned focal in warm-up), L1 on cxcywh
 * (all / xy / hw) and GIoU on image-scale xyxy, for every (segment, layer) of one loss() call, deterministic sums.
 *
 * Replaces  DINODETRSSODHead.loss / loss_single / loss_single_dn / get_targets_dn / _get_target_single_dn
 *               detr_od/models/dense_heads/dino_detr_ssod_head.py:508-985, with mmdet FocalLoss (py_sigmoid_focal_loss),
 *               L1Loss, GIoULoss + bbox_overlaps(mode='giou', is_aligned=True)
 *
 * A segment is (num_layers, num_images, num_query, num_classes) of logits (class dimension unit stride, other strides in
 * elements: layer, image, query) and boxes (cxcywh, coordinate dimension unit stride; NULL: no box terms) plus its targets:
 *   MATCHED / WARMUP: labels (nl*B, Q) int64 in [0, C] (C = background), label_weights (nl*B, Q) (NULL = 1; MATCHED only),
 *     bbox_targets / bbox_weights (nl*B, Q, 4), metrics (nl*B, Q) normalised alignment metrics (WARMUP only; the
 *     classification term is then the task-aligned focal loss of semidetr_tal_loss_f32 on the logits, box terms cover the
 *     rows with label < C only);
 *   DN: built in the kernel from gt_offsets (B+1,) int32, gt_boxes (sumG, 4) xyxy image scale, gt_labels (sumG,) int64,
 *     single_pad, dn_groups (num_query = single_pad * dn_groups, every G_b <= single_pad): row q of image b is positive iff
 *     q % single_pad < G_b, label_weights = 1 if G_b > 0 else 0 (_get_target_single_dn).
 *   img_wh (B, 2) fp32 (w, h) of each image: the GIoU scale factors (and the dn targets' normalisation).
 * Per (segment, layer) t (segments in table order, layers ascending):
 *   stats (T, 10) fp64 = cls sum, L1 sum, L1 xy, L1 hw, GIoU sum (weight mean_k w_k), rows with label < C, rows with
 *     sum_k w_k > 0, rows with any w_k > 0, sum over rows with label < C of w_0, sum of metrics;
 *   norms (T, 2) fp32 = normaliser inputs before any cross-rank mean (cls: num_pos + num_neg * bg_cls_weight, or the
 *     metric sum in WARMUP; reg: rows with sum w > 0 (MATCHED), num_pos (DN), sum w_0 of positives (WARMUP));
 *   losses / scales (T, 5) fp32 in the order cls, bbox (L1), iou, bbox_xy, bbox_hw: scale = loss_weight / max(norm, 1)
 *     (0 for iou when no bbox weight is > 0), loss = sum * scale.
 * forward: the two launches; losses / scales NULL -> not finalized (several ranks: all-reduce-mean the norms, then
 *   finalize, which takes the reduced reg normaliser always and the reduced cls one for WARMUP or sync_cls).
 * backward: grad_logits (nl, B, Q, C) / grad_boxes (nl, B, Q, 4) dense fp32 of each segment (NULL: not wanted) =
 *   sum_k scales[t, k] * grad_out[t, k] * d sum_k / d input (scales NULL = 1); grad_out (T, 5) fp32.
 * Limits: <= 3 segments, <= 64 (segment, layer) pairs, rows * C < 2^31 per segment.
 * ------------------------------------------------------------------------------------------- */
#define SEMIDETR_SET_LOSS_MATCHED 0
#define SEMIDETR_SET_LOSS_DN 1
#define SEMIDETR_SET_LOSS_WARMUP 2
#define SEMIDETR_SET_LOSS_MAX_SEGMENTS 3
#define SEMIDETR_SET_LOSS_MAX_LAYERS 64
#define SEMIDETR_SET_LOSS_NUM_STATS 10
#define SEMIDETR_SET_LOSS_NUM_TERMS 5
typedef struct semidetr_set_loss_segment {
    int kind, num_layers, num_images, num_query, num_classes;
    const float *logits;
    int64_t logit_stride[3];
    const float *boxes;
    int64_t box_stride[3];
    const int64_t *labels;
    const float *label_weights, *bbox_targets, *bbox_weights, *metrics;
    const int32_t *gt_offsets;
    const float *gt_boxes;
    const int64_t *gt_labels;
    int single_pad, dn_groups;
    const float *img_wh;
    float alpha, gamma, cls_weight, l1_weight, iou_weight, iou_eps, bg_cls_weight;
    int sync_cls;
    float *grad_logits, *grad_boxes;
} semidetr_set_loss_segment;
int64_t semidetr_set_loss_workspace_bytes(const semidetr_set_loss_segment *segs, int num_segments);
int semidetr_set_loss_forward_f32(void *stream, const semidetr_set_loss_segment *segs, int num_segments, void *workspace,
                                  int64_t workspace_bytes, double *stats, float *norms, float *losses, float *scales);
int semidetr_set_loss_finalize_f32(void *stream, const semidetr_set_loss_segment *segs, int num_segments,
                                   const double *stats, const float *norms_local, const float *norms_reduced,
                                   float *losses, float *scales);
int semidetr_set_loss_backward_f32(void *stream, const semidetr_set_loss_segment *segs, int num_segments,
                                   const float *scales, const float *grad_out);

/* ---------------------------------------------------------------------------------------------
 * De-noising and consistency queries (ABI 7, additive): the producer of the `dn_meta` that the DN segment above consumes.
 *
 * Replaces  prepare_for_cdn / prepare_for_cdn_plus   detr_od/models/dense_heads/dn_components.py:6-125,128-274
 *           DinoDetrSSOD.prepare_unsup_cdn           detr_ssod/models/dino_detr_ssod.py:484-760
 *           (without RoIAlign and the projector, which stay calls of the caller)
 *
 * Every size follows from the LENGTHS of the per-image lists, which the caller has on the host, so the tables below are
 * host data passed by value and nothing is read back.  A layout places N = offsets[num_images] list rows into
 * (num_images, groups * single_pad) slots: slot s = i * single_pad + j of image b holds row k = i * N + offsets[b] + j iff
 * j < offsets[b + 1] - offsets[b]; the other slots are padding.  K = groups * N rows exist in all.
 *
 * semidetr_dn_build_f32 -- one launch, three jobs on disjoint workgroups, every element of every output written:
 *   (a) the contrastive de-noising queries (dn.groups = 2 * num_dn_group; even i = positive, odd i = negative).  Image b's
 *       ground truths are labels[b] (src_counts[b],) int64 and boxes[b] (src_counts[b] rows of box_stride floats, normalised
 *       cx,cy,w,h first).  An image with src_counts[b] == 0 whose layout count is 1 gets the reference's stand-in: box
 *       (.5,.5,.5,.5), label (int)(image_noise[b] * 80), pad_mask 1.  noise (K, 10) uniform in [0, 1):
 *       column 0 = p (label flipped iff p < label_noise_threshold = label_noise_ratio / 2; <= 0: never),
 *       1 -> new label min((int)(u * num_classes), num_classes - 1) in fp32, 2..5 -> sign (+1 iff u >= .5) of x1,y1,x2,y2,
 *       6..9 = rand_part of x1,y1,x2,y2 (+1 for negatives).  box_noise_scale <= 0: boxes pass unchanged.
 *       query_label (B, pad, hidden) = rows of label_weight (num_embeddings, hidden) at the noised labels (a label outside
 *       the table gives a NaN row), 0 in padding; query_bbox (B, pad, 4) = inverse_sigmoid(noised box, eps 1e-5), 0 in
 *       padding; known_bid / map_known_indice / noised_labels (K,) int64; pad_mask (B, pad) int64 or NULL.
 *   (b) cons_rows != NULL: cons_label (B, cons.groups * cons.single_pad, hidden) = cons_rows (K1, hidden) scattered by `cons`.
 *   (c) attn_mask != NULL: (tgt, tgt) bytes, tgt = pad1 + pad + num_queries with pad1 = cons.groups * cons.single_pad
 *       (cons.groups == 0: no consistency part): mask[r][c] = c < pad1 + pad && (r >= pad1 + pad || group(r) != group(c)),
 *       groups = the cons.groups blocks of cons.single_pad followed by the num_dn_group blocks of 2 * dn.single_pad.
 *       attn_mask must be 16-byte aligned.
 * semidetr_dn_consistency_f32 -- one launch: image b's pseudo boxes pseudo_boxes[b] (src_counts[b] rows of pseudo_stride
 *   floats, x1,y1,x2,y2 pixels of the target view, tgt_wh[b] = (w, h)) -> query_bbox (B, pad1, 4) = inverse_sigmoid of the
 *   normalised, clamped cx,cy,w,h (0 in padding), known_bid (K1,) fp32, map_known_indice (K1,) int64; rois (K1, 5) or NULL
 *   = (image, det_boxes[b] row); loss_weights (K1,) or NULL = loss_weight.  An image without boxes has layout count 1:
 *   its box is (w/4, h/4, 3w/4, 3h/4) of tgt_wh (rois: of src_wh) and its weight 0.
 * semidetr_dn_label_backward_f32 -- grad_weight (num_embeddings, hidden), every element written: row e = sum over k with
 *   noised_labels[k] == e, in ascending k, of grad_query_label[known_bid[k], map_known_indice[k], :].  No atomics: one
 *   workgroup per row, so the result is bitwise reproducible.
 * semidetr_dn_gather_rows_f32 -- grad_rows (K1, hidden) = grad_label (B, pad1, hidden) at the layout's slots (backward of (b)).
 * ------------------------------------------------------------------------------------------- */
#define SEMIDETR_DN_MAX_IMAGES 64
#define SEMIDETR_DN_NOISE_COLS 10
typedef struct semidetr_dn_layout {
    int num_images, single_pad, groups;
    int32_t offsets[SEMIDETR_DN_MAX_IMAGES + 1];   /* HOST values */
} semidetr_dn_layout;
typedef struct semidetr_dn_build {
    semidetr_dn_layout dn, cons;
    int32_t src_counts[SEMIDETR_DN_MAX_IMAGES];
    const int64_t *labels[SEMIDETR_DN_MAX_IMAGES];
    const float *boxes[SEMIDETR_DN_MAX_IMAGES];
    int box_stride, num_known;                      /* num_known = K = dn.groups * dn.offsets[num_images] */
    const float *label_weight;
    int num_embeddings, hidden_dim, num_classes, num_queries;
    const float *noise, *image_noise;
    float label_noise_threshold, box_noise_scale;
    float *query_label, *query_bbox;
    int64_t *known_bid, *map_known_indice, *noised_labels, *pad_mask;
    const float *cons_rows;
    float *cons_label;
    unsigned char *attn_mask;
} semidetr_dn_build;
typedef struct semidetr_dn_consistency {
    semidetr_dn_layout cons;
    int32_t src_counts[SEMIDETR_DN_MAX_IMAGES];
    const float *pseudo_boxes[SEMIDETR_DN_MAX_IMAGES];
    const float *det_boxes[SEMIDETR_DN_MAX_IMAGES];
    int pseudo_stride, det_stride, num_known;       /* num_known = K1 = cons.groups * cons.offsets[num_images] */
    float tgt_wh[SEMIDETR_DN_MAX_IMAGES][2], src_wh[SEMIDETR_DN_MAX_IMAGES][2];
    float *query_bbox, *known_bid;
    int64_t *map_known_indice;
    float *loss_weights, *rois;
    float loss_weight;                              /* written for an image that has boxes (1, or 0 past the warm-up) */
} semidetr_dn_consistency;
int semidetr_dn_build_f32(void *stream, const semidetr_dn_build *params /* host */);
int semidetr_dn_consistency_f32(void *stream, const semidetr_dn_consistency *params /* host */);
int semidetr_dn_label_backward_f32(void *stream, const float *grad_query_label, const int64_t *known_bid,
                                   const int64_t *map_known_indice, const int64_t *noised_labels, int num_known,
                                   int num_images, int pad_size, int hidden_dim, int num_embeddings, float *grad_weight);
int semidetr_dn_gather_rows_f32(void *stream, const semidetr_dn_layout *layout /* host */, const float *grad_label,
                                int hidden_dim, float *grad_rows);

/* ---------------------------------------------------------------------------------------------
 * Two-stage query selection (ABI 7, additive): what DINOTransformer.forward runs between the encoder and the decoder.
 *
 * Replaces  gen_encoder_output_proposals             detr_od/models/utils/transformer.py:525-575 (learnedwh is None)
 *           max(-1) + torch.topk + the three gathers transformer.py:1325-1334
 *           refpoint_embed_undetach.sigmoid()        transformer.py:1398
 *           (the enc_output / enc_output_norm / head GEMMs between them stay calls of the caller)
 *
 * fp32, on `stream`, no host synchronisation, nothing read back; every element of every output is written (no memset).
 *
 * semidetr_qsel_proposals_f32 -- one launch.  memory (N, S, D), padding_mask (N, S) bytes (non-zero = padded), the levels
 *   as (num_levels, 2) int64 (H, W) rows either on the host (validated: they must hold S tokens) or on the device (exactly one
 *   of the two pointers; a device table that does not fit S yields masked tokens, never an out-of-bounds access).  For token
 *   (y, x) of level l:  p = ((x + .5) / valid_W, (y + .5) / valid_H, .05 * 2^l, .05 * 2^l) with valid_H / valid_W the number of
 *   unmasked entries in column 0 / row 0 of the level (IEEE correctly rounded fp32 quotients),
 *   valid = all(p > 0.01f & p < 0.99f) & !mask;  output_proposals (N, S, 4) = valid ? log(p / (1 - p)) : +inf;
 *   output_memory (N, S, D) = valid ? memory : 0;  valid (N, S) bytes.
 * semidetr_qsel_proposals_backward_f32 -- one launch: grad_memory = valid ? grad_output_memory : 0.
 * semidetr_qsel_topk_f32 -- two launches (class max over all CUs; one workgroup per image selects).  logits (N, S, C):
 *   key = max over C (NaN propagates and ranks above +inf, -0 == +0);  indices (N, k) int64 = the k largest keys sorted by
 *   (key descending, token index ascending), a total order;  inverse (N, S) int32 = slot of the token or -1.
 *   workspace: semidetr_qsel_topk_workspace_bytes(N, S) bytes.  k <= min(S, SEMIDETR_QSEL_MAX_K).
 * semidetr_qsel_gather_f32 -- one launch: refpoint (N, k, 4) = rows of coord (N, S, 4), init_box = sigmoid(rows of
 *   proposals), tgt (N, k, D) = rows of memory (N, S, D), ref_enc = sigmoid(refpoint).  An index outside [0, S) gives NaN.
 * semidetr_qsel_gather_backward_f32 -- one launch, no atomics, bitwise reproducible: through `inverse`,
 *   grad_coord (N, S, 4) = grad_refpoint + grad_ref_enc * ref_enc * (1 - ref_enc) of the token's slot, grad_memory (N, S, D)
 *   = grad_tgt of the slot, zero for unselected tokens.  Any of the three incoming gradients may be NULL (= zero), and one
 *   of the two outputs.
 * Limits (SEMIDETR_E_TOOLARGE beyond them): N * S < 2^31, N <= 65535, D <= 65536, and for the two gather entry points
 *   N * k < 2^24.
 * ------------------------------------------------------------------------------------------- */
#define SEMIDETR_QSEL_MAX_LEVELS 8
#define SEMIDETR_QSEL_MAX_K 4096
int semidetr_qsel_proposals_f32(void *stream, const float *memory, const unsigned char *padding_mask,
                                const int64_t *spatial_shapes_host, const int64_t *spatial_shapes_dev, int num_levels, int N,
                                int S, int D, float *output_memory, float *output_proposals, unsigned char *valid);
int semidetr_qsel_proposals_backward_f32(void *stream, const float *grad_output_memory, const unsigned char *valid, int N, int S,
                                         int D, float *grad_memory);
size_t semidetr_qsel_topk_workspace_bytes(int N, int S);
int semidetr_qsel_topk_f32(void *stream, const float *logits, int N, int S, int C, int k, void *workspace,
                           size_t workspace_bytes, int64_t *indices, int32_t *inverse);
int semidetr_qsel_gather_f32(void *stream, const int64_t *indices, const float *coord, const float *proposals,
                             const float *memory, int N, int S, int k, int D, float *refpoint, float *init_box, float *tgt,
                             float *ref_enc);
int semidetr_qsel_gather_backward_f32(void *stream, const int32_t *inverse, const float *grad_refpoint, const float *grad_tgt,
                                      const float *grad_ref_enc, const float *ref_enc, int N, int S, int k, int D,
                                      float *grad_coord, float *grad_memory);

/* ---------------------------------------------------------------------------------------------
 * Detection decode (ABI 7, additive): what evaluation and inference run on every image after the head.
 *
 * Replaces  get_bboxes (for_pseudo_label=False)       detr_od/models/dense_heads/dino_detr_ssod_head.py:1316-1330
 *           _get_bboxes_single, sigmoid + flat topk   dino_detr_ssod_head.py:1366-1369, 1396-1400; dino_detr_head.py:1129-1137
 *           box decode, clamp, rescale, cat           dino_detr_ssod_head.py:1404-1413; dino_detr_head.py:1143-1152
 *           bbox2result                               thirdparty/mmdetection/mmdet/core/bbox/transforms.py:100-117
 *           (the NMS branch of the same function is semidetr_pseudo_nms_f32; the softmax branch, dino_detr_head.py:1138-1141,
 *           is not built)
 *
 * fp32, on `stream`, two launches for the whole batch, no host synchronisation, nothing read back, no memset, no float
 * atomics; bitwise reproducible.
 *
 * semidetr_det_decode_f32 -- cls_logits (B, Q, C) raw logits, bbox_pred (B, Q, 4) normalised cxcywh, img_hw (B, 2) = (height,
 *   width) of img_shape, scale_factor (B, 4) on the device or NULL (rescale=False).  Per image the k largest of the Q * C
 *   LOGITS, sorted by (logit descending, flat index q * C + c ascending): a total order (NaN above +inf, -0 == +0) and one valid
 *   resolution of every tie torch.topk over the sigmoids leaves open.  For rank r with flat index i:
 *     out_labels (B, k) int64 = i % C;  q = i / C;  score = 1 / (1 + exp(-logit))
 *     (x1, y1, x2, y2) = (cx - .5 w, cy - .5 h, cx + .5 w, cy + .5 h) * (W, H, W, H), clamped to [0, W] / [0, H], then, with a
 *     scale_factor, divided by it element-wise (IEEE correctly rounded);  out_dets (B, k, 5) = (x1, y1, x2, y2, score).
 *   With out_dets_by_class (B, k, 5) and out_class_offsets (B, C + 1) int32 (both or neither): the same rows stably partitioned
 *   by label (score order kept inside a class); class c of image b is rows [offsets[b][c], offsets[b][c + 1]).
 *   workspace: semidetr_det_workspace_bytes(batch, num_query, num_classes, k) bytes, 8-byte aligned (0 for sizes outside the
 *   limits); its contents need no initialisation.
 * Limits: 1 <= k <= min(Q * C, SEMIDETR_DET_MAX_K) (SEMIDETR_E_BADARG for k outside [1, Q * C], SEMIDETR_E_TOOLARGE above
 *   SEMIDETR_DET_MAX_K), Q * C < 2^31, batch <= 65535.
 * ------------------------------------------------------------------------------------------- */
#define SEMIDETR_DET_MAX_K 2048
size_t semidetr_det_workspace_bytes(int batch, int num_query, int num_classes, int k);
int semidetr_det_decode_f32(void *stream, const float *cls_logits, const float *bbox_pred, const float *img_hw,
                            const float *scale_factor /* (B, 4) device, NULL = no rescale */, int batch, int num_query,
                            int num_classes, int k, void *workspace, size_t workspace_bytes, float *out_dets /* (B, k, 5) */,
                            int64_t *out_labels /* (B, k) */, float *out_dets_by_class /* (B, k, 5), nullable */,
                            int32_t *out_class_offsets /* (B, C + 1), nullable together */);

/* ---------------------------------------------------------------------------------------------
 * Cross-view query consistency loss (ABI 7, additive): the last block of DinoDetrSSOD.unsup_loss, every decoder layer fused.
 *
 * Replaces  the `for layer_id in range(len(hs_v1))` loop   detr_ssod/models/dino_detr_ssod.py:472-481
 *           (slice, two index gathers, two F.normalize, mse_loss, weights, mean, x 10 -- and their backward)
 *
 *   loss_l = scale * mean over (k, d) of  w_k (y1 - y2)_d^2,   y = x / max(||x||_2, eps),
 *   x1 = hs_v1[l][bid_k, idx_k, :], x2 = hs_v2[l][bid_k, idx_k, :] (detached), k < K = num_known, d < D = dim.
 *
 * fp32, on `stream`, no host synchronisation, nothing read back, no memset, no float atomics; bitwise reproducible.
 * The parameter block is read on the host during the call.  Per layer and view: a base pointer and the batch / query strides in
 * ELEMENTS (the reference's hs[l] is a transposed view of a (Q, B, D) buffer); the last dimension has stride 1, every row
 * starts 16-byte aligned (base aligned, strides multiples of 4).  D % 4 == 0; D == 256 is the tuned instantiation.
 * known_bid is fp32 (what prepare_unsup_cdn produces) or int64 (bid_is_int64); loss_weights (K) may be NULL = all zero (past
 * the warm-up).  The `[:, :pad_size]` slice is a bound: a pair with bid outside [0, batch) or idx outside [0, pad_size) is
 * never dereferenced, it makes every layer's loss NaN and gets no gradient row.  The (bid, idx) pairs must be distinct.
 *
 * semidetr_consis_loss_forward_f32 -- two launches (rows -> fixed partial slots; one workgroup reduces them in index order
 *   in fp64 and builds the inverse map (b, q) -> k in the workspace): losses (num_layers) =
 *   (float)(sum_l * (double)(scale / (K * D))).
 * semidetr_consis_loss_backward_f32 -- one launch; the workspace is the one the forward filled (same parameter block).
 *   grad_losses (num_layers) upstream gradients; layer[l].grad_v1 the DENSE gradient (batch, num_query, D) contiguous of
 *   hs_v1[l], every element written: selected rows get  g / n1 - x1 (x1 . g) / n1^3  with g = 2 c_k (y1 - y2),
 *   c_k = scale w_k upstream_l / (K D)  (n1 < eps: g / eps, torch's clamp_min gate), all other rows zeros.
 * workspace: semidetr_consis_loss_workspace_bytes(num_layers, num_known, batch, pad_size) bytes, 8-byte aligned (0 for sizes
 *   outside the limits); no initialisation needed.
 * Limits: num_layers <= SEMIDETR_CONSIS_MAX_LAYERS, batch * num_query < 2^27, num_known < 2^24.
 * ------------------------------------------------------------------------------------------- */
#define SEMIDETR_CONSIS_MAX_LAYERS 16
typedef struct semidetr_consis_layer {
    const float *v1, *v2;                      /* hs_v1[l], hs_v2[l] */
    int64_t v1_stride[2], v2_stride[2];        /* (batch, query) strides in elements */
    float *grad_v1;                            /* backward only: (batch, num_query, dim) contiguous */
} semidetr_consis_layer;
typedef struct semidetr_consis_loss {
    int num_layers, batch, num_query, dim, pad_size, num_known;
    int bid_is_int64;                          /* known_bid: 0 = float32, 1 = int64 */
    float scale, eps;                          /* 10, 1e-12 in the reference */
    const void *known_bid;                     /* (num_known) */
    const int64_t *map_known_indice;           /* (num_known) */
    const float *loss_weights;                 /* (num_known), NULL = zeros */
    semidetr_consis_layer layer[SEMIDETR_CONSIS_MAX_LAYERS];
} semidetr_consis_loss;
size_t semidetr_consis_loss_workspace_bytes(int num_layers, int num_known, int batch, int pad_size);
int semidetr_consis_loss_forward_f32(void *stream, const semidetr_consis_loss *params /* host */, void *workspace,
                                     size_t workspace_bytes, float *losses);
int semidetr_consis_loss_backward_f32(void *stream, const semidetr_consis_loss *params /* host */, const void *workspace,
                                      size_t workspace_bytes, const float *grad_losses);

/* ---------------------------------------------------------------------------------------------
 * Decoder self-attention core (ABI 7, additive): out = softmax(scale * Q K^T + mask) V and its backward, head dimension 32.
 *
 * Replaces  the attention between the two projections of `self.self_attn(q, k, tgt, attn_mask=self_attn_mask)[0]`
 *           detr_od/models/utils/transformer.py:975-1039 (nn.MultiheadAttention: bmm, mask add, softmax, bmm, head average)
 *
 * fp32 in / arithmetic / out, on `stream`, no host synchronisation, no memset, no float atomics; bitwise reproducible.  The
 * parameter block is read on the host during the call.  q (len_q, batch, heads * 32) and k, v (len_k, batch, heads * 32) are
 * read through their (length, batch) strides in ELEMENTS; the last dimension has stride 1, every row starts 16-byte aligned
 * (base aligned, strides multiples of 4), so the three may be slices of one in-projection output.  out (len_q, batch,
 * heads * 32) and grad_out are contiguous; lse (batch, heads, len_q) is the row log-sum-exp the forward writes and the backward
 * reads.  mask is NULL or (len_q, len_k) bytes, non-zero = blocked, shared by images and heads.  32 x 32 tiles of the mask are
 * classed by one small launch: a tile blocked everywhere is skipped, a tile open everywhere reads no mask byte.  A row with
 * every key blocked is NaN in out; its backward is outside the contract.  head_dim != 32 is SEMIDETR_E_BADARG.
 *
 * semidetr_self_attn_forward_f32  -- two launches (one without a mask): writes out and lse.
 * semidetr_self_attn_backward_f32 -- three launches at most (tile classes; delta = rowsum(dO * O) and dQ; dK and dV).
 *   grad_q / grad_k / grad_v may each be NULL (not computed; at least one is not); they are written through their own
 *   (length, batch) strides, every element of every row.
 * workspace: semidetr_self_attn_workspace_bytes(batch, heads, len_q, len_k) bytes, 16-byte aligned, no initialisation; the
 *   backward may use another one than the forward.
 * Limits: batch * heads <= 65535, len_q and len_k < 2^24.
 * ------------------------------------------------------------------------------------------- */
typedef struct semidetr_self_attn {
    int batch, heads, head_dim, len_q, len_k;
    float scale;
    const float *q, *k, *v;
    int64_t q_stride[2], k_stride[2], v_stride[2];        /* (length, batch) strides in elements */
    const uint8_t *mask;                                  /* (len_q, len_k) or NULL */
    float *out, *lse;                                     /* forward: written; backward: read */
    const float *grad_out;                                /* backward only from here on */
    float *grad_q, *grad_k, *grad_v;
    int64_t gq_stride[2], gk_stride[2], gv_stride[2];
} semidetr_self_attn;
size_t semidetr_self_attn_workspace_bytes(int batch, int heads, int len_q, int len_k);
int semidetr_self_attn_forward_f32(void *stream, const semidetr_self_attn *params /* host */, void *workspace,
                                   size_t workspace_bytes);
int semidetr_self_attn_backward_f32(void *stream, const semidetr_self_attn *params /* host */, void *workspace,
                                    size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * The same core on fp16 / bf16 operands, computed on the 16-bit MFMA (ABI 7, additive): the "operand" arithmetic beside the
 * fp32 one above.  It is a second, named arithmetic with a numerics contract of its own, NOT the fp32 entry points on up-cast
 * operands: the probabilities and dS are rounded to the operand type before their products.
 *
 * `type` is SEMIDETR_ROW_FP16 or SEMIDETR_ROW_BF16 (below) and is the element type of q, k, v, out, grad_out, grad_q, grad_k and
 * grad_v alike; lse and the workspace are fp32.  All of them are read and written in place as 16-bit: no fp32 copy of an
 * operand is made in memory or in LDS.  Layout as above -- q, k, v and the three gradients through their (length, batch)
 * strides in ELEMENTS, last stride 1; out and grad_out contiguous -- but a row starts 8-byte aligned (base 8-byte aligned,
 * strides non-negative multiples of 4), so a 16-bit slice whose rows sit 8 bytes into a 16-byte line is read in place, and
 * grad_q and grad_k may be the two halves of one packed (len, batch, 2 * heads * 32) buffer.  mask, tile classes, the NaN row,
 * launch counts, semidetr_self_attn_workspace_bytes and the limits are those of the fp32 pair.  No float atomics, no memset,
 * every sum in a fixed order: bitwise reproducible.
 *
 * Numerics contract, in this order (u16 = 2^-11 fp16, 2^-8 bf16):
 *   - the scores are the fp32 MFMA sum of the exact products q_id k_jd, times scale in fp32 (the fp32 score is scaled, never q:
 *     32^-0.5 has no 16-bit representation);
 *   - the running maximum, exp2, the row sum l and lse = m + log(l) are fp32, on the UNROUNDED probabilities;
 *   - P is rounded once to the operand type for P V (forward) and P^T dO (dV);
 *   - dP = dO V^T is an fp32 MFMA sum of exact products; delta_i = sum_d dO_id out_id is formed in fp32 from dO and the saved
 *     16-bit out;
 *   - dS = P o (dP - delta) is fp32 from the unrounded P, then rounded once to the operand type for dS K (dQ) and dS^T Q (dK);
 *     scale is applied to the fp32 accumulators of dQ and dK;
 *   - every result (out, grad_q, grad_k, grad_v) is rounded once, to nearest even, on the way out (fp16 overflows to inf).
 * The order and rounding mode of the additions inside a 16-bit MFMA are not documented; the contract takes them as n exact
 * products summed in any order with at most 2 u (u = 2^-24) relative error per addition.
 *
 * semidetr_self_attn_forward_h16  -- two launches (one without a mask): writes out and lse.
 * semidetr_self_attn_backward_h16 -- three launches at most; grad_q / grad_k / grad_v may each be NULL (at least one is not).
 * Checked on the host before any launch: type SEMIDETR_ROW_F32 or unknown, head_dim != 32, a misaligned row, a NULL operand
 * and all three gradients NULL are SEMIDETR_E_BADARG, with a message.
 * ------------------------------------------------------------------------------------------- */
typedef struct semidetr_self_attn_h16 {
    int batch, heads, head_dim, len_q, len_k;
    float scale;
    int type;                                             /* SEMIDETR_ROW_FP16 or SEMIDETR_ROW_BF16: every 16-bit tensor */
    const void *q, *k, *v;
    int64_t q_stride[2], k_stride[2], v_stride[2];        /* (length, batch) strides in elements */
    const uint8_t *mask;                                  /* (len_q, len_k) or NULL */
    void *out;                                            /* forward: written; backward: read */
    float *lse;
    const void *grad_out;                                 /* backward only from here on */
    void *grad_q, *grad_k, *grad_v;
    int64_t gq_stride[2], gk_stride[2], gv_stride[2];
} semidetr_self_attn_h16;
int semidetr_self_attn_forward_h16(void *stream, const semidetr_self_attn_h16 *params /* host */, void *workspace,
                                   size_t workspace_bytes);
int semidetr_self_attn_backward_h16(void *stream, const semidetr_self_attn_h16 *params /* host */, void *workspace,
                                    size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * Residual add + LayerNorm + positional add (ABI 7, additive): the epilogue of a transformer sub-block and the with_pos_embed
 * that opens the next one, row width 256.
 *
 * Replaces  `x = x + dropout(branch); x = norm(x)` and the following `with_pos_embed(x, pos)`
 *           detr_od/models/utils/transformer.py:628-629, 636-637, 789-790, 811-812, 838-839 (and 624, 785)
 *
 *   s = x + residual;  mean = mean(s);  var = mean((s - mean)^2)  (biased, two passes over registers);
 *   rstd = 1 / sqrt(var + eps);  y = (s - mean) * rstd * weight + bias;  q = y + pos.
 *
 * fp32 in / arithmetic / out, on `stream`, no host synchronisation, no memset, no float atomics; bitwise reproducible: the grid,
 * the row -> wave map and the order of every sum depend on rows = rows0 * rows1 alone.  The parameter block is read on the host
 * during the call.  x, residual, pos, gy and gq are (rows0, rows1, dim) tensors read through the strides of their two leading
 * dimensions in ELEMENTS; the last dimension has stride 1 and every row starts 16-byte aligned (base aligned, strides
 * non-negative multiples of 4), so transposed views and slices are read in place.  y, q and grad_x are contiguous
 * (rows0, rows1, dim), mean and rstd contiguous (rows0 * rows1); weight, bias, y, q and grad_x are 16-byte aligned.
 * dim != 256 is SEMIDETR_E_BADARG.
 *
 * semidetr_add_norm_forward_f32  -- one launch.  residual may be NULL (s = x).  pos and q are both NULL or both set.  Writes y,
 *   q, mean, rstd.  Uses no workspace (NULL, 0 is accepted).
 * semidetr_add_norm_backward_f32 -- two launches (one where grad_weight and grad_bias are both NULL).  gy and gq are the
 *   upstream gradients of y and q; either may be NULL, not both.  With g = gy + gq and xhat = (x + residual - mean) * rstd
 *   recomputed from the forward's inputs, mean and rstd:
 *     grad_x = rstd * (g * weight - mean(g * weight) - xhat * mean(g * weight * xhat))   every element written once; it is the
 *              gradient of x AND of residual, and gq is the gradient of pos;
 *     grad_weight = sum_rows g * xhat,  grad_bias = sum_rows g   (each may be NULL): fp32 per lane over the 16 consecutive rows
 *              of a wave in row order, the 4 waves of a workgroup in wave order into one slot of the workspace per 64 rows, the
 *              slots in 16 contiguous chunks in index order in fp64, the chunks in order, one rounding.
 *   bias, y, q and pos are not read.
 * workspace: semidetr_add_norm_workspace_bytes(rows0 * rows1) bytes, 16-byte aligned, no initialisation needed (0 for rows
 *   outside the limits); needed only where grad_weight or grad_bias is asked for.
 * Limits: 1 <= rows0 * rows1 < 2^31, dim == 256.
 * ------------------------------------------------------------------------------------------- */
typedef struct semidetr_add_norm {
    int rows0, rows1, dim;
    float eps;
    const float *x, *residual, *pos;                      /* residual, pos: NULL = absent */
    const float *gy, *gq;                                 /* backward only */
    int64_t x_stride[2], residual_stride[2], pos_stride[2], gy_stride[2], gq_stride[2];   /* in elements */
    const float *weight, *bias;                           /* (dim) */
    float *y, *q;                                         /* forward: written */
    float *mean, *rstd;                                   /* forward: written; backward: read */
    float *grad_x, *grad_weight, *grad_bias;              /* backward: written */
} semidetr_add_norm;
size_t semidetr_add_norm_workspace_bytes(int64_t rows);
int semidetr_add_norm_forward_f32(void *stream, const semidetr_add_norm *params /* host */, void *workspace,
                                  size_t workspace_bytes);
int semidetr_add_norm_backward_f32(void *stream, const semidetr_add_norm *params /* host */, void *workspace,
                                   size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * The same op on rows of mixed element types (ABI 7, additive): what torch.autocast and .half() modules hand the epilogue,
 * without fp32 copies of the operands and without cast passes over the results.
 *
 * Every row operand (x, residual, pos, gy, gq) and every row result (y, q, grad_x, grad_residual, grad_pos) carries its own
 * element type in the `<name>_type` field: SEMIDETR_ROW_F32, SEMIDETR_ROW_FP16 (IEEE binary16) or SEMIDETR_ROW_BF16
 * (bfloat16), in any mixture; the types of the results do not depend on those of the operands.  The type field of a NULL
 * pointer is not read.  weight, bias, mean, rstd, grad_weight, grad_bias and the workspace are fp32.
 * Contract: the arithmetic, the grid, the row -> wave map, the slots and the order of every sum are those of the fp32 entry
 * points above.  A 16-bit operand is up-cast exactly when it is loaded; a 16-bit result is rounded ONCE, to nearest even, from
 * the unrounded fp32 value when it is stored (fp16 overflows to inf, as the conversion does); q is rounded from the unrounded
 * y + pos, never from a rounded y.  So every result is bit for bit the result of the fp32 entry point on the up-cast operands,
 * converted once; mean, rstd, grad_weight and grad_bias are those of the fp32 entry point.
 * Layout: as above -- operands through the strides of their two leading dimensions in ELEMENTS, last stride 1, results
 * contiguous (rows0, rows1, dim).  Alignment per type: an fp32 row starts 16-byte aligned (base 16-byte aligned, strides
 * non-negative multiples of 4); a 16-bit row starts 8-byte aligned (base 8-byte aligned, strides non-negative multiples of 4), so
 * a 16-bit slice whose rows sit at 8 but not 16 bytes is read in place.  A result is 16-byte (fp32) or 8-byte (16-bit) aligned;
 * weight, bias and the workspace 16-byte.
 *
 * semidetr_add_norm_forward_mixed  -- one launch.  Reads x, residual (may be NULL), pos (NULL exactly where q is NULL), weight,
 *   bias.  Writes y, q, mean, rstd.  Uses no workspace (NULL, 0 is accepted).
 * semidetr_add_norm_backward_mixed -- two launches (one where grad_weight and grad_bias are both NULL).  Reads x, residual, gy,
 *   gq (either may be NULL, not both), weight, mean, rstd.  From the one fp32 dx = grad_x of the fp32 entry point it writes
 *     grad_x         in grad_x_type          (the gradient of x),
 *     grad_residual  in grad_residual_type   (the gradient of residual where its type differs from x's; needs residual);
 *   either may be NULL, not both.  grad_pos (may be NULL; needs gq) receives gq converted to grad_pos_type: the gradient of
 *   pos where its type differs from gq's.  grad_weight and grad_bias (each may be NULL) as above; bias, y, q and pos are not read.
 * workspace: semidetr_add_norm_workspace_bytes(rows0 * rows1), as above.
 * Every argument is checked on the host before anything is launched: an unknown type code, a misaligned row, q without pos (or
 * pos without q), no grad_x and no grad_residual, grad_residual without residual, grad_pos without gq and the checks of the
 * fp32 entry points are SEMIDETR_E_BADARG; rows0 * rows1 >= 2^31 is SEMIDETR_E_TOOLARGE.
 * ------------------------------------------------------------------------------------------- */
#define SEMIDETR_ROW_F32 0
#define SEMIDETR_ROW_FP16 1
#define SEMIDETR_ROW_BF16 2
typedef struct semidetr_add_norm_mixed {
    int rows0, rows1, dim;
    float eps;
    const void *x, *residual, *pos;                       /* residual, pos: NULL = absent */
    const void *gy, *gq;                                  /* backward only */
    int64_t x_stride[2], residual_stride[2], pos_stride[2], gy_stride[2], gq_stride[2];   /* in elements */
    const float *weight, *bias;                           /* (dim) */
    void *y, *q;                                          /* forward: written */
    float *mean, *rstd;                                   /* forward: written; backward: read */
    void *grad_x, *grad_residual, *grad_pos;              /* backward: written */
    float *grad_weight, *grad_bias;                       /* backward: written */
    int x_type, residual_type, pos_type, gy_type, gq_type;                        /* SEMIDETR_ROW_* of the operands */
    int y_type, q_type, grad_x_type, grad_residual_type, grad_pos_type;           /* SEMIDETR_ROW_* of the results */
} semidetr_add_norm_mixed;
int semidetr_add_norm_forward_mixed(void *stream, const semidetr_add_norm_mixed *params /* host */, void *workspace,
                                    size_t workspace_bytes);
int semidetr_add_norm_backward_mixed(void *stream, const semidetr_add_norm_mixed *params /* host */, void *workspace,
                                     size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * Input projection: GroupNorm(32, 256) of every pyramid level written straight into the token tensor (ABI 7, additive)
 * (csrc/group_norm_tokens.hip).
 * Replaces, per level l, the GroupNorm of  nn.Sequential(Conv2d, GroupNorm(32, 256))  (dino_detr_ssod_head.py:251-259,
 * dino_detr_head.py:223-231) and, in the transformer,  src.flatten(2).transpose(1, 2),  torch.cat(src_flatten, 1)  and the
 * src + pos  in front of encoder layer 0 (detr_od/models/utils/transformer.py:1276-1287, 635).
 *
 *   per (image n, level l, group g of 8 channels):  mean = mean(x),  var = mean((x - mean)^2)  (biased) over the 8 * hw[l]
 *   elements of the group;  rstd = 1 / sqrt(var + eps);
 *   tokens[n, start[l] + p, c] = (x_l[n, c, p] - mean) * rstd * weight_l[c] + bias_l[c];   q = tokens + pos.
 * A call writes the rows [start[l], start[l] + hw[l]) of its levels and no other row of tokens and q: the levels of a pyramid may
 * be written by more than one call into the same tensors (a level whose input is computed from an earlier level's rows).
 *
 * x[l] is (batch, 256, hw[l]): element (n, c, p) at x[l] + n * x_batch_stride[l] + c * hw[l] + p (every image a contiguous
 * NCHW block; the batch stride, in ELEMENTS, is free), of type x_type (SEMIDETR_ROW_*).  tokens and q are contiguous
 * (batch, S, 256) of type out_type: fp32, or x_type where that is a 16-bit type.  pos (type pos_type, any of the three), gy and gq
 * (type out_type) are (batch, S, 256) read through the strides of their two leading dimensions in ELEMENTS, last stride 1.
 * grad_x[l] is contiguous (batch, 256, hw[l]) of type x_type.  weight[l], bias[l], grad_weight[l], grad_bias[l] are fp32 vectors
 * of 256; mean and rstd are fp32 (batch, levels, 32).  Alignment: x[l], grad_x[l] and every token row 16-byte (fp32) or 8-byte
 * (16-bit), batch strides and token strides multiples of 4 elements, the parameter vectors and the workspace 16-byte.  A plane
 * (n, c) starts wherever c * hw[l] puts it: the kernels read and write planes 16 (8) bytes per lane where hw[l] % 4 == 0 and one
 * element per lane otherwise.
 * Arithmetic in fp32 on exactly up-cast operands; a 16-bit result is rounded once, to nearest even, from the unrounded fp32
 * value (q from the unrounded tokens + pos).  No float atomics, no memset, bitwise reproducible: every grid, map and order of a
 * sum depends on batch, levels and hw[] alone.
 *
 * semidetr_gn_tokens_forward  -- two launches for the whole pyramid.
 *   1. statistics: one workgroup per chunk of 8192 consecutive elements of a group (a group of level l has
 *      ceil(8 * hw[l] / 8192) chunks).  Reads x; writes per chunk its sum and the sum of squared deviations from ITS OWN mean
 *      into the workspace.
 *   2. normalise + transpose: one workgroup per (image, level, tile of 64 pixels).  Reads the chunks of its 32 groups and merges
 *      them in a fixed order in fp64 (mean = sum of sums / count; M2 = sum of (M2_c + count_c * (mean_c - mean)^2); one rounding
 *      each), reads x, weight[l], bias[l] and pos (NULL exactly where q is NULL); writes complete 256-channel rows of tokens
 *      and q through a transposing LDS tile, and mean and rstd (the workgroup of a level's first tile).
 * semidetr_gn_tokens_backward -- three launches, two where every grad_weight[l] and grad_bias[l] is NULL.  gy and gq are the
 *   upstream gradients of tokens and q; either may be NULL, not both; gq itself is the gradient of pos.  With g = gy + gq and
 *   xhat = (x - mean) * rstd recomputed:
 *   1. sums: one workgroup per (image, level, unit of 128 pixels).  Reads x, gy, gq, mean, rstd, weight[l]; writes one slot of
 *      the workspace: per channel sum g * xhat and sum g over its pixels, per group sum g * w and sum g * w * xhat.
 *   2. dx: one workgroup per (image, level, tile of 64 pixels).  Merges the group sums of its level's units in a fixed order in
 *      fp64 (one rounding), reads gy, gq token-major and x, writes
 *      grad_x = rstd * (g * w - mean_group(g * w) - xhat * mean_group(g * w * xhat))  as NCHW through the same tile.
 *   3. parameter reduce: per level, the slots in 16 contiguous parts in index order in fp64, the parts in order, one rounding:
 *      grad_weight[l] = sum g * xhat, grad_bias[l] = sum g  (each may be NULL; a level with both NULL is skipped).
 *   bias, tokens, q and pos are not read.  grad_x[l] is written for every level.
 * workspace: semidetr_gn_tokens_workspace_bytes(params, for_backward) bytes, 16-byte aligned, no initialisation needed; 0 for
 *   a block outside the limits.  The forward and the backward may share one buffer.
 * Checked on the host before any launch (SEMIDETR_E_BADARG, nothing is written): channels != 256, groups != 32, levels outside
 *   1 .. SEMIDETR_GN_MAX_LEVELS, batch < 1, hw[l] < 1, levels whose rows overlap, are out of order or pass tokens_per_image, a
 *   NULL operand, q without pos or pos without q, neither gy nor gq, an unknown type code, an out_type that is neither fp32 nor
 *   x_type, a misaligned pointer or stride, a workspace that is too small.
 *   SEMIDETR_E_TOOLARGE: batch * tokens_per_image * 256 >= 2^31, batch > 65535 or a batch stride >= 2^31.
 * ------------------------------------------------------------------------------------------- */
#define SEMIDETR_GN_MAX_LEVELS 8
typedef struct semidetr_gn_tokens {
    int batch, levels, channels, groups;                  /* channels == 256, groups == 32 */
    float eps;
    int64_t hw[SEMIDETR_GN_MAX_LEVELS], start[SEMIDETR_GN_MAX_LEVELS];   /* pixels of level l; its first token row */
    int64_t tokens_per_image;                             /* S: rows of tokens per image, >= start[l] + hw[l] */
    const void *x[SEMIDETR_GN_MAX_LEVELS];                /* (batch, 256, hw[l]) */
    int64_t x_batch_stride[SEMIDETR_GN_MAX_LEVELS];       /* in elements */
    const float *weight[SEMIDETR_GN_MAX_LEVELS], *bias[SEMIDETR_GN_MAX_LEVELS];
    void *grad_x[SEMIDETR_GN_MAX_LEVELS];                 /* backward: written */
    float *grad_weight[SEMIDETR_GN_MAX_LEVELS], *grad_bias[SEMIDETR_GN_MAX_LEVELS];   /* backward: written; NULL = not wanted */
    void *tokens, *q;                                     /* forward: written; q NULL = no pos */
    const void *pos, *gy, *gq;                            /* pos: forward; gy, gq: backward */
    int64_t pos_stride[2], gy_stride[2], gq_stride[2];    /* in elements */
    float *mean, *rstd;                                   /* (batch, levels, 32); forward: written; backward: read */
    int x_type, out_type, pos_type;                       /* SEMIDETR_ROW_* */
} semidetr_gn_tokens;
size_t semidetr_gn_tokens_workspace_bytes(const semidetr_gn_tokens *params /* host */, int for_backward);
int semidetr_gn_tokens_forward(void *stream, const semidetr_gn_tokens *params /* host */, void *workspace,
                               size_t workspace_bytes);
int semidetr_gn_tokens_backward(void *stream, const semidetr_gn_tokens *params /* host */, void *workspace,
                                size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * Reference-point chain of the decoder (csrc/ref_points.hip): everything DINOTransformerDecoder.forward does to the reference
 * points between two layers (detr_od/models/utils/transformer.py:972-987, 1029-1036) and the head's coordinate loop
 * (dino_detr_ssod_head.py:393-398), one launch forward and one backward.  A ROW is one (i, j) pair of a segment's two leading
 * dimensions, i < rows0, j < rows1; `width` in {2, 4} coordinates per row.  The parts of a launch:
 *
 *   refine   mode SEMIDETR_REF_REFINE:   new_ref = sigmoid(delta + inverse_sigmoid(ref, eps))
 *            mode SEMIDETR_REF_SIGMOID:  new_ref = sigmoid(ref)            (ref holds the unsigmoided points; delta is not read)
 *            mode SEMIDETR_REF_NONE:     new_ref = ref                     (delta is not read; new_ref may be NULL)
 *            inverse_sigmoid (transformer.py:435-451): x = clamp(x, 0, 1); x1 = max(x, eps); x2 = max(1 - x, eps);
 *            log(x1 / x2).  sigmoid(t) = 1 / (1 + expf(-t)).  A NaN operand gives NaN.
 *   scale    valid_ratios != NULL (then num_segments == 1, rows0 = queries, rows1 = images, 1 <= levels <= 8):
 *            ref_input[j, i, l, c] = new_ref[i, j, c] * valid_ratios[j, l, c & 1]   -- contiguous (rows1, rows0, levels, width)
 *   embed    embed != NULL (needs the scale part): gen_sineembed_for_position (transformer.py:467-493) of ref_input[:, :, 0, :]:
 *            embed[i, j, k * 128 + t] = (t even ? sinf : cosf)(fl(fl(coord_k * fp32(2 pi)) / dim_t[t])), the blocks k in the order
 *            (y, x, w, h) = coordinates (1, 0, 2, 3), or (y, x) for width 2; contiguous (rows0, rows1, 128 * width) fp32.  dim_t is
 *            the caller's table of 128 fp32 divisors (the kernel evaluates no pow).
 *
 * delta and ref are elements of delta_type / ref_type (SEMIDETR_ROW_*), read in place through the strides of their two leading
 * dimensions, in ELEMENTS, last stride 1.  Arithmetic is fp32 on exactly up-cast operands, every operation rounded on its own;
 * new_ref has out_type and is rounded once; scale and embed start from the ROUNDED new_ref.  out_type is fp32, or the common
 * 16-bit type of the operands the mode reads.  valid_ratios, ref_input, embed, dim_t and their gradients are fp32.
 *
 * semidetr_ref_points_forward   one launch: a wave takes 8 consecutive rows of a segment, one lane per (row, coordinate) for
 *   refine and scale, then all 64 lanes write each row of the embed 16 bytes per lane with the lane's dim_t entries in registers.
 * semidetr_ref_points_backward  one launch, the same map.  With y = new_ref as the forward stored it (read back) and G the
 *   gradient arriving at new_ref:
 *     G = g_new + sum_l g_ref_input[j, i, l, c] * vr[j, l, c & 1] + ((sum_t term_t) * fp32(2 pi)) * vr[j, 0, c & 1],
 *     term_t = (g_embed[.., t] * (t even ? cosf : -sinf)(arg_t)) / dim_t[t], added four per lane in index order, then over 32 lanes
 *     by a xor butterfly (16, 8, 4, 2, 1): a fixed order.  g_new, g_ref_input, g_embed may each be NULL (a zero).
 *     REFINE: g_delta = (G * (1 - y)) * y;  g_ref = g_delta * ([x >= eps] / x1 + [1 - x >= eps] / x2), 0 where x is outside
 *     [0, 1] (torch's clamp rule: the gradient passes at equality).  SIGMOID: g_ref = (G * (1 - y)) * y.  NONE: g_ref = G.
 *   g_new has out_type and strides; g_delta / g_ref are contiguous (rows0, rows1, width) of delta_type / ref_type, each may be
 *   NULL (not wanted).  No gradient goes to valid_ratios.  No float atomics, no memset, no workspace: two runs are bitwise equal.
 * Checked on the host before any launch (SEMIDETR_E_BADARG, nothing is written): width not 2 or 4, an unknown mode or type code,
 *   num_segments outside 1 .. SEMIDETR_REF_MAX_SEGMENTS, scale or embed with more than one segment, levels outside
 *   1 .. SEMIDETR_REF_MAX_LEVELS with valid_ratios (or != 0 without), embed without valid_ratios or dim_t, rows0 or rows1 < 1, a
 *   NULL operand the mode reads, an out_type torch's promotion would not give, a negative stride, a misaligned pointer (element
 *   size; 16 bytes for embed, g_embed and dim_t), eps NaN or negative.  SEMIDETR_E_TOOLARGE: rows0 * rows1 * 128 * width >= 2^31.
 * ------------------------------------------------------------------------------------------- */
#define SEMIDETR_REF_MAX_SEGMENTS 8
#define SEMIDETR_REF_MAX_LEVELS 8
#define SEMIDETR_REF_NONE 0
#define SEMIDETR_REF_SIGMOID 1
#define SEMIDETR_REF_REFINE 2
typedef struct semidetr_ref_segment {
    int rows0, rows1;
    const void *delta, *ref;                              /* (rows0, rows1, width) through the strides below */
    int64_t delta_stride[2], ref_stride[2];               /* in elements */
    void *new_ref;                                        /* forward: written; backward: read */
    int64_t new_ref_stride[2];
    const void *g_new;                                    /* backward: upstream gradient of new_ref, or NULL */
    int64_t g_new_stride[2];
    void *g_delta, *g_ref;                                /* backward: written, contiguous; NULL = not wanted */
} semidetr_ref_segment;
typedef struct semidetr_ref_points {
    int width, mode, num_segments, levels;                /* mode: SEMIDETR_REF_*; levels == 0 without valid_ratios */
    float eps;
    int delta_type, ref_type, out_type;                   /* SEMIDETR_ROW_* */
    const float *valid_ratios;                            /* (rows1, levels, 2), or NULL: no scale, no embed */
    const float *dim_t;                                   /* 128 divisors of the embed */
    float *ref_input;                                     /* forward: written, (rows1, rows0, levels, width) */
    float *embed;                                         /* forward: written, (rows0, rows1, 128 * width), or NULL */
    const float *g_ref_input, *g_embed;                   /* backward: upstream gradients, each may be NULL */
    semidetr_ref_segment segment[SEMIDETR_REF_MAX_SEGMENTS];
} semidetr_ref_points;
int semidetr_ref_points_forward(void *stream, const semidetr_ref_points *params /* host */);
int semidetr_ref_points_backward(void *stream, const semidetr_ref_points *params /* host */);

/* ---------------------------------------------------------------------------------------------
 * Pyramid inputs of the transformer (csrc/pyramid_inputs.hip): the level masks, SinePositionalEncodingHW of every level with the
 * level_embed row added, flattened and concatenated (positional_encoding.py:57-99, transformer.py:1271-1289), mask_flatten,
 * get_valid_ratio (:1237-1244, 1292) and the encoder's get_reference_points (:676-691) -- two launches forward for the whole
 * pyramid and batch, two backward.  Token row `start[l] + i * w[l] + j` of image n is pixel (i, j) of level l.
 *
 * The level masks.  from_sizes != 0: pixel (i, j) of level l is masked iff src(i, input_h, h[l]) >= img_h[n] or
 *   src(j, input_w, w[l]) >= img_w[n], src(d, in, out) = min((int)floorf(d * ((float)in / (float)out)), in - 1): the nearest rule
 *   of F.interpolate on the (input_h, input_w) image mask whose top-left (img_h[n], img_w[n]) corner is valid (0 <= img_h[n] <=
 *   input_h, likewise w).  from_sizes == 0: masks[l] holds (batch, h[l], w[l]) bytes, contiguous; non-zero = masked.
 * Counts.  cnt_y(i, j) = valid pixels of column j in rows 0 .. i, tot_y(j) = cnt_y(h - 1, j); cnt_x / tot_x the same along the
 *   row.  Exact integers (16-bit: h, w < 65536).
 * pos[n, row, c], every operation rounded on its own in fp32, IEEE division, precise sinf / cosf:
 *   normalize != 0:  y = ((cnt_y + offset) / (tot_y + eps)) * scale,  else y = cnt_y;  x likewise from cnt_x, tot_x.
 *   c < 128:   (c even ? sinf : cosf)(y / dim_ty[c]);   c >= 128:  (c even ? sinf : cosf)(x / dim_tx[c - 128]);
 *   + level_embed[l, c] (exactly up-cast) where level_embed != NULL; rounded once to pos_type.
 *   dim_ty / dim_tx are the caller's tables of 128 fp32 divisors (the kernels evaluate no pow).
 * mask_flatten[n, row] = 0 / 1 bytes.  valid_ratios[n, l] = ((float)tot_x(row 0) * (1.0f / w[l]), (float)tot_y(column 0) *
 *   (1.0f / h[l])): the product with the fp32 reciprocal, which is what torch's division of a GPU tensor by a host number computes
 *   (get_valid_ratio's `valid_W.float() / W`); it differs from the IEEE quotient by an ulp for some counts.
 * reference_points[n, row, l', :] (NULL = not wanted), vr = valid_ratios[n]:
 *   ((j + 0.5f) / (vr[l][0] * w[l])) * vr[l'][0],  ((i + 0.5f) / (vr[l][1] * h[l])) * vr[l'][1]   -- a level without a valid pixel
 *   in row 0 or column 0 gives what IEEE gives (x / 0, inf * 0), as stock torch does.
 *
 * semidetr_pyramid_inputs_forward   launch 1, one 64-lane workgroup per 64 columns and one per 64 rows of an (image, level) -- a
 *   grid of batch * (ceil(w / 64) + ceil(h / 64)) summed over the levels: a lane walks its column down (its row along), writes the
 *   mask bytes (column walk), the running counts into the workspace and, from column 0 and row 0, the valid ratios.  Launch 2, a workgroup per 32 token rows of an
 *   (image, level): one lane handles 4 consecutive channels of a token, a wave stores a whole row (16 bytes per lane, 8 for a
 *   16-bit pos_type), lanes 0 .. 2 * levels - 1 the row's reference points.
 * semidetr_pyramid_inputs_backward  grad_level_embed[l, c] = sum over n and the rows of level l of g[n, row, c]; g has g_type and
 *   is read in place through g_stride (elements, last stride 1).  Launch 1: a workgroup adds 256 rows of an (image, level) in
 *   fp32 in a fixed order into a slot of the workspace; launch 2 adds a level's slots in fp64 in a fixed order and rounds once
 *   to level_embed_type.  Nothing else receives a gradient.
 * No float atomics, no memset; every grid and order depends on the sizes alone: two runs are bitwise equal.
 * semidetr_pyramid_inputs_workspace_bytes  the bytes either call needs (sizes only; 0 for sizes the calls refuse).
 * Checked on the host before any launch (SEMIDETR_E_BADARG, nothing is written): levels outside 1 .. SEMIDETR_PYR_MAX_LEVELS,
 *   batch outside 1 .. SEMIDETR_PYR_MAX_BATCH, h[l] or w[l] outside 1 .. 65535, levels whose rows overlap, are out of order or
 *   pass tokens_per_image, an image size outside the input shape, normalize with eps <= 0 or a NaN setting, an unknown type
 *   code, a NULL or misaligned pointer (16 bytes: pos, g, dim_ty, dim_tx, level_embed, the workspace; 8 for 16-bit pos and g), a
 *   workspace smaller than the query says.  SEMIDETR_E_TOOLARGE: batch * tokens_per_image * 256 >= 2^31.
 * ------------------------------------------------------------------------------------------- */
#define SEMIDETR_PYR_MAX_LEVELS 8
#define SEMIDETR_PYR_MAX_BATCH 64
typedef struct semidetr_pyramid_inputs {
    int batch, levels;
    int h[SEMIDETR_PYR_MAX_LEVELS], w[SEMIDETR_PYR_MAX_LEVELS];
    int64_t start[SEMIDETR_PYR_MAX_LEVELS];               /* first token row of level l */
    int64_t tokens_per_image;
    int from_sizes, input_h, input_w;                     /* batch_input_shape */
    int img_h[SEMIDETR_PYR_MAX_BATCH], img_w[SEMIDETR_PYR_MAX_BATCH];     /* by value: no staging copy */
    const void *masks[SEMIDETR_PYR_MAX_LEVELS];           /* from_sizes == 0: (batch, h[l], w[l]) bytes */
    int normalize;
    float offset, eps, scale;
    const float *dim_ty, *dim_tx;                         /* 128 divisors each */
    const void *level_embed;                              /* (levels, 256) of level_embed_type, or NULL */
    int level_embed_type, pos_type, g_type;               /* SEMIDETR_ROW_* */
    void *pos;                                            /* forward: written, (batch, tokens_per_image, 256) */
    void *mask_flatten;                                   /* forward: written, (batch, tokens_per_image) bytes */
    float *valid_ratios;                                  /* forward: written, (batch, levels, 2) */
    float *reference_points;                              /* forward: written, (batch, tokens_per_image, levels, 2), or NULL */
    const void *g;                                        /* backward: upstream gradient of pos */
    int64_t g_stride[2];                                  /* in elements */
    void *grad_level_embed;                               /* backward: written, (levels, 256) of level_embed_type */
} semidetr_pyramid_inputs;
size_t semidetr_pyramid_inputs_workspace_bytes(const semidetr_pyramid_inputs *params /* host */, int for_backward);
int semidetr_pyramid_inputs_forward(void *stream, const semidetr_pyramid_inputs *params /* host */, void *workspace,
                                    size_t workspace_bytes);
int semidetr_pyramid_inputs_backward(void *stream, const semidetr_pyramid_inputs *params /* host */, void *workspace,
                                     size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SEMIDETR_HIP_H */
