/*
 * cloudct.h — C ABI of libcloudct.so, the MI355X (gfx950) implementation of the
 * Multi-Headed Cloud Transform hot path.
 *
 * Every entry point is `extern "C"`, takes plain device pointers + sizes and a
 * HIP stream (passed as void* so that this header needs no HIP include), never
 * allocates, never synchronises the device, keeps no global state — but for the
 * process-wide deterministic switch ct_set_deterministic, the process-wide precision
 * mode of the pointwise GEMMs ct_set_pw_precision, that of the grouped convolutions
 * ct_set_gconv_precision and the ct_debug_* test
 * hooks below, host-side atomics that no kernel reads — and returns
 * an int status: CT_OK (0) or a negative CT_E* code (ct_strerror() names it).
 * All tensors are fp32, contiguous, channels-first with the point index N
 * fastest — the reference's layout (layers/cloud_transform.py:140,156).  Work is
 * enqueued on the given stream (the caller's torch current stream), never on
 * the legacy default stream the reference's extensions use
 * (chamfer_extension/chamfer.cu:142, emd_linear/emd_cuda.cu:257).
 *
 * Notation: B batch, H heads, C features per head, N points, dim in {2,3},
 * W[dim] grid extents (x slowest), G = prod(W), V = 2^dim corners.
 *
 * Each function cites the reference interface it replaces (paths are into the
 * reference repository).
 */
#ifndef CLOUDCT_H
#define CLOUDCT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 6): ct_plane_sort / ct_plane_sort_bytes / ct_slice_bwd_ps / ct_bn_group_reduce_bwd_copy added, ct_debug_set_pw_kernel
 * removed, since version 1 — a stale library selected by CLOUDCT_LIB fails this check instead of failing at symbol binding.
 * (The test-hook flag CT_DEBUG_NO_WIDE was added later without a bump: an additive debug bit, no symbol or signature changed.
 * The neighbour-search entry points ct_nbr_* and the item assembly ct_kp_items were added under version 2 as well: additive
 * symbols, which the loader's missing-symbol scan checks.  ct_completion_items was added the same way.)
 * 3: the item table is the only norm interface.  Removed: the positional forms ct_bn_relu_fwd / _bwd (and _amax), ct_bn_stats_fwd,
 * ct_bn_apply_fwd / _bwd (and _amax), ct_bn_reduce_bwd, ct_bn_eval_fwd, ct_adain_fwd / _bwd (and _amax) — a single norm is a table
 * with n = 1 — and ct_bn_group_reduce_bwd_copy, whose sums_copy is now a nullable argument of ct_bn_group_reduce_bwd.  Changed:
 * the four exchange phases ct_bn_group_{stats,apply}_fwd / {reduce,apply}_bwd take the whole table plus the run of items to launch.
 * (ct_scan_items was added under version 3 without a bump: an additive symbol, which the loader's missing-symbol scan checks;
 * ct_block_items and ct_seg_confusion the same way; then the index table ct_nbr_table_bytes / ct_nbr_table_set /
 * ct_nbr_radius_multi and the device plan ct_kp_plan / ct_kp_plan_workspace_bytes; then ct_image_items; then the voxel-grid
 * subsampling ct_voxel_bounds / ct_voxel_keys / ct_voxel_reduce and their workspace queries; then the resident ShapeNet
 * completion gather ct_completion_gather; then the deterministic switch ct_set_deterministic / ct_get_deterministic / ct_deterministic_override;
 * then Chamfer with per-cloud counts and the metric table: ct_chamfer_fwd_counts / ct_chamfer_bwd_counts / ct_rows_compact /
 * ct_chamfer_metrics; then the backward of the eval-mode norm, ct_bn_eval_group_bwd; then the precision mode of the pointwise
 * GEMMs ct_set_pw_precision / ct_get_pw_precision / ct_pw_precision_override; then that of the grouped convolutions,
 * ct_set_gconv_precision / ct_get_gconv_precision / ct_gconv_precision_override / ct_gconv_precision_covers; then the EMD auction for any cloud size and per-cloud counts,
 * ct_emd_fwd_counts / ct_emd_bwd_counts; then the k-nearest query and its interpolation, ct_nbr_knn / ct_nbr_knn_multi /
 * ct_nbr_interp.) */
#define CT_ABI_VERSION 3

/* status codes */
#define CT_OK 0
#define CT_EINVAL (-1)    /* bad argument (null pointer, size, dim, reduce ...) */
#define CT_ELAUNCH (-2)   /* HIP reported an error at launch                     */
#define CT_EWORKSPACE (-3)/* workspace too small: see ct_*_workspace_bytes       */
#define CT_EPRECOND (-4)  /* reference precondition violated (e.g. EMD n%1024)   */

/* reduce modes of Splat */
#define CT_REDUCE_MAX0 0  /* max with a zero floor: what the reference executes
                             (torch_scatter.scatter_max into zeros,
                             layers/cloud_transform.py:164-173)                  */
#define CT_REDUCE_SUM 1   /* scatter-add: the variant BASELINE.json names        */

/* dtype of the optional pts_padding mask (B,N) */
#define CT_PAD_NONE 0
#define CT_PAD_F32 1
#define CT_PAD_I32 2      /* datasets/s3dis_closer.py:330,336 builds an int32 mask */

typedef void* ct_stream_t; /* hipStream_t */

int ct_abi_version(void);
const char* ct_strerror(int status);

/* ------------------------------------------------------------------------
 * Deterministic mode.  Process-wide host state, atomic: set on one thread, read ONCE per call by the entry points on any
 * thread (autograd runs the backward entry points on threads of its own, so the state cannot be thread-local), never read
 * by a kernel.  Off by default; the default path is unchanged by it.  Added under CT_ABI_VERSION 3 (additive symbols).
 * While it is on, equal inputs give bit-equal outputs from run to run:
 *   - Splat(max) backward (ct_splat_bwd, _ex, _tk, ct_splat_lc_bwd and the Splat step of ct_mhct_core_bwd / _tk): the winner
 *     of a (cell, channel) is the LOWEST POINT INDEX among the contributions whose product is positive and bit-equal to z
 *     (the lowest corner of that point if two of its corners name the cell) — on every shape, by a two-phase claim
 *     (csrc/ct_raster_det.h: splat_max_bwd_det_kernel); point segments are not used and g_keys is summed in a fixed order
 *     (one workgroup per plane, or per-group partials in the workspace added in group order).  The launch tag carries
 *     "splat_max_bwd_det".  CT_DEBUG_FORCE_BAND still selects the banded kernels, which follow the same rule.
 *     The workspace queries ct_splat_bwd_workspace_bytes / _ex_ are sized BY THE MODE: they read the switch, and a query and
 *     a launch must be made under the same setting (the partial g_keys of the channel-chunk groups differ between the
 *     modes).  Grids whose single-channel tile exceeds a CU's LDS (4 G bytes: 256^2) keep the claim words in the workspace:
 *     CT_EWORKSPACE without it; without the partials' share one workgroup walks all chunks of its plane.
 *   - the generic corner-cotangent pass behind ct_slice_lc_bwd, ct_slice_bwd / ct_slice_bwd_keys off the hot shapes and
 *     Splat(sum) backward: a plane's channel chunks are not dealt to groups of workgroups (whose g_keys / g_local_coord sums
 *     went through float atomics); a thread adds the chunks of its own points in order.
 *   - the scatter-ADD onto a grid whose single-channel tile exceeds a CU's LDS (256^2, 36^3: the `scatter_global_atomics` form
 *     behind ct_splat_fwd with CT_REDUCE_SUM, ct_slice_bwd* / ct_slice_lc_bwd / ct_slice_bwd_grid where the banded kernels do
 *     not take the call) is global float atomics in arrival order and has no ordered form: CT_EPRECOND in the mode, before
 *     anything is written.  (The same grids' scatter-MAX is an atomic max, which no order changes.)
 *   - ct_chamfer_bwd, ct_chamfer_bwd_counts: every destination row written once: its own term first, then its sources in
 *     ascending index.
 *   - ct_gconv_bwd_weight and ct_lattice_bwd: CT_EPRECOND for a NULL workspace where the shape would take float atomics
 *     (the ring kernel without a workspace; the lattice parameter sums), and for the tile form of rows that are not a
 *     multiple of 4 floats, which has atomics only.
 * Every other entry point computes the same bits in either mode on finite values within the fixed-point range of the scatter-adds
 * (DESIGN.md §4.11 has the table and its exceptions).
 * ct_deterministic_override(on): on = 0 / 1 sets the mode for the entry points the CALLING THREAD invokes, whatever the
 * process-wide switch says, on < 0 ends the override — how a caller runs ONE refused call in its ordinary form (torch's
 * warn_only) without switching other threads' calls, which sit between their workspace query and their launch, to the
 * other mode.  ct_get_deterministic() returns the mode in effect for the calling thread.
 * ---------------------------------------------------------------------- */
void ct_set_deterministic(int on);
int ct_get_deterministic(void);
void ct_deterministic_override(int on);

/* ------------------------------------------------------------------------
 * DifferentiablePositions  (layers/cloud_transform.py:72-121,
 *                           layers/utils.py:100-186 bi/tri-linear corners)
 * keys f32[B,H*dim,N] -> local_coord f32[B,H,V,N], flat_idx i64[B,H,V,N]
 * ---------------------------------------------------------------------- */
int ct_positions_fwd(const float* keys, float* local_coord, int64_t* flat_idx,
                     int B, int H, int N, int dim, const int* W, ct_stream_t s);
/* g_keys[B,H*dim,N] = d(local_coord)/d(keys)^T g_local_coord, with the
 * GradientBalancing rule (cloud_transform.py:12-26: no (W-1)/2 factor) and the
 * clamp mask (:91).  Overwrites g_keys. */
int ct_positions_bwd(const float* keys, const float* g_local_coord, float* g_keys,
                     int B, int H, int N, int dim, const int* W, ct_stream_t s);

/* ------------------------------------------------------------------------
 * Fused hot path: corners are recomputed from `keys` inside the kernels, so
 * local_coord / flat_idx never touch HBM.  Used by the MultiHead* blocks.
 *
 * Splat.forward  (layers/cloud_transform.py:131-180)
 *   grid f32[B,H*C,G] (fully overwritten)
 * Splat backward (torch_scatter.scatter_max backward: the single arg-max
 *   contribution of a cell receives the cotangent; on EXACT ties exactly one of
 *   the tied contributions receives it — as in torch_scatter, whose CPU and CUDA
 *   paths differ in WHICH one.  Here: a single chance tie in a plane is awarded
 *   to the lowest point index; with more ties (duplicated points) the winner is
 *   unspecified — unless ct_set_deterministic(1): then always the lowest point index.
 *   HISTORY.md §2 has the rule per kernel family.)
 *   DEVIATION, deliberate: a candidate whose product is exactly +-0 (a point exactly on a cell boundary: one corner weight is 0;
 *   or a feature that is exactly 0, e.g. under a padding mask) aimed at a cell whose maximum stays at the zero floor receives
 *   NOTHING here.  torch_scatter.scatter_max records it as the arg-max (0 == 0) and routes the cell's cotangent to it.  Values
 *   and every cotangent not itself multiplied by that zero agree; what differs is g_keys of a point exactly on a boundary
 *   (through d(weight)/d(key): a few elements per million points) and g_feat of an exactly-zero feature.  Pinned by
 *   tests/test_tie_rule_gpu.py; INTEGRATION.md "Known deviations".
 *   needs `grid` = the forward output, g_grid f32[B,H*C,G];
 *   writes g_feat f32[B,H*C,N] and g_keys f32[B,H*dim,N] (both overwritten).
 * workspace: scratch of ct_splat_bwd_workspace_bytes(...) bytes (may be 0).
 * ---------------------------------------------------------------------- */
int ct_splat_fwd(const float* keys, const float* feat, const void* pad, int pad_dtype,
                 float* grid, int B, int H, int C, int N, int dim, const int* W,
                 int reduce, ct_stream_t s);
size_t ct_splat_bwd_workspace_bytes(int B, int H, int C, int N, int dim, const int* W, int reduce);
int ct_splat_bwd(const float* keys, const float* feat, const void* pad, int pad_dtype,
                 const float* grid, const float* g_grid, float* g_feat, float* g_keys,
                 void* workspace, size_t workspace_bytes,
                 int B, int H, int C, int N, int dim, const int* W, int reduce, ct_stream_t s);

/* ct_splat_bwd with options.  CT_BWD_ACCUMULATE_KEYS: g_keys += result instead of g_keys = result — the
 * keys of a block feed both Splat and Slice (layers/multihead_ct.py:99-107), so their two key cotangents are
 * summed by autograd; accumulating in the second backward saves that extra pass over (B,H*dim,N).
 * workspace: ct_splat_bwd_ex_workspace_bytes(..., flags) bytes. */
#define CT_BWD_ACCUMULATE_KEYS 1
size_t ct_splat_bwd_ex_workspace_bytes(int B, int H, int C, int N, int dim, const int* W, int reduce, int flags);
int ct_splat_bwd_ex(const float* keys, const float* feat, const void* pad, int pad_dtype,
                    const float* grid, const float* g_grid, float* g_feat, float* g_keys,
                    void* workspace, size_t workspace_bytes,
                    int B, int H, int C, int N, int dim, const int* W, int reduce, int flags, ct_stream_t s);

/* Test hooks (process-wide host state, never read by a kernel): flags select kernel families so that the
 * parity tests can compare them on identical inputs (atomic: set on one thread, read by entry points on any); the tag string
 * names the kernels the last Splat / Slice or grouped-convolution entry point launched — whichever thread called it, e.g. autograd's — and is
 * returned as a copy owned by the calling thread (writers and readers serialise on a mutex). */
#define CT_DEBUG_NO_HOT 1      /* keep the hot-shape kernels (csrc/ct_raster_hot.h) off */
#define CT_DEBUG_FORCE_HOT 2   /* use them for every eligible layout, however few (b,h) planes there are */
#define CT_DEBUG_NO_BAND 4     /* keep the banded four-channel kernels (csrc/ct_raster_band.h) off */
#define CT_DEBUG_FORCE_BAND 8  /* try them first, on every layout they can take (small grids in the tests) */
#define CT_DEBUG_NO_SORTED 16  /* keep the sorted-plane kernels (csrc/ct_raster_sorted.h) off */
#define CT_DEBUG_FORCE_SORTED 32 /* use them on every layout they can take, however few (b,h) planes there are */
#define CT_DEBUG_FORCE_SORTED_SEG 64 /* 2D: the sorted-SEGMENT kernel (csrc/ct_raster_sorted3d.h, DIM = 2) wherever it is legal; 3D grids
                                        take it under CT_DEBUG_FORCE_SORTED already */
#define CT_DEBUG_NO_WIDE 128   /* keep the 1024-thread WIDE launches of the hot backward kernels off (as CLOUDCT_WIDE=0, which is read
                                  once per process): the narrow and the wide form compared within one process */
void ct_debug_set_flags(unsigned flags);
const char* ct_debug_last_launch(void);
/* point segments of the hot Splat(max) backward (ct_splat_bwd_tk): 0 automatic, 1 never, n > 1: n wherever legal */
void ct_debug_set_nseg(int nseg);

/* Slice.forward  (layers/cloud_transform.py:190-227): out f32[B,H*C,N].
 * Slice backward (autograd of torch.gather = scatter-add, :216-221):
 *   g_grid f32[B,H*C,G] and g_keys f32[B,H*dim,N], both overwritten. */
int ct_slice_fwd(const float* keys, const float* grid, const void* pad, int pad_dtype,
                 float* out, int B, int H, int C, int N, int dim, const int* W, ct_stream_t s);
int ct_slice_bwd(const float* keys, const float* grid, const void* pad, int pad_dtype,
                 const float* g_out, float* g_grid, float* g_keys,
                 int B, int H, int C, int N, int dim, const int* W, ct_stream_t s);
/* Splat(max) forward and Slice forward on the same keys in ONE launch: grid = ct_splat_fwd(keys, feat), out = ct_slice_fwd(keys,
 * grid), both written, with the bits the two calls write (csrc/ct_raster_fwd_fused.h: a plane's tile stays in LDS between the two
 * halves; `grid` is written once and not read back).  For callers that chain the two ops directly (SplatSliceStep); a block with a
 * grouped convolution between them uses ct_mhct_core_fwd.
 * ct_splat_slice_fwd_supported: 1 where the call takes the shape under the current switches, else 0.  Legal are dim == 2, reduce ==
 * CT_REDUCE_MAX0, N % 4 == 0, N <= 4096, C % 4 == 0, G % 4 == 0, the tiles of a workgroup within its LDS budget, with or without a
 * padding mask; of these it answers 1 where the kernel was measured against the two calls and won, wherever it is
 * legal under CT_DEBUG_FORCE_HOT or CLOUDCT_FUSED_FWD=1 (read once per process), and nowhere under CT_DEBUG_NO_HOT.
 * ct_splat_slice_fwd: CT_EINVAL, before anything is launched or written, where the query answers 0 and for a null or not 16-byte
 * aligned keys / feat / grid / out; the launch tag is "splat_slice_fwd_fused".  Added under CT_ABI_VERSION 3 (additive symbols). */
int ct_splat_slice_fwd_supported(int B, int H, int C, int N, int dim, const int* W, int reduce, int pad_dtype);
int ct_splat_slice_fwd(const float* keys, const float* feat, const void* pad, int pad_dtype,
                       float* grid, float* out, int B, int H, int C, int N, int dim, const int* W,
                       int reduce, ct_stream_t s);
/* Slice backward and Splat(max) backward on the same keys in ONE launch (csrc/ct_raster_bwd_fused.h): what
 *   ct_slice_bwd_tk(keys, grid, g_out) -> g_grid, g_keys_slice   followed by
 *   ct_splat_bwd_tk(keys, feat, grid, g_grid, add = g_keys_slice) -> g_feat, g_keys
 * write, with their bits: g_grid is stored once and not read back, grid and the keys are read once, and Slice's key cotangent
 * never leaves the workgroup (g_keys_slice may be NULL; given, it receives that cotangent alone).  For callers that chain the two
 * ops directly (SplatSliceStep).
 * ct_slice_splat_bwd_supported: 1 where the call takes the shape under the current switches, else 0.  Legal are dim == 2, reduce ==
 * CT_REDUCE_MAX0, N % 4 == 0, N <= 4096, C % 4 == 0, C <= 256, a grid of G % 4 == 0 and G <= 1024 cells, one workgroup per plane
 * within the sorted kernels' LDS budget, NO padding mask (pad_dtype != CT_PAD_NONE: 0 — that instance of the kernel spills in its
 * loop and is not built), outside the deterministic mode (ct_set_deterministic(1): 0); of these it answers 1 where the kernel was measured against the two calls and won, wherever it is legal
 * under CT_DEBUG_FORCE_HOT or CLOUDCT_FUSED_BWD=1 (read once per process), and nowhere under CT_DEBUG_NO_HOT, CT_DEBUG_NO_SORTED or
 * CLOUDCT_FUSED_BWD=0.
 * ct_slice_splat_bwd: CT_EINVAL, before anything is launched or written, where the query answers 0, for a null or not 16-byte
 * aligned pointer (g_keys_slice excepted: NULL is legal) and for g_keys aliasing an input or g_keys_slice; no host
 * synchronisation, no state left behind (graph-safe); the launch tag is "slice_splat_bwd_fused".  Added under CT_ABI_VERSION 3
 * (additive symbols). */
int ct_slice_splat_bwd_supported(int B, int H, int C, int N, int dim, const int* W, int reduce, int pad_dtype);
int ct_slice_splat_bwd(const float* keys, const float* feat, const void* pad, int pad_dtype,
                       const float* grid, const float* g_out,
                       float* g_grid, float* g_feat, float* g_keys_slice /* may be NULL */, float* g_keys,
                       int B, int H, int C, int N, int dim, const int* W, int reduce, ct_stream_t s);
/* ct_slice_bwd with scratch: with few (b,h) planes (the zoo's H = 16 blocks) the channel chunks of a plane are dealt to
 * several workgroups, whose partial g_keys go through `workspace` (ct_slice_bwd_workspace_bytes(...) bytes, may be 0).
 * Same results as ct_slice_bwd, which has to keep one workgroup per plane there. */
size_t ct_slice_bwd_workspace_bytes(int B, int H, int C, int N, int dim, const int* W);
int ct_slice_bwd_ws(const float* keys, const float* grid, const void* pad, int pad_dtype,
                    const float* g_out, float* g_grid, float* g_keys, void* workspace, size_t workspace_bytes,
                    int B, int H, int C, int N, int dim, const int* W, ct_stream_t s);
/* Arrival tickets: ct_slice_bwd_ws / ct_splat_bwd_ex with the sums over a plane's workgroups done INSIDE the kernel.
 * Where a (b,h) plane is shared by several workgroups (few planes: channel-chunk groups, point segments) each leaves a
 * partial g_keys / g_grid in `workspace`; without tickets a second small launch adds them.  With `tickets` — a device
 * buffer of CT_TICKETS_BYTES that is ZERO on entry (ct_tickets_init once after allocation) — every workgroup takes a
 * ticket of its plane when its partials are out and the holder of the last ticket adds them, in the same fixed order
 * (same bits as the two-launch form), and resets the ticket: the buffer is zero again when the kernel ends.  One
 * launch per pass instead of two or three.  The buffer carries state between launches: launches that share it must be
 * ordered (one buffer per stream), and it must be re-initialised after a launch that faulted.  tickets == NULL: exactly
 * ct_slice_bwd_ws / ct_splat_bwd_ex.  Same workspace sizes, same results. */
#define CT_TICKETS_BYTES 65536
int ct_tickets_init(void* tickets, ct_stream_t s);
int ct_slice_bwd_tk(const float* keys, const float* grid, const void* pad, int pad_dtype,
                    const float* g_out, float* g_grid, float* g_keys, void* workspace, size_t workspace_bytes,
                    void* tickets, int B, int H, int C, int N, int dim, const int* W, ct_stream_t s);
/* Sorted planes (csrc/ct_raster_sorted.h; no counterpart in the reference, whose Splat / Slice re-derive everything from
 * local_coordinate / flattened_index per call, layers/cloud_transform.py:72-124).  One diff_poss(lattice) feeds the Splat and
 * the Slice of a block (layers/multihead_ct.py:99-107), so the four raster passes of a step see the SAME keys: ct_plane_sort
 * counting-sorts every (b, h) plane's points by base cell once (the record is a function of the keys alone) and leaves
 * per plane the sorted positions, the fractional corner weights in sorted order and the plane's work items in `sorted`
 * (ct_plane_sort_bytes; 0: this layout has no sorted form — dim 3, N > 4096 ...).  The *_ps entry points take the record of
 * THEIR keys (NULL: they behave as the *_tk entry points and sort inside where they use the sorted form); a record made from
 * other keys gives wrong results, not an error. */
size_t ct_plane_sort_bytes(int B, int H, int N, int dim, const int* W);
int ct_plane_sort(const float* keys, void* sorted, size_t sorted_bytes, int B, int H, int N, int dim, const int* W, ct_stream_t s);
int ct_slice_bwd_ps(const float* keys, const float* grid, const void* pad, int pad_dtype,
                    const float* g_out, float* g_grid, float* g_keys, void* workspace, size_t workspace_bytes,
                    void* tickets, const void* sorted, int B, int H, int C, int N, int dim, const int* W, ct_stream_t s);
/* ct_splat_bwd_tk: g_keys = g_keys_add + (key cotangent of this Splat); g_keys_add NULL: g_keys = the cotangent;
 * g_keys_add == g_keys: in place, as CT_BWD_ACCUMULATE_KEYS.  With tickets AND a g_keys_add that is not g_keys (or NULL) a
 * plane's POINTS may be dealt to several workgroups (point segments: no partial sums at all, every workgroup walks all
 * channel chunks for its points); the plane's exact-tie test then runs across them through the tickets (a 64-bit word per
 * plane in the buffer's second half: the buffer must be 8-byte aligned for this form), and a plane with more than one tie
 * is redone by its last workgroup from g_keys_add — which is why it must not alias the output.
 * workspace: ct_splat_bwd_ex_workspace_bytes(..., CT_BWD_ACCUMULATE_KEYS if g_keys_add else 0). */
/* > 1: with tickets and a g_keys_add that is not g_keys, ct_splat_bwd_tk(reduce = max) deals the points of a plane of this
 * shape to that many workgroups — worth a second key-cotangent tensor; 1: it would not (adding in place is as good). */
int ct_splat_bwd_tk_segments(int B, int H, int C, int N, int dim, const int* W);
int ct_splat_bwd_tk(const float* keys, const float* feat, const void* pad, int pad_dtype,
                    const float* grid, const float* g_grid, float* g_feat, const float* g_keys_add, float* g_keys,
                    void* workspace, size_t workspace_bytes, void* tickets,
                    int B, int H, int C, int N, int dim, const int* W, int reduce, ct_stream_t s);
/* The two halves of ct_slice_bwd, for callers that need only one cotangent
 * (autograd's needs_input_grad) and for per-kernel timing: each is one launch. */
int ct_slice_bwd_grid(const float* keys, const void* pad, int pad_dtype, const float* g_out,
                      float* g_grid, int B, int H, int C, int N, int dim, const int* W, ct_stream_t s);
int ct_slice_bwd_keys(const float* keys, const float* grid, const void* pad, int pad_dtype,
                      const float* g_out, float* g_keys,
                      int B, int H, int C, int N, int dim, const int* W, ct_stream_t s);

/* ------------------------------------------------------------------------
 * The same four passes with EXPLICIT local_coord / flat_idx tensors — the
 * signature-compatible Splat / Slice nn.Modules call these when handed
 * arbitrary (local_coordinate, flattened_index) inputs.  g_local_coord
 * f32[B,H,V,N] is overwritten.  Every flat_idx must be in [0, G).
 * ---------------------------------------------------------------------- */
int ct_splat_lc_fwd(const float* local_coord, const int64_t* flat_idx, const float* feat,
                    const void* pad, int pad_dtype, float* grid,
                    int B, int H, int C, int N, int dim, const int* W, int reduce, ct_stream_t s);
int ct_splat_lc_bwd(const float* local_coord, const int64_t* flat_idx, const float* feat,
                    const void* pad, int pad_dtype, const float* grid, const float* g_grid,
                    float* g_feat, float* g_local_coord, void* workspace, size_t workspace_bytes,
                    int B, int H, int C, int N, int dim, const int* W, int reduce, ct_stream_t s);
int ct_slice_lc_fwd(const float* local_coord, const int64_t* flat_idx, const float* grid,
                    const void* pad, int pad_dtype, float* out,
                    int B, int H, int C, int N, int dim, const int* W, ct_stream_t s);
int ct_slice_lc_bwd(const float* local_coord, const int64_t* flat_idx, const float* grid,
                    const void* pad, int pad_dtype, const float* g_out,
                    float* g_grid, float* g_local_coord,
                    int B, int H, int C, int N, int dim, const int* W, ct_stream_t s);

/* Occupancy statistic of a rasterised grid (layers/multihead_ct.py:104-105):
 * count[0] = number of elements with |z| > 1e-9 (the caller divides by B*C*H).
 * count is a device int64 and is overwritten. */
int ct_grid_occupancy(const float* grid, int64_t n_elements, int64_t* count, ct_stream_t s);
/* The same statistic as the blocks report it, in ONE launch: out[0] = float(count) * inv_denominator (what torch computes for
 * `count.float() / (B*C*H)`, layers/multihead_ct.py:104-105), a device float that is overwritten.  `workspace`: CT_OCC_WORKSPACE_BYTES
 * of device memory, 8-byte aligned, zeroed ONCE by the caller (per-workgroup counts and an arrival ticket that the kernel hands
 * back as zero); launches that share a workspace must be ordered (one per stream).  n_elements <= 2^31 - 1. */
#define CT_OCC_WORKSPACE_BYTES 4096
int ct_grid_occupancy_ratio(const float* grid, int64_t n_elements, float inv_denominator, float* out, void* workspace, ct_stream_t s);

/* ------------------------------------------------------------------------
 * Lattice of an MHCT block: per-head rigid transform of (xyz + key residual) followed by tanh
 * (VolTransformer / PlaneTransformer: layers/utils.py:9-61; layers/multihead_ct.py:93-97,
 *  layers/multihead_ct_adain.py:112-116 with its learnable scalar on the residual):
 *   p = xyz + kscale*residual + shift_h;  keys_n = (sum_c p_c R_h[c][n]) * scales_h[n], n < dim;
 *   lattice = tanh(keys)
 * xyz f32[B,3,N], residual f32[B,H*3,N], R f32[H,3,3] (= so3_exponential_map(log_R), computed by the
 * caller), shift f32[H,3], scales f32[H,dim] | NULL, kscale device f32[1] | NULL (= 1).
 * Forward writes keys and lattice f32[B,H*dim,N].  Backward takes the cotangents of the lattice and /
 * or of the pre-tanh keys (either may be NULL, not both) and overwrites g_xyz, g_residual, g_R, g_shift (and g_scales / g_kscale iff scales / kscale given).
 * With a workspace of ct_lattice_bwd_workspace_bytes the per-head parameter cotangents are summed in a fixed order (reproducible);
 * with workspace NULL they are accumulated with one float atomic per workgroup and parameter.
 * ---------------------------------------------------------------------- */
size_t ct_lattice_fwd_workspace_bytes(int B, int H, int N);
int ct_lattice_fwd(const float* xyz, const float* residual, const float* R, const float* shift,
                   const float* scales, const float* kscale, float* keys, float* lattice,
                   float* key_stats /* NULL | f32[2]: mean and unbiased variance of the keys (the blocks' lattice statistics,
                                       layers/multihead_ct.py:109-112); needs the workspace */,
                   void* workspace, size_t workspace_bytes, int B, int H, int N, int dim, ct_stream_t s);
size_t ct_lattice_bwd_workspace_bytes(int B, int H, int N);
int ct_lattice_bwd(const float* xyz, const float* residual, const float* R, const float* shift,
                   const float* scales, const float* kscale, const float* lattice, const float* g_lattice,
                   const float* g_keys, float* g_xyz, float* g_residual, float* g_R, float* g_shift, float* g_scales,
                   float* g_kscale, void* workspace, size_t workspace_bytes, int B, int H, int N, int dim, ct_stream_t s);

/* The transformer of a block in its fewest launches (layers/utils.py:25-34,53-61 with the so3 map of :29,56 inside):
 *   ct_lattice_so3_fwd: R = so3_exponential_map(log_R, so3_eps) computed per head inside the lattice launch (R f32[H,3,3] is an
 *     OUTPUT, kept for the backward) and the key statistics finished by the launch's last workgroup — ONE launch where
 *     ct_so3_exp_fwd + ct_lattice_fwd are three.  `ticket`: one zero 32-bit word of device memory that the launch leaves zero
 *     (needed with key_stats; launches that share it must be ordered: e.g. the last word of a ct_tickets_init buffer).
 *   ct_lattice_so3_bwd: ct_lattice_bwd whose tail launch also turns every head's g_R into g_log_R f32[H,3] (the workgroup
 *     that sums a head's g_R finishes with the so3 map's backward) — two launches where ct_lattice_bwd + ct_so3_exp_bwd are
 *     three; g_R f32[H,3,3] is scratch the caller provides; the workspace is required. */
int ct_lattice_so3_fwd(const float* xyz, const float* residual, const float* log_R, float so3_eps, const float* shift,
                       const float* scales, const float* kscale, float* R, float* keys, float* lattice, float* key_stats,
                       void* workspace, size_t workspace_bytes, void* ticket, int B, int H, int N, int dim, ct_stream_t s);
int ct_lattice_so3_bwd(const float* xyz, const float* residual, const float* log_R, float so3_eps, const float* R,
                       const float* shift, const float* scales, const float* kscale, const float* lattice,
                       const float* g_lattice, const float* g_keys, float* g_xyz, float* g_residual, float* g_log_R, float* g_R,
                       float* g_shift, float* g_scales, float* g_kscale, void* workspace, size_t workspace_bytes, int B, int H,
                       int N, int dim, ct_stream_t s);

/* so3 exponential map of the per-head rotation parameters — the third-party call of the transformers
 * (pytorch3d.transforms.so3.so3_exponential_map, layers/utils.py:6,29,56; eps = 1e-4 there):
 *   theta = sqrt(max(|v|^2, eps));  R = I + (sin theta / theta) K + ((1 - cos theta) / theta^2) K^2,  K = hat(v)
 * log_R f32[H,3] -> R f32[H,3,3];  backward: g_R f32[H,3,3] -> g_log_R f32[H,3] (overwritten).
 * H = 0 is CT_OK with nothing read or written (the pointers may be NULL then: an empty tensor has none). */
int ct_so3_exp_fwd(const float* log_R, float* R, int H, float eps, ct_stream_t s);
int ct_so3_exp_bwd(const float* log_R, const float* g_R, float* g_log_R, int H, float eps, ct_stream_t s);

/* ------------------------------------------------------------------------
 * Training-mode BatchNorm1d fused with the ReLU that follows it in the blocks' `after` stacks
 * (nn.Sequential(nn.BatchNorm1d(C), nn.ReLU(inplace=True)): layers/multihead_ct.py:67-68,149-153), one launch
 * forward and one backward:
 *   y[b,c,n] = relu?( (x - mean_c) * rsqrt(var_c + eps) * weight[c] + bias[c] ) [+ residual[b,c,n]],
 *   mean / biased var over (b, n); `residual` (nullable) is the union block's skip connection
 *   (layers/multihead_ct.py:198: `residual + self.after(...)`), its cotangent is gy itself;
 *   num_batches_tracked (nullable, int64[1]) is incremented, as nn.BatchNorm1d.forward does
 * x, y, gy, gx f32[B,C,N], rows of N contiguous floats, 16-byte aligned; each has a batch stride in floats (0 = C*N,
 * contiguous; a multiple of 4 >= C*N for a channel slice of a wider tensor: key_bn / values_bn act on the two halves
 * of the keys_values_pred output, layers/multihead_ct.py:89-91, and their input cotangents are written straight into
 * the two halves of that tensor's cotangent).  weight, bias f32[C]; save_mean, save_rstd f32[C] are written by the
 * forward and read by the backward.  running_mean / running_var f32[C] (both or neither) are updated in place as
 * torch does: r = (1 - momentum) * r + momentum * (mean | unbiased var).  Backward overwrites gx, g_weight, g_bias;
 * with relu != 0 the mask is recomputed from x.  Shapes: 2 <= B*N < 2^31 (ct_bn_relu_supported(B, C, N) != 0); a channel
 * with N % 4 == 0 and B*N <= 32768 is held in registers between the statistics and the normalisation (one read, one
 * write), longer channels and rows that are not float4-addressable are re-read per pass.
 * ---------------------------------------------------------------------- */
int ct_bn_relu_supported(int B, int C, int N);
/* One to eight norms over the same (B, N) in ONE launch — a single norm is a table with n = 1; the key / values norms of a
 * block's heads on channel ranges of the stacked projection, the heads' `after` norms on ranges of the concatenation
 * (layers/multihead_ct.py:89-91,67-68) are tables of several — one workgroup per channel of every norm.  amax_out f32[C]
 * (nullable): max |y| (after ReLU and skip) / max |g_x| per channel, a by-product of the pass — the operand maxima
 * ct_pw_gemm needs for the pointwise convolution that reads y / g_x next (n_amax = C). */
typedef struct {
  const float* x; long long x_batch_stride; const float* weight; const float* bias; float* running_mean; float* running_var;
  long long* num_batches_tracked; const float* residual; long long residual_batch_stride; float* y; long long y_batch_stride;
  float* save_mean; float* save_rstd; float* amax_out; int C; float eps; float momentum; int relu;
} ct_bn_fwd_item;
typedef struct {
  const float* x; long long x_batch_stride; const float* weight; const float* bias; const float* save_mean; const float* save_rstd;
  const float* gy; long long gy_batch_stride; float* gx; long long gx_batch_stride; float* g_weight; float* g_bias; float* amax_out;
  int C; int relu;
} ct_bn_bwd_item;
int ct_bn_group_fwd(const ct_bn_fwd_item* items, int n, int B, int N, ct_stream_t s);
int ct_bn_group_bwd(const ct_bn_bwd_item* items, int n, int B, int N, ct_stream_t s);
/* The same group around ONE statistics exchange between ranks — nn.SyncBatchNorm under data parallelism
 * (train_segmentation.py:128-130 converts every BatchNorm of the model): every phase of the group's norms in one launch — 2
 * launches + 1 collective per group and direction instead of 2 n + 1.  `items` is the WHOLE group (n >= 1, not capped): Ct
 * = sum of all n items' C and item i's channel offset c0_i in the buffers below come from all of them.  A call launches the
 * items [first, first + run), 1 <= run <= 8; first = 0, run = n is the whole group at once.  A bad range is CT_EINVAL.
 *   ct_bn_group_stats_fwd : local f32[2 Ct + 1] = [mean | sum (x - mean)^2 | count] of THIS rank's batch (only x, C and
 *                           x_batch_stride of the items are read); the count is written by the run that holds item 0;
 *   ct_bn_group_apply_fwd : gathered f32[world][2 Ct + 1] (the ranks' `local` blocks, one all_gather), merged per channel by
 *                           the parallel-variance rule -> y, save_mean, save_rstd, running statistics, amax_out of the run's
 *                           items; count_total f32[1] (nullable) = values per channel of the whole job (run of item 0);
 *   ct_bn_group_reduce_bwd: sums f32[2 Ct] = [sum g' | sum g' xhat] of this rank (g_weight / g_bias / gx of the items unused);
 *                           sums_copy f32[2 Ct] (nullable) receives the same values: the all_reduce runs in place on `sums`,
 *                           the copy stays this rank's g_bias / g_weight (torch: the gradient of a SyncBatchNorm's affine
 *                           parameters is local, DDP averages it) — one launch less than cloning the buffer;
 *   ct_bn_group_apply_bwd : sums all-reduced over the ranks + count -> gx, amax_out of the run's items. */
int ct_bn_group_stats_fwd(const ct_bn_fwd_item* items, int n, int first, int run, int B, int N, float* local, ct_stream_t s);
int ct_bn_group_apply_fwd(const ct_bn_fwd_item* items, int n, int first, int run, int B, int N, const float* gathered,
                          int world, float* count_total, ct_stream_t s);
int ct_bn_group_reduce_bwd(const ct_bn_bwd_item* items, int n, int first, int run, int B, int N, float* sums,
                           float* sums_copy /* nullable */, ct_stream_t s);
int ct_bn_group_apply_bwd(const ct_bn_bwd_item* items, int n, int first, int run, int B, int N, const float* sums,
                          const float* count, ct_stream_t s);

/* Eval-mode BatchNorm1d / SyncBatchNorm (+ ReLU, + skip): a per-channel affine on the stored statistics, forward only,
 *   y[b,c,n] = relu?( ((x - running_mean[c]) * rstd_c) * weight[c] + bias[c] ) [+ residual[b,c,n]],
 *   rstd_c = 1 / sqrt(running_var[c] + eps)
 * in torch's operation order (the mean is subtracted first).  x, y, residual and their batch strides as ct_bn_group_fwd (0 =
 * contiguous; a channel slice of a wider tensor is read, a channel range of a concatenation written, where it lies); y does
 * not overlap x or residual.  Rows that are 16-byte addressable (N % 4 == 0, strides % 4 == 0, aligned bases) move as
 * float4, all others float by float.  Nothing is written but y and amax_out f32[C] (nullable): max |y| per channel of the
 * values as stored (after ReLU and skip), the contract of ct_bn_group_fwd's; the running statistics are read-only here
 * and both are required.  Shapes: B*N >= 1 (one value per channel is legal: no variance is taken), B*N < 2^31
 * (ct_bn_eval_supported != 0).  Channels are cut over several workgroups when the launch has few of them; a channel
 * whose amax_out is asked for stays with one workgroup, which folds the maximum itself (no second launch, no atomics).
 * ct_bn_eval_group_fwd: 1 <= n <= 8 norms over the same (B, N) in one launch, as ct_bn_group_fwd; of ct_bn_fwd_item it reads x,
 * weight, bias, running_mean, running_var, residual, y, amax_out, the strides, C, eps and relu — save_mean, save_rstd,
 * momentum and num_batches_tracked are ignored and may be null.  Added under CT_ABI_VERSION 2 (additive). */
int ct_bn_eval_supported(int B, int C, int N);
int ct_bn_eval_group_fwd(const ct_bn_fwd_item* items, int n, int B, int N, ct_stream_t s);
/* Backward of ct_bn_eval_group_fwd: a norm whose statistics are frozen, in a forward that records gradients.  1 <= n <= 8
 * norms over the same (B, N) in one launch.  Per element, contraction off, with rs = 1.0f / sqrtf(running_var[c] + eps) and
 * xh = (x - running_mean[c]) * rs:
 *   o = xh * weight[c] + bias[c]            (the forward's expression: with relu != 0 an element passes only if the forward
 *                                            stored a positive value for it)
 *   g' = (relu && !(o > 0)) ? 0 : gy,   gx = g' * (weight[c] * rs),   g_bias[c] = sum g',   g_weight[c] = sum g' * xh
 * The cotangent of the forward's residual is gy itself and needs no kernel work.  x, gy, gx and their batch strides as
 * ct_bn_eval_group_fwd's x and y (0 = contiguous; a channel slice of a wider tensor is read, a channel range of one cotangent
 * tensor written, where it lies); gx overlaps neither x nor gy.  Rows of an item that are 16-byte addressable (N % 4 == 0,
 * strides % 4 == 0, aligned bases) move as float4, all others float by float — decided per item, so a norm gives the same
 * bits alone and inside a table.  g_weight and g_bias f32[C] are given both or neither (neither: the affine parameters are
 * frozen); gx may be null (the input needs no gradient); a call asks for at least one of gx and the pair.  amax_out f32[C]
 * (nullable): max |gx| per channel as stored, the contract of ct_bn_group_bwd's (with a null gx: of the values it would have
 * stored).  weight, bias, running_mean, running_var, x and gy are always required and read-only.  No workspace, no
 * allocation, no float atomics: an item that asks for the sums or the maxima keeps one workgroup per channel and adds in an
 * order fixed by (B, N) and its own addressability, so results are bit-equal from run to run; an item that asks for neither
 * is cut over workgroups as the forward is.  CT_EINVAL, before anything is launched, for a null required pointer, n outside
 * [1, 8], a batch stride that is neither 0 nor >= C*N, eps < 0 (or NaN), C < 1, B*N outside [1, 2^31), or only one of
 * g_weight / g_bias.  Added under CT_ABI_VERSION 3 (additive: the loader's missing-symbol scan checks it). */
typedef struct {
  const float* x; long long x_batch_stride; const float* weight; const float* bias;
  const float* running_mean; const float* running_var;
  const float* gy; long long gy_batch_stride; float* gx; long long gx_batch_stride;
  float* g_weight; float* g_bias; float* amax_out; int C; float eps; int relu;
} ct_bn_eval_bwd_item;
int ct_bn_eval_group_bwd(const ct_bn_eval_bwd_item* items, int n, int B, int N, ct_stream_t s);

/* ------------------------------------------------------------------------
 * Adaptive instance normalisation of the AdaIN blocks (AdaIn1dUpd: layers/utils.py:82-97 =
 * InstanceNorm1d(affine=False, eps) -> * (gamma + 1) -> + beta; followed by ReLU in `after`,
 * layers/multihead_ct_adain.py:64-66,183-187), one launch forward and one backward:
 *   y[b,c,n] = relu?( (x - mean_n x) * rsqrt(var_n x + eps) * (gamma[b,c] + 1) + beta[b,c] )
 * x, y, gy, gx f32[B,C,N]; gamma_beta f32[B,2,C] (the Linear(style) output: [:,0] scale, [:,1] bias);
 * mean, rstd f32[B*C] are written by the forward and read by the backward (biased variance).
 * Backward overwrites gx and g_gamma_beta f32[B,2,C]; with relu != 0 the mask is recomputed from x.
 * Every [B,C,N] argument has a batch stride in floats (0 = C*N, contiguous; >= C*N for a channel slice of a wider
 * tensor — keys_bn / values_bn on the halves of keys_values_pred, multihead_ct_adain.py:108-111); `residual` (nullable)
 * is added after the ReLU (the union's skip connection, :216), its cotangent is gy itself.
 * One to eight adaptive instance norms over the same (B, N) in ONE launch, as ct_bn_group_fwd / _bwd (a single norm is a table
 * with n = 1).  B >= 1, N >= 1 and every C >= 1: the empty shapes are the caller's.  amax_out (nullable):
 * amax_out[b * amax_batch_stride + c] = max |y| / max |g_x| of row (b, c), a by-product of the pass (amax_batch_stride 0 = C)
 * — operand maxima for ct_pw_gemm, as ct_bn_group_fwd's.
 * ---------------------------------------------------------------------- */
typedef struct {
  const float* x; long long x_batch_stride; const float* gamma_beta; const float* residual; long long residual_batch_stride;
  float* y; long long y_batch_stride; float* mean; float* rstd; float* amax_out; long long amax_batch_stride; int C; float eps;
  int relu;
  long long gamma_beta_batch_stride;   /* floats between clouds in gamma_beta (0 = 2*C: contiguous [B,2,C]); larger for a column
                                          range of a stacked style projection [B, sum 2*C_i] */
} ct_adain_fwd_item;
typedef struct {
  const float* x; long long x_batch_stride; const float* gamma_beta; const float* mean; const float* rstd; const float* gy;
  long long gy_batch_stride; float* gx; long long gx_batch_stride; float* g_gamma_beta; float* amax_out;
  long long amax_batch_stride; int C; int relu;
  long long gamma_beta_batch_stride;   /* as in ct_adain_fwd_item (g_gamma_beta is written contiguous [B,2,C]) */
} ct_adain_bwd_item;
int ct_adain_group_fwd(const ct_adain_fwd_item* items, int n, int B, int N, ct_stream_t s);
int ct_adain_group_bwd(const ct_adain_bwd_item* items, int n, int B, int N, ct_stream_t s);

/* ------------------------------------------------------------------------
 * Grouped 3^dim convolution over the rasterised planes / volumes, stride 1, padding 1
 * (MultiHead.conv: layers/multihead_ct.py:50-65 with bias; Res2DBlock / Res3DBlock:
 * unet2d/unet_parts.py:13-16, layers/v2v_groups.py:26-29 without), fp32 on the matrix
 * cores (v_mfma_f32_16x16x4_f32: exact fp32, one rounding per product, k-ordered).
 *   x f32[B, groups*Cin, *W]   w f32[groups*Cout, Cin, 3^dim]   bias f32[groups*Cout] | NULL
 *   y f32[B, groups*Cout, *W]
 * bwd_data : g_x from g_y and w.   bwd_weight: g_w (and g_bias unless NULL) from x and g_y;
 * both outputs are overwritten.  bwd_weight sums over (batch, positions) in workgroup-sized chunks:
 * with a workspace of ct_gconv_bwd_weight_workspace_bytes (0 = the shape does not use one) the chunk
 * sums are stored and added in a fixed order (bitwise reproducible); with workspace NULL they are
 * accumulated into g_w with float atomics (order not fixed, and several times slower).
 * ---------------------------------------------------------------------- */
int ct_gconv_fwd(const float* x, const float* w, const float* bias, float* y,
                 int B, int groups, int Cin, int Cout, int dim, const int* W, ct_stream_t s);
int ct_gconv_bwd_data(const float* g_y, const float* w, float* g_x,
                      int B, int groups, int Cin, int Cout, int dim, const int* W, ct_stream_t s);
int ct_gconv_supported(int B, int groups, int Cin, int Cout, int dim, const int* W);   /* 1: all three passes have a tile plan; 0: fall back to the library conv
                                                                                              (very wide rows with many channels per group) */
size_t ct_gconv_bwd_weight_workspace_bytes(int B, int groups, int Cin, int Cout, int dim, const int* W);
int ct_gconv_bwd_weight(const float* x, const float* g_y, float* g_w, float* g_bias,
                        void* workspace, size_t workspace_bytes,
                        int B, int groups, int Cin, int Cout, int dim, const int* W, ct_stream_t s);

/* ------------------------------------------------------------------------
 * The forward convolution with the eval-mode BatchNorm, the skip connection and the ReLU of a grouped Res block
 * (Res2DBlock / Res3DBlock / Basic2DBlock / Basic3DBlock in eval mode) in its write-out:
 *   y = relu?( bn(conv(x)) + bn'?(skip) )
 * Per output element, every operation one fp32 rounding (contraction is off for the whole library), c its channel:
 *   v = the value ct_gconv_fwd stores (the same bits, bias included)
 *   o = ((v - running_mean[c]) * rs[c]) * weight[c] + bias[c],   rs[c] = 1.0f / sqrtf(running_var[c] + eps)
 *       (the operation sequence of ct_bn_eval_group_fwd; no folded scale or shift)
 *   with skip:      t = skip_norm ? ((s - mean'[c]) * rs'[c]) * weight'[c] + bias'[c] : s;   o = o + t
 *   with relu != 0: o = fmaxf(o, 0.0f), after the add
 * Bit-equality contract: y holds exactly the bits of (1) ct_gconv_fwd into a scratch tensor, (2) ct_bn_eval_group_fwd on it
 * viewed as [B, C, volume], with relu = 0 when a skip is given and the caller's relu otherwise, (3) with skip_norm the same
 * on skip with relu = 0, (4) torch.add, (5) torch.relu.  One difference: a NaN sum is stored as 0 here (fmaxf) and as NaN by
 * torch.relu.
 *   norm       required; weight / bias / running_mean / running_var f32[groups*Cout], all required; eps >= 0
 *   skip       f32[B, groups*Cout, *W] | NULL, read with the index and width of the y store;  skip_norm  NULL = added as it is
 * Only y is written; y overlaps neither x nor skip.  No atomics: bitwise reproducible.
 * The write-out exists on the K-split, quad and dense 2^d forward kernels; ct_gconv_fwd_norm_supported is 1 exactly where
 * ct_gconv_fwd takes one of them for tensors on the 16-byte grid, and 0 on the four-channel kernels and the one-position form
 * (compose the sequence above there).  The call launches the one kernel ct_gconv_fwd launches for the same arguments
 * (ct_debug_last_launch: the same tags) and has no two-launch fallback.  CT_EINVAL before any launch: a NULL required pointer,
 * skip_norm without skip, eps < 0 or NaN, x / w / y / skip off the 16-byte grid, a shape ct_gconv_fwd_norm_supported refuses.
 * ---------------------------------------------------------------------- */
typedef struct { const float* weight; const float* bias; const float* running_mean; const float* running_var; float eps; } ct_gconv_norm;
int ct_gconv_fwd_norm_supported(int B, int groups, int Cin, int Cout, int dim, const int* W);
int ct_gconv_fwd_norm(const float* x, const float* w, const float* bias, const ct_gconv_norm* norm,
                      const float* skip, const ct_gconv_norm* skip_norm, int relu, float* y,
                      int B, int groups, int Cin, int Cout, int dim, const int* W, ct_stream_t s);

/* ------------------------------------------------------------------------
 * Precision mode of the grouped convolution: the counterpart of ct_set_pw_precision for ct_gconv_fwd, ct_gconv_bwd_data and
 * ct_gconv_fwd_norm.  Process-wide host state, atomic, never read by a kernel: each of the three entry points reads the
 * effective value ONCE, where it plans its launch.  Added under CT_ABI_VERSION 3 (additive).  Independent of the pointwise
 * GEMMs' mode.
 *   CT_GCONV_PRECISION_HIGHEST (the default): everything above, bit for bit.
 *   CT_GCONV_PRECISION_HIGH: the quad and K-split kernels (ct_gconv_precision_covers) multiply ONE f16 term per operand on
 *     v_mfma_f32_16x16x16_f16 with fp32 accumulators: 11-bit significands, the precision of TF32, for which gfx950 has no matrix
 *     instruction.  h = f16(s v) under power-of-two scales s with s M in [2^13, 2^14), taken inside the kernel from the operands
 *     the workgroup has staged: M = the largest finite magnitude of the staged input tile (K-split: of the tile of each
 *     16-channel contraction block) and of each output-channel row of the staged bank (K-split: per row and block); no
 *     pre-pass, no workspace, the same signatures.  The accumulators are multiplied by the exact 1/s_x and 1/s_w (K-split: per
 *     block, then added in fp32) before the bias is added; the stores, the NORM write-out and the launch tags are those of the
 *     default mode, and within the mode ct_gconv_fwd_norm keeps its bit-equality contract with ct_gconv_fwd.  An all-zero tile
 *     or row has s = 1 and contributes exact zeros; inf and NaN do not set a scale and pass through f16 as they are, reaching the
 *     outputs they reach in the default mode.  No atomics: every output is written once, run-to-run bit-equal.
 *     Error bound.  For an element v under a scale with maximum M:  |f16(s v)/s - v| <= 2^-11 |v| + 2^-38 M  (the rounding of a
 *     normal f16; a subnormal's 2^-25 over s >= 2^13 / M).  f16 x f16 products are exact in fp32, so with dw, dx these element
 *     errors one product is off by w dx + x dw + dw dx: (2^-10 + 2^-22) |w x| from the normal parts, 2^-38 (M_w |x| + M_x |w|) from
 *     the subnormal parts against the other operand's value, 2^-11 of that again against its normal error, subnormal against
 *     subnormal at most 2^-38 M_w |x| once more.  Any tile's maximum is at most the maximum M_x of the output's (batch, group)
 *     slab, any block's row maximum at most the row's M_w.  With K = Cin 3^dim terms and eps_acc = (K + 2) 2^-24, the fp32
 *     accumulation allowance of the default mode (the products are exact here; the K-split folds are fp32 additions like its):
 *       |err| <= (2^-10 + 2^-22 + eps_acc) * sum |w x|  +  2^-37 * ( M_w * sum |x|  +  M_x * sum |w| )
 *   The mode is a permission, not an order: the one-position form, the dense 2^d form, the four-channel kernels, quad shapes
 *   below 16 input channels per group, every weight-gradient kernel and the 1x1 skip GEMM stay fp32.  Other values of p select
 *   CT_GCONV_PRECISION_HIGHEST.
 * ct_gconv_precision_override(p): p = 0 / 1 sets the mode for the entry points the CALLING THREAD invokes, whatever the
 * process-wide value says, p < 0 ends the override: how a backward-data runs in its forward's precision on whichever thread it
 * is called.  ct_get_gconv_precision() returns the value in effect for the calling thread.
 * ct_gconv_precision_covers(pass, ...): pass 0 = ct_gconv_fwd / ct_gconv_fwd_norm, 1 = ct_gconv_bwd_data; 1 when that call takes a
 * one-term kernel under CT_GCONV_PRECISION_HIGH for tensors on the 16-byte grid, else 0.  The host planner's answer: no device, and
 * independent of the current mode.
 * HIP graphs: the mode is read when a launch is recorded; a replay runs the captured kernels.
 * ---------------------------------------------------------------------- */
#define CT_GCONV_PRECISION_HIGHEST 0   /* fp32 MFMA: the default, as before */
#define CT_GCONV_PRECISION_HIGH    1   /* one f16 term per operand: 11-bit significands (TF32-class), fp32 accumulation */
void ct_set_gconv_precision(int p);      /* process-wide, atomic; other values -> HIGHEST */
int  ct_get_gconv_precision(void);       /* the effective value for the calling thread */
void ct_gconv_precision_override(int p); /* this thread's entry points only; -1: none */
int  ct_gconv_precision_covers(int pass, int B, int groups, int Cin, int Cout, int dim, const int* W);

/* ------------------------------------------------------------------------
 * Plane-resident MHCT core: the part of a MultiHead block between its norms,
 *   out = Slice(lattice, conv(Splat(lattice, values)))                (layers/multihead_ct.py:99-107:
 *   DifferentiablePositions -> Splat (max, zero floor) -> grouped 3^dim conv with bias -> Slice;
 *   layers/multihead_ct_adain.py:118-125 and layers/cloud_transform.py:72-227 likewise)
 * as ONE kernel per direction-independent plane: the rasterised grid z and the convolved grid y of a (batch, head)
 * plane stay in LDS.  Shapes: the grids whose two tiles fit a CU beside the filter bank — 2D 32x32 C16, 2D 16x16 C16,
 * 3D 8x8x8 C32 (ct_mhct_core_supported != 0), N % 4 == 0, 16-byte aligned tensors.
 *   keys f32[B,H*dim,N] (the lattice), feat f32[B,H*C,N], pad as for Splat, conv_w f32[H*C,C,3^dim], conv_b f32[H*C] | NULL
 *   out f32[B,H*C,N] (overwritten)
 *   z_save, y_save f32[B,H*C,G] | NULL: the two grids as tensors, for ct_mhct_core_bwd (training); with NULL they never
 *     leave the chip.  occ_count int64[1] | NULL: number of |z| > 1e-9 (layers/multihead_ct.py:104-105).
 * With few planes (B*H < CUs/2) a plane is shared by a cluster of 2..8 workgroups that exchange their partial grids
 * through `workspace` (ct_mhct_core_workspace_bytes).  The workspace also holds the clusters' arrival counters, which
 * must be ZERO when a launch starts: call ct_mhct_core_workspace_init once after allocating it (one small memset); every
 * launch leaves the counters zeroed again, so the workspace can be reused launch after launch (stream-ordered) without
 * further resets.  A cluster spins on its partners (bounded): do not run two of these launches concurrently on different
 * streams of one device, nor share one workspace between streams.
 * Backward (ct_mhct_core_bwd): from the saved grids, as Slice backward -> conv backward (data, weight) -> Splat backward
 * on this library's kernels; overwrites g_feat f32[B,H*C,N], g_keys f32[B,H*dim,N] (Slice's and Splat's key cotangents
 * summed), g_w f32[H*C,C,3^dim], g_b f32[H*C] | NULL; workspace of ct_mhct_core_bwd_workspace_bytes.
 * ---------------------------------------------------------------------- */
int ct_mhct_core_supported(int B, int H, int C, int N, int dim, const int* W);
size_t ct_mhct_core_workspace_bytes(int B, int H, int C, int N, int dim, const int* W);
int ct_mhct_core_workspace_init(void* workspace, size_t workspace_bytes, int B, int H, int C, int N, int dim, const int* W,
                                ct_stream_t s);
int ct_mhct_core_fwd(const float* keys, const float* feat, const void* pad, int pad_dtype, const float* conv_w,
                     const float* conv_b, float* out, float* z_save, float* y_save, int64_t* occ_count,
                     void* workspace, size_t workspace_bytes, int B, int H, int C, int N, int dim, const int* W,
                     ct_stream_t s);
size_t ct_mhct_core_bwd_workspace_bytes(int B, int H, int C, int N, int dim, const int* W);
int ct_mhct_core_bwd(const float* keys, const float* feat, const void* pad, int pad_dtype, const float* conv_w,
                     const float* z, const float* y, const float* g_out, float* g_feat, float* g_keys, float* g_w,
                     float* g_b, void* workspace, size_t workspace_bytes, int B, int H, int C, int N, int dim,
                     const int* W, ct_stream_t s);
/* the same with arrival tickets (ct_tickets_init; NULL = none) handed to its Slice / Splat backward passes */
int ct_mhct_core_bwd_tk(const float* keys, const float* feat, const void* pad, int pad_dtype, const float* conv_w,
                        const float* z, const float* y, const float* g_out, float* g_feat, float* g_keys, float* g_w,
                        float* g_b, void* workspace, size_t workspace_bytes, void* tickets, int B, int H, int C, int N,
                        int dim, const int* W, ct_stream_t s);
/* The LDS-resident BACKWARD of the core, for the grid whose five tiles fit a CU (2D 16x16 with 16 features per head:
 * ct_mhct_core_bwd_fused_supported): nothing of the forward is read back — one workgroup per plane recomputes z and conv(z)
 * from the points and walks Slice backward -> conv^T / filter cotangent -> Splat backward in LDS (ct_mhct_core_fwd may then be
 * called with z_save = y_save = NULL in training too).  Same outputs as ct_mhct_core_bwd; the per-plane filter / bias
 * cotangents go through `workspace` (ct_mhct_core_bwd_fused_workspace_bytes) and are added over the batch in a fixed order. */
int ct_mhct_core_bwd_fused_supported(int B, int H, int C, int N, int dim, const int* W);
size_t ct_mhct_core_bwd_fused_workspace_bytes(int B, int H, int C, int N, int dim, const int* W);
int ct_mhct_core_bwd_fused(const float* keys, const float* feat, const void* pad, int pad_dtype, const float* conv_w,
                           const float* conv_b, const float* g_out, float* g_feat, float* g_keys, float* g_w, float* g_b,
                           void* workspace, size_t workspace_bytes, int B, int H, int C, int N, int dim, const int* W,
                           ct_stream_t s);
/* A cluster whose workgroup gives up waiting for its partners (never in a correct run: co-residency of a plane's workgroups
 * rests on in-order dispatch and a grid of at most one workgroup per CU) sets the workspace's status word, writes NaN where
 * its results would have gone, and still takes part in the counters' bookkeeping — the workspace stays usable, the failure
 * cannot pass for a result; ct_mhct_core_status reads the word (callers check it at their flush points and re-initialise).
 * Test hooks: bit 0 = one workgroup per plane (no clusters); bit 1 = fault injection: the last workgroup of plane 0 arrives
 * late and its partners time out after a short spin; bits 8.. = force that many workgroups per plane (1, 2, 4, 8).
 * ct_mhct_core_status copies the workspace's status word to the host AFTER synchronising the stream (a test helper, the
 * only call of this library that waits for the device): 0 = no cluster gave up waiting for its partners. */
void ct_debug_set_core(unsigned flags);
/* Test hook of the grouped convolution (process-wide, read by the three ct_gconv entry points):
 *   bit 0 (1)   small-volume weight gradients take the vector-ALU kernel instead of the matrix-core one (A/B measurements,
 *               tools/gconv64_bench.py);
 *   bit 1 (2)   four-channel 3D groups never take the matrix-core kernels (forward, backward-data and weight gradient);
 *   bit 2 (4)   four-channel 3D groups take the matrix-core forward / backward-data kernel wherever its plan fits, whatever the
 *               size (default: from 2 M positions); bit 1 wins over bit 2;
 *   bits 8..15  input channels per group from which forward / backward-data take the K-split kernel (0: the default, 32).
 * The three entry points name the kernels they launched through ct_debug_last_launch, as the Splat / Slice entry points do: one
 * tag per kernel and per host-side choice that changes its code path, joined with '+' (tests/gconv_families.py lists them). */
void ct_debug_set_gconv(unsigned flags);
/* Test hook of the EMD auction: bit 0 = the per-batch update (GetMax, Assign, next list) on one workgroup per batch in every
 * iteration (default: several workgroups per batch while the batch has more than 1024 unassigned points). */
void ct_debug_set_emd(unsigned flags);
int ct_mhct_core_status(const void* workspace, size_t workspace_bytes, int B, int H, int C, int N, int dim, const int* W,
                        int* host_status, ct_stream_t s);

/* ------------------------------------------------------------------------
 * Chamfer distance (chamfer_extension/chamfer_cuda.cpp:30-33 `forward`,
 * `backward`; kernels chamfer.cu:12-195).  xyz1 f32[B,n,3], xyz2 f32[B,m,3];
 * dist1 f32[B,n], idx1 i32[B,n] (nearest point of cloud 2, lowest index on
 * ties), dist2/idx2 symmetric.  Backward overwrites g_xyz1, g_xyz2.
 * ---------------------------------------------------------------------- */
int ct_chamfer_fwd(const float* xyz1, const float* xyz2, float* dist1, float* dist2,
                   int32_t* idx1, int32_t* idx2, int B, int n, int m, ct_stream_t s);
int ct_chamfer_bwd(const float* xyz1, const float* xyz2, const float* g_dist1, const float* g_dist2,
                   const int32_t* idx1, const int32_t* idx2, float* g_xyz1, float* g_xyz2,
                   int B, int n, int m, ct_stream_t s);

/* ------------------------------------------------------------------------
 * Chamfer distance of clouds of different lengths in one batch, and the metric table of an evaluation on top of it
 * (utils/grdnet_utils.py:9-23 `ChamferDistance(ignore_zeros)`, whose boolean index works at B == 1 only, and :105-129
 * `Metrics._get_f_score / _get_chamfer_distance`; eval_inpainting.py:187-226, the per-sample loop they are called from).
 * Added under CT_ABI_VERSION 3 (additive symbols).  All five return CT_EINVAL for a null required pointer, B <= 0, n <= 0,
 * m <= 0 or B > 65535; they enqueue on the stream s, allocate nothing and read nothing back to the host.
 *
 * ct_chamfer_fwd_counts: cnt1, cnt2 i32[B] in device memory, either may be null ("all n" / "all m").  Cloud b of set 1 is
 *   the rows [0, cnt1[b]) of xyz1[b]; rows at or beyond a count are never read, as queries or as targets (they may hold
 *   anything, NaN included).  Rows [0, cnt) of every output carry exactly the bits ct_chamfer_fwd returns for that pair of
 *   clouds alone (B = 1, n = cnt1[b], m = cnt2[b]): the same distance expression, the lowest index on ties.  Rows at or
 *   beyond the count get dist = 0, idx = -1, and so does every row of a cloud whose target cloud is empty; no output
 *   element is left unwritten.  A count outside [0, n] is clamped into it.
 * ct_chamfer_bwd_counts: ct_chamfer_bwd with the same two counts.  Rows at or beyond the count contribute nothing and
 *   receive an exact +0.0.  Under ct_set_deterministic(1): the ordered form, per-cloud n and m, the bits of ct_chamfer_bwd
 *   on each pair alone.
 * ct_rows_compact: x f32[B,n,3] -> y f32[B,n,3], count i32[B].  Per cloud, the rows with (x + y) + z != 0.0f in their
 *   input order (`torch.sum(xyz, dim=2).ne(0)` of grdnet_utils.py:20-21: a row such as (1, -1, 0) is dropped too, a NaN
 *   row is kept), then zero rows; count[b] = the number kept.  Out of place: y must not overlap x (x == y: CT_EINVAL).
 *   No atomics, so the result is the same on every run.
 * ct_chamfer_metrics: dist1 f32[B,n], dist2 f32[B,m] (squared, as ct_chamfer_fwd* writes them), counts as above, either
 *   may be null -> stats f64[B,2,3] (may be null), table f32[B,4].  stats[b][k] = (hits, sum d, sum (double)sqrtf(d)) over
 *   rows [0, cnt_k), hits = the number of rows with sqrtf(d) < th in float32, both sums accumulated in float64.
 *   table[b] = (fscore, precision, recall, chamfer) in calculate_fscore's convention (utils/f1_metric.py:14-28) with cloud
 *   1 as its `gt` and cloud 2 as its `pr`: precision = (float)hits1 * (1.0f / (float)cnt1), recall = (float)hits2 *
 *   (1.0f / (float)cnt2) (the rounding of torch's float32 mean of the 0/1 flags, which multiplies the sum by the reciprocal
 *   of the length: the columns equal metrics.fscore_batch's bit for bit; a plain division differs from it in the last bit
 *   for some pairs, 15 / 129 for one), fscore = 2 * recall * precision / (recall + precision) in float32, 0 when recall +
 *   precision == 0, and
 *   chamfer = (float)(sum d1 / cnt1 + sum d2 / cnt2).  If either count is 0: fscore = precision = recall = 0 (what
 *   calculate_fscore returns for an empty cloud) and chamfer = NaN (the mean of nothing).  One workgroup per cloud, a fixed
 *   reduction order: bit-equal from run to run.
 * ---------------------------------------------------------------------- */
int ct_chamfer_fwd_counts(const float* xyz1, const float* xyz2, const int32_t* cnt1, const int32_t* cnt2, float* dist1,
                          float* dist2, int32_t* idx1, int32_t* idx2, int B, int n, int m, ct_stream_t s);
int ct_chamfer_bwd_counts(const float* xyz1, const float* xyz2, const int32_t* cnt1, const int32_t* cnt2, const float* g_dist1,
                          const float* g_dist2, const int32_t* idx1, const int32_t* idx2, float* g_xyz1, float* g_xyz2,
                          int B, int n, int m, ct_stream_t s);
int ct_rows_compact(const float* x, float* y, int32_t* count, int B, int n, ct_stream_t s);
int ct_chamfer_metrics(const float* dist1, const float* dist2, const int32_t* cnt1, const int32_t* cnt2, float th, double* stats,
                       float* table, int B, int n, int m, ct_stream_t s);

/* ------------------------------------------------------------------------
 * Approximate EMD by auction (emd_linear/emd.cpp:28-31 `forward`, `backward`;
 * kernels emd_cuda.cu:23-316).  xyz1, xyz2 f32[B,n,3] in [0,1]^3; outputs
 * dist f32[B,n] (squared distance to the assigned target) and assignment
 * i32[B,n].  Preconditions as the reference (emd_cuda.cu:236-249): n % 1024 == 0,
 * B <= 512 -> CT_EPRECOND otherwise; iters >= 1.  The reference's 12 caller-allocated
 * scratch tensors (emd_module.py:41-54) become one opaque workspace.
 * Results: the reference's own kernels (built for gfx950, oracle/Makefile `ref_emd`) return
 * the same assignment exactly and the same distances (bit for bit against their
 * -ffp-contract=off build, <= 2 ulp against the default-contraction one) wherever they are
 * deterministic; where several bidders are within 1e-6 of a target's best increment the
 * reference lets the last store win (emd_cuda.cu:181-194) — here: the highest bidder index,
 * always (tests/test_emd_gpu.py, tests/golden/emd_reference.npz).
 * ---------------------------------------------------------------------- */
size_t ct_emd_workspace_bytes(int B, int n);
int ct_emd_fwd(const float* xyz1, const float* xyz2, float* dist, int32_t* assignment,
               void* workspace, size_t workspace_bytes, int B, int n, float eps, int iters,
               ct_stream_t s);
/* g_xyz1 = 2 g_dist (x1 - x2[assignment]); no gradient to xyz2 (emd_module.py:66-70). */
int ct_emd_bwd(const float* xyz1, const float* xyz2, const float* g_dist, const int32_t* assignment,
               float* g_xyz1, int B, int n, ct_stream_t s);

/* ------------------------------------------------------------------------
 * The auction for any cloud size and clouds of different lengths in one batch.  Added under CT_ABI_VERSION 3 (additive
 * symbols); ct_emd_fwd / ct_emd_bwd above keep their preconditions, their results and their launches.
 *
 * xyz1, xyz2 f32[B,n,3]; n is the ROW STRIDE.  Cloud b is the rows [0, c_b) of BOTH tensors, c_b = count[b] clamped into
 * [0, n] on the device; count is i32[B] in device memory, or null = every row (c_b = n).  The host never reads count: no
 * synchronisation, the same launches for every value, so a captured graph replays with new counts in the same buffer.
 * Any n >= 1; B <= 512 (CT_EPRECOND otherwise); iters >= 1.  The workspace is that of ct_emd_workspace_bytes(B, n).
 *
 * ct_emd_fwd_counts: rows [0, c_b) of dist and assignment carry the auction of oracle/emd_ref.c run on that pair of clouds
 *   alone with its n = c_b: value = (float)(3.0 - sqrt(d2) - price) evaluated in double and rounded once, d2 by two fmaf;
 *   the lowest target index on value ties; the highest bidder index on GetMax window ties; every remaining bidder is
 *   force-assigned to its bid in the last iteration.  Where c_b % 1024 == 0 those rows are exactly the bits ct_emd_fwd
 *   returns for that pair at B = 1, n = c_b.  Rows at or beyond c_b are never read, neither as bidders nor as targets (they
 *   may hold anything, NaN included), and get dist = 0, assignment = -1; no output element is left unwritten.  c_b = 0:
 *   nothing to do; c_b = 1: assignment[0] = 0.
 * ct_emd_bwd_counts: g_xyz1 = 2 g_dist (x1 - x2[assignment]) on the rows below c_b; the rows at or beyond it receive an
 *   exact +0.0 by a store, their g_dist and assignment are not read (a NaN there does not leak).
 *
 * CT_EINVAL for a null required pointer (everything but count), B <= 0, n <= 0 or iters < 1; CT_EPRECOND for B > 512;
 * CT_EWORKSPACE for a short workspace — all before any launch and without touching a device.  The deterministic switch
 * (ct_set_deterministic) neither changes nor refuses these entries, as it does not ct_emd_fwd: the auction has one outcome.
 * Not covered: n != m, a gradient for xyz2.
 * ---------------------------------------------------------------------- */
int ct_emd_fwd_counts(const float* xyz1, const float* xyz2, const int32_t* count, float* dist, int32_t* assignment,
                      void* workspace, size_t workspace_bytes, int B, int n, float eps, int iters, ct_stream_t s);
int ct_emd_bwd_counts(const float* xyz1, const float* xyz2, const int32_t* count, const float* g_dist,
                      const int32_t* assignment, float* g_xyz1, int B, int n, ct_stream_t s);

/* ------------------------------------------------------------------------
 * Long auctions: the tail in one launch per cloud, and what the auction came to.  Added under CT_ABI_VERSION 3 (additive
 * symbols); the four entries above keep their results, their launches and their workspace size.
 *
 * ct_emd_fwd_tail computes what ct_emd_fwd (count null and n % 1024 == 0) or ct_emd_fwd_counts (otherwise) computes, bit for
 * bit, with another schedule: the ordinary iterations are enqueued as there; after iteration tail_from (0-based; negative = the
 * library's default) and after every few iterations from then on, one launch gives each cloud whose bidder list has become short
 * to ONE workgroup, which runs all remaining iterations of that cloud, the forced last one and the distances included; the
 * launches that follow skip such a cloud.  tail_from >= iters - 1 enqueues the ordinary iterations alone.  No host
 * synchronisation; the launches depend on (B, n, iters, tail_from, count == null) only, so a captured graph replays with other
 * clouds and other counts in the same buffers.
 *
 * info, i32[B,2] in device memory or null, is written on the device: info[b,0] = the index of the first iteration at whose start
 * cloud b had no bidder left, or iters if there was none; info[b,1] = the number of bidders of the last iteration, which it
 * force-assigns — 0 exactly when the auction finished.  A cloud without rows has {0, 0}.
 *
 * ct_emd_tail_supported(B, n): 1 where ct_emd_fwd_tail takes the shape (1 <= B <= 512, 1 <= n <= 16384), else 0.
 * ct_emd_tail_workspace_bytes(B, n): its workspace (that of ct_emd_workspace_bytes and the per-cloud state); 0 for B or n <= 0.
 * CT_EINVAL for a null required pointer (everything but count and info), B <= 0, n <= 0, iters < 1 or a shape the query
 * declines; CT_EPRECOND for B > 512; CT_EWORKSPACE for a short workspace — all before any launch.  ct_emd_bwd /
 * ct_emd_bwd_counts serve this forward as they are.  The deterministic switch neither changes nor refuses it.
 * ct_debug_set_emd_tail(u_tail, every): test hook — the longest list the tail launch takes (at most 2048; negative = default)
 * and the number of iterations between two tail launches (<= 0 = default).  The defaults come from a measurement (DESIGN.md
 * §4.20): on an MI355X one workgroup does not run an iteration faster than the ordinary launches at any bidder count, so by
 * default the tail launch takes a cloud only once its list is empty (it writes the distances; later launches skip the cloud).
 * ---------------------------------------------------------------------- */
int ct_emd_tail_supported(int B, int n);
size_t ct_emd_tail_workspace_bytes(int B, int n);
int ct_emd_fwd_tail(const float* xyz1, const float* xyz2, const int32_t* count, float* dist, int32_t* assignment, int32_t* info,
                    void* workspace, size_t workspace_bytes, int B, int n, float eps, int iters, int tail_from, ct_stream_t s);
void ct_debug_set_emd_tail(int u_tail, int every);

/* ------------------------------------------------------------------------
 * Pointwise (kernel size 1) convolutions of the MHCT blocks and their gradients
 * (layers/multihead_ct.py:31-33,62-66,89-91: nn.Conv1d(Ci, Co, 1) on [B,Ci,N]), fp32 in /
 * fp32 out on the f16 matrix pipes: operands are scaled by a per-tensor power of two
 * and split into two f16 terms (22 bits), three MFMA terms per product, fp32 accumulation.
 *   CT_PW_FWD:   a = W f32[Co,Ci], b = x f32[B,Ci,N]   -> out = y f32[B,Co,N]   (y[b] = W x[b])
 *   CT_PW_DGRAD: a = W f32[Co,Ci], b = g_y f32[B,Co,N] -> out = g_x f32[B,Ci,N] (W^T g_y[b]; W^T goes
 *                through the workspace)
 *   CT_PW_WGRAD: a = g_y f32[B,Co,N], b = x f32[B,Ci,N] -> out = g_W f32[Co,Ci] (sum_b g_y[b] x[b]^T,
 *                partial sums added in a fixed order: deterministic)
 * amax_a / amax_b: device f32[n_amax_*] whose maximum is (an upper bound within ~2^10 of) max |.| of the
 * whole operand tensor; the GEMM folds them when it starts.  Either ct_amax_f32's ct_amax_len()
 * partial maxima, or what the kernel that produced the operand left behind (ct_bn_group_fwd /
 * _bwd: one per channel; ct_adain_group_*: one per (cloud, channel)); n_amax_* <= 32768.  NULL = scale 1 (the caller then guarantees
 * |values| < 65504).  Co, Ci, N multiples of 4,
 * 16-byte aligned pointers -> CT_EINVAL otherwise.  Workspace: ct_pw_gemm_workspace_bytes.
 * ---------------------------------------------------------------------- */
#define CT_PW_FWD 0
#define CT_PW_DGRAD 1
#define CT_PW_WGRAD 2
#define CT_PW_DGRAD_T 3 /* as CT_PW_DGRAD with a = W^T f32[Ci,Co] already (ct_pw_prep_weight): no workspace */
int ct_amax_f32(const float* x, int64_t n, float* amax, ct_stream_t s);
int ct_amax_len(void);
/* a layer's weight for all three products in one launch: its partial maxima (ct_pw_prep_weight_partials(Co, Ci) of them, 0 =
 * too many: use ct_amax_f32) and, when wt != NULL, W^T for CT_PW_DGRAD_T */
int ct_pw_prep_weight_partials(int Co, int Ci);
int ct_pw_prep_weight(const float* w, float* wt, float* amax, int Co, int Ci, ct_stream_t s);
size_t ct_pw_gemm_workspace_bytes(int mode, int B, int Co, int Ci, int N);
int ct_pw_gemm(int mode, const float* a, const float* b, float* out, const float* amax_a, int n_amax_a,
               const float* amax_b, int n_amax_b, void* workspace, size_t workspace_bytes, int B, int Co, int Ci,
               int N, ct_stream_t s);
/* Per-ROW scales.  The split keeps 22 bits of an element relative to its SCALE, and f16's exponent range ends the story below
 * ~2^-17 of it: with one scale per tensor an element 2^-17 .. 2^-24 below the tensor's maximum keeps 22 .. 15 bits, and below
 * 2^-24 it is flushed.  Error bound of one output, eps = 2^-21, M_a / M_b the maxima the scales were taken from:
 *     |err_ij| <= eps * sum_k |a_ik b_kj|  +  2^-38 * ( M_a * sum_k |b_kj|  +  M_b * sum_k |a_ik| ).
 * The second term is invisible while the rows of an operand are of one magnitude (post-norm activations) and takes over for
 * an output whose OWN operand row is tiny against its tensor: the weight gradient's row co sees only channel co of g_y — a
 * nearly-dead channel group 2^-24 below the tensor's maximum came out at 1e-5 relative, 2^-26 at 7e-5 (rocBLAS fp32: 1e-7).
 * ct_pw_gemm_rs takes the maxima PER ROW of an operand's k-contiguous arrangement — rows_a > 0: amax_a is
 * f32[n_amax_a / rows_a][rows_a], rows_a = Co (CT_PW_FWD: rows of W; CT_PW_WGRAD: channels of g_y) or Ci (CT_PW_DGRAD_T: rows
 * of W^T); rows_b = Ci for the channels of x in CT_PW_WGRAD — scales every row by its own power of two and takes the factor
 * out of that row's (column's) outputs, exactly: M_a, M_b in the bound become the ROW's maxima, i.e. the bound holds relative to
 * every output's own operands.  Both operands of the weight gradient can be row-scaled (its summed index is the point, not
 * the channel); in the forward and the data gradient the activation's summed index IS the channel, so it keeps one scale
 * (rows_b is ignored there) and its term of the bound stays M_b * sum_k |a_ik|: a contribution that is itself 2^-17 of the
 * row's largest.  Producers of per-row maxima: ct_bn_group_* / ct_bn_eval_group_fwd (per channel), ct_adain_group_* (per
 * (cloud, channel)), ct_amax_rows_f32 (x f32[B,C,N] -> f32[C]), ct_pw_prep_weight_rs (W -> rowmax f32[ceil(Ci/32)][Co] for
 * CT_PW_FWD, colmax f32[ceil(Co/32)][Ci] for CT_PW_DGRAD_T, and W^T).  n_amax_* <= 32768.  rows_* = 0: ct_pw_gemm. */
int ct_amax_rows_f32(const float* x, int B, int C, int N, float* amax, ct_stream_t s);
int ct_pw_prep_weight_rs(const float* w, float* wt, float* rowmax, float* colmax, int Co, int Ci, ct_stream_t s);
int ct_pw_gemm_rs(int mode, const float* a, const float* b, float* out, const float* amax_a, int n_amax_a, int rows_a,
                  const float* amax_b, int n_amax_b, int rows_b, void* workspace, size_t workspace_bytes, int B, int Co,
                  int Ci, int N, ct_stream_t s);
/* ct_pw_gemm_rs with out = product + addend, the addend read in the kernel's epilogue (f32 laid out as `out`, 16-byte aligned,
 * not `out` itself; NULL = ct_pw_gemm_rs).  For the data gradient of a projection whose INPUT also feeds a skip connection
 * (layers/multihead_ct.py:170-198: `residual = shortcut(x)` beside `keys_values_pred(x)`): autograd's sum of the two cotangents
 * of x — a pass over three tensors the size of x — becomes one more read inside the GEMM.  CT_PW_FWD / CT_PW_DGRAD /
 * CT_PW_DGRAD_T; CT_PW_WGRAD (its output is a fold of slabs) -> CT_EINVAL. */
int ct_pw_gemm_rs_add(int mode, const float* a, const float* b, float* out, const float* addend, const float* amax_a, int n_amax_a,
                      int rows_a, const float* amax_b, int n_amax_b, int rows_b, void* workspace, size_t workspace_bytes, int B,
                      int Co, int Ci, int N, ct_stream_t s);
/* CT_PW_FWD with the eval-mode BatchNorm1d (+ ReLU, + skip) that follows the projection applied in the GEMM's epilogue — the
 * inference path's `keys_values_pred` -> key_bn / values_bn of every head and the union block's `after` (PointwiseConv1d ->
 * BatchNorm1d -> ReLU, + the skip connection: layers/multihead_ct.py:149-153,198), where a norm launch of its own would read
 * back the tensor the GEMM has just written:
 *   y_i[b] = relu?( bn_i( (W x[b])[rows of item i] ) ) [+ residual_i[b]],   i = 0 .. n-1,  1 <= n <= 8
 * The items cover the output rows [0, Co) in order (sum of C = Co; an item's rows may begin at any row) and follow the
 * ct_bn_fwd_item contract ct_bn_eval_group_fwd reads: weight, bias, running_mean, running_var f32[C] (all required, read-only),
 * eps >= 0, relu, y with y_batch_stride, residual (nullable) with residual_batch_stride (0 = contiguous, else >= C*N); x of an
 * item is ignored and should be NULL, its amax_out must be NULL.  y and residual must be 16-byte addressable (aligned bases,
 * strides % 4 == 0; N % 4 == 0 as for every ct_pw_gemm); y does not overlap x or a residual.  w, x, the operand maxima and
 * rows_a as ct_pw_gemm_rs (the activation keeps one scale); the workspace arguments are unused.
 * Bit equality: every stored value goes through the operation sequence of ct_pw_gemm_rs's epilogue and then
 * ct_bn_eval_group_fwd's ( v = acc * 2^-ea * 2^-eb;  ((v - mean) * (1 / sqrt(var + eps))) * weight + bias;  max(., 0);
 * + residual ), so each y_i holds exactly the bits of ct_pw_gemm_rs into a scratch tensor followed by ct_bn_eval_group_fwd
 * with the same items.
 * amax_out f32[ct_pw_gemm_norm_amax_len(B, Co, N)] (nullable): one partial maximum per workgroup, max |y| over its output tile
 * as stored (after ReLU and skip) — partials of ONE maximum in the sense of ct_amax_f32 (rows_* = 0 for the GEMM that reads
 * the outputs next), written without atomics, nothing to zero.  ct_pw_gemm_norm_amax_len returns 0 when there would be more
 * partials than a GEMM folds (32768): pass NULL then.
 * CT_EINVAL: n outside 1..8, sum of C != Co, a missing y / weight / bias / running statistic, a negative eps, a per-item
 * amax_out, a refused or misaligned stride or pointer, amax_out where the length is 0, and whatever ct_pw_gemm_rs refuses.
 * Added under CT_ABI_VERSION 3 (additive: the loader's missing-symbol scan checks it). */
int ct_pw_gemm_norm_amax_len(int B, int Co, int N);
int ct_pw_gemm_rs_norm(const float* w, const float* x, const ct_bn_fwd_item* items, int n, float* amax_out, const float* amax_a,
                       int n_amax_a, int rows_a, const float* amax_b, int n_amax_b, void* workspace, size_t workspace_bytes, int B,
                       int Co, int Ci, int N, ct_stream_t s);
/* Precision mode of the pointwise GEMMs.  Process-wide host state, atomic, never read by a kernel, as the deterministic switch:
 * every ct_pw_gemm* entry point (ct_pw_gemm, _rs, _rs_add, _rs_norm) reads the effective value ONCE, where it plans its
 * launch.  Added under CT_ABI_VERSION 3 (additive: the loader's missing-symbol scan checks them).
 *   CT_PW_PRECISION_HIGHEST (the default): everything above, bit for bit.
 *   CT_PW_PRECISION_HIGH: ONE f16 term per operand — h = f16(s x) under the same per-tensor / per-row power-of-two scale
 *     (s M in [2^13, 2^14)), one convert per element, no l term formed or staged, one v_mfma_f32_32x32x16_f16 per product,
 *     fp32 accumulation, the exact 1/(s_a s_b) in the epilogue.  An 11-bit significand: the precision of TF32, for which gfx950
 *     has no matrix instruction.  All four modes (CT_PW_WGRAD keeps its slabs and their fixed-order sum: still run-to-run
 *     bit-equal), the addend and the norm epilogues; within the mode ct_pw_gemm_rs_add and ct_pw_gemm_rs_norm keep their bit
 *     equalities with ct_pw_gemm_rs.  Zeros, NaN and inf propagate as in the default mode.
 *     Error bound.  For an element x with scale maximum M:  |f16(s x)/s - x| <= 2^-11 |x| + 2^-38 M  (the rounding of a normal
 *     f16; a subnormal's 2^-25 over s >= 2^13 / M).  f16 x f16 products are exact in fp32, so with da, db these element errors
 *     one product is off by a db + b da + da db: (2^-10 + 2^-22) |a b| from the normal parts; 2^-38 (M_a |b| + M_b |a|) from
 *     the subnormal parts against the other operand's value, 2^-11 of that again against its normal error, and subnormal
 *     against subnormal at most 2^-38 M_a |b| once more (an element that is not flushed has |b| >= 2^-25 / s_b, a flushed one
 *     has |db| = |b|).  With eps_acc the fp32-accumulation allowance of the default mode (2^-21 above covers it there):
 *       |err_ij| <= (2^-10 + 2^-22 + eps_acc) * sum_k |a_ik b_kj|  +  2^-37 * ( M_a * sum_k |b_kj|  +  M_b * sum_k |a_ik| )
 *     M_a, M_b as in ct_pw_gemm_rs: the ROW's own maxima wherever per-row scales apply.
 *   The mode is a permission, not an order: a product the one-term kernel does not take, or does not win on, keeps three terms.
 *   Workspace sizes do not depend on it.  Other values of p select CT_PW_PRECISION_HIGHEST.
 * ct_pw_precision_override(p): p = 0 / 1 sets the mode for the entry points the CALLING THREAD invokes, whatever the
 * process-wide value says, p < 0 ends the override — how a backward runs its products in its forward's precision on
 * whichever thread it is called.  ct_get_pw_precision() returns the value in effect for the calling thread.
 * HIP graphs: the mode is read when a launch is recorded; a replay runs the captured kernels. */
#define CT_PW_PRECISION_HIGHEST 0   /* three terms, 22-bit operands: the default, as before */
#define CT_PW_PRECISION_HIGH    1   /* one f16 term per operand: 11-bit significands (TF32-class), fp32 accumulation */
void ct_set_pw_precision(int p);     /* process-wide, atomic; other values -> HIGHEST */
int  ct_get_pw_precision(void);      /* the effective value for the calling thread */
void ct_pw_precision_override(int p);/* this thread's entry points only; -1: none */
/* Slice forward with the eval-mode BatchNorm1d (+ ReLU) that follows it applied in the gather's store — the heads' `after`
 * pairs on the Slice output (layers/multihead_ct.py:67-68,107: `self.after(self.slice(...))` = slice -> BatchNorm1d -> ReLU, and
 * the union block's concatenation of the heads' results, :196), where a norm launch of its own would read back the tensor Slice
 * has just written:
 *   y[b, h*C + c, n] = relu?( bn( Slice(keys, grid)[b, h*C + c, n] ) )
 * keys, grid, pad, the sizes and W as ct_slice_fwd.  `norm` is ONE ct_bn_fwd_item with C == H*C; read of it: y with
 * y_batch_stride in floats (0 = dense, else >= H*C*N: the head writes its channel range of a wider [B, Ct, N] tensor, the row of
 * (cloud b, channel c) at y + b*y_batch_stride + c*N), weight, bias, running_mean, running_var f32[H*C] (all required,
 * read-only), eps >= 0 and relu; x is ignored; residual and the item's own amax_out must be NULL.
 * Bit equality: the value ct_slice_fwd would have stored (after the pad multiply) goes through ct_bn_eval_group_fwd's operation
 * sequence ( ((v - mean) * (1 / sqrt(var + eps))) * weight + bias; max(., 0) ), so y holds exactly the bits of ct_slice_fwd into
 * a dense scratch tensor followed by ct_bn_eval_group_fwd with the same item.
 * Dispatch: the kernel family ct_slice_fwd takes for the shape, the switches and the debug flags, with y and its stride in the
 * alignment tests where `out` stands; ct_debug_last_launch names it as the family's tag followed by "+norm".
 * amax_out f32[ct_slice_fwd_norm_amax_len(B, H, C, N, dim, W)] (nullable): one partial maximum per workgroup, max |y| over what
 * it stored — partials of ONE maximum in the sense of ct_amax_f32, as ct_pw_gemm_rs_norm leaves them: plain stores, nothing to
 * zero, every slot written by the launch.  The length is that of the launch planned for 16-byte aligned tensors and strides
 * under the current switches and debug flags (query and launch share the plan); 0 where there would be more partials than a GEMM
 * folds (32768) or the shape is refused: pass NULL then.
 * CT_EINVAL, before anything is launched: a null required pointer, norm->C != H*C, eps < 0 or NaN, a stride below H*C*N, a
 * residual or per-item amax_out, amax_out where the length is 0 or keys, grid, y or the stride are not 16-byte aligned, a grid
 * whose single-channel tile exceeds a CU's LDS with more than 4096 channels per head, and whatever ct_slice_fwd refuses.
 * Added under CT_ABI_VERSION 3 (additive: the loader's missing-symbol scan checks it). */
int ct_slice_fwd_norm_amax_len(int B, int H, int C, int N, int dim, const int* W);
int ct_slice_fwd_norm(const float* keys, const float* grid, const void* pad, int pad_dtype, const ct_bn_fwd_item* norm,
                      float* amax_out, int B, int H, int C, int N, int dim, const int* W, ct_stream_t s);
/* The same for the plane-resident core (layers/multihead_ct.py:99-107 with the `after` pair of :67-68 in its Slice write-out):
 * ct_mhct_core_fwd's arguments with `out` replaced by (norm, amax_out), the item read as above (y_batch_stride % 4 == 0: the
 * rows move as float4), C the features per head.  Every output element holds exactly the bits of ct_mhct_core_fwd into a dense
 * scratch tensor followed by ct_bn_eval_group_fwd with the same item; z_save, y_save, occ_count and the workspace (clusters,
 * status word, ct_debug_set_core) behave as ct_mhct_core_fwd's.  A cluster that gives up waiting still writes NaN where its
 * results would have gone — un-normed: a ReLU would turn the marker into 0 — and NaN into its partial maximum.
 * amax_out f32[ct_mhct_core_fwd_norm_amax_len(...)] (nullable): one partial maximum per workgroup (planes x cluster size under
 * the current ct_debug_set_core flags), as above; 0 beyond 32768 partials or where ct_mhct_core_supported is 0.
 * CT_EINVAL as above (every pointer must be 16-byte aligned here, as for ct_mhct_core_fwd) and whatever ct_mhct_core_fwd
 * refuses; CT_EWORKSPACE as ct_mhct_core_fwd.  Added under CT_ABI_VERSION 3 (additive). */
int ct_mhct_core_fwd_norm_amax_len(int B, int H, int C, int N, int dim, const int* W);
int ct_mhct_core_fwd_norm(const float* keys, const float* feat, const void* pad, int pad_dtype, const float* conv_w,
                          const float* conv_b, const ct_bn_fwd_item* norm, float* amax_out, float* z_save, float* y_save,
                          int64_t* occ_count, void* workspace, size_t workspace_bytes, int B, int H, int C, int N, int dim,
                          const int* W, ct_stream_t s);

/* ------------------------------------------------------------------------
 * Neighbour search of the S3DIS KPConv protocol over a uniform grid (replaces the CPU
 * sklearn.neighbors.KDTree of datasets/s3dis_closer.py:204 `KDTree(sub_points)`,
 * :262-265,319-322 `query_radius(pick_point, r, sort_results=True)` cut to num_points,
 * :290 `query(points)`).  Added under CT_ABI_VERSION 2 (additive: the loader's
 * missing-symbol scan refuses a library built before them).
 *
 * Grid: origin f32[3] and dims int[3] (host arrays), cell edge h > 0, at most 2^26 cells;
 * cell of p = floor((p - origin) / h) per axis, clamped to the grid (points outside the
 * box land in an edge cell and are still found exactly), cell id (iz*ny + iy)*nx + ix,
 * so one x-row of cells is one contiguous range of the order.
 * Squared distances are ((dx*dx) + (dy*dy)) + (dz*dz), d = p - c, in fp32 without
 * contraction: numpy float32 computes the same bits.
 *
 * ct_nbr_index_build: points f32[M,3] (1 <= M < 2^31) -> cell_start i32[ncells+1] (points of
 * cell c are order[cell_start[c] .. cell_start[c+1])), order i32[M] (a counting sort of the
 * point ids by cell; the order inside a cell follows atomics), sorted f32[M,4] (x, y, z and
 * the point id's bits, in that order: what the queries read; 16-byte aligned, CT_EINVAL
 * otherwise, in the build and in both queries).  Workspace:
 * ct_nbr_index_workspace_bytes (0 = bad arguments).
 * ct_nbr_radius: for each of Q centres f32[Q,3], count i64[Q] = #points with d2 <= r*r (not
 * truncated); idx i64[Q,K] / d2 f32[Q,K] = the first min(count, K) of them by (d2, index)
 * ascending, then -1 / +inf.  K <= 16384, r >= 0.  One workgroup per centre.
 * ct_nbr_nearest: for each of Q queries f32[Q,3] (any position; 1 <= Q < 2^31 per call, one
 * launch: larger sets go in several calls), the nearest point's index i64[Q] (lowest index on
 * ties) and d2 f32[Q]; no workspace.
 * ---------------------------------------------------------------------- */
size_t ct_nbr_index_workspace_bytes(int64_t M, const int* dims);
int ct_nbr_index_build(const float* points, int64_t M, const float* origin, float h, const int* dims,
                       int32_t* cell_start, int32_t* order, float* sorted, void* workspace, size_t workspace_bytes,
                       ct_stream_t s);
int ct_nbr_radius(const int32_t* cell_start, const float* sorted, const float* origin, float h, const int* dims,
                  const float* centres, int Q, float r, int K, int64_t* idx, float* d2, int64_t* count, ct_stream_t s);
int ct_nbr_nearest(const int32_t* cell_start, const float* sorted, const float* origin, float h, const int* dims,
                   const float* queries, int64_t Q, int64_t* idx, float* d2, ct_stream_t s);

/* ------------------------------------------------------------------------
 * The index table: the grids of several clouds in device memory, so that a query can take its
 * cloud from a device tensor.  Added under CT_ABI_VERSION 3 (additive, as ct_nbr_*).
 *
 * One record per cloud; the record layout is private to the library.  ct_nbr_table_bytes: the
 * size of a table of n_clouds records (0 = n_clouds < 1).  ct_nbr_table_set writes record i
 * (0 <= i < n_clouds) into a HOST buffer of that size (8-byte aligned) from the cloud's index
 * (cell_start, sorted, origin, h, dims as ct_nbr_radius takes them, with the same checks: the
 * grid's bounds, sorted 16-byte aligned), its point count M (1 <= M < 2^31) and offset >= 0, the
 * cloud's first row in the concatenated sub-clouds; CT_EINVAL otherwise.  The caller uploads the
 * filled buffer once (8-byte aligned on the device) and keeps the indices alive.
 * ct_nbr_radius_multi: ct_nbr_radius with the grid of centre q taken from record cloud[q]
 * (cloud i64[Q], device; clamped into [0, n_clouds - 1] as a guard): the same workgroup, the
 * same (d2, index) order, the same outputs idx i64[Q,K], d2 f32[Q,K], count i64[Q].
 * ---------------------------------------------------------------------- */
size_t ct_nbr_table_bytes(int n_clouds);
int ct_nbr_table_set(void* host_table, int n_clouds, int i, const int32_t* cell_start, const float* sorted, const float* origin,
                     float h, const int* dims, int64_t M, int64_t offset);
int ct_nbr_radius_multi(const void* table, int n_clouds, const int64_t* cloud, const float* centres, int Q, float r, int K,
                        int64_t* idx, float* d2, int64_t* count, ct_stream_t s);

/* ------------------------------------------------------------------------
 * The exact k-nearest query (KDTree.query(X, k), 1 <= k <= CT_NBR_KNN_K_MAX) over the same index,
 * and inverse-distance interpolation over its result.  Added under CT_ABI_VERSION 3 (additive, as
 * ct_nbr_table_*).
 *
 * ct_nbr_knn: for each of Q queries f32[Q,3], idx i64[Q,K] / d2 f32[Q,K] = the K nearest points
 * by (d2, index) ascending: d2 ascends, and among equal d2 the lower index goes first (the order
 * of ct_nbr_radius, the tie rule of ct_nbr_nearest).  A cloud of fewer than K points fills the tail
 * with -1 / +inf.  Queries may lie anywhere, the outside of the grid's box included; the result is
 * exact, and for every query with finite coordinates K = 1 gives ct_nbr_nearest's idx and d2 bit
 * for bit (at a +-inf coordinate ct_nbr_nearest keeps the lowest index it visits, with d2 = +inf).
 * One wavefront per query: the
 * shells of cells of ct_nbr_nearest, each run of cells read 64 records at a time, the K best kept
 * in the wave's registers; the walk stops once the K-th d2 is below the squared gap to the nearest
 * unvisited cell (less ct_nbr_nearest's slack) or no unvisited cell remains, so it is bounded by
 * the grid's dimensions for every input.  A query with a non-finite coordinate ends through the
 * second condition and gets -1 / +inf in every slot.  One launch per call, 1 <= Q < 2^31 (larger
 * sets go in several calls), no workspace, no allocation.
 * ct_nbr_knn_multi: ct_nbr_knn with the grid of query q taken from record cloud[q] of a
 * ct_nbr_table_* table (cloud i64[Q], device; clamped into [0, n_clouds - 1] as a guard), as
 * ct_nbr_radius_multi relates to ct_nbr_radius.  idx counts inside the query's own cloud.
 * ct_nbr_interp: from such a table idx i64[Q,K] / d2 f32[Q,K] and values f32[M,C], out f32[Q,C] in
 * fp32 with true divisions and no contraction, in this order (numpy float32 gives the same bits):
 *   w_j = 1.0f / (d2_j + eps) for the slots with idx_j >= 0 (the others are skipped throughout);
 *   s = ((w_0 + w_1) + ...) in slot order;
 *   out[c] = ((w_0 / s) * values[idx_0][c] + (w_1 / s) * values[idx_1][c]) + ... in slot order.
 * values[idx] (Q * K * C elements) is never formed.  A row without a slot to use is NaN.  An idx
 * value at or above M is the caller's error: there is no device check.
 *
 * CT_EINVAL before any launch: a null pointer, K outside [1, 64], Q < 1 or Q >= 2^31, a grid
 * outside the bounds of ct_nbr_index_build, `sorted` not 16-byte aligned, a table not 8-byte
 * aligned or n_clouds < 1; for ct_nbr_interp C < 1, M < 1, or eps negative or NaN.
 * ---------------------------------------------------------------------- */
#define CT_NBR_KNN_K_MAX 64
int ct_nbr_knn(const int32_t* cell_start, const float* sorted, const float* origin, float h, const int* dims,
               const float* queries, int64_t Q, int K, int64_t* idx, float* d2, ct_stream_t s);
int ct_nbr_knn_multi(const void* table, int n_clouds, const int64_t* cloud, const float* queries, int64_t Q, int K,
                     int64_t* idx, float* d2, ct_stream_t s);
int ct_nbr_interp(const int64_t* idx, const float* d2, int64_t Q, int K, const float* values, int64_t M, int C,
                  float eps, float* out, ct_stream_t s);

/* ------------------------------------------------------------------------
 * The epoch plan of the S3DIS KPConv sampler (datasets/s3dis_closer.py:247-276): n picks by the
 * potential field, enqueued by one call; the host reads nothing back.  Added under CT_ABI_VERSION 3
 * (additive, as ct_nbr_table_*).
 *
 * Inputs (device): table (ct_nbr_table_*, n_clouds records, 1 <= n_clouds <= 65535), points
 * f32[total,3] (the concatenated sub-clouds the records' offsets index), noise f32[n,3] (already
 * scaled).  Updated: potentials f32[total] (cloud c's are potentials[offset_c .. offset_c + M_c)),
 * min_potentials f32[n_clouds].  Outputs: cloud i64[n], point i64[n], picks f32[n,3].  Host values:
 * r >= 0 (a double: the query gets (float)r), 1 <= K <= 16384, n >= 1, max_points = the largest
 * M_c (it sizes the reduction's grid and the workspace only: the kernels take every M_c from the
 * table).  All arithmetic is fp32, one rounding per operation, no contraction.
 *
 * On entry, for every cloud c: min_potentials[c] = min(potentials of c) and arg_c = the lowest
 * index holding it, recomputed from the buffers (nothing is cached between calls).  Then for
 * i = 0 .. n-1, in order:
 *   cloud[i] = the lowest c among the minima of min_potentials; point[i] = arg_c of that cloud;
 *   picks[i] = points[offset_c + point[i]] + noise[i], one add per component;
 *   (idx, d2, count) = ct_nbr_radius_multi at picks[i] in cloud[i] with (float)r and K;
 *   for each of the first min(count, K) entries: t = 1 - d2 * inv, pot[idx] = pot[idx] + t*t, with
 *     inv = 1.0f / (float)(r*r), r*r formed in double (torch: tensor / Python number);
 *   min_potentials[c] = min(potentials of c), arg_c = its lowest index.
 * Potentials must not be NaN (a NaN never wins a minimum).  cloud ids and point indices are clamped
 * into range as a guard; valid inputs never need it.
 *
 * Launches: one begin kernel, then per pick one query workgroup and one multi-workgroup reduction
 * whose last-arriving workgroup writes the next pick; kernel boundaries order the picks.
 * Workspace: ct_kp_plan_workspace_bytes (0 = bad arguments), 8-byte aligned, contents irrelevant
 * on entry; too small or null -> CT_EWORKSPACE.
 * ---------------------------------------------------------------------- */
size_t ct_kp_plan_workspace_bytes(int n_clouds, int64_t max_points);
int ct_kp_plan(const void* table, int n_clouds, int64_t max_points, const float* points, float* potentials,
               float* min_potentials, const float* noise, double r, int K, int n, int64_t* cloud, int64_t* point, float* picks,
               void* workspace, size_t workspace_bytes, ct_stream_t s);

/* ------------------------------------------------------------------------
 * Batch assembly of the S3DIS KPConv items (datasets/s3dis_closer.py:319-361) with the optional
 * rotation / scale / jitter of its training transforms (datasets/s3dis_closer_utils.py:38-93), one
 * launch.  Added under CT_ABI_VERSION 2 (additive, as ct_nbr_*).
 *
 * B items (1 <= B <= 65535), N slots (1 <= N <= 16384, the K of ct_nbr_radius), nvalid_b =
 * min(count_b, N).  Inputs (device): qidx i64[B,N] / count i64[B] (ct_nbr_radius of the pick
 * points), perm i64[B,N] (the argsort of the slot keys), u_pad f32[B,N] (padding draws), offset
 * i64[B] (the item's cloud in the concatenated sub-clouds), pick f32[B,3], drop f32[B] (0 or 1),
 * points f32[M,3], colors f32[M,3] (0..1), labels i64[M]; color_mean / color_std: host f32[3].
 * Optional augmentation, all three or none (CT_EINVAL otherwise): R f32[B,3,3], s f32[B,3],
 * j f32[B,N,3].  Per slot n: pad = clamp((int64)floorf(u_pad * (float)nvalid), 0, N-1),
 * src = n < nvalid ? perm[n] : perm[pad], ind = max(qidx[src], 0), g = offset + ind;
 * p = points[g] - pick; with augmentation p'_i = (((R_i0*p_x + R_i1*p_y) + R_i2*p_z) * s_i) + j_i;
 * colour = ((colors[g] - mean) / std) * drop.  Outputs: out_points p' f32[B,N,3], mask i32
 * (n < nvalid), features f32[B,F,N] (F in {1,3,4,5,6,7}: the layout of get_scene_seg_features,
 * height = the un-augmented points[g].z, F = 6/7 take p'), out_labels labels[g] i64, input_inds
 * ind i64.  src and g are clamped into range as a guard; valid inputs never need it.
 * ---------------------------------------------------------------------- */
int ct_kp_items(const int64_t* qidx, const int64_t* count, const int64_t* perm, const float* u_pad, const int64_t* offset,
                const float* pick, const float* drop, const float* points, const float* colors, const int64_t* labels,
                int64_t M, const float* color_mean, const float* color_std, const float* R, const float* s, const float* j,
                int B, int N, int F, float* out_points, int32_t* mask, float* features, int64_t* out_labels,
                int64_t* input_inds, ct_stream_t st);

/* ------------------------------------------------------------------------
 * Batch assembly of the ShapeNet completion items (utils/pcd_utils.py:24-51, partial_postproces,
 * fed `scale * partial` as train_inpainter.py:180 feeds it 2 * partial), one launch, every random
 * draw passed in.  Added under CT_ABI_VERSION 2 (additive, as ct_nbr_* and ct_kp_items).
 *
 * B clouds (1 <= B <= 65535) of n_in rows (1 <= n_in <= 16384), gt columns (n_in <= gt <= 2^24).
 * Inputs (device): partial f32[B,n_in,3] (zero rows are padding), perm i64[B,n_in] (a permutation of
 * 0..n_in-1 per cloud: the argsort of plain random keys), u_dup f32[B,n_in] in [0,1), sphere
 * f32[B,3,gt] (candidate noise points); scale: host float, finite and non-zero.
 * With q_i = scale * partial[b,i] (one fp32 multiply): row i is valid unless q_i.x == 0 && q_i.y == 0
 * && q_i.z == 0 (IEEE ==: -0 is zero, a NaN row is valid); v = count[b] = the number of valid rows;
 * c[0..v) = the valid q_i in ascending i.  Outputs: part f32[B,n_in,3]: for j < v the j-th valid row
 * met walking perm[b,0], perm[b,1], ...; for j >= v, c[k] with k = clamp((int)floorf(u_dup[b,j] *
 * (float)v), 0, v-1).  noise f32[B,4,gt]: columns m < gt-v are sphere[b,:,m] with label 0, columns
 * m >= gt-v are c[m-(gt-v)] with label 1.  count i32[B].
 * v == 0 (the reference raises there: randint with high <= 0): part[b] is all zeros, noise[b] is all
 * sphere columns with label 0 and count[b] = 0; callers can look at count.  perm entries outside
 * 0..n_in-1 are clamped into range as a guard; when perm is not a permutation, rows of part below v
 * may be left unwritten, nothing is written out of bounds.
 * Null pointers, sizes outside the limits and a zero or non-finite scale -> CT_EINVAL before anything
 * touches the device.
 * ---------------------------------------------------------------------- */
int ct_completion_items(const float* partial, const int64_t* perm, const float* u_dup, const float* sphere, float scale,
                        int B, int n_in, int64_t gt, float* part, float* noise, int32_t* count, ct_stream_t s);

/* ------------------------------------------------------------------------
 * The ShapeNet completion items themselves, gathered from a split that stays on the device
 * (datasets/grnet_completion.py:371-397 Dataset.__getitem__, :107-135 Compose with :246-258
 * RandomSamplePoints and :297-314 RandomMirrorPoints, :351-368 collate_fn), one launch, every random
 * draw passed in.  Added under CT_ABI_VERSION 3 (additive, as ct_image_items).  It does not
 * allocate, does not synchronise and runs on the stream s.  ct_completion_items takes its
 * out_partial as it is.
 *
 * The split (device): partial_points f32[Pt,3] and partial_offsets i64[M*R+1] (cloud m*R + r is
 * rendering r of model m, 0 .. p_cap points), gt_points f32[Gt,3] and gt_offsets i64[M+1] (0 ..
 * g_cap points); M >= 1 models, R >= 1 renderings of each, M * R below 2^63.
 * A batch is B rows (1 <= B <= 65535): item i64[B] names the model (repeats allowed), m =
 * clamp(item[b], 0, M-1); rendering i64[B] the rendering, r = clamp(rendering[b], 0, R-1) (the
 * clamps are guards).  The partial cloud of row b is m*R + r, its gt cloud is m.
 *
 * Partial sampling (RandomSamplePoints): perm_in i64[B,p_cap] is a permutation of 0..p_cap-1 per
 * row (the argsort of plain random keys).  With P the partial cloud's length (cut to p_cap): slot
 * j < min(n_in, P) of out_partial[b] takes the j-th entry of perm_in[b] that is below P, in order
 * (the order-preserving compaction of ct_image_items: a uniform permutation of p_cap restricted
 * this way is a uniform permutation of P, here cut to n_in); slots j >= P are rows of +0.
 * gt sampling: the same rule with perm_gt i64[B,g_cap], g_cap and n_out into out_gt[b]; with
 * perm_gt null the first min(n_out, G) rows of the cloud are copied in order, the rest are +0.
 * Entries of a perm outside 0..length-1 are never followed; when it is not a permutation, slots
 * below min(n, length) may be left unwritten, nothing is read or written out of bounds.
 * Mirror (RandomMirrorPoints): u = u_mirror[b] (f32[B]); sx = -1 iff u <= 0.5; sz = -1 iff
 * u <= 0.25 or 0.5 < u <= 0.75 (a NaN draw mirrors nothing); every gathered row of both clouds
 * becomes (sx * x, y, sz * z), a sign flip (so a zero coordinate may become -0).  u_mirror null:
 * no mirror.
 * Scale: out_gt = gt_scale * (mirrored row), one fp32 multiply (train_inpainter.py:178's 2 *);
 * out_partial is not scaled.  Outputs: out_partial f32[B,n_in,3], out_gt f32[B,n_out,3].
 * Limits: 1 <= n_in <= 16384, 1 <= n_out <= 65536, 1 <= p_cap, g_cap <= 65536, gt_scale finite
 * and non-zero.  Null required pointers and sizes outside the limits -> CT_EINVAL before anything
 * touches the device.
 * ---------------------------------------------------------------------- */
int ct_completion_gather(const float* partial_points, const int64_t* partial_offsets, const float* gt_points,
                         const int64_t* gt_offsets, int64_t M, int R, int p_cap, int g_cap, const int64_t* item,
                         const int64_t* rendering, const int64_t* perm_in, const int64_t* perm_gt /* nullable */,
                         const float* u_mirror /* nullable */, float gt_scale, int B, int n_in, int n_out, float* out_partial,
                         float* out_gt, ct_stream_t s);

/* ------------------------------------------------------------------------
 * Batch assembly of the ScanObjectNN classification items (datasets/scanobjectnn.py:102-122: jitter,
 * rotation about y, subsample; the collate and the permute of train_classification.py:195), one
 * launch, every random draw passed in.  Added under CT_ABI_VERSION 3 (additive, as ct_kp_items and
 * ct_completion_items).
 *
 * The split stays on the device: data f32[M,P,3] (centred and normalised on the host), mask u8[M,P]
 * (0 background, 1 object), label i64[M]; M >= 1.  A batch is B rows (1 <= B <= 65535) of N slots
 * (1 <= N <= P <= 16384): item i64[B] names the cloud of each row (repeats allowed); perm i64[B,P]
 * (nullable) is the argsort of plain random keys, whose first N entries are a draw of N points
 * without replacement (np.random.choice(P, N, replace=False)), NULL: slot n takes point n.
 * Augmentation, both or neither (CT_EINVAL otherwise): rot f32[B,2] = (cos, sin) of the cloud's
 * angle, jit f32[B,N,3] standard normal draws; sigma (finite) and clip (> 0): host floats.  The draws
 * are finite by construction; what the clip does to a NaN draw is not specified.
 * Per slot (b, n), each operation one fp32 rounding, in this order:
 *   g = clamp(item[b], 0, M-1); src = perm ? clamp(perm[b,n], 0, P-1) : n; p = data[g,src];
 *   without augmentation q = p is the output; with it d_i = min(max(sigma * jit[b,n,i], -clip), clip),
 *   q_i = p_i + d_i (jitter before rotation), then x' = (q.x * c) - (q.z * s), y' = q.y,
 *   z' = (q.x * s) + (q.z * c): q @ [[c,0,s],[0,1,0],[-s,0,c]].
 * Outputs: out_points f32[B,3,N] (the model's layout: [B,3,1,N] is a view of it), out_mask f32[B,N]
 * = mask[g,src], out_label i64[B] = label[g].  The clamps are guards; valid inputs never need them.
 * Null pointers (other than perm, rot, jit), half an augmentation and sizes outside the limits ->
 * CT_EINVAL before anything touches the device.
 * ---------------------------------------------------------------------- */
int ct_scan_items(const float* data, const uint8_t* mask, const int64_t* label, int64_t M, int P, const int64_t* item,
                  const int64_t* perm, const float* rot, const float* jit, float sigma, float clip, int B, int N,
                  float* out_points, float* out_mask, int64_t* out_label, ct_stream_t s);

/* ------------------------------------------------------------------------
 * Batch assembly of the S3DIS 1x1 m block items (datasets/s3dis_v2.py:537-560: shuffle, rotation
 * about z, anisotropic scale, mirror in x, jitter, auto-contrast, colour translation, colour jitter,
 * hue / saturation translation; the collate and the permute of train_segmentation.py:180), one
 * launch, every random draw passed in.  Added under CT_ABI_VERSION 3 (additive, as ct_scan_items).
 * It does not allocate, does not synchronise and runs on the stream s.
 *
 * The split stays on the device: data f32[M,P,6] (x, y, z, r, g, b: columns 0..5 of the stored
 * [M,4096,9] blocks, colours in [0,1]), label u8[M,P]; M >= 1.  A batch is B rows (1 <= B <= 65535)
 * of N slots (1 <= N <= P <= 16384); the pool of a row is its block's first N points
 * (s3dis_v2.py:537).  item i64[B] names the block of each row (repeats allowed); perm i64[B,N]
 * (nullable) is a permutation of 0..N-1 per row, NULL: slot n takes point n.
 * Augmentation, all three or none (CT_EINVAL otherwise): aug f32[B,16], jit f32[B,N,3] and cjit
 * f32[B,N,3] (standard normal draws); sigma, cstd (finite) and clip (> 0): host floats.
 *   aug[b,0], aug[b,1]   c, s: cos and sin of the angle about z
 *   aug[b,2..4]          per-axis scale; the x entry carries the mirror's sign
 *   aug[b,5]             w, the auto-contrast's blend factor; negative: the stage is skipped
 *   aug[b,6..8]          colour shift, already (u - 0.5) * 2 * ratio
 *   aug[b,9]             colour translation applied (0 or 1)
 *   aug[b,10]            colour jitter applied (0 or 1)
 *   aug[b,11]            hue shift
 *   aug[b,12]            saturation factor
 *   aug[b,13..15]        zero
 * Per slot (b, n), each operation one fp32 rounding, in this order:
 *   g = clamp(item[b], 0, M-1); src = perm ? clamp(perm[b,n], 0, N-1) : n; (x, y, z, rgb) = data[g,src].
 *   Without augmentation that row is the output.  With it:
 *   1. x' = (x * c) - (y * s), y' = (x * s) + (y * c);
 *   2. p_i = p_i * aug[b,2+i];
 *   3. p_i = p_i + min(max(sigma * jit[b,n,i], -clip), clip);
 *   4. when w >= 0, per channel: lo, hi = min, max of the channel over data[g,0..N-1] (exact; -0 sorts
 *      below +0); when hi != lo: st = (rgb - lo) * (1 / (hi - lo)), rgb = ((1 - w) * rgb) + (w * st).
 *      A channel with hi == lo is left as it is — a deviation: the reference divides by zero there and
 *      fills the channel with NaN;
 *   5. when aug[b,9] != 0: rgb = min(max(aug[b,6+i] + rgb, 0), 1);
 *   6. when aug[b,10] != 0: rgb = min(max((cjit[b,n,i] * cstd) + rgb, 0), 1);
 *   7. (r, g, b) = rgb * 255; mx, mn = max, min of the three; span = mx - mn; grey = span == 0;
 *      rc = (mx - r) / span (gc, bc alike); h = r == mx ? bc - gc : g == mx ? (2 + rc) - bc :
 *      (4 + gc) - rc, 0 when grey; sat = span / (mx == 0 ? 1 : mx), 0 when grey; h = rem1(h / 6) with
 *      rem1(t) = np.remainder(t, 1) = t - trunc(t), + 1 when that is negative;
 *      h = rem1((aug[b,11] + h) + 1); sat = min(max(aug[b,12] * sat, 0), 1);
 *      h6 = h * 6; sector = trunc(h6); f = h6 - sector; p = mx * (1 - sat), q = mx * (1 - (sat * f)),
 *      t = mx * (1 - (sat * (1 - f))); sector mod 6 picks (mx,t,p) (q,mx,p) (p,mx,t) (p,q,mx) (t,p,mx)
 *      (mx,p,q); sat == 0: (mx,mx,mx);
 *   8. rgb = trunc(min(max(value, 0), 255)) / 255 (the reference's 8-bit levels; the clamp is a guard).
 * The draws are finite by construction; what the stages do to a NaN or infinite value is not specified.
 * Outputs: out f32[B,6,N] (the model's layout: [B,6,1,N] is a view of it), out_label i64[B,N] =
 * label[g,src].  The clamps of g and src are guards; valid inputs never need them.
 * Null pointers (other than perm, aug, jit, cjit), a partial augmentation, clip <= 0 and sizes outside
 * the limits -> CT_EINVAL before anything touches the device.
 * ---------------------------------------------------------------------- */
int ct_block_items(const float* data, const uint8_t* label, int64_t M, int P, const int64_t* item, const int64_t* perm,
                   const float* aug, const float* jit, const float* cjit, float sigma, float clip, float cstd, int B, int N,
                   float* out, int64_t* out_label, ct_stream_t s);

/* ------------------------------------------------------------------------
 * The confusion matrix of a segmentation batch (train_segmentation.py:198-205 without the copy of
 * the predictions to the host), one launch, one pass over pred.  Added under CT_ABI_VERSION 3
 * (additive).
 * pred f32[B,C,N] (1 <= C <= 64, B * N < 2^31), labels i64[B,N]; conf i64[C*C], rows truth, columns
 * prediction: conf[t*C + p] += the number of points with label t and prediction p.  It ADDS: the
 * caller zeroes conf.  The prediction of a point is the first index of the maximum over C, a NaN
 * counting as the maximum (np.argmax).  Points whose label is outside 0..C-1 are not counted.
 * Integer counts only: the result does not depend on the order of the workgroups.
 * ---------------------------------------------------------------------- */
int ct_seg_confusion(const float* pred, const int64_t* labels, int B, int C, int N, int64_t* conf, ct_stream_t s);

/* ------------------------------------------------------------------------
 * Batch assembly of the What3D single-view reconstruction items (datasets/image_point.py:128-150:
 * Resize, ToTensor, Normalize of the rendering, resample_pcd of the cloud; the collate), one launch,
 * every random draw passed in.  Added under CT_ABI_VERSION 3 (additive, as ct_scan_items).
 * It does not allocate, does not synchronise and runs on the stream s.
 *
 * The split stays on the device: images u8[M,H,W,3] (RGB, interleaved; the pointer 4-byte aligned),
 * points f32[T,3] (all clouds concatenated), offsets i64[M+1] (cloud g is points[offsets[g] ..
 * offsets[g+1]), 1 .. p_cap points), class_id i64[M]; M >= 1.  A batch is B rows (1 <= B <= 65535);
 * item i64[B] names the object of each row (repeats allowed), g = clamp(item[b], 0, M-1).
 *
 * Image: out_img f32[B,3,OH,OW] is Pillow's 8-bit resize((OW, OH), BILINEAR) of images[g], then
 * ToTensor and Normalize.  The resample is Pillow's integer arithmetic, horizontal pass first into
 * 8-bit intermediates, the vertical pass on those; its coefficients come in as four tables built
 * once per (H, W, OH, OW) in float64 (data/image_point.py resize_tables):
 *   kx i32[OW,ksx], bx i32[OW,2] = (xmin, taps); ky i32[OH,ksy], by i32[OH,2] = (ymin, taps);
 *   per axis with scale = in / out, fs = max(scale, 1), support = fs: ks = 2 * ceil(support) + 1,
 *   center = (i + 0.5) * scale, min = max(int(center - support + 0.5), 0),
 *   taps = min(int(center + support + 0.5), in) - min, w[x] = max(0, 1 - |(x + min - center + 0.5) / fs|)
 *   divided by their sum when it is not zero, k[x] = int(0.5 + w[x] * 2^22) (entries past taps: 0).
 *   byte = clamp((2^21 + sum_x pixel[min + x] * k[x]) >> 22, 0, 255) in 32-bit integers.
 * Float stage, each operation one fp32 rounding, IEEE division:
 *   v = ((float)byte / 255.0f - mean[c]) / std[c]; mean, std: HOST arrays of three finite floats, std != 0.
 * Limits: 1 <= H, OH, OW <= 4096, 1 <= W <= 2048, 1 <= ksx, ksy <= 64 (CT_IMAGE_TAPS_MAX), and one
 * output row's source rows after the horizontal pass, min(H, ksy) * 3 * OW bytes, within the 36 KiB
 * of LDS the kernel stages them in.  The table entries are clamped to the image; the clamps are
 * guards, valid tables never need them.
 *
 * Points: out_pcd f32[B,3,n] (1 <= n <= 2^20) is resample_pcd(cloud g, n) transposed, on the draws
 * perm i64[B,p_cap] (the argsort of plain random keys; 1 <= p_cap <= 65536, p_cap >= every cloud's
 * length) and u_dup f32[B,n] in [0, 1).  With P the cloud's length: slot j < min(n, P) takes the
 * j-th entry of perm[b] that is below P, in order (an order-preserving compaction: a uniform
 * permutation of p_cap restricted this way is a uniform permutation of P); slot j >= P takes point
 * min((int)(u_dup[b,j] * (float)P), P - 1) (one fp32 multiply; a NaN draw gives point 0).
 * out_class i64[B] = class_id[g].
 * Null pointers, a misaligned images pointer, sizes outside the limits, more taps than
 * CT_IMAGE_TAPS_MAX and an output row that does not fit the LDS budget -> CT_EINVAL before anything
 * touches the device.
 * ---------------------------------------------------------------------- */
#define CT_IMAGE_TAPS_MAX 64
int ct_image_items(const uint8_t* images, int64_t M, int H, int W, int OH, int OW, const int32_t* kx, const int32_t* bx,
                   int ksx, const int32_t* ky, const int32_t* by, int ksy, const float* mean, const float* std,
                   const float* points, const int64_t* offsets, const int64_t* class_id, int p_cap, const int64_t* item,
                   const int64_t* perm, const float* u_dup, int B, int n, float* out_img, float* out_pcd, int64_t* out_class,
                   ct_stream_t s);

/* ------------------------------------------------------------------------
 * Barycentre voxel-grid subsampling of KPConv on the device
 * (cpp_wrappers/cpp_subsampling/grid_subsampling/grid_subsampling.cpp:4-104, called by
 * datasets/s3dis_closer.py:13-31): the twin of ct_grid_subsample (cloudct_host.h), with the same
 * rows in the same order with the same bits.  Added under CT_ABI_VERSION 3 (additive, as
 * ct_image_items).  Neither call allocates or synchronises; both run on the stream s.
 *
 * ct_voxel_bounds: points f32[N,3] (device, 1 <= N < 2^31) -> bounds f32[6] (device): the per-axis
 * minimum lo[3] then maximum hi[3]; a NaN anywhere makes all six NaN.  Two launches (partial bounds
 * of up to 1024 workgroups, then their fold).  Workspace: ct_voxel_bounds_workspace_bytes(N) (host
 * arithmetic; 0 = bad N), 4-byte aligned; null, misaligned or too small -> CT_EWORKSPACE.
 *
 * ct_voxel_keys: points as above, dl > 0 and finite, bounds f32[6] (device) as ct_voxel_bounds
 * writes them (any exact reduction will do; a NaN point must give a NaN bound).  All fp32, one rounding per operation, true divisions, no contraction:
 *   inv = 1 / dl (on the host); org[a] = floor(lo[a] * inv) * dl; n[a] = floor((hi[a] - org[a]) / dl) + 1;
 *   i[a] = floor((p[a] - org[a]) / dl); key = ix + nx * iy + nx * ny * iz in 64 bits.
 * Outputs (device): grid, 40 bytes, 8-byte aligned, read by the host in one copy:
 *   f32 origin[3]; i32 status (0, or 1: a bound is not finite); i64 nx, ny, nz (each cut to 2^62 + 1:
 *   the caller refuses nx * ny * nz >= 2^62, below which no key wraps);
 * keys i64[N] = key ^ 2^63: signed ascending order of these IS unsigned ascending order of the
 * keys, the order of the host file's size_t keys — also for a point one rounding below the
 * origin (floor(lo * inv) may round up), whose index -1 wraps there and here alike.
 *
 * ct_voxel_reduce: keys_sorted i64[N] and order i64[N], the STABLE ascending sort of keys and its
 * permutation; points as above, features f32[N,fdim] and classes i32[N,ldim] (null when the dim
 * is 0).  Each run of equal keys is one output row, rows in ascending key order:
 *   out_points f32[.,3] = sum * (float)(1.0 / (double)count), out_features f32[.,fdim] =
 *   sum / (float)count, each sum from 0.0f over the run's points IN INPUT ORDER (the loads may
 *   come in any order; the additions of one (row, column) do not), out_classes i32[.,ldim] = the
 *   per-column maximum; inverse i64[N] (nullable) = each input point's row; counts i64[.]
 *   (nullable) = points per row; M i64[1] (device, 8-byte aligned) = the number of rows.
 * The row arrays are sized for N rows; rows past M are not written.  order entries are clamped to
 * [0, N - 1] as a guard; a permutation never needs it.
 * Workspace: ct_voxel_reduce_workspace_bytes(N) (host arithmetic; 0 = bad N), 4-byte aligned,
 * contents irrelevant on entry; null or too small -> CT_EWORKSPACE.  Null pointers, N outside
 * [1, 2^31), negative dims, dl <= 0 -> CT_EINVAL before anything touches the device.
 * Launches: two scan kernels and a row kernel over N, then one wave per run (a fixed grid of
 * one-wave workgroups looping over rows; a run is never split, so the longest run bounds the time).
 * ---------------------------------------------------------------------- */
size_t ct_voxel_bounds_workspace_bytes(int64_t N);
int ct_voxel_bounds(const float* points, int64_t N, float* bounds, void* workspace, size_t workspace_bytes, ct_stream_t s);
int ct_voxel_keys(const float* points, int64_t N, float dl, const float* bounds, void* grid, int64_t* keys, ct_stream_t s);
size_t ct_voxel_reduce_workspace_bytes(int64_t N);
int ct_voxel_reduce(const int64_t* keys_sorted, const int64_t* order, const float* points, const float* features,
                    const int32_t* classes, int64_t N, int fdim, int ldim, float* out_points, float* out_features,
                    int32_t* out_classes, int64_t* inverse, int64_t* counts, int64_t* M, void* workspace, size_t workspace_bytes,
                    ct_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* CLOUDCT_H */
