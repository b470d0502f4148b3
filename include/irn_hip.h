/*
 * irn_hip.h — C ABI of libirn_hip.so: the MI355X (gfx950) implementation of IRN's pseudo-label
 * hot path (inter-pixel affinity random walk + label epilogues + instance front-end).
 *
 * The reference (jiwoon-ahn/irn) is pure Python and has no FFI layer of its own; the seam this
 * library sits behind is the reference's *operator tier* (SURVEY.md §8b):
 *   misc/indexing.py            PathIndex, edge_to_affinity, affinity_sparse2dense,
 *                               to_transition_matrix, propagate_to_edge
 *   step/make_sem_seg_labels.py lines 43-49   (x4 upsample, /max, bg plane, argmax, keys LUT)
 *   step/make_ins_seg_labels.py find_centroids_with_refinement, cluster_centroids,
 *                               separte_score_by_mask, lines 137-147
 * Each entry point below names the reference lines it replaces.  A reference-side binding is a
 * ctypes stub; irn_amd/_lib.py is the one this repo ships.
 *
 * Conventions
 *   - every function returns an int status (IRN_OK = 0); irn_last_error() gives the message of
 *     the calling thread's last failure.  Nothing throws across the boundary.
 *   - all `dev` pointers are caller-owned device memory (fp32 unless noted), contiguous,
 *     row-major.  The library never allocates or frees device memory the caller can see;
 *     scratch comes from the caller through a workspace pointer whose size the library reports.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all work is
 *     enqueued on it and nothing synchronises unless stated.
 *   - one host thread per context; contexts are independent (one process per GPU, no
 *     communication on the path — reference misc/torchutils.py:66-68 sharding).
 */
#ifndef IRN_HIP_H
#define IRN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IRN_OK 0
#define IRN_ERR_ARG 1          /* bad argument (null pointer, non-positive size, unsupported radius/beta) */
#define IRN_ERR_HIP 2          /* a HIP runtime call or kernel launch failed */
#define IRN_ERR_STATE 3        /* call order violated (e.g. run before configure / workspace too small) */

#define IRN_MAX_RADIUS 16

/* The version of this header's argument lists.  irn_version() returns the IRN_ABI_VERSION the library was built with, and
 * it moves whenever an entry's arguments change: a binding that finds another value has loaded a library of another commit
 * (irn_amd/_lib.py refuses to import it). */
#define IRN_ABI_VERSION 106
int irn_version(void);
const char *irn_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * PathIndex  (replaces misc/indexing.py:6-56, `PathIndex.get_search_paths_dst`)
 * order = 0: the reference's channel order (paths grouped by length, discovery order inside a
 *            group) — the order of edge_to_affinity's channel axis and of `search_dst`;
 * order = 1: raster (dy, dx) order — the plane order of the walk's internal weight table.
 * irn_path_count reports sizes; irn_path_table fills host arrays:
 *   dst_dydx   [n_dirs][2]   destination (dy,dx) of every direction
 *   path_start [n_dirs+1]    CSR offsets into cells_dydx
 *   cells_dydx [n_cells][2]  path cells, far-to-near (element 0 of a path is its destination)
 * ------------------------------------------------------------------------------------------- */
int irn_path_count(int radius, int *n_dirs, int *n_cells);
int irn_path_table(int radius, int order, int32_t *dst_dydx, int32_t *path_start, int32_t *cells_dydx);

/* ---------------------------------------------------------------------------------------------
 * edge_to_affinity  (replaces misc/indexing.py:91-109 and the identical gather in
 * net/resnet50_irn.py:162-175).  edge: dev [B, Hp, Wp]; aff: dev [B, n_dirs, (Hp-rf)*(Wp-2rf)],
 * rf = radius-1, channel order 0 (reference).  aff[b,d,s] = 1 - max over path(d) of edge.
 * No index tensors are built or uploaded (reference :58-88, :96-99).
 * ------------------------------------------------------------------------------------------- */
int irn_edge_to_affinity(const float *edge_dev, int batch, int hp, int wp, int radius,
                         float *aff_dev, void *stream);

/* Its vector-Jacobian product, for the training seam (net/resnet50_irn.py:162-175 under autograd: the
 * gradient of aff[b,d,s] goes, negated, to the first path cell that attains the maximum).
 * grad_aff: dev [B, n_dirs, (Hp-rf)*(Wp-2rf)] -> grad_edge: dev [B, Hp, Wp] (overwritten).  The arg-max
 * is recomputed from `edge`; nothing from the forward call is needed. */
int irn_edge_to_affinity_backward(const float *edge_dev, const float *grad_aff_dev, int batch, int hp, int wp,
                                  int radius, float *grad_edge_dev, void *stream);

/* Pair displacement of the training seam (AffinityDisplacementLoss.to_pair_displacement,
 * net/resnet50_irn.py:177-193).  disp: dev fp32 [batch, channels, hp, wp]; out: dev fp32
 * [batch, channels, |S|, (hp-rf)*(wp-2rf)], out[b,c,d,y,x] = disp[b,c,y,rf+x] - disp[b,c,y+dy_d,rf+x+dx_d]
 * with d in the reference's channel order (search_dst).  The backward writes the full gradient
 * [batch, channels, hp, wp] (no accumulation, no atomics). */
int irn_pair_displacement(const float *disp_dev, int batch, int channels, int hp, int wp, int radius, float *out_dev,
                          void *stream);
int irn_pair_displacement_backward(const float *grad_out_dev, int batch, int channels, int hp, int wp, int radius,
                                   float *grad_disp_dev, void *stream);

/* Fused affinity / displacement loss of IRNet training (replaces, for the training step, the chain
 * net/resnet50_irn.py:198-213 + step/train_irn.py:58-64 + voc12/dataloader.py:80-106 without writing any
 * [batch, |S|, N] tensor).  edge: dev fp32 [batch, hp, wp], already through the sigmoid; dp: dev fp32
 * [batch, 2, hp, wp]; label: dev uint8 [batch, hp, wp], 0 = background, 1..ignore_from-1 = a class, >= ignore_from = ignore
 * (a dataset of C foreground classes passes C + 1; the usual value is IRN_EVAL_CLASSES = 21).  Nothing else in the arithmetic
 * depends on it: the loss only asks which labels are equal, which are 0 and which are ignored.
 * Geometry as irn_edge_to_affinity / irn_pair_displacement: with rf = radius-1, source cell (y, rf+x), y < hp-rf,
 * x < wp-2rf, pairs with (y+dy_d, rf+x+dx_d).  With a, b the labels of the two cells: valid = a<ignore_from && b<ignore_from,
 * bg = valid && a==b==0, fg = valid && a==b>0, neg = valid && a!=b; aff = 1 - max of edge over path(d);
 * pd_c = dp_c[src] - dp_c[dst]:
 *   sums[0] = sum bg * -log(aff+1e-5)        sums[1] = sum fg * -log(aff+1e-5)     sums[2] = sum neg * -log(1+1e-5-aff)
 *   sums[3] = sum_c sum fg * |pd_c - (dy_d, dx_d)_c|                              sums[4] = sum_c sum bg * |pd_c|
 *   counts[0..2] = sum bg, sum fg, sum neg (exact)
 * sums (dev fp64 [5]) and counts (dev int64 [3]) are device memory.  Per-element arithmetic is fp32, accumulation
 * fp64 through per-workgroup partials in the workspace that a second kernel adds in a fixed order: no float atomics,
 * the forward is bit-reproducible.
 * The backward recomputes everything from the three maps.  coef: dev fp32 [5], the upstream gradients of the five
 * sums (read on the device, nothing synchronises).  With g_aff = -(c0*bg + c1*fg)/(aff+1e-5) + c2*neg/(1+1e-5-aff),
 * -g_aff goes to the first path cell that attains the maximum (the rule of irn_edge_to_affinity_backward), and
 * g_c = c3*fg*sgn(pd_c - dst_c) + c4*bg*sgn(pd_c), sgn(0) = 0, is added at the source cell and subtracted at the
 * destination.  grad_edge [batch, hp, wp] and grad_dp [batch, 2, hp, wp] are fully written (zero where nothing
 * lands).  The gradients are gathered with float atomics (LDS, then one global atomic per touched cell of a tile):
 * reproducible to rounding, NOT bit for bit.
 * irn_aff_loss_backward_ordered takes the same arguments and means the same, as a gather: a workgroup owns a tile of
 * output cells and every thread adds what reaches its cell in the path table's order (direction ascending, path cell
 * ascending; for grad_dp per direction the cell as source, then as destination).  No atomics of any kind: identical bits
 * for identical inputs, and an image's gradients do not depend on the images it is batched with.  Every cell of grad_edge
 * and grad_dp is written exactly once with a plain store, nothing is cleared first.  It differs from
 * irn_aff_loss_backward by the order of the additions only, and costs more (it re-walks a path for each of its cells).
 * ws: irn_aff_loss_workspace_bytes(batch, hp, wp, radius) bytes of device memory (0 = bad geometry); the backward
 * checks it like the forward and leaves it untouched.  Null pointers, batch outside [1, 65535], radius outside
 * [2, IRN_MAX_RADIUS] (the path table's range), hp <= rf or wp <= 2 rf, ignore_from outside 1..255 (labels are bytes and
 * 255 is always void) give IRN_ERR_ARG, a workspace that is too small IRN_ERR_STATE, all before any device is touched. */
size_t irn_aff_loss_workspace_bytes(int batch, int hp, int wp, int radius);
int irn_aff_loss_forward(const float *edge, const float *dp, const uint8_t *label, int batch, int hp, int wp, int radius,
                         int ignore_from, double *sums, int64_t *counts, void *ws, size_t ws_bytes, void *stream);
int irn_aff_loss_backward(const float *edge, const float *dp, const uint8_t *label, int batch, int hp, int wp, int radius,
                          int ignore_from, const float *coef, float *grad_edge, float *grad_dp, void *ws, size_t ws_bytes,
                          void *stream);
int irn_aff_loss_backward_ordered(const float *edge, const float *dp, const uint8_t *label, int batch, int hp, int wp,
                                  int radius, int ignore_from, const float *coef, float *grad_edge, float *grad_dp, void *ws,
                                  size_t ws_bytes, void *stream);

/* Fused bilinear upsampling + softmax cross-entropy of segmentation training (replaces F.interpolate(scale_factor = factor,
 * mode = 'bilinear', align_corners = False) followed by F.cross_entropy(ignore_index = 255) without writing any
 * [batch, C, H, W] tensor), and the arg-max of inference.
 *   logits dev fp32 [batch, C, h, w], contiguous; z[b, c, Y, X] = their bilinear interpolation at fine pixel (Y, X) of the
 *   H x W window at the top left of the full upsampling, 1 <= H <= h * factor, 1 <= W <= w * factor, with exactly the
 *   arithmetic of irn_upsample_bilinear (one piece of device code serves both).  factor 1..64, C 2..IRN_EVAL_MAX_CLASSES (81),
 *   h and w 1..32768.
 *   label dev uint8 [batch, H, W]: a byte >= C is ignored (255 = void, or a label of another class list).
 * irn_seg_loss_forward: per valid pixel l = logsumexp_c z - z[label] with the maximum subtracted (finite logits of any size
 *   neither overflow nor give NaN): interpolation, maximum, exponentials and their sum in fp32 as torch computes them, the one
 *   logarithm of a pixel and the additions around it in fp64 (the device's fp32 logarithm is biased, and a bias does not average
 *   out over a sum).  sums dev fp64 [batch] = the per-image sum of l, counts dev int64 [batch] = the valid pixels per image;
 *   both are overwritten.  Accumulation in fp64 through per-workgroup partials in the workspace that a second kernel adds in a
 *   fixed order: no float atomics, identical bits for identical inputs, and sums[b] does not depend on the other images.
 *   lse dev fp64 [batch, H, W] or NULL: receives the log-sum-exp of every pixel, ignored ones included, for the backward
 *   (fp64: an fp32 log-sum-exp of logits near 1e4 is off by up to 5e-4, which exp(z - lse) turns into a relative error).
 * irn_seg_loss_backward: coef dev fp32 [batch], image b's upstream gradient of sums[b] (read on the device, nothing synchronises);
 *   grad_logits[b, c, y, x] = coef[b] * sum over the valid (Y, X) of wgt((Y, X) -> (y, x)) * (exp(z[b, c, Y, X] - lse[b, Y, X])
 *   - [label == c]), wgt the weight the interpolation gave coarse cell (y, x) in fine pixel (Y, X).  A gather: a workgroup owns a
 *   tile of 8 x 8 coarse cells and keeps their logits with a one-cell halo in LDS, every thread adds what reaches its
 *   (cell, class) over the cell's footprint of at most 2 factor x 2 factor fine pixels, Y ascending and X ascending within a
 *   row, in fp32.  No atomics of any kind: every element of grad_logits dev fp32 [batch, C, h, w] is written exactly once with
 *   a plain store, nothing is cleared first, identical inputs give identical bits and an image's gradient does not depend on
 *   the images batched with it.
 * irn_seg_argmax: out dev uint8 [batch, H, W] = the first channel that attains the maximum of z; a NaN counts as the maximum
 *   (torch.argmax, irn_label_epilogue).
 * ws: irn_seg_loss_workspace_bytes(batch, C, h, w, factor, H, W) bytes of device memory, 8-byte aligned (0 = bad geometry); the
 *   backward checks it like the forward and leaves it untouched.  Null pointers, batch outside [1, 65535], C, factor, h, w, H or W
 *   outside their ranges and pointers that are not aligned to their element give IRN_ERR_ARG, a workspace that is too small
 *   IRN_ERR_STATE, all before any device is touched. */
size_t irn_seg_loss_workspace_bytes(int batch, int C, int h, int w, int factor, int H, int W);
int irn_seg_loss_forward(const float *logits, const uint8_t *label, int batch, int C, int h, int w, int factor, int H, int W,
                         double *sums, int64_t *counts, double *lse, void *ws, size_t ws_bytes, void *stream);
int irn_seg_loss_backward(const float *logits, const uint8_t *label, const double *lse, const float *coef, int batch, int C, int h,
                          int w, int factor, int H, int W, float *grad_logits, void *ws, size_t ws_bytes, void *stream);
int irn_seg_argmax(const float *logits, int batch, int C, int h, int w, int factor, int H, int W, uint8_t *out, void *stream);

/* Multi-scale segmentation inference of ONE image in one launch: the mean over M logit maps of different sizes
 * of the softmax of their bilinear upsampling to the image's size, and its arg-max, without any [C, H, W] tensor but the one
 * asked for.
 *   maps HOST array of M device pointers, 1 <= M <= IRN_SEG_FUSE_MAX_MAPS: maps[m] dev fp32 [C, h[m], w[m]], contiguous.
 *   h, w, Hs, Ws HOST int32 [M]: the map's size, and the size Hs[m] x Ws[m] of the rescaled image it was computed from.
 *   stride 1..64 (the network's output stride), C 2..IRN_EVAL_MAX_CLASSES, output H x W, each 1..32768, as are h[m] and w[m].
 *   1 <= Hs[m] <= h[m] * stride and Hs[m] <= stride * H (a map is never finer than the output), likewise the widths.
 * Definition (not claimed bit-equal to any torch op):
 *   ry_m = (float)((double)Hs[m] / ((double)stride * H)), rx_m likewise;
 *   z_m[c, Y, X] = upsample_blend over upsample_tap(Y, h[m], ry_m) and upsample_tap(X, w[m], rx_m), the device functions of
 *     irn_upsample_bilinear and irn_seg_argmax (for Hs[m] == H theirs bit for bit), every operation rounded;
 *   p_m = softmax_c(z_m) in fp32 with the maximum subtracted: exp(z - max) * (1 / sum); finite logits of any size neither
 *     overflow nor give NaN;
 *   P = (p_0 + p_1 + ... + p_{M-1}) * (float)(1.0 / M), added in map order in fp32;
 *   label[Y, X] = the first class that attains the maximum of P, a NaN counting as the maximum (irn_seg_argmax's rule).
 * Outputs, either may be NULL but not both: label dev uint8 [H, W], prob dev fp32 [C, H, W] (= P).  Every element is written
 * once with a plain store: no atomics, nothing synchronises, identical inputs give identical bits, and label is the arg-max
 * of the very P that prob receives.
 * A workgroup owns a T x T tile of the output and keeps, for all maps at once, the cells its taps touch in LDS; T is the
 * largest of 32, 16, 8 at which that fits in 64 KB.  Null pointers, M, C, stride or a size outside its range, a misaligned
 * pointer and a geometry that fits at no T give IRN_ERR_ARG with the entry and the argument named, before any device is
 * touched. */
#define IRN_SEG_FUSE_MAX_MAPS 16
int irn_seg_fuse(const float *const *maps, const int32_t *h, const int32_t *w, const int32_t *Hs, const int32_t *Ws, int M, int C,
                 int stride, int H, int W, uint8_t *label, float *prob, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Random-walk context  (replaces misc/indexing.py:141-165 `propagate_to_edge` and everything it
 * calls: PathIndex :148, edge_to_affinity :151, affinity_sparse2dense :154, to_transition_matrix
 * :160, the final matmul :164 — as sparse stencil sweeps, never densified).
 *
 * A context is bound to one radius and serves batches of independent images ("units").
 *   irn_walk_create      host-side tables for `radius` are built and uploaded once
 *   irn_walk_configure   describe a batch: n images with grid (h[i], w[i]) and c[i] walk channels
 *                        (c = #classes for semantic labels, #classes x #instances for instance
 *                        labels); returns the scratch bytes the batch needs
 *   irn_walk_run         for every image i:  out[i][c,h,w] = (cam[i][c] * (1-edge[i])) . T_i^n_sweeps
 *                        with T_i the column-normalised beta-powered affinity of edge[i]
 *                        (n_sweeps = 2^exp_times).  Pointer arrays are HOST arrays of device
 *                        pointers.  `inst_map` (optional, may be NULL or hold NULLs): per image an
 *                        int32 [h,w] cluster map with k_inst[i] instances — then cam[i] is
 *                        [c/k_inst, h, w] and channel (cls*k_inst + k) starts from
 *                        cam[cls] * (inst_map == k)   (step/make_ins_seg_labels.py:77-80,:133).
 * beta must be > 0 (beta == 0 would make the reference's dense matrix all-ones).
 * ------------------------------------------------------------------------------------------- */
typedef struct irn_walk_ctx irn_walk_ctx;

int irn_walk_create(int radius, irn_walk_ctx **ctx_out);
int irn_walk_destroy(irn_walk_ctx *ctx);
int irn_walk_configure(irn_walk_ctx *ctx, int n_images, const int32_t *h, const int32_t *w,
                       const int32_t *c, size_t *workspace_bytes);
int irn_walk_run(irn_walk_ctx *ctx, const float *const *edge_dev, const float *const *cam_dev,
                 const int32_t *const *inst_map_dev, const int32_t *k_inst,
                 float *const *out_dev, float beta, int n_sweeps,
                 void *workspace_dev, size_t workspace_bytes, void *stream);

/* How x . T^n_sweeps is evaluated (round 3).  T is similar to a symmetric matrix with spectrum in [-1, 1], and
 * lambda^n = sum_k c_k T_k(lambda) (Chebyshev polynomials) with c_k = 2^(1-n) C(n, (n-k)/2) ~ exp(-k^2 / 2n): the terms
 * beyond K ~ sqrt(2 n ln(1/tol)) are dropped (their sum is the bound `tol` on the change of the result, 1e-7 by default:
 * below the rounding of the fp32 state) and the walk runs the three-term recurrence y_{t+1} = 2 T y_t - y_{t-1} for K
 * operator applications instead of n (84 instead of 256 at exp_times = 8), accumulating s = sum_k c_k y_k.  Measured
 * against the fp64 oracle the result is as close as that of the plain iteration (tests/test_gpu_schedule.py).
 *   option "accel" = 1 (default) / 0: truncated Chebyshev series / plain powers (n applications, bit-identical to the
 *   recurrence-free kernels of rounds 1-2); "accel_tol_exp" = e: tol = 10^-e (default 7: 84 applications for n = 256; 6: 78).
 *   irn_walk_steps reports the operator applications a run with `n_sweeps` would execute (for flop accounting).
 * The caller's edge / cam / inst_map device buffers must stay valid and unmodified until irn_walk_sync (or the next
 * irn_walk_run) returns: a run that irn_walk_sync has to repeat reads them again. */
int irn_walk_steps(irn_walk_ctx *ctx, int n_sweeps, int *n_steps);
/* The series itself (host only, no device needed): *n_steps = K operator applications, *recurrence = 1 for the
 * three-term recurrence / 0 for plain powers (n < 8 or nothing to gain), coef_out[0..K] = c_k renormalised to sum 1
 * (may be NULL; coef_cap = its capacity). */
int irn_power_series(int n, int tol_exp, double *coef_out, int coef_cap, int *n_steps, int *recurrence);

/* Tuning knobs (performance only, never results): name/value pairs, e.g. "variant" = 0 generic table-driven sweep
 * (any radius; the default for radii other than 5 and 10), 1 = register-blocked streaming sweep (radius 5/10),
 * 2 = weights-stationary persistent walk (radius 5/10; the DEFAULT there, with a per-batch fall-back to variant 1
 * when an image does not fit one round of workgroups or the grid cannot be co-resident); "cooperative" = 1 (default)
 * launches the persistent kernel with hipLaunchCooperativeKernel.  Unknown names fail. */
int irn_walk_set_option(irn_walk_ctx *ctx, const char *name, int value);

/* The weights-stationary persistent kernel ("variant" = 2) runs one workgroup per compute unit and its tiles wait for
 * each other inside the launch, with a bounded wait: when the grid does not become co-resident in time (another
 * process, stream or partition holds compute units) a launch gives up instead of hanging.
 *   irn_walk_sync   waits for the last irn_walk_run; if that launch gave up, runs the batch again on the streaming
 *                   sweeps (same operator, kernel boundaries instead of in-launch hand-offs) and waits for it, so the
 *                   outputs are valid whenever it returns IRN_OK.  *fell_back (may be NULL) = 1 when that happened.
 *                   This is the call to make before consuming the outputs of a run.
 *   irn_walk_check  no waiting, no repair: IRN_ERR_STATE if a launch completed so far gave up and irn_walk_sync has
 *                   not handled it (the outputs of that run are invalid) — what a benchmark wants, where a silent
 *                   fall-back would misreport.  Always IRN_OK for the streaming variants.
 *   irn_walk_fallback_runs   how many batches irn_walk_sync has re-run so far (monitoring). */
int irn_walk_sync(irn_walk_ctx *ctx, int *fell_back);
int irn_walk_check(irn_walk_ctx *ctx);
int irn_walk_fallback_runs(irn_walk_ctx *ctx);

/* Start-up self-checks of the weights-stationary walk's two measured assumptions (speed only, never results; the
 * reference has no counterpart — its walk is dense sgemm, misc/indexing.py:132-139):
 *   placement   0 not checked yet, 1 "blocks with equal b % 8 share an XCD, the eight residues eight XCDs" holds on this device (the tiles of an image are
 *               then packed onto one XCD), 2 it does not (tiles keep launch order; one line on stderr says so);
 *   poll_delay  the delay (units of 64 clocks) between a single-channel tile's stores and its first poll in use now;
 *   probe_ms4   launch times in ms the start-up probe measured for delays 8, 10, 12, 14 on this context's first representative
 *               batch (zeros: this context did not probe — too small a batch, another context of the process probed
 *               before, or option "poll_delay" pinned the value; "poll_delay_auto" = 0 switches the probe off).
 * Any pointer may be null. */
int irn_walk_tuning(irn_walk_ctx *ctx, int *poll_delay, int *placement, float *probe_ms4);

/* How the weights-stationary walk packs a batch onto the device — host arithmetic only, no device and no context needed
 * (the CPU tests check it; the reference has no counterpart: it walks one image at a time, step/make_sem_seg_labels.py:41).
 * Images i = 0..n_images-1 of h[i] x w[i] grid pixels and channels[i] walk channels are cut into tiles (one workgroup each)
 * and packed into rounds of at most n_workgroups tiles; the workgroups run their rounds back to back, so inside a round the
 * heaviest image goes to the slot range that is free first.  placement as irn_walk_tuning reports it (1: consecutive slots
 * share an XCD, 2: launch order).  jobs_out: int32 [cap_rounds][n_workgroups][4] = {image or -1, tile y0, tile x0, tiles of
 * the image}; *n_rounds = rounds needed, 0 when the batch does not fit the persistent launch (an image with more tiles than
 * workgroups, or narrower than the radius: such batches run on the streaming sweeps).  cap_rounds = 0 only asks for *n_rounds. */
int irn_walk_plan_rounds(int radius, int n_images, const int32_t *h, const int32_t *w, const int32_t *channels,
                         int n_workgroups, int placement, int32_t *jobs_out, int cap_rounds, int *n_rounds);

/* Diagnostic (option "profile" = 1, resident walk only): per-sweep time stamps of two workgroups of
 * the first round — host_out is int64 [2][256][4] = {sweep start, state staged, first partial sums
 * in LDS, sweep stored} in ticks of the 100 MHz wall clock.  Synchronises the device. */
int irn_walk_read_profile(irn_walk_ctx *ctx, long long *host_out);

/* Kernel timing hook for bench.py: when enabled, every irn_walk_run brackets its sweep kernels
 * with a pair of HIP events on `stream` (no synchronisation).  irn_walk_last_sweep_ms waits for the
 * pairs recorded since its previous call, returns their summed elapsed time and the number of
 * sweeps (one sweep = one pass of the transition operator over the whole batch) they cover, and
 * forgets them. */
int irn_walk_enable_timing(irn_walk_ctx *ctx, int enable);
int irn_walk_last_sweep_ms(irn_walk_ctx *ctx, float *ms, int *n_launches);

/* Intermediate products of the last irn_walk_run, for parity tests of the build stage:
 * weights of image i as [n_dirs, h, w] in raster direction order (order = 1) and 1/degree
 * as fp64 [h, w], copied device-to-device out of the workspace. */
int irn_walk_export_weights(irn_walk_ctx *ctx, int image, float *w_dev, double *inv_deg_dev,
                            void *workspace_dev, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Label epilogue  (replaces step/make_sem_seg_labels.py:43-49 and
 * step/make_ins_seg_labels.py:137-145).  For every image: bilinear x4 upsample
 * (align_corners=False) of rw [c,h,w] cropped to (out_h,out_w); divide by the global max;
 * argmax over {bg_thres, channels} with the first maximum winning.
 *   labels_dev[i]  uint8 [out_h,out_w] = 0 for background else keys[i][argmax-1]+1
 *                  (keys: host array of device int64 pointers, the CAM dict's `keys`); may be NULL
 *   argmax_dev[i]  int32 [out_h,out_w] raw argmax index (0 = background); may be NULL
 *   rw_up_dev[i]   fp32 [c,out_h,out_w] normalised upsampled scores (instance scoring); may be NULL
 * scratch: n_images * 4 bytes of device memory (per-image max), provided by the caller.
 * ------------------------------------------------------------------------------------------- */
int irn_label_epilogue(int n_images, const float *const *rw_dev, const int32_t *c, const int32_t *h,
                       const int32_t *w, const int32_t *out_h, const int32_t *out_w, float bg_thres,
                       const int64_t *const *keys_dev, uint8_t *const *labels_dev,
                       int32_t *const *argmax_dev, float *const *rw_up_dev, void *scratch_dev,
                       void *stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-scale CAM merge  (replaces step/make_cam.py:38-52).  src[s]: dev fp32 [n_classes, hs[s], ws[s]]
 * activation maps of scale s (original + flipped-back, net/resnet50_cam.py:66-70); keys: dev int64
 * [n_keys] present classes (torch.nonzero(label)).  Writes
 *   cam      dev fp32 [n_keys, ceil(out_h/4), ceil(out_w/4)]   sum over scales of bilinear resizes
 *   high_res dev fp32 [n_keys, out_h, out_w]                   same at 16*ceil(./16), cropped
 * each channel divided by (its maximum + 1e-5).  scratch: 8 * n_keys bytes.  At most 8 scales.
 * ------------------------------------------------------------------------------------------- */
int irn_cam_merge(int n_scales, const float *const *src_dev, const int32_t *hs, const int32_t *ws, int n_classes,
                  const int64_t *keys_dev, int n_keys, int out_h, int out_w, float *cam_dev, float *high_res_dev,
                  void *scratch_dev, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-scale input pipeline  (replaces the per-scale loop of VOC12ClassificationDatasetMSF.__getitem__,
 * voc12/dataloader.py:191-201: pil_rescale misc/imutils.py:8-22 -> TorchvisionNormalize
 * voc12/dataloader.py:65-78 -> HWC_to_CHW -> stack([img, flip(img, -1)])).
 *
 * The resampling is Pillow's 8-bit bicubic (Image.resize(size, Image.BICUBIC): separable, 22-bit fixed-point
 * weights, int32 accumulation, 8-bit intermediate) and is bit-exact.
 *
 *   irn_bicubic_plan        host only: the fixed-point tap table of one axis (lo[out], count[out],
 *                           weights[out * ksize]); call with null arrays to query ksize.
 *   irn_bicubic_resize_u8   dev u8 [h, w, channels] -> dev u8 [hs, ws, channels]  (= misc/imutils.py pil_resize
 *                           order 3); channels 1, 3 or 4; scratch: irn_bicubic_scratch_bytes.
 *   irn_msf_pack            dev u8 [h, w, 3] -> for each scale s a dev fp32 [2, 3, hs[s], ws[s]]: resized,
 *                           normalised through lut (dev fp32 [3 * 256], lut[c * 256 + v] = the fp32 value of
 *                           (v / 255. - mean[c]) / std[c] computed in double), channel-major, image followed by
 *                           its horizontal flip.  hs/ws equal to h/w skip the resize like the reference's
 *                           `s == 1` branch.  scratch: max over scales of irn_bicubic_scratch_bytes(.., 3).
 * ------------------------------------------------------------------------------------------- */
int irn_bicubic_plan(int in_size, int out_size, int32_t *ksize, int32_t *lo, int32_t *count, int32_t *weights,
                     size_t weights_capacity);
size_t irn_bicubic_scratch_bytes(int h, int w, int hs, int ws, int channels);
int irn_bicubic_resize_u8(const uint8_t *img_dev, int h, int w, int channels, int hs, int ws, uint8_t *out_dev,
                          void *scratch_dev, void *stream);
int irn_msf_pack(const uint8_t *img_dev, int h, int w, int n_scales, const int32_t *hs, const int32_t *ws,
                 const float *lut_dev, float *const *out_dev, void *scratch_dev, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Training-input pipeline of the CAM step, batched  (replaces VOC12ClassificationDataset.__getitem__,
 * voc12/dataloader.py:129-156 as step/train_cam.py:44-46 configures it: random_resize_long misc/imutils.py:25-34 ->
 * TorchvisionNormalize -> random_lr_flip -> random_crop / top_left_crop -> HWC_to_CHW) for n_images ragged images in
 * two launches: a horizontal pass over the source rows the crop shows, a vertical pass that writes every cell of
 * out fp32 [n_images, 3, crop, crop] once (lut[c * 256 + byte] inside an image's box, 0.0f outside; lut as irn_msf_pack).
 * Bit-exact against the PIL / numpy pipeline: the taps are Pillow's (irn_bicubic_plan), the arithmetic is integer.
 *
 * meta: HOST int32 [meta_words] = n_images descriptors of IRN_AUGMENT_DESC_WORDS words followed by the tap tables:
 *   word 0 h, 1 w                 source size; the image is u8 [h, w, 3] at byte word 10 of pixels_dev
 *   2 c_top, 3 c_left, 4 rows, 5 cols   the image's box in the crop
 *   6 r0, 7 n_rows                source rows [r0, r0 + n_rows) go through the horizontal pass into
 *                                 scratch u8 [n_rows, cols, 3] at byte word 11 of scratch_dev
 *   8 kx, 9 ky                    weights per entry of the X / Y table
 *   12 x_table, 13 y_table        word index in meta of a table: lo [n] | count [n] | weights [n, k]; X has `cols`
 *                                 entries over source columns (a mirrored image lists them reversed), Y has `rows`
 *                                 entries over the scratch rows (lo counted from r0);  14, 15 unused
 * Every bound is checked on the host before any HIP call (lo >= 0, lo + count <= extent, box inside the crop, offsets
 * inside pixels_bytes / scratch_bytes / meta_words, out_elems >= n_images * 3 * crop^2): a bad descriptor is IRN_ERR_ARG
 * and nothing is launched.  meta is then copied to meta_dev (>= meta_words words) on the stream; it must stay valid until
 * that copy has run when it is page-locked memory.  n_images == 0 is IRN_OK without a launch.
 * ------------------------------------------------------------------------------------------- */
#define IRN_AUGMENT_DESC_WORDS 16
int irn_augment_batch(int n_images, int crop, const int32_t *meta, size_t meta_words, const uint8_t *pixels_dev,
                      size_t pixels_bytes, const float *lut_dev, float *out_dev, size_t out_elems, void *scratch_dev,
                      size_t scratch_bytes, int32_t *meta_dev, size_t meta_dev_words, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Label half of the IRNet step's (image, label) pair, batched  (replaces the label's share of
 * VOC12AffinityDataset.__getitem__, voc12/dataloader.py:251-267: random_scale with order 0 misc/imutils.py:36-43 ->
 * random_lr_flip -> random_crop / top_left_crop with fill 255 -> pil_rescale(label, 0.25, 0)) for n_images ragged
 * u8 [h, w] IR label maps in ONE launch.  out u8 [n_images, crop / reduce, crop / reduce], every cell written once:
 * cell (y, x) looks at container position (Y, X) = (reduce * y + reduce / 2, reduce * x + reduce / 2), the cell Pillow's
 * NEAREST reads when it shrinks crop -> crop / reduce; it is 255 outside the image's box and
 * label[row_table[Y - c_top], col_table[X - c_left]] inside.  reduce == 1 returns the whole cropped label.
 * The tables are Pillow's NEAREST source indices of the box's rows and columns (irn_amd.ops.nearest_plan: (int) of a
 * double that starts at 0.5 * in / out and grows by in / out per cell — not floor((x + 0.5) * in / out)); a mirrored
 * image lists its columns reversed.  Integers only, no atomics: bit-exact and bit-reproducible.
 *
 * meta: HOST int32 [meta_words] = n_images descriptors of IRN_AUGMENT_LABEL_DESC_WORDS words followed by the tables:
 *   word 0 h, 1 w                 source size; the map is u8 [h, w] at byte word 6 of labels_dev
 *   2 c_top, 3 c_left, 4 rows, 5 cols   the image's box in the crop (the same box irn_augment_batch takes)
 *   7 row_table, 8 col_table      word index in meta of an index table: `rows` source rows / `cols` source columns;
 *                                 9 .. 11 unused
 * As with irn_augment_batch every bound is checked on the host before any HIP call (table entries inside [0, h) / [0, w),
 * box inside the crop, offsets inside labels_bytes / meta_words, reduce >= 1 and crop % reduce == 0,
 * out_elems >= n_images * (crop / reduce)^2): a bad descriptor is IRN_ERR_ARG and nothing is launched.  meta is then copied
 * to meta_dev (>= meta_words words) on the stream; n_images == 0 is IRN_OK without a launch.
 * ------------------------------------------------------------------------------------------- */
#define IRN_AUGMENT_LABEL_DESC_WORDS 12
int irn_augment_label_batch(int n_images, int crop, int reduce, const int32_t *meta, size_t meta_words,
                            const uint8_t *labels_dev, size_t labels_bytes, uint8_t *out_dev, size_t out_elems,
                            int32_t *meta_dev, size_t meta_dev_words, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Trunk epilogue  (replaces the elementwise tail of reference net/resnet50.py:34-54 Bottleneck.forward —
 * FixedBatchNorm :11-14, `out += residual`, ReLU — and of the stem :94-97, on the inference path)
 *
 *   x dev fp32 [n_images, n_channels, plane_elems] (a convolution's output, contiguous NCHW), IN PLACE:
 *       x[n, c, i] = act(x[n, c, i] * scale[c] + shift[c] (+ r[n, c, i]))      act = ReLU if relu else identity
 *       r = res, or res * res_scale[c] + res_shift[c] when res_scale / res_shift are given (the projection shortcut's own
 *       batch norm, net/resnet50.py:48-49, folded into the same pass)
 *   scale / shift (/ res_scale / res_shift) dev fp32 [n_channels]: weight / sqrt(running_var + eps) and
 *   bias - running_mean * scale, folded by the caller; res (may be NULL) like x.  One fused multiply-add per element and
 *   operand, then one addition; NaNs propagate.  x and res 16-byte aligned; at most 2^31 - 1 elements per call.
 * ------------------------------------------------------------------------------------------- */
int irn_bn_act(float *x_dev, const float *res_dev, const float *scale_dev, const float *shift_dev, const float *res_scale_dev,
               const float *res_shift_dev, int64_t n_images, int n_channels, int64_t plane_elems, int relu, void *stream);

/* The same pass over a channels-last tensor: x dev fp32 [n_pixels, n_channels] (= an [N, C, H, W] tensor in
 * torch.channels_last memory format, n_pixels = N*H*W), n_channels a multiple of 4, constants 16-byte aligned.  Same
 * arithmetic (one fmaf per element), same reference lines (net/resnet50.py:11-14, :34-54); for a trunk whose convolutions
 * run on MIOpen's NHWC solvers (IRN_CHANNELS_LAST=1). */
int irn_bn_act_nhwc(float *x_dev, const float *res_dev, const float *scale_dev, const float *shift_dev, const float *res_scale_dev,
                    const float *res_shift_dev, int64_t n_pixels, int n_channels, int relu, void *stream);

/* The same tail as a differentiable operator, for the training seam (net/resnet50.py TRAIN_FUSED_TAIL, ops.bn_act): the
 * reference trains through FixedBatchNorm -> `out += residual` -> ReLU (net/resnet50.py:11-14, :34-54) with autograd's
 * composed kernels.  All three entries are free of atomics: the same inputs give the same bits.
 *
 * irn_bn_fold: weight, bias, mean, var dev fp32 [n_channels] -> scale = weight / sqrt(var + eps), shift = bias - mean * scale,
 *   dev fp32 [n_channels], every operation in double with its own rounding (no contraction) and ONE rounding to fp32 at the
 *   end: bit for bit `FrozenBatchNorm._fold64()` followed by `.float()`.  One launch.
 * irn_bn_act_forward: irn_bn_act out of place — x is left as it is (the weight gradient needs it), out dev fp32 like x, not
 *   overlapping it, receives act(x * scale[c] + shift[c] (+ r)); same arithmetic, same bits as irn_bn_act.
 * irn_bn_act_backward: with dz = grad_out where out > 0 or NaN (relu = 1; torch's threshold_backward), else grad_out itself:
 *       grad_x = dz * scale[c]                                         (written if grad_x_dev != NULL; needs scale_dev)
 *       grad_res = dz, or dz * res_scale[c] if res_scale_dev != NULL   (written if grad_res_dev != NULL)
 *       sums[0 * C + c] = sum dz,  sums[1 * C + c] = sum dz * x,  and with res_scale_dev: sums[2 * C + c] = sum dz * res
 *                                                                      (dev fp64 [2 or 3, C], if sums_dev != NULL; needs x_dev)
 *   over images and plane, accumulated in double: per thread, then a fixed tree per workgroup, then a channel's workgroup
 *   partials in ascending order by a second small launch.  From them the caller has grad_weight = (S1 - mean * S0) /
 *   sqrt(var + eps), grad_bias = S0, and the shortcut's batch norm likewise with S2.  grad_out, out (needed with relu = 1), x,
 *   res, grad_x, grad_res dev fp32 [n_images, n_channels, plane_elems] contiguous, 16-byte aligned; what is not needed may be
 *   NULL and is then neither read nor written.  workspace: caller device memory of
 *   irn_bn_act_backward_workspace_bytes(n_images, n_channels, plane_elems) bytes (0 = bad geometry), needed with sums_dev.
 *   At most 2^31 - 1 elements per call; enqueued on `stream`, nothing synchronises. */
int irn_bn_fold(const float *weight_dev, const float *bias_dev, const float *mean_dev, const float *var_dev, double eps,
                int n_channels, float *scale_dev, float *shift_dev, void *stream);
int irn_bn_act_forward(const float *x_dev, const float *res_dev, const float *scale_dev, const float *shift_dev,
                       const float *res_scale_dev, const float *res_shift_dev, float *out_dev, int64_t n_images, int n_channels,
                       int64_t plane_elems, int relu, void *stream);
size_t irn_bn_act_backward_workspace_bytes(int64_t n_images, int n_channels, int64_t plane_elems);
int irn_bn_act_backward(const float *grad_out_dev, const float *out_dev, const float *x_dev, const float *res_dev,
                        const float *scale_dev, const float *res_scale_dev, float *grad_x_dev, float *grad_res_dev, double *sums_dev,
                        int64_t n_images, int n_channels, int64_t plane_elems, int relu, void *workspace_dev, size_t workspace_bytes,
                        void *stream);

/* 1x1 convolution of a channels-last activation with its whole elementwise tail in the GEMM's epilogue (hipBLASLt, fp32
 * compute): conv1 -> bn1 -> ReLU and conv3 -> bn3 -> (+ residual) -> ReLU of Bottleneck.forward, reference
 * net/resnet50.py:34-54 (FixedBatchNorm :11-14 is a constant affine map: its scale is folded into `w` by the caller in
 * double precision, its shift is `bias`), and the projection shortcut :48-49.
 *   x dev fp32 [m, cin] (= [N, cin, H, W] in torch.channels_last, m = N*H*W), w dev fp32 [cout, cin] (the convolution's
 *   weight, scale folded in), bias dev fp32 [cout] or NULL, residual dev fp32 [m, cout] or NULL (may be `out`),
 *   out dev fp32 [m, cout]:      out = act(x . w^T + bias (+ residual)),   act = ReLU if relu else identity.
 *   algo_rank: 0 = hipBLASLt's first heuristic choice for the problem, k = its k-th (irn_conv1x1_algo_count gives how many
 *   there are): a function of the problem only, never of a timing made in this process, so that every process computes
 *   the same bits.  workspace: caller device memory of irn_conv1x1_workspace_bytes() (may be 0 / NULL: fewer kernels
 *   qualify).  Enqueued on `stream`; nothing synchronises. */
size_t irn_conv1x1_workspace_bytes(void);
int irn_conv1x1_algo_count(int64_t m, int cin, int cout, int has_bias, int has_residual, int relu, size_t workspace_bytes,
                           int *count_out);
int irn_conv1x1_nhwc(const float *x_dev, const float *w_dev, const float *bias_dev, const float *residual_dev, float *out_dev,
                     int64_t m, int cin, int cout, int relu, int algo_rank, void *workspace_dev, size_t workspace_bytes,
                     void *stream);

/* Split-precision form of the same layers (round 6): the fp32 GEMM runs at <= 0.9 of the 157 TFLOP/s fp32 matrix peak; an fp16
 * MFMA GEMM with fp32 accumulation runs ~2.5x faster over a 3x longer K, and two fp16 numbers carry 22 mantissa bits:
 *       x = x_hi + 2^-11 x_lo',  x_hi = fp16(x),  x_lo' = fp16((x - x_hi) 2^11)          (irn_split16, per element)
 *       x . w ~ x_hi w_hi + x_hi w_lo + x_lo' (w_hi 2^-11)                                (the dropped term: 2^-22 |x w|)
 * Measured on every 1x1 layer of the CAM network: 5.4e-6 / 9.2e-6 from fp64 on the normalised CAM where the fp32 GEMMs give
 * 5.9e-6 / 7.6e-6 (tools/bf16x3_cam_error.py; bar 1e-4); per layer 3.4e-7 .. 1.9e-6 against 2.6e-7 .. 1.3e-6 (profiles/r06_s2_*).
 * Same reference lines as irn_conv1x1_nhwc (net/resnet50.py:34-54).
 *
 * irn_split16: x dev fp32 [n_pixels, n_channels] (channels-last activation, n_channels a multiple of 8, 16-byte aligned)
 *   -> out dev fp16 [n_pixels, 3 n_channels] = [hi | hi | lo'] per pixel.  With scale / shift (dev fp32 [n_channels], both or
 *   neither) the element is first y = x * scale[c] + shift[c] (one fmaf, the FixedBatchNorm of the 3x3 convolution in front,
 *   net/resnet50.py:40-42) and, with relu, max(y, 0) — the fp32 tensor is read once and never written back.  flags_dev
 *   (dev uint32) gets bit 0 set (atomicOr; the other bits are left alone) when an element was beyond fp16's range
 *   (|y| > 65504, y = the value that is split) or NaN: the caller's signal that this activation needs the fp32 path.  The
 *   caller zeroes it and reads it behind the stream.  pixels_per_sample = 0, the usual value: flags_dev is ONE word for the
 *   call and may be NULL.  pixels_per_sample >= 1: the overflow is attributed PER SAMPLE (a sample = one leading row of the
 *   network input) — flags_dev is dev uint32 [n_pixels / pixels_per_sample], never NULL, row r flags word
 *   r / pixels_per_sample and the words of other samples are left alone; n_pixels must be a multiple of pixels_per_sample.
 *   The fp16 output does not depend on pixels_per_sample.
 * irn_gemm16_nhwc: a16 dev fp16 [m, k] (irn_split16's output, k = 3 cin), b16 dev fp16 [cout, k] = [w_hi | w_lo | w_hi 2^-11] of
 *   the batch-norm-folded weight scaled by 2^p (prepared by the caller in double precision), alpha = 2^-p:
 *       out = act(alpha a16 . b16^T + bias (+ residual)),  fp32 [m, cout]; algo_rank / workspace as irn_conv1x1_nhwc. */
int irn_split16(const float *x_dev, const float *scale_dev, const float *shift_dev, int relu, void *out_dev, int64_t n_pixels,
                int n_channels, int64_t pixels_per_sample, unsigned *flags_dev, void *stream);
/* The same pass between a dense map [n_images, h, w, n_channels] and its zero-bordered form [n_images, h+2, w+2, .] (pixel (n, y, x)
 * at row n (h+2)(w+2) + (y+1)(w+2) + x+1): in_padded = x is the bordered fp32 form (interior read), out_padded = out is the
 * bordered fp16 form (interior split from the pixels, border rows written as zeros: the buffer needs no preparation).
 * per_sample = 0, the usual value: flags_dev is one word for the call (may be NULL); per_sample != 0: one word per image, dev
 * uint32 [n_images], never NULL (irn_split16's pixels_per_sample = h w); border rows flag nothing and are never read.  On the
 * bordered form a 3x3 / pad 1 / stride 1 convolution (conv2 of Bottleneck.forward, net/resnet50.py:40) is NINE fp16 GEMMs that
 * accumulate over row-shifted views of one operand — tap (ky, kx) reads row r + (ky-1)(w+2) + (kx-1):
 * irn_conv3x3_split_gemm: a16 dev fp16 = the bordered operand [n (h+2)(w+2), 3 cin] with (w+3) rows of valid memory in front of
 *   and behind it (any content), w16 dev fp16 [9, cout, 3 cin] (one irn_gemm16_nhwc operand per tap, raster order, one common
 *   scale), out dev fp32 [n (h+2)(w+2), cout] = alpha sum_taps a16[shifted] . w16[tap]^T, accumulated tap after tap in fp32 in a
 *   fixed order; border rows of `out` hold garbage.  row_fused = 1: w16 = [3, cout, 9 cin] (the three taps of a kernel row side by
 *   side) and THREE GEMMs over K = 9 cin — the taps (ky, 0..2) of a pixel are three consecutive memory rows, so a kernel row's
 *   operand is the same buffer read with leading dimension 3 cin and 9 cin columns.  algo_rank / workspace as irn_conv1x1_nhwc. */
int irn_split16_pad(const float *x_dev, const float *scale_dev, const float *shift_dev, int relu, void *out_dev, int64_t n_images,
                    int h, int w, int n_channels, int in_padded, int out_padded, int per_sample, unsigned *flags_dev,
                    void *stream);
int irn_conv3x3_split_gemm(const void *a16_dev, const void *w16_dev, float *out_dev, int64_t n_images, int h, int w, int cin, int cout,
                           float alpha, int row_fused, int algo_rank, void *workspace_dev, size_t workspace_bytes, void *stream);
int irn_gemm16_algo_count(int64_t m, int k, int cout, int has_bias, int has_residual, int relu, size_t workspace_bytes,
                          int *count_out);
int irn_gemm16_nhwc(const void *a16_dev, const void *b16_dev, const float *bias_dev, const float *residual_dev, float *out_dev,
                    int64_t m, int k, int cout, int relu, float alpha, int algo_rank, void *workspace_dev, size_t workspace_bytes,
                    void *stream);

/* Stem: batch norm + ReLU + max pool 3x3 / stride 2 / pad 1 in one pass (reference net/resnet50.py:94-97; the nets'
 * stage1, net/resnet50_cam.py:14, net/resnet50_irn.py:15).
 *   x dev fp32 [n_images, n_channels, h, w] (conv1's output) -> out dev fp32 [n_images, n_channels, (h-1)/2+1, (w-1)/2+1]
 *   = max over the window's in-image taps of relu(x * scale[c] + shift[c]); NaNs propagate. */
int irn_stem_pool(const float *x_dev, const float *scale_dev, const float *shift_dev, int64_t n_images, int n_channels, int h,
                  int w, float *out_dev, void *stream);

/* IRNet heads: bilinear upsampling by an integer factor, align_corners = False, (+ ReLU) — nn.Upsample(scale_factor = f,
 * mode = 'bilinear') followed by nn.ReLU, reference net/resnet50_irn.py:36,42,48,72,78,84.  ATen's source index and
 * weights (src = (dst + 0.5) / f - 0.5 clamped at 0) and its operation order, in fp32 without contraction.
 *   x dev fp32 [n_planes, h, w] -> out dev fp32 [n_planes, h * f, w * f] (16-byte aligned) */
int irn_upsample_bilinear(const float *x_dev, int64_t n_planes, int h, int w, int factor, int relu, float *out_dev,
                          void *stream);
/* Its exact adjoint: grad_in[y, x] = sum over the outputs (yo, xo) of grad_out[yo, xo] * (out[yo, xo] > 0, with relu) * the
 * weight the forward gave input (y, x) in output (yo, xo) — the same fp32 source index and weights, second tap clamped to
 * the last row / column.  A gather: one thread per input cell, output rows ascending and columns ascending within a row,
 * fp32 accumulation, one plain store per cell.  No atomics: identical bits for identical inputs (ATen's
 * upsample_bilinear2d_backward scatters with atomics).
 *   grad_out dev fp32 [n_planes, h * f, w * f]; out: the forward's output (needed with relu = 1, else may be null)
 *   -> grad_in dev fp32 [n_planes, h, w], fully written */
int irn_upsample_bilinear_backward(const float *grad_out_dev, const float *out_dev, int64_t n_planes, int h, int w, int factor,
                                   int relu, float *grad_in_dev, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Instance front-end
 *   irn_find_centroids_batch   replaces step/make_ins_seg_labels.py:18-56
 *       dp dev [2,h,w] -> centroids dev int32 [2,h,w]; float32 state, float64 increment in the
 *       reference's operation order, no FMA contraction, round-half-even at the end.
 *   irn_cluster_centroids_batch replaces step/make_ins_seg_labels.py:58-75 (+ misc/imutils.py:182-190):
 *       weak = |dp| < thres; 4-connected components numbered in raster order of first pixel;
 *       label at each pixel's centroid; renumbered 0..K-1 ascending.
 *       -> cluster_map dev int32 [h,w], k_dev[i] = K.
 * Both take a batch (the loop over images of step/make_ins_seg_labels.py:119-133; one image is a batch of one): HOST
 * arrays of device pointers and sizes, one launch sequence for the whole batch, and NOTHING synchronises — the counts stay on the device
 * (k_dev: dev int32 [n_images]) and the caller fetches all of them with one transfer before it configures the walk
 * (c[i] = n_classes[i] * K[i]).  scratch: irn_cluster_batch_scratch_bytes. */
int irn_find_centroids_batch(int n_images, const float *const *dp_dev, const int32_t *h, const int32_t *w,
                             int iterations, int32_t *const *centroids_dev, void *stream);
size_t irn_cluster_batch_scratch_bytes(int n_images, const int32_t *h, const int32_t *w);
int irn_cluster_centroids_batch(int n_images, const int32_t *const *centroids_dev, const float *const *dp_dev,
                                const int32_t *h, const int32_t *w, float thres, int32_t *const *cluster_map_dev,
                                int32_t *k_dev, void *scratch_dev, void *stream);

/* 4-connected component labelling of a byte mask [n,h,w] (non-zero = foreground), ids 1.. per
 * image in raster order of first pixel, 0 = background — the skimage.measure.label(connectivity=1,
 * background=0) call of step/make_ins_seg_labels.py:66,92.  n_labels_dev: int32 [n] component
 * counts.  scratch: irn_ccl_scratch_bytes(n,h,w). */
size_t irn_ccl_scratch_bytes(int n, int h, int w);
int irn_label4(const uint8_t *mask_dev, int n, int h, int w, int32_t *labels_dev, int32_t *n_labels_dev,
               void *scratch_dev, void *stream);

/* ---------------------------------------------------------------------------------------------
 * detect_instance  (replaces step/make_ins_seg_labels.py:82-105 and the one-hot of :145-147).
 * rw_up dev fp32 [n_channels,h,w] (normalised scores), argmax dev int32 [h,w] (0 = background,
 * c+1 = channel c) -> one detection per 4-connected component of every channel's mask, ordered
 * channel ascending then raster order of the component's first pixel (skimage label order).
 *   _batch_count : labels the components of every image of a batch in one pass sequence (state kept in
 *            `scratch`) and writes the detection counts to n_det_dev (dev int32 [n_images]).  Does NOT
 *            synchronise: the caller reads the counts with one transfer and sizes the outputs.
 *   _batch_emit  : after _batch_count with the same inputs and scratch plus the counts (host): score[d] =
 *            area < min_area ? 0 : max(score * mask) (:96-99), channel[d] (index into the caller's class_id
 *            array), mask dev uint8 [n_det,h,w].  Images with n_det[i] == 0 are skipped (their output
 *            pointers may be NULL).  min_area: host [n_images].
 * One image is a batch of one.  scratch: irn_detect_batch_scratch_bytes.
 * ------------------------------------------------------------------------------------------- */
size_t irn_detect_batch_scratch_bytes(int n_images, const int32_t *n_channels, const int32_t *h, const int32_t *w);
int irn_detect_instance_batch_count(int n_images, const float *const *rw_up_dev, const int32_t *const *argmax_dev,
                                    const int32_t *n_channels, const int32_t *h, const int32_t *w, int32_t *n_det_dev,
                                    void *scratch_dev, void *stream);
int irn_detect_instance_batch_emit(int n_images, const float *const *rw_up_dev, const int32_t *const *argmax_dev,
                                   const int32_t *n_channels, const int32_t *h, const int32_t *w, const int32_t *n_det,
                                   const double *min_area, float *const *score_dev, int32_t *const *channel_dev,
                                   uint8_t *const *mask_dev, void *scratch_dev, void *stream);

/* Detections as COCO run lengths, straight from the labelled map: what step/make_ins_seg_labels.py:82-105 detects, in
 * the form step/make_cocoann.py:38-46 exports, with no dense mask in between.  The masks of one image are disjoint, so
 * after irn_detect_instance_batch_count the scratch describes all of them as ONE int32 map of detection ids; every
 * detection's run lengths (the "COCO mask encoding" convention below: column-major, a leading zero-run that may be 0,
 * no trailing zero count when the last pixel is set), area and box are read off that map.
 * The outputs are batch-wide arrays over G = sum(n_det) detections, image i's at [g0_i, g0_i + n_det[i]) with g0 the
 * exclusive prefix of n_det, in detect_instance's order.  n_det: host int32 [n_images], as read from n_det_dev.
 *
 * irn_detect_instance_batch_rle_count: after _batch_count with the same inputs and scratch.  score dev fp32 [G] and
 *   channel dev int32 [G] as irn_detect_instance_batch_emit gives them (area < min_area -> score 0); area dev int32
 *   [G]; n_runs dev int32 [G]; bbox dev int32 [G][4] = [x0, y0, width, height].  Nothing synchronises: the caller
 *   reads the five arrays with one transfer and sizes counts.
 * irn_detect_instance_batch_rle_emit: after _rle_count on the same stream with rle_scratch untouched.  runs: host
 *   int64 [n_images], the sum of n_runs over each image's detections.  counts dev uint32 [sum(runs)] receives the run
 *   lengths of every detection back to back in batch order (detection g at the exclusive prefix of n_runs).  A key that
 *   would fall outside an image's share of the workspace is not written.  Nothing synchronises.
 * scratch: the one _batch_count used.  rle_scratch: irn_detect_instance_batch_rle_scratch_bytes.  ws:
 *   irn_detect_instance_batch_rle_sort_bytes(sum(runs), G) bytes (0 = bad argument, or nothing to sort).
 * n_images == 0 is valid (nothing is done); n_images < 0, a null pointer, h*w above 2^30 (so every h*w >= 2^31 - 1)
 * and n_det outside [0, h*w] give IRN_ERR_ARG before any device is touched.  Integer arithmetic apart from the score
 * maximum; the atomics are integer sums, minima and maxima and the run lengths come out of a sort of distinct keys:
 * bit-reproducible, and independent of the batch an image is part of. */
size_t irn_detect_instance_batch_rle_scratch_bytes(int n_images, const int32_t *h, const int32_t *w, const int32_t *n_det);
int irn_detect_instance_batch_rle_count(int n_images, const float *const *rw_up_dev, const int32_t *const *argmax_dev,
                                        const int32_t *n_channels, const int32_t *h, const int32_t *w,
                                        const int32_t *n_det, const double *min_area, float *score_dev,
                                        int32_t *channel_dev, int32_t *area_dev, int32_t *n_runs_dev, int32_t *bbox_dev,
                                        void *scratch_dev, void *rle_scratch_dev, void *stream);
size_t irn_detect_instance_batch_rle_sort_bytes(int64_t total_runs, int total_det);
int irn_detect_instance_batch_rle_emit(int n_images, const int32_t *h, const int32_t *w, const int32_t *n_det,
                                       const int64_t *runs, uint32_t *counts_dev, void *rle_scratch_dev, void *ws,
                                       size_t ws_bytes, void *stream);

/* Detections against the ground truth, straight from the labelled map: the counts irn_mask_overlap (below) gives for the
 * dense masks irn_detect_instance_batch_emit would have written, with no mask in between — the detection of a pixel is
 * read from the one int32 id map the scratch describes after irn_detect_instance_batch_count.
 *
 * irn_detect_instance_batch_overlap: after _batch_count with the same inputs and scratch; n_det: host int32 [n_images], as
 *   read from n_det_dev; min_area: host [n_images].  inst_dev[i]: dev uint8 [h][w], 0 = no instance, 1..g[i] = a GT
 *   instance (any alignment); g: host int32 [n_images], 0..255 each.  Outputs, batch-wide, image i's detections at the
 *   exclusive prefix of n_det, its GT instances at the exclusive prefix of g, its inter block at the exclusive prefix of
 *   n_det * g; all WRITTEN (not added into):
 *     score dev fp32 [G], channel dev int32 [G]   as irn_detect_instance_batch_emit / _rle_count give them
 *     area_pred dev int64 [G]                     pixels of the detection
 *     inter     dev int64 [sum n_det[i] * g[i]]   image i's block is [n_det[i]][g[i]]: |detection & GT instance|
 *     area_gt   dev int64 [sum g[i]]              pixels of each GT instance (also of an image without detections)
 *   bad dev int64 [1] is ADDED into: pixels whose GT id lies above g[i] (they belong to no instance, as in
 *   irn_mask_overlap).  An output whose size is 0 may be NULL.  Nothing synchronises and no workspace is needed beyond
 *   `scratch`: an image whose (n_det + 1) x (g + 1) table of counts has at most 4096 cells is counted in LDS per workgroup
 *   and flushed with integer atomics, a larger one with integer atomics on the outputs directly.
 * n_images == 0 is valid (nothing is done), and so are n_det[i] == 0 and g[i] == 0; n_images < 0, a null pointer, h*w
 * above 2^30, n_det outside [0, h*w] and g outside [0, 255] give IRN_ERR_ARG before any device is touched.  Integer
 * arithmetic apart from the score maximum (a maximum of int bit patterns): bit-reproducible, and independent of the batch
 * an image is part of.
 *
 * irn_argmax_rethreshold_batch: the argmax map irn_label_epilogue writes at background threshold `thres`, from the
 *   outputs of ONE epilogue at a threshold not above it: rw_up_dev[i] fp32 [n_channels][h][w] and argmax_dev[i] int32
 *   [h][w] of that call -> out_dev[i] int32 [h][w] (may be argmax_dev[i] itself).  A pixel keeps its channel where that
 *   channel's score is NaN or > thres (the epilogue's strict >) and becomes 0 elsewhere: bit for bit the epilogue's map.
 *   A NaN threshold gives IRN_ERR_ARG.  Nothing synchronises. */
int irn_detect_instance_batch_overlap(int n_images, const float *const *rw_up_dev, const int32_t *const *argmax_dev,
                                      const int32_t *n_channels, const int32_t *h, const int32_t *w, const int32_t *n_det,
                                      const double *min_area, const uint8_t *const *inst_dev, const int32_t *g,
                                      float *score_dev, int32_t *channel_dev, int64_t *area_pred_dev, int64_t *inter_dev,
                                      int64_t *area_gt_dev, int64_t *bad_dev, void *scratch_dev, void *stream);
int irn_argmax_rethreshold_batch(int n_images, const float *const *rw_up_dev, const int32_t *const *argmax_dev,
                                 const int32_t *n_channels, const int32_t *h, const int32_t *w, float thres,
                                 int32_t *const *out_dev, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Dense CRF  (replaces misc/imutils.py:156-170 crf_inference_label over pydensecrf, and
 *             step/cam_to_ir_label.py:22-39)
 * densecrf numerics: float32, DIAG_KERNEL, NORMALIZE_SYMMETRIC, Potts compatibility; unary from labels
 * (gt_prob, zero_unsure=False); Gaussian kernel (x/3, y/3) compat 3, bilateral (x/50, y/50, RGB/5)
 * compat 10; t mean-field iterations.  Lattices are built per image by sort/unique (no float atomics):
 * every output is bit-reproducible.  Images whose lattice keys would not fit 64 bits give IRN_ERR_ARG.
 *
 * irn_crf_filter: the permutohedral filter alone (densecrf Permutohedral::init + compute).
 *   feat dev fp32 [n][d] (1 <= d <= 5), in / out dev fp32 [n][channels];
 *   n_vertices (host, may be NULL) receives the lattice size M; keys_dev (dev int32 [M][d], vertices in
 *   ascending lexicographic key order) and nbr_dev (dev int32 [d+1][M][2], blur neighbours n1 / n2 along
 *   each axis, -1 = none) are written when not NULL; allocate them for M <= n*(d+1).
 *   SYNCHRONISES the stream (it reads M back).  workspace: irn_crf_filter_workspace_bytes(n, d, channels).
 * irn_crf_inference_label: one CRF.  rgb dev uint8 [h][w][3], labels dev int32 [h][w] in [0, n_labels);
 *   q_dev (dev fp32 [n_labels][h][w], may be NULL) and labels_out_dev (dev int32 [h][w], argmax of Q,
 *   first maximum) out.  n_labels <= 32.
 * irn_crf_ir_label: step/cam_to_ir_label.py for one image.  high_res dev fp32 [k][h][w], keys dev int64
 *   [k] (0-based class ids); the fg / bg seeds are argmax([thr, high_res]) for both thresholds, both CRFs
 *   run as one filter over 2*(k+1) channels on the shared lattices, and conf dev uint8 [h][w] receives
 *   fg (0 = background, else key+1), 255 where fg is background, 0 where fg and bg both are.  k == 0
 *   writes zeros and needs no workspace (ws may be NULL).
 * workspace of both: irn_crf_workspace_bytes(h, w, n_labels) (n_labels = k+1 for irn_crf_ir_label);
 *   0 = unsupported size.
 * irn_crf_label_sweep: the CRF label maps of one image at t_count thresholds (step/tune_ir_label.py).
 *   thres HOST fp32 [t_count], 1 <= t_count <= IRN_CRF_MAX_SWEEP, strictly ascending, no NaN.  Plane i
 *   of planes dev uint8 [t_count][h][w] is the CRF seeded with argmax([thres[i], high_res]) (strict >,
 *   the first class wins: the seeds of irn_crf_ir_label), its argmax taken through the keys: 0 =
 *   background, else keys[c]+1.  It is what irn_crf_ir_label computes for thres[i] as fg or as bg
 *   threshold, bit for bit: conf(fg, bg) = plane_fg, 255 where plane_fg == 0, 0 where plane_bg == 0
 *   too.  Features, both lattices and the normalisations are built once per call; the mean field runs
 *   over the thresholds in chunks of max(1, 64 / (k+1)) CRFs, so one filter pass carries at most 64
 *   channels (what irn_crf_ir_label carries at k = 31), and a CRF's result does not depend on its
 *   chunk.  k == 0 writes zeros and needs no workspace.  k + 1 <= 32.  Bad arguments (t_count, the
 *   thresholds, k, the image size, null pointers) give IRN_ERR_ARG before any device work, a short
 *   workspace IRN_ERR_STATE.  Nothing synchronises.
 *   workspace: irn_crf_sweep_workspace_bytes(h, w, n_labels = k+1, t_count) (0 = unsupported): at most
 *   irn_crf_workspace_bytes(h, w, 32) + 4 * t_count * h * w bytes (+ alignment); the lattice value
 *   arrays do not grow with t_count.
 * irn_crf_score_sweep: the CRF seeded with SCORES instead of labels (make_sem_seg_labels
 *   --sem_seg_crf_iters, tune_sem_seg).  scores dev fp32 [c][h][w] (the rw_up of irn_label_epilogue),
 *   thres HOST fp32 [t_count], 1 <= t_count <= IRN_CRF_MAX_SWEEP, strictly ascending, each >= 1e-5, no
 *   NaN.  CRF i has l = c+1 labels with -U = log(max(s, 1e-5)), s = [thres[i], scores]; a pixel with a
 *   NaN score has s' = 1 at its first NaN channel and 1e-5 at every other label.  Pairwise terms,
 *   iterations and softmax are those above.  Plane i of planes dev uint8 [t_count][h][w] is the first
 *   maximum of Q through the keys (0 = background, else keys[j]+1); q_dev (dev fp32
 *   [t_count][c+1][h][w], may be NULL) receives Q.  Lattices are built once per call, the thresholds
 *   run in chunks of max(1, 64 / (c+1)) CRFs and a plane does not depend on its chunk.  c == 0 writes
 *   zeros (Q = 1) and needs no workspace.  c + 1 <= 32.  Bad arguments give IRN_ERR_ARG before any
 *   device work, a short workspace IRN_ERR_STATE.  Nothing synchronises.
 *   workspace: irn_crf_score_sweep_workspace_bytes(h, w, n_labels = c+1, t_count) (0 = unsupported).
 * irn_crf_prob: the CRF seeded with PROBABILITIES (infer_sem_seg --seg_crf_iters).  prob dev
 *   fp32 [l][h][w], 2 <= l <= 32 (the prob of irn_seg_fuse): -U_i = log(max(p_i, 1e-5)); a pixel with a NaN
 *   has s' = 1 at its first NaN channel and 1e-5 at every other one (irn_crf_score_sweep's rule).
 *   Pairwise terms, the t iterations and the softmax are those above.  labels dev uint8 [h][w] is the
 *   first maximum of Q, the label index itself; q_dev (dev fp32 [l][h][w], may be NULL) receives Q.
 *   t == 0 gives the arg-max of the clipped, normalised prob.  Bad arguments give IRN_ERR_ARG before any
 *   device work, a short workspace IRN_ERR_STATE.  Nothing synchronises.
 *   workspace: irn_crf_prob_workspace_bytes(h, w, l) (0 = unsupported, l outside 2..32 included).
 * ------------------------------------------------------------------------------------------- */
#define IRN_CRF_MAX_SWEEP 16
size_t irn_crf_filter_workspace_bytes(int n, int d, int channels);
int irn_crf_filter(const float *feat_dev, int n, int d, const float *in_dev, int channels, float *out_dev,
                   int32_t *n_vertices, int32_t *keys_dev, int32_t *nbr_dev, void *ws, size_t ws_bytes, void *stream);
size_t irn_crf_workspace_bytes(int h, int w, int n_labels);
int irn_crf_inference_label(const uint8_t *rgb_dev, const int32_t *labels_dev, int h, int w, int n_labels, int t,
                            float gt_prob, float *q_dev, int32_t *labels_out_dev, void *ws, size_t ws_bytes,
                            void *stream);
int irn_crf_ir_label(const uint8_t *rgb_dev, const float *high_res_dev, const int64_t *keys_dev, int k, int h, int w,
                     float fg_thres, float bg_thres, int t, float gt_prob, uint8_t *conf_dev, void *ws,
                     size_t ws_bytes, void *stream);
size_t irn_crf_sweep_workspace_bytes(int h, int w, int n_labels, int t_count);
int irn_crf_label_sweep(const uint8_t *rgb_dev, const float *high_res_dev, const int64_t *keys_dev, int k, int h, int w,
                        const float *thres, int t_count, int t, float gt_prob, uint8_t *planes_dev, void *ws,
                        size_t ws_bytes, void *stream);
size_t irn_crf_score_sweep_workspace_bytes(int h, int w, int n_labels, int t_count);
int irn_crf_score_sweep(const uint8_t *rgb_dev, const float *scores_dev, const int64_t *keys_dev, int c, int h, int w,
                        const float *thres, int t_count, int t, uint8_t *planes_dev, float *q_dev, void *ws,
                        size_t ws_bytes, void *stream);
size_t irn_crf_prob_workspace_bytes(int h, int w, int l);
int irn_crf_prob(const uint8_t *rgb_dev, const float *prob_dev, int l, int h, int w, int t, uint8_t *labels_dev, float *q_dev,
                 void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Evaluation counts  (replace the chainercv counting behind step/eval_cam.py:10-20,
 *                     step/eval_sem_seg.py:10-17 and step/eval_ins_seg.py:21-22)
 * Every output is an int64 count in caller-owned device memory that each call ADDS into, so one
 * accumulator can stay on the device for a whole split; integer counts are exact and independent
 * of launch order and block count.  n_classes (nc below) = classes including the background,
 * 2 <= nc <= IRN_EVAL_MAX_CLASSES; the usual value is IRN_EVAL_CLASSES (VOC12's 21), and one kernel
 * serves every count.  GT values are 0..nc-1, or 255 (void: not in a confusion row, but
 * counted in `void` when it is not NULL, so the caller can reproduce the size chainercv's growing
 * matrix reaches).  A value outside its documented range (GT nc..254, a NaN CAM, a class key outside
 * 0..nc-2, a prediction or plane value above nc-1, unsorted thresholds, an instance id above g) is
 * skipped and counted in `bad_dev` (int64 [1]).  nc outside its range, or more than nc-1 planes (k)
 * per image, gives IRN_ERR_ARG before any device work.  Nothing synchronises.
 * The cap is 80 foreground classes because the per-workgroup LDS tables are sized by it ((nc+1)*nc
 * uint32 bins, 26.6 KB at nc = 81); labels stay uint8 with 255 = void.
 *
 * irn_cam_confusion: step/eval_cam.py for one image at T thresholds in one pass.  high_res dev fp32
 *   [k][h][w] (0 <= k <= nc-1; may be NULL when k == 0), keys dev int64 [k] (0-based classes), gt dev
 *   uint8 [h][w], thres dev fp32 [t] (ascending, 1 <= t <= IRN_EVAL_MAX_THRES).  Per pixel, with m the
 *   max over the k planes and c the first plane that reaches it, the prediction at threshold i is 0 if
 *   k == 0 or m <= thres[i], else keys[c] + 1 (= argmax of [thres[i], high_res] through the padded
 *   keys).  hist dev int64 [nc+1][nc][t+1] receives the pixel at [row][keys[c]+1][j], j = number of
 *   thresholds < m (row nc = GT 255; k == 0: column 0, j = 0).
 * irn_cam_confusion_reduce: hist -> conf dev int64 [t][nc][nc] (row = GT, column = prediction) and,
 *   when not NULL, void dev int64 [t][nc] (predictions at GT-255 pixels); adds into both.
 * irn_label_confusion: step/eval_sem_seg.py.  pred, gt dev uint8 [h][w]; pred 255 reads as
 *   pred_255_as when that is in 0..nc-1 (< 0: 255 is out of range).  conf dev int64 [nc][nc],
 *   void dev int64 [nc] (may be NULL).
 * irn_mask_overlap: the mask_iou counts of step/eval_ins_seg.py.  masks dev uint8 [n][h][w] (nonzero =
 *   in the mask; may be NULL when n == 0), inst dev uint8 [h][w] (0 = no instance, 1..g = instance).
 *   inter dev int64 [n][g] (pixels in mask i and instance j+1), area_pred dev int64 [n], area_gt dev
 *   int64 [g]; n == 0 and g == 0 are valid (the arrays of size 0 may be NULL).
 * irn_ir_label_confusion: step/cam_to_ir_label.py:36-39 + the confusion count for every (fg, bg) pair of
 *   a threshold grid, from the planes of irn_crf_label_sweep; no IR label map is written.  planes dev
 *   uint8 [t_count][h][w] (1 <= t_count <= IRN_CRF_MAX_SWEEP; values 0..nc-1), fg_idx HOST int32 [f] and
 *   bg_idx HOST int32 [b] (1 <= f, b <= 16; plane numbers in [0, t_count), repeats allowed), gt dev uint8
 *   [h][w].  Per pixel and pair, with fgv = planes[fg_idx[i]] and bgv = planes[bg_idx[j]], the label is
 *   fgv if fgv != 0, else 0 if bgv == 0, else 255, and the pixel is one count in hist dev int64
 *   [f][b][nc+1][nc+1] at [i][j][row][col]: row = GT 0..nc-1 or nc for GT 255, col = label 0..nc-1 or nc
 *   for 255.  A GT of nc..254, or a value above nc-1 in ANY of the t_count planes, skips the pixel for
 *   every pair and counts once in bad.  It needs f*(nc+1)*nc + f*b*(nc+1) words of LDS per workgroup and
 *   runs the fg axis in as many launches as that takes (one for 16 x 16 at nc = 21, eight at nc = 81); the
 *   histogram does not depend on the grouping.  Bad arguments give IRN_ERR_ARG before any device work.
 * ------------------------------------------------------------------------------------------- */
#define IRN_EVAL_CLASSES 21
#define IRN_EVAL_MAX_CLASSES 81
#define IRN_EVAL_MAX_THRES 256
int irn_cam_confusion(const float *high_res_dev, const int64_t *keys_dev, int k, const uint8_t *gt_dev, int h, int w,
                      const float *thres_dev, int t, int n_classes, int64_t *hist_dev, int64_t *bad_dev, void *stream);
int irn_cam_confusion_reduce(const int64_t *hist_dev, int t, int n_classes, int64_t *conf_dev, int64_t *void_dev,
                             void *stream);
int irn_label_confusion(const uint8_t *pred_dev, const uint8_t *gt_dev, int h, int w, int pred_255_as, int n_classes,
                        int64_t *conf_dev, int64_t *void_dev, int64_t *bad_dev, void *stream);
int irn_mask_overlap(const uint8_t *masks_dev, int n, const uint8_t *inst_dev, int g, int h, int w,
                     int64_t *inter_dev, int64_t *area_pred_dev, int64_t *area_gt_dev, int64_t *bad_dev,
                     void *stream);
int irn_ir_label_confusion(const uint8_t *planes_dev, int t_count, const int32_t *fg_idx, int f, const int32_t *bg_idx,
                           int b, const uint8_t *gt_dev, int h, int w, int n_classes, int64_t *hist_dev, int64_t *bad_dev,
                           void *stream);

/* ---------------------------------------------------------------------------------------------
 * Boundary counts  (Boundary IoU, Cheng et al., CVPR 2021, and its detection form Boundary AP.  The
 *                   reference has no such code: these replace the per-class / per-instance cv2.erode
 *                   loop of the published measure; the definition is DESIGN.md "Boundary IoU")
 * band(L, d) of a uint8 map L[h][w]: 1 at (y, x) iff the square window |dy| <= d, |dx| <= d around it
 * leaves the image or holds a byte other than L[y][x]; for every value c that is (L == c) minus its
 * erosion by a 3x3 kernel, d times, behind a one-pixel zero border.  All 256 bytes are labels, 254 and
 * 255 included.  1 <= d <= IRN_BAND_MAX_D; the caller computes d per image
 * (max(1, round(ratio * sqrt(h*h + w*w)))).  Integers only; counts are int64 that every call ADDS into,
 * `bad` and n_classes (nc) are those of the evaluation counts above.  Null pointers, d or nc outside
 * their ranges and non-positive sizes give IRN_ERR_ARG before any device work; nothing synchronises.
 *
 * irn_label_band: band dev uint8 [h][w] = band(map, d), written as 0 / 1.
 * irn_label_boundary_counts: pred, gt dev uint8 [h][w]; pred 255 reads as pred_255_as first (as for
 *   irn_label_confusion).  With P = band(pred, d), G = band(gt, d) (GT 255, void, is a label there) and
 *   valid = gt != 255, counts dev int64 [nc][3] receives per class c
 *     [c][0] #{valid & P & G & pred == c & gt == c}   [c][1] #{valid & P & pred == c}   [c][2] #{G & gt == c}
 *   A pixel whose pred (after the mapping) is above nc-1 or whose gt is nc..254 goes to bad and into no count.
 * irn_mask_boundary_overlap: masks dev uint8 [n][h][w] (nonzero = in the mask, each banded on its own as a
 *   two-valued map, the band kept where the mask is set), inst dev uint8 [h][w] (0 = none, 1..g), as for
 *   irn_mask_overlap.  inst_band dev uint8 [h][w] is caller-owned scratch the call fills with band(inst, d).
 *   inter_b dev int64 [n][g] (pixels in mask i's band and in instance j+1's band), band_pred dev int64 [n],
 *   band_gt dev int64 [g]; instance ids above g are counted in bad, once per pixel.  Sizes of 0 as for
 *   irn_mask_overlap.
 * ------------------------------------------------------------------------------------------- */
#define IRN_BAND_MAX_D 64
int irn_label_band(const uint8_t *map_dev, int h, int w, int d, uint8_t *band_dev, void *stream);
int irn_label_boundary_counts(const uint8_t *pred_dev, const uint8_t *gt_dev, int h, int w, int d, int pred_255_as,
                              int n_classes, int64_t *counts_dev, int64_t *bad_dev, void *stream);
int irn_mask_boundary_overlap(const uint8_t *masks_dev, int n, const uint8_t *inst_dev, uint8_t *inst_band_dev, int g, int h,
                              int w, int d, int64_t *inter_b_dev, int64_t *band_pred_dev, int64_t *band_gt_dev,
                              int64_t *bad_dev, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Label threshold sweep  (step/make_sem_seg_labels.py:43-49 + step/eval_sem_seg.py:10-17 at T values
 * of sem_seg_bg_thres in one pass; no label map and no [c,out_h,out_w] tensor is written).
 * Images, sizes, keys and scratch (n_images * 4 bytes) as for irn_label_epilogue; keys are required
 * and c <= nc-1, nc = n_classes as for irn_cam_confusion (usually IRN_EVAL_CLASSES), GT and key ranges
 * likewise.  gt_dev[i]: dev uint8 [out_h][out_w], 255 = void, ANY alignment (a batch's maps may be
 * packed back to back).  thres dev fp32 [t], ascending, 1 <= t <= IRN_EVAL_MAX_THRES.
 * Per output pixel, with v_c the score irn_label_epilogue compares (x4 bilinear upsample of channel
 * c divided by the image's global maximum): if some v_c is NaN, c* is the first such channel and
 * j = t (the epilogue, like torch.argmax, takes a NaN for the maximum: the pixel is keys[c*]+1 at
 * every threshold); otherwise c* is the first channel that reaches the maximum m and j the number
 * of thresholds < m (thres[i] == m is background: the epilogue compares with a strict >).  The
 * pixel is one count in hist dev int64 [nc+1][nc][t+1] at [row][keys[c*]+1][j] — the layout of
 * irn_cam_confusion, so irn_cam_confusion_reduce turns hist into the T confusion matrices, each
 * equal to irn_label_confusion of the labels irn_label_epilogue writes at that threshold.
 * hist and bad (int64 [1]) are added into; GT nc..254 and a key outside 0..nc-2 are skipped and
 * counted per pixel, a NaN or descending threshold once per call.  Nothing synchronises.
 * An image has (t+1)*(nc+1)*c bins and a workgroup counts them in passes of at most 15 360 (60 KiB of
 * LDS), so 80 channels at 256 thresholds take 110 passes per 4096 pixels where 20 channels take 8.
 * ------------------------------------------------------------------------------------------- */
int irn_label_sweep_confusion(int n_images, const float *const *rw_dev, const int32_t *c, const int32_t *h,
                              const int32_t *w, const int32_t *out_h, const int32_t *out_w,
                              const int64_t *const *keys_dev, const uint8_t *const *gt_dev,
                              const float *thres_dev, int t, int n_classes, int64_t *hist_dev, int64_t *bad_dev,
                              void *scratch_dev, void *stream);

/* ---------------------------------------------------------------------------------------------
 * COCO mask encoding  (replaces the pycococreatortools / pycocotools arithmetic behind
 *                      step/make_cocoann.py:38-46: per mask a run-length code, an area and a box)
 * masks dev uint8 [n][h][w], row-major, nonzero = in the mask (what make_ins_seg_labels writes and
 * irn_mask_overlap takes).  The code is pycocotools' rleEncode: pixels in COLUMN-major order
 * (j = x*h + y); counts[0] is the length of the leading run of zeros (0 when pixel (0,0) is set),
 * then runs of ones and zeros alternate and the counts of a mask sum to h*w (an empty mask is the
 * single count h*w, a full one [0, h*w]).  area = number of nonzero pixels; bbox = [x0, y0, width,
 * height] of the nonzero pixels, [0,0,0,0] for an empty mask (= rleArea, rleToBbox).
 * The number of counts depends on the data, so the work is two calls on the same inputs and scratch:
 *
 * irn_mask_rle_count: n_runs dev int32 [n] (counts of every mask), area dev int64 [n], bbox dev
 *   int32 [n][4]; all three are written, not added into.  Nothing synchronises: the caller reads
 *   n_runs (one transfer for the whole call), forms offsets = exclusive scan of n_runs and sizes
 *   counts.
 * irn_mask_rle_emit: offsets dev int64 [n+1]; counts dev uint32 [offsets[n]] receives the finished
 *   run lengths of every mask, mask i at offsets[i].  A count that would fall outside
 *   [offsets[i], offsets[i+1]) is not written.  Nothing synchronises.  Must follow _count on the
 *   same stream with the scratch untouched in between.
 * scratch: irn_mask_rle_scratch_bytes(n, h, w) bytes of caller-owned device memory (0 = bad
 *   argument, or n == 0).
 * n == 0 is valid (every array may then be NULL).  1 <= h, w and h*w < 2^31 - 1.  Integer
 * arithmetic with one writer per output word: bit-reproducible.
 * ------------------------------------------------------------------------------------------- */
size_t irn_mask_rle_scratch_bytes(int n, int h, int w);
int irn_mask_rle_count(const uint8_t *masks_dev, int n, int h, int w, int32_t *n_runs_dev, int64_t *area_dev,
                       int32_t *bbox_dev, void *scratch_dev, void *stream);
int irn_mask_rle_emit(const uint8_t *masks_dev, int n, int h, int w, const int64_t *offsets_dev,
                      uint32_t *counts_dev, void *scratch_dev, void *stream);

/* ---------------------------------------------------------------------------------------------
 * COCO mask polygons  (replaces pycococreatortools.create_annotation_info(..., tolerance=0) behind
 *                      step/make_cocoann.py:43-44: per mask a list of polygons)
 * masks as above.  The polygons are the boundary of the mask along pixel edges, not skimage's
 * contours: vertex (x, y), 0 <= x <= w, 0 <= y <= h, is the top-left corner of pixel (x, y) (the
 * coordinates of bbox).  Every side of a mask pixel whose neighbour across it is not in the mask is a
 * directed unit edge with the mask on its right (top +x, right +y, bottom -x, left -y); an edge's
 * successor is, at its head vertex, the right turn if that edge exists, else straight on, else the
 * left turn.  The cycles of that map are the loops: a loop with a positive shoelace sum is the outer
 * boundary of one 4-connected component, one with a negative sum a hole.  Outer loops are emitted,
 * holes are counted.  A loop is its corners (the vertices where the direction changes), starting at
 * its smallest vertex in (y, x) order, which it leaves in +x; a mask's loops come in the (y, x)
 * order of their start vertices, masks in order.  Three calls on one stream, the scratch untouched
 * in between, the caller reading one small array after each of the first two:
 *
 * irn_mask_polygon_edges: edge_offsets dev int32 [n+1], the boundary edges before every mask
 *   ([n] = all of them).  The caller reads it: n_edges = edge_offsets[n], max_mask_edges = the
 *   largest difference (the number of pointer-jumping rounds follows from it).
 * irn_mask_polygon_count: n_loops, n_holes, n_vertices dev int32 [n] (outer loops, holes, corners of
 *   the outer loops of every mask), written, not added into.  Given a smaller n_edges or
 *   max_mask_edges than the masks have, it writes wrong numbers and nothing outside its buffers.
 * irn_mask_polygon_emit: loop_sizes dev int32 [loops_room] (corners per outer loop) and xy dev int32
 *   [xy_room][2] (the corners).  An element beyond loops_room or xy_room is not written.
 * scratch: irn_mask_polygon_scratch_bytes(n, h, w) bytes for _edges and _count;
 *   irn_mask_polygon_trace_scratch_bytes(n_edges) bytes (53 per edge) for _count and _emit, NULL when
 *   n_edges == 0.  0 = bad argument, or nothing to do.
 * Nothing synchronises.  8 + 2 * R launches with R = ceil(log2(max_mask_edges)) made even; no
 * kernel waits for another workgroup or follows a chain.  n == 0 is valid.  1 <= h, w,
 * h*w < 2^31 - 1 and 2*n*(h+1)*(w+1) < 2^31.  Integers only, one writer per output word.
 * ------------------------------------------------------------------------------------------- */
size_t irn_mask_polygon_scratch_bytes(int n, int h, int w);
size_t irn_mask_polygon_trace_scratch_bytes(int n_edges);
int irn_mask_polygon_edges(const uint8_t *masks_dev, int n, int h, int w, int32_t *edge_offsets_dev,
                           void *scratch_dev, void *stream);
int irn_mask_polygon_count(const uint8_t *masks_dev, int n, int h, int w, const int32_t *edge_offsets_dev,
                           int n_edges, int max_mask_edges, int32_t *n_loops_dev, int32_t *n_holes_dev,
                           int32_t *n_vertices_dev, void *scratch_dev, void *trace_scratch_dev, void *stream);
int irn_mask_polygon_emit(int n_edges, int32_t *loop_sizes_dev, int64_t loops_room, int32_t *xy_dev,
                          int64_t xy_room, void *trace_scratch_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* IRN_HIP_H */
