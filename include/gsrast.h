/*
 * gsrast.h -- C ABI of the MI355X-native differentiable Gaussian rasterizer (libgsrast.so).
 *
 * Drop-in boundary for the reference's native rasterizer.  The reference binds an un-vendored
 * CUDA/C++ torch extension `diff_gaussian_rasterization._C` (/root/reference/.gitmodules:4-6)
 * through `GaussianRasterizer(...)(...)` at /root/reference/gaussian_renderer/__init__.py:51,85-93
 * (import at :14).  Each entry point below names the upstream native function it replaces
 * (upstream signatures restated in SURVEY.md §8b):
 *
 *   gs_forward_preprocess + gs_forward_render  <-  _C.rasterize_gaussians(...)
 *       (upstream runs both halves in one call with resize callbacks for its three scratch
 *        buffers; here the caller sizes the binning buffer from the returned num_rendered, so no
 *        callback into the host language is needed.  gs_rasterize_forward() is the one-call
 *        variant with the upstream-style allocator callback.)
 *   gs_backward                                <-  _C.rasterize_gaussians_backward(...)
 *   gs_backward_accumulate                     <-  same, adding into caller gradient buffers
 *                                                  (multi-view gradient accumulation; the
 *                                                  reference's `param.grad += g` of autograd,
 *                                                  train.py:93, fused into the last kernel)
 *   gs_mark_visible                            <-  _C.mark_visible(...)
 *   gs_forward_preprocess_views                <-  (extension) the first half of K views' forwards
 *   gs_forward_bounded / gs_bounded_status     <-  (extension) _C.rasterize_gaussians with the
 *                                                  binning buffer sized ahead (no host wait,
 *                                                  HIP-graph capturable)
 *   gs_knn_mean_dist2                          <-  simple_knn._C.distCUDA2(points)
 *                                                  (/root/reference/scene/gaussian_model.py:20,134)
 *   gs_ssim_forward / gs_ssim_backward         <-  utils.loss_utils.ssim(img1, img2)
 *                                                  (/root/reference/utils/loss_utils.py:33-60,
 *                                                   called at train.py:92)
 *   gs_photometric_loss_forward / _backward    <-  train.py:91-92 (l1_loss + ssim, lambda_dssim)
 *   gs_adam_step(_activated)                   <-  torch.optim.Adam.step() of GaussianModel
 *                                                  (/root/reference/scene/gaussian_model.py:163)
 *   gs_densify_stats                           <-  train.py:115-116 / gaussian_model.py:405-407
 *   gs_densify_classify / _split_stds / _emit  <-  GaussianModel.densify_and_prune
 *                                                  (gaussian_model.py:391-403)
 *   gs_activate_forward / gs_activate_backward <-  GaussianModel.get_features / get_opacity /
 *                                                  get_scaling / get_rotation (gaussian_model.py:95-115)
 *
 * Conventions
 *   - Every pointer argument is a DEVICE pointer (HBM of the current HIP device) unless its name
 *     ends in `_host`.  Arrays are dense row-major fp32 unless stated.  Optional inputs are NULL.
 *   - viewmatrix / projmatrix are the 4x4 `world_view_transform` / `full_proj_transform` tensors
 *     of /root/reference/scene/cameras.py:54-56 (row-vector convention), flattened row-major.
 *   - The caller owns every buffer (the host framework's allocator); the library never allocates
 *     or frees device memory.  Buffers returned by forward must stay alive until backward.
 *   - stream: a hipStream_t; all work is enqueued on it.  gs_forward_preprocess synchronises the
 *     stream once to read num_rendered (as upstream does).
 *   - Return value: 0 on success, non-zero on error; gs_last_error() describes the last error of
 *     the calling thread.  With debug != 0 every kernel is followed by a stream synchronisation
 *     and an error check (upstream `debug` semantics).
 */
#ifndef GSRAST_H
#define GSRAST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSRAST_ABI_VERSION 17  /* v17: gs_geom_flags_offset, gs_forward_order_status, gs_set_row_waits; v16: gs_backward_gaussians_adam_stats (v15: gs_backward_gaussians_adam; v14: gs_forward_counted + gs_binning_layout_count) */

/* Aux render outputs (additive, same ABI version): gs_grad_buffer_bytes_aux, gs_forward_render_aux,
 * gs_backward_accumulate_aux. */
#define GSRAST_HAS_AUX 1

/* Skysphere background (additive, same ABI version): gs_sky_scratch_bytes, gs_sky_compose_forward,
 * gs_sky_compose_backward. */
#define GSRAST_HAS_SKY 1

/* The skysphere's view-matrix gradient (additive, same ABI version): gs_sky_camera_scratch_bytes,
 * gs_sky_compose_backward_camera. */
#define GSRAST_HAS_SKY_CAMERA 1

/* Camera gradients (additive, same ABI version): gs_camera_grad_scratch_bytes, gs_backward_camera. */
#define GSRAST_HAS_CAMERA_GRAD 1

/* Deferred aux backward (additive, same ABI version): gs_backward_render_aux (the per-tile half with
 * the aux outputs' gradients), gs_backward_gaussians_adam_stats_aux (the fused per-Gaussian half +
 * Adam with the inverse depth's chain into dL/dmeans3D). */
#define GSRAST_HAS_AUX_DEFERRED 1

/* Antialiasing, the opacity compensation of the 0.3 px^2 dilation (additive, same ABI version):
 * gs_forward_preprocess_aa, gs_backward_accumulate_aa, gs_backward_camera_aa. */
#define GSRAST_HAS_ANTIALIASING 1

/* Per-Gaussian contribution statistics of a rendered view (additive, same ABI version):
 * gs_contrib_scratch_bytes, gs_contrib_stats. */
#define GSRAST_HAS_CONTRIB 1

/* Per-Gaussian feature channels rendered through a view's tile lists, and their gradient (additive,
 * same ABI version): gs_feature_group_channels, gs_feature_scratch_bytes, gs_feature_forward,
 * gs_feature_backward. */
#define GSRAST_HAS_FEATURES 1

/* Absolute screen-space gradients for densification (additive, same ABI version):
 * gs_grad_buffer_bytes_absgrad, gs_backward_accumulate_absgrad. */
#define GSRAST_HAS_ABSGRAD 1

int gs_abi_version(void);
const char* gs_last_error(void);

/* ---- image-size limits ----
 * An image of W x H pixels is a grid of gx x gy tiles of 16 x 16 pixels, gx = ceil(W / 16),
 * gy = ceil(H / 16).  Every entry that takes an image size (image_width / image_height arguments and
 * the sizes inside gs_view_grad) refuses, before any device work and with a message in
 * gs_last_error, a size with
 *   gx > GS_MAX_GRID_DIM or gy > GS_MAX_GRID_DIM: a Gaussian's tile rectangle is kept as two 16-bit
 *     halves per axis (x0 | x1 << 16 with x1 <= gx, likewise y), so W, H <= 1,048,560;
 *   gx * gy > GS_MAX_TILES: a tile's rank in the backward's launch order is kept in 22 bits
 *     (bucket << 22 | rank, rank < gx * gy).  Every narrower use lies within that: the tile sort's
 *     keys (tile ids, at most 22 bits, three 8-bit-or-narrower passes), 32-bit tile and
 *     scheduling-word counts (2 gx gy + 513) and the render grids (4 waves per tile); pixel counts
 *     (at most 2^30) are 64-bit throughout.
 * The sizing queries gs_binning_buffer_bytes, gs_image_buffer_bytes and gs_binning_layout_count
 * return 0 for such a size (and leave the message in gs_last_error): no buffer fits it. */
#define GS_MAX_GRID_DIM 65535
#define GS_MAX_TILES (1 << 22)

/* ---- scratch sizing (bytes) ---- */
size_t gs_geom_buffer_bytes(int P);
size_t gs_binning_buffer_bytes(long long num_rendered, int image_width, int image_height);
size_t gs_image_buffer_bytes(int image_width, int image_height);
size_t gs_grad_buffer_bytes(long long num_rendered);
/* Grad scratch of gs_backward_accumulate_aux: the records of gs_grad_buffer_bytes(num_rendered), then
 * one float per instance slot (dL/d(1/z) of the instance) and one float per Gaussian (their sums). */
size_t gs_grad_buffer_bytes_aux(long long num_rendered, int P);
/* Scratch of gs_backward_camera: one row of 28 doubles (the 27 sums and a zero) per 256 Gaussians,
 * 224 * max(1, ceil(P / 256)) bytes. */
size_t gs_camera_grad_scratch_bytes(int P);
/* Scratch of gs_contrib_stats: one 12-byte record per instance slot (rounded up to 256 bytes). */
size_t gs_contrib_scratch_bytes(long long num_rendered);
/* Scratch of gs_feature_backward: one record of gs_feature_group_channels() floats per instance slot
 * (rounded up to 256 bytes), reused by the channel groups in stream order. */
size_t gs_feature_scratch_bytes(long long num_rendered);
/* The instance count a binning buffer of `bytes` bytes is laid out for: the largest n with
 * gs_binning_buffer_bytes(n, W, H) <= bytes (every such n gives the same layout).  A buffer that
 * gs_forward_counted filled for `capacity` instances goes to the backward with this count in place
 * of num_rendered. */
long long gs_binning_layout_count(size_t bytes, int image_width, int image_height);

/* ---- forward, part 1: preprocess, cull, depth order, instance offsets ----
 * P Gaussians; D = active SH degree; M = SH coefficients per colour (stride of shs, 0 if none).
 * Exactly one of {shs, colors_precomp} and one of {(scales, rotations), cov3D_precomp} is non-NULL.
 * Writes radii_out[P] (int32) and the geometry buffer; returns num_rendered in *num_rendered_host.
 * Ref: upstream rasterize_gaussians (first half: preprocess, InclusiveSum, D2H of num_rendered). */
int gs_forward_preprocess(int P, int D, int M, const float* background, int image_width, int image_height,
                          const float* means3D, const float* shs, const float* colors_precomp,
                          const float* opacities, const float* scales, float scale_modifier,
                          const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                          const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                          int prefiltered, int* radii_out, void* geom_buffer, long long* num_rendered_host,
                          int debug, void* stream);

/* ---- forward, part 1 for K views of one set of Gaussians (1 <= K <= 8, view-parallel steps) ----
 * One preprocess launch projects every Gaussian into the K cameras (its inputs are read from HBM
 * once); view v's radii_out[v] and geom_buffer[v] hold exactly what gs_forward_preprocess writes
 * for that camera.  Then view v's depth order is enqueued on view_streams[v] (NULL: on `stream`)
 * after the preprocess, and one host wait reads the K num_rendered.  Per-view arguments are host
 * arrays of K entries.  Then gs_forward_render per view, on its stream. */
int gs_forward_preprocess_views(int K, int P, int D, int M, const float* const* background, const int* image_width,
                                const int* image_height, const float* means3D, const float* shs,
                                const float* colors_precomp, const float* opacities, const float* scales,
                                float scale_modifier, const float* rotations, const float* cov3D_precomp,
                                const float* const* viewmatrix, const float* const* projmatrix,
                                const float* const* campos, const float* tan_fovx, const float* tan_fovy,
                                int prefiltered, int* const* radii_out, void* const* geom_buffer,
                                long long* num_rendered_host, int debug, void* stream, void* const* view_streams);

/* ---- forward, part 2: duplicate, tile sort, ranges, compositing ----
 * out_color[3, H, W] fp32 (CHW).  binning_buffer >= gs_binning_buffer_bytes(num_rendered, W, H),
 * image_buffer >= gs_image_buffer_bytes(W, H). */
int gs_forward_render(int P, const float* background, int image_width, int image_height,
                      const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                      float tan_fovy, const int* radii, void* geom_buffer, long long num_rendered,
                      void* binning_buffer, void* image_buffer, float* out_color, int debug, void* stream);

/* ---- forward, part 2 with the aux outputs (GSRAST_HAS_AUX) ----
 * gs_forward_render plus two per-pixel by-products of the same tile walk, [H, W] fp32 each, either
 * may be NULL:
 *   out_alpha[p]    = 1.0f - final_T(p), the accumulated opacity (0 for a pixel no splat reaches);
 *   out_invdepth[p] = sum_i (1 / z_i) alpha_i T_i, the expected inverse depth, z_i the view depth of
 *                     splat i, composited in the form and order of a colour channel (exact mode:
 *                     acc + (c alpha) T; fast mode: fma(c, alpha T, acc)), with no background term.
 * alpha_i, T_i and every decision are those of the colour walk; everything else this call writes
 * (out_color, radii-dependent binning, the image buffer) is what gs_forward_render writes, bit for
 * bit.  With both NULL it is gs_forward_render.  Second half after gs_forward_preprocess or
 * gs_forward_preprocess_split. */
int gs_forward_render_aux(int P, const float* background, int image_width, int image_height,
                          const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                          float tan_fovy, const int* radii, void* geom_buffer, long long num_rendered,
                          void* binning_buffer, void* image_buffer, float* out_color, float* out_invdepth,
                          float* out_alpha, int debug, void* stream);

/* ---- forward in one call without a host wait (bounded binning buffer) ----
 * Both halves of gs_forward_preprocess + gs_forward_render, enqueued without reading num_rendered
 * back: the caller sizes binning_buffer for `capacity` instances (gs_binning_buffer_bytes(capacity,
 * W, H)) and passes capacity wherever num_rendered goes afterwards (gs_backward*: num_rendered and
 * gs_grad_buffer_bytes).  The instance count on the device drives every kernel, so outputs are
 * bit-identical to the two-call forward whenever the count fits.  A view with more instances than
 * `capacity` (or a prefiltered cull, or a timed-out look-back) leaves a sticky per-device flag, its
 * image and gradients invalid (zero records, nothing composited, every access in bounds): the next
 * gs_forward_bounded fails with the message, and gs_bounded_status reads / clears it.  Nothing
 * here synchronises, records events or allocates, so a step of bounded forwards and their backwards
 * can be captured into a HIP graph.  shs_rest: split SH rows as gs_forward_preprocess_split
 * (shs = features_dc), or NULL. */
int gs_forward_bounded(int P, int D, int M, const float* background, int image_width, int image_height,
                       const float* means3D, const float* shs, const float* shs_rest, const float* colors_precomp,
                       const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                       const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                       const float* campos, float tan_fovx, float tan_fovy, int prefiltered, int* radii_out,
                       void* geom_buffer, long long capacity, void* binning_buffer, void* image_buffer,
                       float* out_color, int debug, void* stream);
/* ---- forward in one call, count read back at the end (ABI 14) ----
 * _C.rasterize_gaussians' eager path without the mid-call host wait of gs_forward_preprocess: the
 * caller sizes binning_buffer for an estimate `capacity` (gs_binning_buffer_bytes(capacity, W, H)),
 * every launch is queued, then the call waits for the instance count -- stored into pinned memory by
 * the first depth-sort launch, so by then normally long written -- and returns it in
 * *num_rendered_host (exact, as upstream's num_rendered).
 *   0: the count fitted.  The binning buffer is laid out for `capacity` instances: the backward takes
 *      gs_binning_layout_count(its bytes, W, H) (= capacity) where it takes num_rendered.
 *   2 (GS_COUNT_SHORT): the count exceeds `capacity`; nothing was composited.  radii_out and
 *      geom_buffer are complete: gs_forward_render with a binning buffer for *num_rendered_host
 *      finishes the forward exactly as the two-call path does.
 *   1: error (gs_last_error()), as gs_forward_preprocess.
 * shs_rest: split SH rows as gs_forward_preprocess_split (shs = features_dc), or NULL. */
#define GS_COUNT_SHORT 2
int gs_forward_counted(int P, int D, int M, const float* background, int image_width, int image_height,
                       const float* means3D, const float* shs, const float* shs_rest, const float* colors_precomp,
                       const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                       const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                       const float* campos, float tan_fovx, float tan_fovy, int prefiltered, int* radii_out,
                       void* geom_buffer, long long capacity, void* binning_buffer, void* image_buffer,
                       float* out_color, long long* num_rendered_host, int debug, void* stream);
/* The bounded forms of the two-call forward: gs_forward_preprocess_views without the readback
 * (capacity: K binning capacities; nothing waits), then gs_forward_render_bounded per view with
 * that view's capacity in place of num_rendered.  Same sticky status as gs_forward_bounded. */
int gs_forward_preprocess_views_bounded(int K, int P, int D, int M, const float* const* background,
                                        const int* image_width, const int* image_height, const float* means3D,
                                        const float* shs, const float* colors_precomp, const float* opacities,
                                        const float* scales, float scale_modifier, const float* rotations,
                                        const float* cov3D_precomp, const float* const* viewmatrix,
                                        const float* const* projmatrix, const float* const* campos,
                                        const float* tan_fovx, const float* tan_fovy, int prefiltered,
                                        int* const* radii_out, void* const* geom_buffer, const long long* capacity,
                                        int debug, void* stream, void* const* view_streams);
int gs_forward_render_bounded(int P, const float* background, int image_width, int image_height,
                              const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                              float tan_fovy, const int* radii, void* geom_buffer, long long capacity,
                              void* binning_buffer, void* image_buffer, float* out_color, int debug, void* stream);
/* Flags (*flags: 1 prefiltered cull, 4 look-back timeout, 8 / 16 more instances than 2^31 - 1 /
 * than the capacity) that bounded forwards left on the current device since the last call, with the
 * instance count of a view that raised them (*instances); clears them.  Returns non-zero (message in
 * gs_last_error) when a flag is set.  Only forwards whose kernels have run are seen: call it after
 * a synchronisation point to cover every forward before it. */
int gs_bounded_status(unsigned* flags, long long* instances);
/* (ABI v17) Byte offset, inside a geometry buffer laid out for P Gaussians, of the 32-bit word
 * holding that view's forward error flags (the bits above; 0 for a valid view).  Every kernel of
 * the forward that records an error stores it there, and the backward's record sums and the fused
 * backward + Adam read it (an invalid view adds nothing / is skipped).  A caller copies the word
 * out stream-ordered behind the forward to decide, at its next sync, whether that view's update
 * happened (gs_train_step: the fused step's step counts). */
size_t gs_geom_flags_offset(int P);
/* (ABI v17) The ordering flags of every forward queued on the current device whose render has been
 * queued (read-back forwards: a look-back wait of their sorts that timed out): waits for their
 * render kernels, takes the flags (each forward is reported once) and returns non-zero with the
 * message in gs_last_error when one timed out.  Without this call the next forward or backward
 * reports them; a caller that has already seen a view's flags word name ERR_LOOKBACK consumes the
 * report here, in its own call. */
int gs_forward_order_status(void);
/* (ABI v17) Row waits for the next forward preprocess of the calling thread (any forward entry
 * point: counted, two-call, bounded, split, or the K-view gs_forward_preprocess_views): chunk k
 * covers the Gaussian rows [bounds[k], bounds[k + 1]) (bounds[0] == 0, increasing) and `events[k]`
 * is a hipEvent_t recorded when those rows' inputs are ready (null: none).  The preprocess then
 * launches in row chunks, each behind hipStreamWaitEvent on its chunk's event, so it starts on the
 * first rows while later rows are still being written on another stream -- the all-gather of a
 * sharded optimizer step (gs_view_parallel.ShardedAdam: parameters updated by row chunk).  Outputs
 * are those of the whole-grid launch.  The waits are consumed by that preprocess; n = 0 clears
 * them.  This mirrors no upstream entry point (upstream has no optimizer sharding). */
int gs_set_row_waits(int n, const int* bounds, void* const* events);

/* ---- the binning of K prepared views at once (ABI v11) ----
 * After gs_forward_preprocess_views(_bounded): duplicate + tile sort + tile ranges of all K views as
 * one set of launches on `stream` (each view's count on the device bounds its part), then each view
 * stream waits for them.  Each kind of buffer (geometry, binning, image) must be K slices of one
 * allocation, one stride apart; every binning slice sized for the largest num_rendered[v]
 * (gs_binning_buffer_bytes(max, W, H)), which is then the num_rendered of every view afterwards
 * (gs_forward_render_binned, backward, gs_grad_buffer_bytes).  All views share W x H. */
int gs_forward_bin_views(int K, int P, int image_width, int image_height, void* const* geom_buffer,
                         const long long* num_rendered, void* const* binning_buffer, void* const* image_buffer,
                         int debug, void* stream, void* const* view_streams);
/* The compositing of one binned view (gs_forward_render without its binning); bounded: the view
 * came from gs_forward_preprocess_views_bounded (flags to the sticky status). */
int gs_forward_render_binned(int P, const float* background, int image_width, int image_height,
                             const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                             float tan_fovy, void* geom_buffer, long long num_rendered, void* binning_buffer,
                             void* image_buffer, float* out_color, int bounded, int debug, void* stream);

/* ---- one-call forward with an upstream-style allocator callback ----
 * alloc(ctx, which, bytes) returns a device pointer of >= bytes (which: 0 geometry, 1 binning,
 * 2 image) that stays valid until backward.  Returns num_rendered (>= 0) or -1 on error. */
typedef void* (*gs_alloc_fn)(void* ctx, int which, size_t bytes);
long long gs_rasterize_forward(int P, int D, int M, const float* background, int image_width, int image_height,
                               const float* means3D, const float* shs, const float* colors_precomp,
                               const float* opacities, const float* scales, float scale_modifier,
                               const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                               const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                               int prefiltered, float* out_color, int* radii_out, gs_alloc_fn alloc,
                               void* alloc_ctx, void** geom_out, void** binning_out, void** image_out, int debug,
                               void* stream);

/* ---- backward ----
 * dL_dout_color[3, H, W].  grad_buffer >= gs_grad_buffer_bytes(num_rendered) (scratch).
 * Outputs (P rows each): dL_dmeans2D[P,3] (gradient w.r.t. the NDC projected mean; column 2 = 0),
 * dL_dcolors[P,3], dL_dopacity[P,1], dL_dmeans3D[P,3], dL_dcov3D[P,6], dL_dsh[P,M,3],
 * dL_dscales[P,3], dL_drotations[P,4].  dL_dcolors, dL_dcov3D, dL_dsh, dL_dscales and
 * dL_drotations may be NULL when the matching input was not given (they are then not computed).
 * With shs given, dL_dsh is required ("dL_dsh is required with SHs"): the SH colours' dependence on
 * the view direction is part of dL_dmeans3D and is formed together with dL_dsh.
 * Ref: upstream rasterize_gaussians_backward. */
int gs_backward(int P, int D, int M, const float* background, int image_width, int image_height,
                const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                float tan_fovy, const int* radii, const void* geom_buffer, long long num_rendered,
                const void* binning_buffer, const void* image_buffer, const float* dL_dout_color,
                void* grad_buffer, float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity,
                float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations,
                int debug, void* stream);

/* ---- backward, accumulating ----
 * Same arguments and outputs as gs_backward; bit k of `accumulate` (GS_ACC_*) makes output k
 * ADDED to the buffer's current contents (fp32 `old + new`, as autograd's in-place `grad += g`)
 * instead of overwriting it.  Used to sum several views' gradients into one flat gradient
 * bucket with no extra pass over it (view-parallel training).
 * wait_event (hipEvent_t or NULL): the stream waits for it after the per-tile work and before the
 * kernel that writes / adds the gradient outputs, so views rendered on two streams can share one
 * bucket: their forward, sort and tile backward overlap, only the bucket updates are ordered. */
#define GS_ACC_MEANS2D 1u
#define GS_ACC_COLORS 2u
#define GS_ACC_OPACITY 4u
#define GS_ACC_MEANS3D 8u
#define GS_ACC_COV3D 16u
#define GS_ACC_SH 32u
#define GS_ACC_SCALES 64u
#define GS_ACC_ROTATIONS 128u
int gs_backward_accumulate(int P, int D, int M, const float* background, int image_width, int image_height,
                           const float* means3D, const float* shs, const float* colors_precomp,
                           const float* opacities, const float* scales, float scale_modifier,
                           const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                           const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                           const int* radii, const void* geom_buffer, long long num_rendered,
                           const void* binning_buffer, const void* image_buffer, const float* dL_dout_color,
                           void* grad_buffer, float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity,
                           float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales,
                           float* dL_drotations, unsigned accumulate, void* wait_event, int debug, void* stream);

/* ---- backward with the aux outputs' gradients (GSRAST_HAS_AUX) ----
 * gs_backward_accumulate for a forward of gs_forward_render_aux: shs_rest as in gs_forward_bounded
 * (NULL, or the split rows with shs = features_dc), and dL_dout_invdepth / dL_dout_alpha [H, W], either
 * may be NULL (zero).  grad_buffer >= gs_grad_buffer_bytes_aux(num_rendered, P).  Alpha enters the
 * walk as a colour channel of colour 0 and background -1, the inverse depth as one of colour 1 / z_i
 * and background 0; its per-Gaussian sum s9 = dL/d(1 / z_i) gives dL/dz_i = -s9 / z_i^2, which a small
 * kernel adds into dL_dmeans3D (fp32 old + new) along (view[2], view[6], view[10]) after the kernel
 * that writes the gradients.  Same `accumulate` bits and wait_event rule.  With both aux gradients
 * NULL it runs exactly gs_backward_accumulate (/ _split): same launches, same bits. */
int gs_backward_accumulate_aux(int P, int D, int M, const float* background, int image_width, int image_height,
                               const float* means3D, const float* shs, const float* shs_rest,
                               const float* colors_precomp, const float* opacities, const float* scales,
                               float scale_modifier, const float* rotations, const float* cov3D_precomp,
                               const float* viewmatrix, const float* projmatrix, const float* campos,
                               float tan_fovx, float tan_fovy, const int* radii, const void* geom_buffer,
                               long long num_rendered, const void* binning_buffer, const void* image_buffer,
                               const float* dL_dout_color, const float* dL_dout_invdepth,
                               const float* dL_dout_alpha, void* grad_buffer, float* dL_dmeans2D,
                               float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D,
                               float* dL_dsh, float* dL_dscales, float* dL_drotations, unsigned accumulate,
                               void* wait_event, int debug, void* stream);

/* ---- camera gradients (GSRAST_HAS_CAMERA_GRAD, an extension beyond upstream) ----
 * dL/dviewmatrix [16], dL/dprojmatrix [16] and dL/dcampos [3] of one view, in the layout of the inputs
 * (row-vector convention, v[4 r + c]).  Call it on the same stream right after a gs_backward,
 * gs_backward_accumulate, _accumulate_aux or _accumulate_split of the same view, with that call's
 * scene, camera, geom_buffer and num_rendered: it reads the per-Gaussian record sums that call left
 * in the geometry buffer.  aux_grad_buffer / aux_valid: the grad_buffer of a gs_backward_accumulate_aux
 * whose aux gradients were not both NULL, and 1; otherwise NULL / 0 (the inverse-depth sums are then
 * not read).  scratch >= gs_camera_grad_scratch_bytes(P), 16-byte aligned, the caller's until the
 * stream has passed this call.
 *   dL/dview[r][k], k < 3: sum_i ph_r dL/dt_k + (r < 3) (J[0][k] dT0[r] + J[1][k] dT1[r]), ph = (mean, 1),
 *     t = ph view, T = J W: the adjoints of the cov2D and clamp rules of the backward (a clamped tx / ty
 *     is a constant, upstream's rule), plus ph_r (-s9 / z^2) for k = 2 with aux_valid; column 3 is 0.
 *   dL/dproj[r][c]: the NDC mean's gradient, columns 0, 1 and 3; column 2 is 0.
 *   dL/dcampos: minus the sum of the SH colour's dL/dmean term; 0 with colors_precomp.  dL_dcampos may
 *     be NULL (the SH rows are then not read; after an _accumulate_split, whose rows are two tensors,
 *     pass the concatenated rows as shs or NULL here).
 * The three are treated as independent inputs (the caller chains them to a pose); tan_fovx / tan_fovy
 * and the background get no gradient.  The sums run over the Gaussians with instances, in fp64 in a
 * fixed order without atomics: bitwise reproducible.  The outputs are written, not accumulated;
 * P == 0 writes zeros, and so does a view whose forward reported an invalid instance list.  Validation
 * (the scene / camera checks of gs_backward, then the pointers) comes before any device work. */
int gs_backward_camera(int P, int D, int M, const float* background, int image_width, int image_height,
                       const float* means3D, const float* shs, const float* colors_precomp,
                       const float* opacities, const float* scales, float scale_modifier,
                       const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                       const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                       const void* geom_buffer, long long num_rendered, const void* aux_grad_buffer,
                       int aux_valid, void* scratch, float* dL_dviewmatrix, float* dL_dprojmatrix,
                       float* dL_dcampos, int debug, void* stream);

/* ---- contribution statistics (GSRAST_HAS_CONTRIB, an extension beyond upstream) ----
 * How much each Gaussian takes part in one rendered view.  For Gaussian i and pixel p, "composited"
 * means what the colour forward of the same numerics mode decided: the entry's index in the tile's
 * list is below n_contrib[p], alpha = min(0.99, o G) >= 1/255, and in the exact mode power <= 0.
 * The entry that stops a pixel (T (1 - alpha) < 1e-4) is not composited, as upstream.
 * w_i(p) = alpha_i(p) T_i(p), one fp32 product; alpha and T are the floats of the colour walk of
 * that mode, and the T recurrence is the forward's own: T (1 - alpha) in the exact mode,
 * fma(-alpha, T, T) in the fast mode.  pixel_weights is an optional map m [H, W], fp32, m >= 0; NULL
 * means 1.  Three outputs of P entries each (any may be NULL, not all three):
 *     wsum[i]  = sum_p m_p w_i(p)                                            fp32
 *     wmax[i]  = max_p m_p w_i(p), 0 if the Gaussian is never composited     fp32
 *     count[i] = number of pixels where i is composited and m_p != 0         int32
 * A pixel with m_p = 0 adds nothing to any of the three.  Gaussians with radii == 0 get 0, 0, 0; a
 * view whose forward recorded an invalid instance list gives zeros, as the backward's record sums do.
 * Per (tile, Gaussian) instance the walk sums its at most 256 terms in fp32 in a fixed order; a
 * Gaussian's instances are summed in fp64 in slot order and rounded once.  No float atomics: the
 * results are bitwise reproducible.
 *
 * Call it after gs_forward_render or gs_forward_render_aux of a two-call forward (gs_forward_preprocess,
 * _split or _aa; an antialiased view's compensated opacity is already in its splat records), before or
 * after that view's backward: it leaves every word the backward reads as the backward itself would
 * write it.  It is not defined for the bounded forwards (gs_forward_bounded, gs_forward_counted,
 * gs_forward_render_bounded) nor for views prepared by gs_forward_preprocess_views / gs_forward_bin_views.
 * scratch >= gs_contrib_scratch_bytes(num_rendered), 4-byte aligned, the caller's until the kernels
 * have run.  accumulate != 0 combines with what the outputs hold: wsum = old + new (one fp32 add),
 * wmax = max(old, new), count = old + new; otherwise all P entries are written.  Checked before any
 * device work, in this order: P >= 0, a positive image size within the limits above, at least one
 * output ("missing output pointer"), num_rendered in range, and for P > 0 and num_rendered > 0 the
 * three buffers and the scratch ("missing buffer pointer").  P == 0 or num_rendered == 0 launches no
 * walk: the outputs are zero-filled, or left alone when accumulating.  The camera arguments and radii
 * keep the argument order of gs_backward_render; the kernels read the view's buffers only. */
int gs_contrib_stats(int P, int image_width, int image_height, const float* viewmatrix, const float* projmatrix,
                     const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                     const void* geom_buffer, long long num_rendered, const void* binning_buffer,
                     void* image_buffer, const float* pixel_weights, void* scratch, float* wsum, float* wmax,
                     int* count, int accumulate, int debug, void* stream);

/* ---- feature rendering (GSRAST_HAS_FEATURES, an extension beyond upstream) ----
 * Any per-Gaussian quantity as an image: features [P, C] (fp32, row-major) composited through the
 * finished tile lists of one rendered view.  "Composited", alpha_i(p), T_i(p), w_i(p) = alpha_i(p)
 * T_i(p) and the T recurrence are those of gs_contrib_stats above, for the current numerics mode.
 *     forward    out[c, p] = sum_i f_i[c] alpha_i(p) T_i(p)              out [C, H, W]
 *     backward   dL/df_i[c] = sum_p w_i(p) dL_dout[c, p]                 dL_dfeatures [P, C]
 * The forward composites every channel in the form and order of a colour channel: acc + (f alpha) T
 * in the exact mode, fma(f, alpha T, acc) in the fast mode, in list order; there is no background
 * term (compose out + (1 - alpha) bg with the aux alpha) and f is not clamped.  A channel holding a
 * view's colours therefore reproduces its image over a zero background bit for bit, and a channel of
 * 1 / depth its aux inverse depth.  Features must be finite.  Every pixel of out is written.
 * The backward is gs_contrib_stats' wsum with the weight map replaced by channel c of the gradient,
 * of either sign: per (tile, Gaussian) instance a lane adds its four pixels' terms g_c w (one fp32
 * product each) in slot order, the 64 lanes are summed in a fixed tree, a Gaussian's instances are
 * summed in fp64 in slot order and rounded once.  No float atomics: both directions are bitwise
 * reproducible.  The geometry is constant: neither entry differentiates alpha or T, and nothing flows
 * to means, scales, rotations or opacities.
 *
 * Channels are processed gs_feature_group_channels() at a time (one walk of the lists per group, the
 * last group padded with zero features whose channels are not written); any 1 <= C <=
 * GS_MAX_FEATURE_CHANNELS runs, a larger C is refused (render it in slices of columns).
 *
 * Call them after gs_forward_render or gs_forward_render_aux of a two-call forward (gs_forward_preprocess,
 * _split or _aa; an antialiased view's compensated opacity is already in its splat records), before or
 * after that view's backward: they leave every word the backward reads as the backward itself would
 * write it.  They are not defined for the bounded forwards (gs_forward_bounded, gs_forward_counted,
 * gs_forward_render_bounded) nor for views prepared by gs_forward_preprocess_views / gs_forward_bin_views.
 * A view whose forward recorded an invalid instance list gives zeros in both directions.  Gaussians
 * with radii == 0 get zero gradient rows.  One view may be rendered any number of times, with any C.
 * scratch >= gs_feature_scratch_bytes(num_rendered), 16-byte aligned, the caller's until the kernels
 * have run.  accumulate != 0 adds to what dL_dfeatures holds (one fp32 old + new per element);
 * otherwise all P rows are written.  Checked before any device work, in this order: P >= 0, C within
 * [1, GS_MAX_FEATURE_CHANNELS], a positive image size within the limits above, num_rendered in range,
 * the output ("missing output pointer"; dL_dfeatures only for P > 0), and for P > 0 and num_rendered > 0 the three buffers, the
 * input and the scratch ("missing buffer pointer").  P == 0 or num_rendered == 0 launches no walk: out
 * is zero-filled; dL_dfeatures is zero-filled, or left alone when accumulating.  The camera arguments
 * and radii keep the argument order of gs_backward_render; the kernels read the view's buffers only. */
#define GS_MAX_FEATURE_CHANNELS 1024
int gs_feature_group_channels(void);
int gs_feature_forward(int P, int C, int image_width, int image_height, const float* viewmatrix,
                       const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                       const int* radii, const void* geom_buffer, long long num_rendered,
                       const void* binning_buffer, void* image_buffer, const float* features, float* out,
                       int debug, void* stream);
int gs_feature_backward(int P, int C, int image_width, int image_height, const float* viewmatrix,
                        const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                        const int* radii, const void* geom_buffer, long long num_rendered,
                        const void* binning_buffer, void* image_buffer, const float* dL_dout, void* scratch,
                        float* dL_dfeatures, int accumulate, int debug, void* stream);

/* ---- antialiasing (GSRAST_HAS_ANTIALIASING; later upstream revisions' `antialiasing` switch) ----
 * Every projected splat is dilated by 0.3 px^2 (a = c00 + 0.3, b = c01, c = c11 + 0.3 from the EWA
 * covariance c00, c01, c11) and keeps its opacity, so a splat smaller than a pixel is drawn brighter
 * than it is.  With antialiasing != 0 the opacity is scaled by the Mip-Splatting 2D filter
 * normalisation, in fp32, one operation each, no contraction:
 *     D0 = c00 c11 - c01 c01;  D = a c - b b;  r = D0 / D;  s = sqrtf(fmaxf(0.000025f, r));  op' = op s
 * op' takes the opacity's place in the splat record and in the culling limit (a splat with
 * op' < 1/255 gets no instances, as a faint splat does); conic, radius, rectangle, radii, depth,
 * colour, the sorts and the render are unchanged.  The backward recomputes s from the same values:
 * with g = dL/dop', dL/dop = s g, and gr = r > 0.000025f ? op g / (2 s) : 0 enters the covariance
 * chain as dL/dc00 += gr (c11 D - D0 c) / D^2, dL/dc11 += gr (c00 D - D0 a) / D^2,
 * dL/dc01 += gr (-2 c01 (D - D0)) / D^2, ahead of the cov3D, mean, scale / rotation and camera terms.
 *
 * Each entry takes the arguments of the entry it extends plus `antialiasing`, and with
 * antialiasing == 0 it IS that entry: same launches, same bits, same validation order and messages.
 *   gs_forward_preprocess_aa   gs_forward_preprocess; follow it with gs_forward_render or _render_aux.
 *   gs_backward_accumulate_aa  gs_backward_accumulate_aux (aux gradients NULL: gs_backward_accumulate)
 *                              of a view whose forward was antialiased.  opacities is required
 *                              ("missing required input pointer"); shs_rest non-NULL is refused
 *                              (whole SH rows only).  The per-Gaussian kernel is the register-row one
 *                              at every degree.
 *   gs_backward_camera_aa      gs_backward_camera behind a gs_backward_accumulate_aa; opacities required.
 * The forward and the backward of one view must agree on the flag: the gradient is otherwise that of
 * another function.  The K-view preprocess, the bounded forwards, gs_backward_gaussians and the fused
 * backward + Adam have no antialiased form. */
int gs_forward_preprocess_aa(int P, int D, int M, const float* background, int image_width, int image_height,
                             const float* means3D, const float* shs, const float* colors_precomp,
                             const float* opacities, const float* scales, float scale_modifier,
                             const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                             const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                             int prefiltered, int* radii_out, void* geom_buffer, long long* num_rendered_host,
                             int debug, void* stream, int antialiasing);
int gs_backward_accumulate_aa(int P, int D, int M, const float* background, int image_width, int image_height,
                              const float* means3D, const float* shs, const float* shs_rest,
                              const float* colors_precomp, const float* opacities, const float* scales,
                              float scale_modifier, const float* rotations, const float* cov3D_precomp,
                              const float* viewmatrix, const float* projmatrix, const float* campos,
                              float tan_fovx, float tan_fovy, const int* radii, const void* geom_buffer,
                              long long num_rendered, const void* binning_buffer, const void* image_buffer,
                              const float* dL_dout_color, const float* dL_dout_invdepth,
                              const float* dL_dout_alpha, void* grad_buffer, float* dL_dmeans2D,
                              float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D,
                              float* dL_dsh, float* dL_dscales, float* dL_drotations, unsigned accumulate,
                              void* wait_event, int debug, void* stream, int antialiasing);
int gs_backward_camera_aa(int P, int D, int M, const float* background, int image_width, int image_height,
                          const float* means3D, const float* shs, const float* colors_precomp,
                          const float* opacities, const float* scales, float scale_modifier,
                          const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                          const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                          const void* geom_buffer, long long num_rendered, const void* aux_grad_buffer,
                          int aux_valid, void* scratch, float* dL_dviewmatrix, float* dL_dprojmatrix,
                          float* dL_dcampos, int debug, void* stream, int antialiasing);

/* ---- absolute screen-space gradients (GSRAST_HAS_ABSGRAD; AbsGS, gsplat's `absgrad`) ----
 * dL_dmeans2D is a signed sum over a splat's pixels; a large splat over fine detail is pulled both ways
 * and the sum cancels.  dL_dmeans2D_abs [P, 3] sums the per-pixel gradient's absolute value instead:
 * with q = o G dL/dalpha of a composited (pixel, Gaussian) pair (the backward walk's own decisions and
 * floats; a pair that is not composited adds exactly 0), d = mean2D - pixel and (cxx, cxy, cyy) the conic,
 *     abs[i][0] = 0.5 W sum_p |q (cxx dx + cxy dy)|,  abs[i][1] = 0.5 H sum_p |q (cxy dx + cyy dy)|,  abs[i][2] = 0
 * in the units of dL_dmeans2D[:, :2], whose argument is the signed sum of the same terms.  Evaluated as
 * |q| |2A dx + B dy| and |q| |B dx + 2C dy| with the staged falloff coefficients A = -log2(e) cxx / 2,
 * B = -log2(e) cxy, C = -log2(e) cyy / 2 (fp32: 2A = A + A, one product, one FMA, one FMA into the sum);
 * the lane's pixel slots are summed in slot order, the wave in a fixed tree once per tile entry, a
 * Gaussian's tile records in fp64 in slot order with one rounding, and the result is
 * (sum * ln 2) * (0.5 W) (resp. 0.5 H), two fp32 products in that order.  No float atomics: bitwise
 * reproducible.  Written, not accumulated; a Gaussian without instances, P == 0 and a view whose
 * forward reported an invalid instance list give zeros.
 *
 * gs_backward_accumulate_absgrad takes the arguments of gs_backward_accumulate_aa (those of
 * gs_backward_accumulate_aux plus `antialiasing`; shs_rest as in _aux, both aux gradients may be NULL,
 * antialiasing != 0 with shs_rest is refused as there) plus dL_dmeans2D_abs.  With aux gradients the
 * dL/dalpha in q is the aux walk's.  grad_buffer >= gs_grad_buffer_bytes_absgrad(num_rendered, P), which
 * keeps the layout of gs_grad_buffer_bytes_aux in front: gs_backward_camera (/ _aa) may follow with this
 * grad_buffer as its aux_grad_buffer, the record sums in the geometry buffer being what they were.
 * With dL_dmeans2D_abs == NULL it runs exactly gs_backward_accumulate_aa: same launches, same bits (and
 * the smaller grad_buffer of that call suffices). */
size_t gs_grad_buffer_bytes_absgrad(long long num_rendered, int P);
int gs_backward_accumulate_absgrad(int P, int D, int M, const float* background, int image_width, int image_height,
                                   const float* means3D, const float* shs, const float* shs_rest,
                                   const float* colors_precomp, const float* opacities, const float* scales,
                                   float scale_modifier, const float* rotations, const float* cov3D_precomp,
                                   const float* viewmatrix, const float* projmatrix, const float* campos,
                                   float tan_fovx, float tan_fovy, const int* radii, const void* geom_buffer,
                                   long long num_rendered, const void* binning_buffer, const void* image_buffer,
                                   const float* dL_dout_color, const float* dL_dout_invdepth,
                                   const float* dL_dout_alpha, void* grad_buffer, float* dL_dmeans2D,
                                   float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D,
                                   float* dL_dsh, float* dL_dscales, float* dL_drotations, unsigned accumulate,
                                   void* wait_event, int debug, void* stream, int antialiasing,
                                   float* dL_dmeans2D_abs);

/* ---- split SH rows (ABI v8, an extension beyond upstream) ----
 * render() concatenates GaussianModel's features_dc [P,1,3] and features_rest [P,M-1,3] into shs
 * (gaussian_model.py:99-103) once per iteration.  These variants read the two tensors in place:
 * shs_dc / shs_rest replace shs (SH colours only; M >= 2 is the coefficient count of the
 * concatenation); dL_dsh is still the [P,M,3] gradient of the concatenation (what
 * gs_adam_step_activated's features_dc / features_rest modes read).  Results are bit-identical to
 * gs_forward_preprocess / gs_backward_accumulate on the concatenated rows.  Every other argument as
 * there (no dL_dcolors: SH colours). */
int gs_forward_preprocess_split(int P, int D, int M, const float* background, int image_width, int image_height,
                                const float* means3D, const float* shs_dc, const float* shs_rest,
                                const float* opacities, const float* scales, float scale_modifier,
                                const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                                const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                                int prefiltered, int* radii_out, void* geom_buffer, long long* num_rendered,
                                int debug, void* stream);
int gs_backward_accumulate_split(int P, int D, int M, const float* background, int image_width, int image_height,
                                 const float* means3D, const float* shs_dc, const float* shs_rest,
                                 const float* opacities, const float* scales, float scale_modifier,
                                 const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                                 const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                                 const int* radii, const void* geom_buffer, long long num_rendered,
                                 const void* binning_buffer, const void* image_buffer, const float* dL_dout_color,
                                 void* grad_buffer, float* dL_dmeans2D, float* dL_dopacity, float* dL_dmeans3D,
                                 float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations,
                                 unsigned accumulate, void* wait_event, int debug, void* stream);

/* ---- backward, split for multi-view steps (an extension beyond upstream) ----
 * A view-parallel step renders K views of ONE set of Gaussians into one gradient bucket
 * (DESIGN.md §7).  gs_backward splits into its per-tile half and its per-Gaussian half, and the
 * per-Gaussian half runs once for all K views: every Gaussian's inputs are read and its gradient
 * row written (or added) once instead of K times.  The bucket receives exactly the fp32 sums that
 * K gs_backward_accumulate calls in view order produce.
 *
 * gs_backward_render: the tile pass and the per-Gaussian record sums of one view, kept in that
 *   view's geom_buffer (which must stay alive until gs_backward_gaussians has run), plus that
 *   view's dL_dmeans2D [P,3] (written, or added with GS_ACC_MEANS2D; NULL: not produced).
 *   Arguments as gs_backward.
 * gs_backward_gaussians: views[0 .. num_views) in order (any count: more than 8 run as several
 *   passes); outputs and `accumulate` bits as gs_backward_accumulate (dL_dmeans2D excluded);
 *   wait_event as gs_backward_accumulate.  As there, SH inputs without a dL_dsh output are refused
 *   ("dL_dsh is required with SHs") rather than answered with a dL_dmeans3D that lacks the SH
 *   colours' view-direction term; dL_dcolors, dL_dcov3D, dL_dscales and dL_drotations may be NULL. */
typedef struct gs_view_grad {
  const float* viewmatrix; /* 16, device (as the forward's) */
  const float* projmatrix; /* 16, device */
  const float* campos;     /* 3, device (NULL only without SHs) */
  float tan_fovx, tan_fovy;
  int image_width, image_height;
  const void* geom_buffer; /* that view's forward state, after its gs_backward_render */
} gs_view_grad;
int gs_backward_render(int P, int D, int M, const float* background, int image_width, int image_height,
                       const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                       float tan_fovy, const void* geom_buffer, long long num_rendered, const void* binning_buffer,
                       const void* image_buffer, const float* dL_dout_color, void* grad_buffer, float* dL_dmeans2D,
                       unsigned accumulate, int debug, void* stream);
/* gs_backward_render_aux (GSRAST_HAS_AUX_DEFERRED): gs_backward_render with the aux outputs'
 *   gradients dL_dout_invdepth / dL_dout_alpha ([H, W] each, either may be NULL).  Both NULL: exactly
 *   gs_backward_render's launches (invdepth_sums is not touched and may be NULL).  Otherwise
 *   grad_buffer >= gs_grad_buffer_bytes_aux(num_rendered, P) and invdepth_sums [P] (required) receives
 *   every visible Gaussian's sum of dL/d(1 / z_i) over its instances -- the input of the depth chain
 *   that gs_backward_gaussians_adam_stats_aux adds to dL/dmeans3D; the alpha gradient needs nothing
 *   per Gaussian (it is part of the record sums in geom_buffer).  With num_rendered == 0 nothing is
 *   summed and invdepth_sums must not be read (as in gs_backward_accumulate_aux). */
int gs_backward_render_aux(int P, int D, int M, const float* background, int image_width, int image_height,
                           const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                           float tan_fovy, const void* geom_buffer, long long num_rendered,
                           const void* binning_buffer, const void* image_buffer, const float* dL_dout_color,
                           const float* dL_dout_invdepth, const float* dL_dout_alpha, void* grad_buffer,
                           float* dL_dmeans2D, float* invdepth_sums, unsigned accumulate, int debug, void* stream);
int gs_backward_gaussians(int P, int D, int M, const float* means3D, const float* shs, const float* colors_precomp,
                          const float* scales, float scale_modifier, const float* rotations,
                          const float* cov3D_precomp, int num_views, const gs_view_grad* views, float* dL_dcolors,
                          float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
                          float* dL_dscales, float* dL_drotations, unsigned accumulate, void* wait_event, int debug,
                          void* stream);

/* gs_backward_gaussians_range (ABI v9): gs_backward_gaussians for the Gaussians [first, first +
 *   count) of the P only (every pointer is the whole-array one; the views' geom buffers are laid
 *   out for P).  A view-parallel step runs the per-Gaussian half in Gaussian-range chunks and
 *   starts each chunk's gradient all-reduce as soon as that chunk is written (gs_view_parallel
 *   GradBucket chunks); the union of the chunks equals one whole-range call, bit for
 *   bit (every Gaussian's arithmetic is independent of the others). */
int gs_backward_gaussians_range(int P, int first, int count, int D, int M, const float* means3D, const float* shs,
                                const float* colors_precomp, const float* scales, float scale_modifier,
                                const float* rotations, const float* cov3D_precomp, int num_views,
                                const gs_view_grad* views, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D,
                                float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations,
                                unsigned accumulate, void* wait_event, int debug, void* stream);

/* ---- mark_visible: present[P] (uint8 0/1), near-plane test ---- */
int gs_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                    uint8_t* present, void* stream);

/* ---- simple-knn: mean squared distance to the 3 nearest other points ---- */
size_t gs_knn_scratch_bytes(int P);
int gs_knn_mean_dist2(int P, const float* points, float* out, void* scratch, void* stream);

/* ---- launched-kernel log (ABI v15, test support) ----
 * gs_debug_launch_log(enable): record the distinct kernels this library launches from now on (the
 *   initial state comes from GSRAST_LAUNCH_LOG=1); returns the previous state.
 * gs_debug_launched_kernels: the recorded kernels' mangled symbol names (the names of the code
 *   object's kernel descriptors without ".kd"), one per line; returns the text's length and copies it,
 *   NUL-terminated, when buf holds more than that.  tests/test_zz_kernel_coverage.py checks that every
 *   kernel of the code object is launched by some GPU test. */
int gs_debug_launch_log(int enable);
long long gs_debug_launched_kernels(char* buf, long long cap);

/* ---- numerics mode of the render loops (process-wide) ----
 * exact != 0: the render kernels evaluate exp2 with a deterministic polynomial that the CPU oracle
 * mirrors, so the whole forward is bit-identical to the oracle.  exact == 0 (default): the
 * hardware v_exp_f32 (<= 1 ulp); forward images / final_T then match the oracle within float
 * tolerance, with identical integer outputs except near the alpha / T thresholds (tests/
 * test_gpu_parity.py, fast-mode cases).  The initial mode comes from GSRAST_EXACT_EXP=1.
 * Returns the previous mode.  Set it between steps, not while a step is in flight. */
int gs_set_exact_exp(int exact);

/* ---- fused SSIM of the photometric loss  <-  utils/loss_utils.py:ssim (train.py:91-92) ----
 * img1, img2: [planes, H, W] fp32 (planes = images x channels), window11_host: the 11 float32
 * weights of loss_utils.gaussian(11, 1.5) (host memory).  Forward writes per-plane sums of the
 * SSIM map to plane_sum[planes] and the three per-pixel partials to dmaps[3, planes, H, W]
 * (kept for backward); partial has gs_ssim_partial_count(planes, H, W) floats.  Backward writes
 * dimg1 = scale[plane / channels] * dSSIM-sum/dimg1 (scale: device, one per image). */
size_t gs_ssim_partial_count(int planes, int H, int W);
int gs_ssim_forward(int planes, int H, int W, const float* window11_host, const float* img1, const float* img2,
                    float* dmaps, float* partial, float* plane_sum, void* stream);
int gs_ssim_backward(int planes, int channels, int H, int W, const float* window11_host, const float* img1,
                     const float* img2, const float* dmaps, const float* scale, float* dimg1, void* stream);

/* ---- fused photometric loss  <-  train.py:91-92
 *      loss = (1 - lambda) l1_loss(img, gt) + lambda (1 - ssim(img, gt))  (utils/loss_utils.py) ----
 * img, gt: [planes, H, W] fp32.  Forward: one SSIM pass that also sums |img - gt| per tile, then
 * one fixed-order fp64 reduction writing out3 = [loss, l1, ssim] (device floats, means over all
 * planes x H x W elements); dmaps[3, planes, H, W] as gs_ssim_forward; partial holds
 * 2 x gs_ssim_partial_count(planes, H, W) floats.  Backward: dimg = grad[0] x dloss/dimg (grad: the
 * loss's incoming gradient, one device float), the SSIM and L1 terms in one kernel. */
int gs_photometric_loss_forward(int planes, int H, int W, const float* window11_host, const float* img,
                                const float* gt, float lambda_dssim, float* dmaps, float* partial, float* out3,
                                void* stream);
int gs_photometric_loss_backward(int planes, int H, int W, const float* window11_host, const float* img,
                                 const float* gt, const float* dmaps, float lambda_dssim, const float* grad,
                                 float* dimg, void* stream);

/* ---- skysphere background (GSRAST_HAS_SKY, an extension beyond the reference) ----
 * A learnable equirectangular texture[3, Hs, Ws] (fp32 CHW, texel centres at half-integers) sampled
 * along every pixel's camera ray and composited behind the splats:
 *   out_image[c, y, x] = color[c, y, x] + (1 - alpha[y, x]) * sky_c(x, y).
 * Pixel (x, y), integer coordinates at pixel centres as in the rasterizer's projection:
 *   d_cam = (((2x + 1) / W - 1) tanfovx, ((2y + 1) / H - 1) tanfovy, 1),  d_i = sum_j V[i][j] d_cam_j
 *   (V = viewmatrix, the forward's device [4, 4]);  u = atan2(d.x, d.z) / 2pi + 0.5,
 *   v = acos(clamp(-d.y / |d|, -1, 1)) / pi (row 0 is world -y);  tx = u Ws - 0.5, ty = v Hs - 0.5;
 *   bilinear over columns floor(tx), floor(tx) + 1 (wrapping modulo Ws) and rows floor(ty),
 *   floor(ty) + 1 (clamped to [0, Hs - 1]).
 * Forward: color == NULL is a colour of 0, alpha == NULL an alpha of 0 (both NULL: the bare sky).
 * Backward, with g = dL_dimage[3, H, W] (dL/dcolor is g itself):
 *   dL_dalpha[y, x] = -sum_c g_c sky_c (NULL: not produced);
 *   dL_dtexture[c, texel] = sum over pixels of g_c (1 - alpha) w_texel (NULL: not produced), written
 *   (accumulate_texture 0) or added as fp32 old + new (1).  The sums are formed in 64-bit fixed point
 *   with integer atomics, so they are bit-identical from run to run; scratch holds
 *   gs_sky_scratch_bytes(Hs, Ws) bytes (16-byte aligned; needed only with dL_dtexture).
 * Nothing is kept between the two calls: the backward recomputes the rays. */
size_t gs_sky_scratch_bytes(int Hs, int Ws);
int gs_sky_compose_forward(int W, int H, const float* viewmatrix, float tanfovx, float tanfovy, int Hs, int Ws,
                           const float* texture, const float* color, const float* alpha, float* out_image,
                           void* stream);
int gs_sky_compose_backward(int W, int H, const float* viewmatrix, float tanfovx, float tanfovy, int Hs, int Ws,
                            const float* texture, const float* alpha, const float* dL_dimage, float* dL_dalpha,
                            float* dL_dtexture, int accumulate_texture, void* scratch, void* stream);

/* ---- the skysphere's view-matrix gradient (GSRAST_HAS_SKY_CAMERA) ----
 * gs_sky_compose_backward with one more output: dL_dviewmatrix[16], the row-major [4, 4] gradient of
 * the viewmatrix argument through the rays d_i = sum_j V[i][j] d_cam_j (the same row-vector
 * convention; the matrix is an independent input, the caller chains it to a pose).  With
 * gm_c = g_c (1 - alpha), rho^2 = d.x^2 + d.z^2, l^2 = rho^2 + d.y^2, a = sum_c gm_c [(t01 - t00) +
 * fy ((t11 - t10) - (t01 - t00))] (the sample's slope along fx) and b = sum_c gm_c (bot - top) (along
 * fy; 0 where the two rows clamp to one):
 *   dL/dd.x =  a (Ws / 2pi) d.z / rho^2 - b (Hs / pi) d.y d.x / (rho l^2)
 *   dL/dd.z = -a (Ws / 2pi) d.x / rho^2 - b (Hs / pi) d.y d.z / (rho l^2)
 *   dL/dd.y =  b (Hs / pi) rho / l^2
 *   dL_dviewmatrix[4 i + j] = sum over pixels of dL/dd_i d_cam_j   (i, j < 3)
 * floor carries no gradient.  Row 3 and column 3 are structural zeros (a sky at infinity does not see
 * the translation), written as such.  A pixel contributes exactly zero when 1 - alpha == 0, when
 * a == 0 and b == 0, and when rho^2 == 0 or one of its terms is not finite (the exact pole, a
 * degenerate matrix).  tanfovx / tanfovy get no gradient.
 * The sums are fp64 in a fixed order without float atomics (a row of doubles per 16 x 16 pixel block
 * in camera_scratch, one finishing workgroup over the rows in index order): bit-identical from run to
 * run.  The 16 floats are written (accumulate_view 0) or added as fp32 old + new (1).
 * camera_scratch holds gs_sky_camera_scratch_bytes(W, H) bytes (0 for a non-positive size; a multiple
 * of 16), 16-byte aligned, needed only with dL_dviewmatrix.  dL_dviewmatrix == NULL: the call is
 * gs_sky_compose_backward (same checks, launches and bits).  dL_dalpha and dL_dtexture may both be
 * NULL: no texture scratch is needed then.  All argument checks fail on the host. */
size_t gs_sky_camera_scratch_bytes(int W, int H);
int gs_sky_compose_backward_camera(int W, int H, const float* viewmatrix, float tanfovx, float tanfovy, int Hs, int Ws,
                                   const float* texture, const float* alpha, const float* dL_dimage, float* dL_dalpha,
                                   float* dL_dtexture, int accumulate_texture, void* scratch,
                                   float* dL_dviewmatrix /* [16] row-major, may be NULL */, int accumulate_view,
                                   void* camera_scratch, void* stream);

/* ---- fused Adam step  <-  torch.optim.Adam.step() of GaussianModel's optimizer
 *      (/root/reference/scene/gaussian_model.py:154-163, stepped at train.py:123-124) ----
 * count parameter tensors, each with its own lr / step (the reference has one tensor per param
 * group, per-group lr from the schedulers).  The pointer/size arrays are HOST arrays of DEVICE
 * pointers; each tensor is dense fp32 with numel elements and p, grad, exp_avg, exp_avg_sq of equal
 * size.  step[k] >= 1 is the step count AFTER this update (torch increments before updating).
 * lr / weight_decay / betas / eps are the Python doubles of the param groups (rounded to float on the
 * way to the device exactly where torch rounds them).  weight_decay_host may be NULL (all zero).
 * amsgrad is not supported (the reference never sets it). */
int gs_adam_step(int count, float* const* params_host, const float* const* grads_host, float* const* exp_avg_host,
                 float* const* exp_avg_sq_host, const long long* numel_host, const double* lr_host,
                 const long long* step_host, const double* weight_decay_host, double beta1, double beta2, double eps,
                 int maximize, void* stream);

/* gs_adam_step whose gradients are formed from the render() inputs' gradients (the adjoint of
 * gs_activate_forward, applied inside the update: the raw-parameter gradients are never stored).
 * grad_mode_host[k] per tensor, with grad_src_host[k] its source:
 *   0 plain: the tensor's own gradient;
 *   1 features_dc, 2 features_rest: rows of dL/dshs [P, sh_coeffs, 3] (coefficient 0 / 1..M-1);
 *   3 sigmoid (opacity): dL/dopacity * (1 - y) * y, y = sigmoid(p) of the raw value before the update;
 *   4 exp (scaling): dL/dscales * exp(p);
 *   5 normalize (rotation, rows of 4): the F.normalize adjoint of dL/drotations at q = p.
 * Same floats as gs_activate_backward followed by gs_adam_step. */
int gs_adam_step_activated(int count, float* const* params_host, const float* const* grad_src_host,
                           const int* grad_mode_host, int sh_coeffs, float* const* exp_avg_host,
                           float* const* exp_avg_sq_host, const long long* numel_host, const double* lr_host,
                           const long long* step_host, const double* weight_decay_host, double beta1, double beta2,
                           double eps, int maximize, void* stream);

/* gs_backward_gaussians_adam (ABI v15): one view's per-Gaussian backward half fused with the Adam
 * step of GaussianModel's six parameter groups (train.py:93 loss.backward() + train.py:123-124
 * optimizer.step() of one iteration, gaussian_model.py:154-163 groups; the opt-in fused train step
 * of gs_train_step).  Call after the view's gs_backward_render (its dL_dmeans2D, which the
 * densification statistics read, comes from there).  Same floats as gs_backward_accumulate_split
 * (accumulate 0) followed by gs_adam_step_activated in the modes plain / features_dc /
 * features_rest / sigmoid / exp / normalize: every Gaussian's parameters and moments are
 * bit-identical to that pair, and no gradient is stored.
 * M == 16 split SH rows (shs_dc / shs_rest 16-byte aligned), active degree D 0..3 (coefficients
 * past it get zero gradients, as in gs_backward_accumulate_split); scales /
 * rotations are the activated render() inputs the forward read, means3D is params_host[0].
 * params / exp_avg / exp_avg_sq: HOST arrays of 6 DEVICE pointers in group order xyz [P,3],
 * f_dc [P,1,3], f_rest [P,15,3], opacity [P,1], scaling [P,3], rotation [P,4] (raw parameters,
 * rotation 16-byte aligned); lr / step / weight_decay per group as gs_adam_step (weight_decay_host
 * may be NULL).  The kernel reads and writes f_dc, f_rest and rotation with 16-byte accesses: the
 * parameter, exp_avg and exp_avg_sq pointers of these three groups must all be 16-byte aligned, and
 * the call is refused before any launch otherwise (one message, naming the group); the other three
 * groups' tensors need only float alignment.  The Adam update runs in place while the kernel reads the parameters: nothing else
 * may read or write them on another stream until the call's work completes.  A view whose forward
 * recorded an error (its geometry buffer's flags: capacity overflow, look-back timeout, culled
 * prefiltered point) is not updated, so a caller may launch this before reading the forward's status
 * and keep its step counts unchanged when that raises. */
int gs_backward_gaussians_adam(int P, int D, int M, const float* means3D, const float* shs_dc, const float* shs_rest,
                               const float* scales, float scale_modifier, const float* rotations,
                               const gs_view_grad* view, float* const* params_host, float* const* exp_avg_host,
                               float* const* exp_avg_sq_host, const double* lr_host, const long long* step_host,
                               const double* weight_decay_host, double beta1, double beta2, double eps, int maximize,
                               int debug, void* stream);

/* gs_backward_gaussians_adam_stats (ABI v16): gs_backward_gaussians_adam plus the view's
 * densification statistics (train.py:115-116, gaussian_model.py:405-407, i.e. gs_densify_stats) in
 * the same pass: for every i with radii[i] > 0, max_radii2D[i] = max(max_radii2D[i], radii[i]),
 * grad_accum[i] += |grad2d[i * grad_stride + 0..1]|, denom[i] += 1 -- the same floats as
 * gs_densify_stats.  grad2d is the view's dL/dmeans2D (its gs_backward_render output, grad_stride
 * >= 2 floats per row), radii the forward's.  The five stats pointers are all given or all NULL (NULL:
 * exactly gs_backward_gaussians_adam).  A view whose forward recorded an error updates neither its
 * parameters nor its statistics. */
int gs_backward_gaussians_adam_stats(int P, int D, int M, const float* means3D, const float* shs_dc,
                                     const float* shs_rest, const float* scales, float scale_modifier,
                                     const float* rotations, const gs_view_grad* view, float* const* params_host,
                                     float* const* exp_avg_host, float* const* exp_avg_sq_host, const double* lr_host,
                                     const long long* step_host, const double* weight_decay_host, double beta1,
                                     double beta2, double eps, int maximize, const int* radii, const float* grad2d,
                                     int grad_stride, float* max_radii2D, float* grad_accum, float* denom, int debug,
                                     void* stream);

/* gs_backward_gaussians_adam_stats_aux (GSRAST_HAS_AUX_DEFERRED): gs_backward_gaussians_adam_stats
 * after a gs_backward_render_aux that was given an aux gradient.  invdepth_sums [P] is that call's
 * output: every Gaussian with instances gets -invdepth_sums[i] / z_i^2 * (view[2], view[6], view[10])
 * added to its dL/dmeans3D (z_i from the view's geometry buffer) before the Adam update -- the same
 * floats as gs_backward_accumulate_aux's depth chain followed by gs_adam_step_activated.
 * invdepth_sums NULL: exactly gs_backward_gaussians_adam_stats. */
int gs_backward_gaussians_adam_stats_aux(int P, int D, int M, const float* means3D, const float* shs_dc,
                                         const float* shs_rest, const float* scales, float scale_modifier,
                                         const float* rotations, const gs_view_grad* view,
                                         float* const* params_host, float* const* exp_avg_host,
                                         float* const* exp_avg_sq_host, const double* lr_host,
                                         const long long* step_host, const double* weight_decay_host, double beta1,
                                         double beta2, double eps, int maximize, const int* radii,
                                         const float* grad2d, int grad_stride, float* max_radii2D, float* grad_accum,
                                         float* denom, const float* invdepth_sums, int debug, void* stream);

/* ---- render() inputs from GaussianModel's raw parameters  <-  get_features / get_opacity /
 *      get_scaling / get_rotation (/root/reference/scene/gaussian_model.py:95-115, read at
 *      gaussian_renderer/__init__.py:53-80) ----
 * Forward: shs[P, 1 + sh_rest/3, 3] = cat(features_dc[P,1,3], features_rest[P,sh_rest/3,3]);
 * opacity[P] = sigmoid(opacity_raw); scales[P,3] = exp(scaling_raw);
 * rotations[P,4] = rotation_raw / max(|rotation_raw|, 1e-12).
 * Backward: the adjoints (any of the four dL_d* inputs may be NULL: its outputs are not written);
 * opacity / scales are the forward OUTPUTS, rotation_raw the forward input.  Rotation and shs
 * buffers must be 16-byte aligned.  shs == NULL (ABI v8): the SH rows are not concatenated (for the
 * split-SH rasterizer entries); features_dc / features_rest are then not read. */
int gs_activate_forward(int P, int sh_rest, const float* features_dc, const float* features_rest,
                        const float* opacity_raw, const float* scaling_raw, const float* rotation_raw, float* shs,
                        float* opacity, float* scales, float* rotations, void* stream);
int gs_activate_backward(int P, int sh_rest, const float* dL_dshs, const float* dL_dopacity, const float* dL_dscales,
                         const float* dL_drotations, const float* opacity, const float* scales,
                         const float* rotation_raw, float* dL_dfeatures_dc, float* dL_dfeatures_rest,
                         float* dL_dopacity_raw, float* dL_dscaling_raw, float* dL_drotation_raw, void* stream);

/* ---- densify_and_prune  <-  GaussianModel.densify_and_prune (/root/reference/scene/
 *      gaussian_model.py:391-403 with densify_and_clone :375-389, densify_and_split :348-373,
 *      prune_points :289-305, cat_tensors_to_optimizer :307-326), called at train.py:118-120 ----
 * Three steps with one host read in between (the caller allocates the new tensors):
 *  1. gs_densify_classify: per Gaussian flags[P] (u8) and per-block counts
 *     (block_counts: 4 * gs_densify_block_count(P) u32, scanned in place to block bases);
 *     totals[4] (device) = {kept originals, kept clones, split parents, kept split parents}.
 *     Scalars are the Python values of the reference call (grad_threshold = max_grad,
 *     pd_extent = percent_dense * extent, big_extent = 0.1 * extent, has_screen = bool(max_screen_size)).
 *  2. gs_densify_split_stds (totals copied to the host): stds[N * totals[2], 3] = exp(scaling) of the
 *     split parents in the reference's repeat order; the caller draws
 *     samples = torch.normal(mean=zeros, std=stds) exactly as gaussian_model.py:358-360 does.
 *  3. gs_densify_emit: writes the final rows (P' = totals[0] + totals[1] + N * totals[3]) of the six
 *     parameter tensors in order xyz, f_dc, f_rest, opacity, scaling, rotation (row widths
 *     3, 3, 3K, 1, 3, 4) and of their Adam moments (NULL entries: group without state).
 *     When P' == 0 (everything pruned) the entries of out_params_host / out_exp_avg_host /
 *     out_exp_avg_sq_host may be NULL (zero-row tensors have no storage): the call checks its other
 *     arguments as usual, launches nothing and returns 0.  With P' > 0 a NULL output of positive
 *     width is refused ("missing parameter pointer").  A relaxation within ABI v17: no entry point
 *     or argument changed. */
size_t gs_densify_block_count(int P);
int gs_densify_classify(int P, const float* grad_accum, const float* denom, const float* opacity_raw,
                        const float* scaling_raw, double grad_threshold, double pd_extent, double min_opacity,
                        double big_extent, int has_screen, double max_screen, int N, uint8_t* flags,
                        uint32_t* block_counts, uint32_t* totals, void* stream);
int gs_densify_split_stds(int P, int N, const uint32_t* totals_host, const uint8_t* flags,
                          const uint32_t* block_counts, const float* scaling_raw, float* stds, void* stream);
int gs_densify_emit(int P, int N, const uint32_t* totals_host, const uint8_t* flags, const uint32_t* block_counts,
                    const float* samples, const float* const* params_host, const float* const* exp_avg_host,
                    const float* const* exp_avg_sq_host, float* const* out_params_host,
                    float* const* out_exp_avg_host, float* const* out_exp_avg_sq_host, const int* widths_host,
                    void* stream);

/* ---- densification statistics  <-  train.py:115-116 + GaussianModel.add_densification_stats
 *      (/root/reference/scene/gaussian_model.py:405-407) ----
 * For every i with radii[i] > 0:  max_radii2D[i] = max(max_radii2D[i], radii[i]);
 * grad_accum[i] += |grad2d[i * grad_stride + 0..1]|_2;  denom[i] += 1.  (grad_accum, denom: [P, 1]) */
int gs_densify_stats(int P, const int* radii, const float* grad2d, int grad_stride, float* max_radii2D,
                     float* grad_accum, float* denom, void* stream);

/* ---- debug export of forward intermediates (tests) ----
 * Copies (device -> device) whichever outputs are non-NULL: point_list[num_rendered] (Gaussian ids
 * of the tile-sorted instance list), ranges[tiles*2] (u32), xy[P*2], conic_opacity[P*4],
 * rgb[P*3], depth[P], tiles_touched[P] (u32), final_T[H*W], n_contrib[H*W] (u32). */
int gs_debug_export(int P, int image_width, int image_height, long long num_rendered, const void* geom_buffer,
                    const void* binning_buffer, const void* image_buffer, uint32_t* point_list,
                    uint32_t* ranges, float* xy, float* conic_opacity, float* rgb, float* depth,
                    uint32_t* tiles_touched, float* final_T, uint32_t* n_contrib, void* stream);

/* ---- test hook: spin limit of the offsets scan's look-back waits (process-wide) ----
 * 0 makes every waiting workgroup time out at once: the forward must then fail with
 * "look-back wait timed out" (gs_forward_render).  Returns the previous limit (default 1 << 22). */
unsigned gs_debug_set_scan_spin_limit(unsigned limit);

/* ---- test hook: the packed two-pass tile sort (process-wide, default on) ----
 * 0 sends every binning through the (key, slot) pair sort and the key-reading range kernel; the
 * lists, ranges and everything after them are the same either way.  Returns the previous value.
 * gs_debug_tile_sort_packed_count: binnings that took the packed path since load. */
int gs_debug_set_tile_sort_packed(int on);
long long gs_debug_tile_sort_packed_count(void);

/* ---- test hook: eligibility of an SH layout for the K-view preprocess's LDS-staged row loader ----
 * 1 for rows of exactly M = (D + 1)^2 coefficients that are whole 16-B pieces (3 M a multiple of
 * 4) at a 16-B aligned `shs`, else 0.  A library built with -DGS_PREVIEWS_ROWS=1 launches
 * gs_forward_preprocess_views(_bounded) by it; the default build holds every layout's rows in
 * registers instead (csrc/gs_forward.hip).  No GPU call; `shs` is only inspected as an address. */
int gs_debug_sh_rows_staged(int D, int M, const void* shs);

/* ---- debug export of the raw tile-sorted instance slots (tests) ----
 * slots[num_rendered]: the depth-ordered instance slot of every entry of the tile-sorted list
 * (the backward writes entry k's gradient record at slots[k]); tile_cut[tiles]: 1 + the slot
 * of the last instance each tile's backward walk reaches (valid after a backward).  Within a
 * tile the slots must be strictly increasing (the record cut relies on it). */
int gs_debug_export_slots(int image_width, int image_height, long long num_rendered, const void* binning_buffer,
                          const void* image_buffer, uint32_t* slots, uint32_t* tile_cut, void* stream);

/* ---- per-kernel timing with HIP events on the launch stream (bench / profiling) ----
 * While enabled every launch is bracketed by a hipEvent pair.  gs_profile_collect() waits for the
 * recorded events and folds them into per-kernel totals; gs_profile_stat(i, ...) reads entry i
 * (returns 0 past the end). */
void gs_profile_enable(int on);
int gs_profile_collect(void);
void gs_profile_reset(void);
int gs_profile_stat(int i, char* name, int name_len, double* total_ms, long long* launches);

#ifdef __cplusplus
}
#endif
#endif /* GSRAST_H */
