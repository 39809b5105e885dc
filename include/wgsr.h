/*
 * wgsr.h -- C ABI of the MI355X-native WildGS Gaussian-splatting hot path.
 *
 * This is the drop-in boundary for the two native extensions WildGS-SLAM
 * loads on its mapping path:
 *
 *   diff_gaussian_rasterization._C  (empty submodule in the reference,
 *       .gitmodules:7-9; bound by the Python layer that
 *       thirdparty/gaussian_splatting/gaussian_renderer/__init__.py:15-18,
 *       58-74 and 130-141 imports)
 *   simple_knn._C.distCUDA2          (.gitmodules:10-12; called at
 *       thirdparty/gaussian_splatting/scene/gaussian_model.py:18,201-207)
 *
 * Each entry point below names the upstream `_C` function it replaces.  All
 * pointers are DEVICE pointers (HIP, gfx950) unless stated, all arrays are
 * contiguous fp32 (int32 where noted), and every launch goes on `stream`
 * (a hipStream_t; NULL = the null stream).  Scratch memory is obtained through
 * caller-supplied allocation callbacks -- the C analogue of upstream's
 * `std::function<char*(size_t)>` resize functors -- so the caller's allocator
 * (e.g. the torch caching allocator) owns every byte and the library keeps no
 * global device state.
 *
 * Return value: 0 on success, a WGSR_E* code otherwise; wgsr_last_error()
 * returns a thread-local message for the last failure.
 */
#ifndef WGSR_H
#define WGSR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WGSR_OK 0
#define WGSR_EINVAL 1   /* argument misuse (upstream: AT_ERROR / Exception) */
#define WGSR_EHIP 2     /* HIP runtime / launch failure                     */
#define WGSR_EALLOC 3   /* an allocation callback returned NULL             */

/* Returns a device pointer to at least `bytes` bytes, 256-byte aligned, that
 * stays valid until the caller releases it.  `bytes` may be 0.  Within one
 * library call a callback may be called twice for the same buffer (the
 * forward's binning buffer: a predicted size before its host wait, then the
 * exact size) only when the predicted size was too small: the library then
 * uses the pointer of the second call and has written nothing through the
 * first, which the callback may release or grow.  A large-enough prediction
 * is used as it is (no second call). */
typedef void* (*wgsr_alloc_fn)(void* ctx, size_t bytes);

/* The rasterisation inputs shared by forward and backward: the tensors and
 * scalars of upstream's rasterize_gaussians / rasterize_gaussians_backward
 * argument lists (GaussianRasterizationSettings + per-Gaussian tensors). */
typedef struct wgsr_raster_args {
  int P;                        /* number of Gaussians                        */
  int D;                        /* active SH degree (sh_degree)               */
  int M;                        /* stored SH coefficients per Gaussian        */
  int W, H;                     /* image_width, image_height                  */
  const float* bg;              /* [3]                                        */
  const float* means3D;         /* [P,3]                                      */
  const float* colors;          /* [P,3] colors_precomp, or NULL             */
  const float* opacities;       /* [P,1]                                      */
  const float* scales;          /* [P,3] or NULL (then cov3D_precomp)         */
  const float* rotations;       /* [P,4] (w,x,y,z) or NULL                    */
  const float* cov3D_precomp;   /* [P,6] or NULL                              */
  const float* shs;             /* [P,M,3] or NULL (then colors)              */
  const float* viewmatrix;      /* [4,4] world_view_transform (row-vector)    */
  const float* projmatrix;      /* [4,4] full_proj_transform                  */
  const float* projmatrix_raw;  /* [4,4] projection_matrix                    */
  const float* campos;          /* [3]  camera_center                         */
  float scale_modifier;
  float tan_fovx, tan_fovy;
  int prefiltered;              /* upstream: trap if a prefiltered point is culled */
  int debug;                    /* synchronise + check after every kernel     */
} wgsr_raster_args;

/* Replaces _C.rasterize_gaussians (forward).
 * Outputs (caller-allocated, fully written): out_color [3,H,W],
 * out_depth [1,H,W], out_opacity [1,H,W] (= 1 - T), radii [P] int32,
 * n_touched [P] int32.  Three state buffers are requested through the
 * callbacks (geometry ~ P, binning ~ num_rendered, image ~ H*W); the caller
 * must keep them for wgsr_rasterize_backward.  *num_rendered receives the
 * number of (Gaussian, tile) pairs.  One device->host read (num_rendered)
 * synchronises `stream`, as upstream does. */
int wgsr_rasterize_forward(const wgsr_raster_args* args,
                           wgsr_alloc_fn geom_alloc, wgsr_alloc_fn binning_alloc,
                           wgsr_alloc_fn image_alloc, void* alloc_ctx,
                           float* out_color, float* out_depth, float* out_opacity,
                           int32_t* radii, int32_t* n_touched, int64_t* num_rendered,
                           void* stream);

/* Capacity mode of wgsr_rasterize_forward (no upstream counterpart): the
 * same outputs with NO host synchronisation, so that a whole mapping
 * iteration can be captured in a HIP graph (wgsr/online.py).  The state
 * buffers are sized for `cap` (Gaussian, tile) rectangle pairs (upstream's
 * num_rendered bounds the exact and bin pairs); pass cap as num_rendered to
 * wgsr_rasterize_backward.  counts (device, 5 uint32): N_rect, N_exact,
 * N_bin (saturating), overflow (N_rect > cap), min(N_bin, cap).  After an
 * overflow the images are undefined and the backward writes zero gradients;
 * callers skip their optimizer step on counts[3] (wgsr_adam_step_dev).
 * Needs the default sort-bin configuration (WGSR_EINVAL otherwise) and
 * prefiltered = 0. */
int wgsr_rasterize_forward_cap(const wgsr_raster_args* args, int64_t cap,
                               wgsr_alloc_fn geom_alloc, wgsr_alloc_fn binning_alloc,
                               wgsr_alloc_fn image_alloc, void* alloc_ctx,
                               float* out_color, float* out_depth, float* out_opacity,
                               int32_t* radii, int32_t* n_touched, uint32_t* counts,
                               void* stream);
/* Bytes of the binning buffer wgsr_rasterize_forward_cap requests for `cap`. */
size_t wgsr_binning_bytes_cap(const wgsr_raster_args* args, int64_t cap);

/* Consistency check of a forward's tile lists (test and debug aid, no
 * upstream counterpart): for every tile, its [start, end) lies inside the
 * list region the forward sized from num_rendered (the capacity in capacity
 * mode) and matches its list length, every listed Gaussian id is < P, and no
 * pixel's last contributor lies beyond its tile's list.  Adds the number of
 * bad tiles, bad ids and bad pixels to bad[0..2] (device uint32 words, not
 * zeroed here).  Stream-ordered with no host wait, so it can sit inside a
 * captured graph between the forward and the backward. */
int wgsr_check_tile_lists(const wgsr_raster_args* args, int64_t num_rendered, const void* binning,
                          const void* image, uint32_t* bad, void* stream);

/* Replaces _C.rasterize_gaussians_backward.
 * Inputs: the forward's radii, state buffers and num_rendered; upstream
 * gradients dL_dcolor [3,H,W] and dL_ddepth [1,H,W].
 * Outputs (caller-allocated, fully written, zeros for culled Gaussians):
 * dL_dmeans2D [P,3] (w.r.t. NDC xy; z = 0), dL_dcolors [P,3],
 * dL_dopacity [P,1], dL_dmeans3D [P,3], dL_dcov3D [P,6], dL_dsh [P,M,3]
 * (NULL when M == 0), dL_dscales [P,3], dL_drotations [P,4],
 * dL_dtau [P,6] (per-Gaussian pose gradient, rho then theta).
 * A scratch buffer of ~48 bytes per rendered pair is requested through
 * `scratch_alloc`.  The binning buffer's per-pair flag bytes and the image
 * buffer's backward launch order are written (the same values on every
 * backward of one forward). */
int wgsr_rasterize_backward(const wgsr_raster_args* args, const int32_t* radii,
                            const void* geom_buffer, void* binning_buffer,
                            void* image_buffer, int64_t num_rendered,
                            const float* dL_dcolor, const float* dL_ddepth,
                            wgsr_alloc_fn scratch_alloc, void* alloc_ctx,
                            float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity,
                            float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
                            float* dL_dscales, float* dL_drotations, float* dL_dtau,
                            void* stream);

/* ---- view-sharded data-parallel backward ----------------
 * No upstream counterpart (the reference is single-GPU; its mapper renders
 * one keyframe view per step, src/mapper.py:1089-1170).  Splits
 * wgsr_rasterize_backward at the per-Gaussian screen-space partial sums so
 * ranks exchange 48 bytes per Gaussian per view instead of all-reducing the
 * 59-float parameter gradients (wgsr/dp.py). */
#define WGSR_VIEW_RECORD_FLOATS 12  /* g[10] (as k_gauss_bwd), radius, SH clamp bits */
#define WGSR_VIEW_CAMERA_FLOATS 64  /* view[16] proj[16] proj_raw[16] campos[3] tanx tany W H, pad */

/* Packs args' camera (viewmatrix, projmatrix, projmatrix_raw, campos,
 * tan_fovx/y, W, H) into one device row of WGSR_VIEW_CAMERA_FLOATS floats. */
int wgsr_pack_view_camera(const wgsr_raster_args* args, float* camera_row, void* stream);

/* First half of wgsr_rasterize_backward for one view: render backward, then
 * per Gaussian i < P_pad one record of WGSR_VIEW_RECORD_FLOATS floats in
 * records [P_pad, 12]: dL/dmean2D (NDC x, y), dL/dconic (3), dL/dopacity,
 * dL/dcolor (3), dL/ddepth, radius (float), SH clamp bits (float).  Rows of
 * culled Gaussians and rows >= P are zero (radius 0 = not visible). */
int wgsr_rasterize_backward_records(const wgsr_raster_args* args, const int32_t* radii,
                                    const void* geom_buffer, void* binning_buffer,
                                    void* image_buffer, int64_t num_rendered,
                                    const float* dL_dcolor, const float* dL_ddepth,
                                    wgsr_alloc_fn scratch_alloc, void* alloc_ctx, int P_pad,
                                    float* records, void* stream);

/* Number of pose-gradient partial rows wgsr_gauss_backward_views writes. */
int wgsr_gauss_backward_views_blocks(int lo, int hi);

/* Second half, for Gaussians [lo, hi) over n_views views: view v's camera is
 * row v of `cameras` [n_views, 64] and its records for the shard start at
 * records + v * record_view_stride (floats; row i - lo).  Writes rows
 * [lo, hi) of dL_dmeans3D [P,3], dL_dsh [P,M,3], dL_dopacity [P,1],
 * dL_dscales [P,3], dL_drotations [P,4] = the SUM over the views of what
 * wgsr_rasterize_backward returns per view.  tau_partials (or NULL):
 * [wgsr_gauss_backward_views_blocks(lo, hi)][n_views][6] per-block sums of
 * the pose gradient (rho, theta) per view.  stats (or NULL): [hi - lo][3] =
 * sum over views of ||dL/dmean2D[:2]||, number of views with radius > 0,
 * max radius (the reference's add_densification_stats inputs).  params uses
 * P, D, M, means3D, scales, rotations, shs, scale_modifier; cov3D_precomp is
 * not supported. */
int wgsr_gauss_backward_views(const wgsr_raster_args* params, int lo, int hi, int n_views,
                              const float* cameras, const float* records,
                              int64_t record_view_stride, float* dL_dmeans3D, float* dL_dsh,
                              float* dL_dopacity, float* dL_dscales, float* dL_drotations,
                              float* tau_partials, float* stats, void* stream);

/* ---- sparse view-sharded exchange (csrc/dp_sparse.hip, wgsr/dp.py) ----
 * Most visible Gaussians get no gradient from a view (their pixels saturate
 * before them), so ranks move only rows with a non-zero record / gradient.
 * No reference counterpart: this replaces the dense exchange behind
 * ViewShardedBackward, which stands in for the reference's per-view
 * optimiser.step() accumulation (mapper.py:1089-1219). */

/* Floats per packed gradient row: index, dL/dmeans3D (3), dL/dsh (3M),
 * dL/dopacity, dL/dscales (3), dL/drotations (4). */
int wgsr_sparse_grad_row_floats(int M);

/* 32-bit mask words per owner segment of S rows: ceil(S / 32). */
int64_t wgsr_sparse_mask_words(int64_t S);

/* records [P_pad, 12] of one view -> per owner o (segment [o S, (o+1) S)),
 * the rows with a non-zero partial sum compacted to packed + o S * 12, field
 * 10 replaced by the row's index inside the segment (uint32 bits).
 * counts[P_pad / S] (zeroed by the caller) receive the rows per owner; with
 * nzmask (zeroed, [P_pad / S][wgsr_sparse_mask_words(S)], may be null) bit j
 * of owner o's words is set for each packed row j.  Row order inside a
 * segment is unspecified. */
int wgsr_sparse_pack_records(const float* records, int64_t P_pad, int64_t S, uint32_t* counts,
                             float* packed, uint32_t* nzmask, void* stream);

/* uint32 words of one rank's block in the exchange's small all-gather:
 * WGSR_VIEW_CAMERA_FLOATS (the camera row's float bits) + world (rows sent to
 * each owner) + world x wgsr_sparse_mask_words(S) (non-zero row masks). */
int64_t wgsr_sparse_summary_block_words(int world, int64_t S);

/* blocks [world][wgsr_sparse_summary_block_words] (every rank's block,
 * gathered) -> summary [world * world + world]: count[v][o] (rows view v sends
 * owner o) then owner o's union row count (rows some view gives gradient);
 * offsets [world + 1]: exclusive prefix over v of count[v][rank] (where view
 * v's rows land in this rank's all_to_all output) and the total; cams
 * [world][WGSR_VIEW_CAMERA_FLOATS]. */
int wgsr_sparse_exchange_summary(const uint32_t* blocks, int world, int rank, int64_t S, uint32_t* summary,
                                 uint32_t* offsets, float* cams, void* stream);

/* Owner side: received [offsets[n_views]][12], view v's packed rows at
 * [offsets[v], offsets[v + 1]), scattered into records [n_views][S][12]
 * (zeroed by the caller) and mask[S] (zeroed) set for every received row.
 * keep_radius: keep the radius field already in `records`
 * (wgsr_sparse_fill_radius), else 1. */
int wgsr_sparse_unpack_records(const float* received, const uint32_t* offsets, int n_views, int64_t S,
                               int keep_radius, float* records, uint8_t* mask, void* stream);

/* records[j].radius = radii[j] for j < n (rows of WGSR_VIEW_RECORD_FLOATS). */
int wgsr_sparse_fill_radius(const float* radii, int64_t n, float* records, void* stream);

/* Gradient rows [lo, hi) whose mask[i - lo] is set -> packed rows of
 * wgsr_sparse_grad_row_floats(M) floats; *count (zeroed) = rows written. */
int wgsr_sparse_pack_grads(int64_t lo, int64_t hi, int M, const uint8_t* mask, const float* dL_dmeans3D,
                           const float* dL_dsh, const float* dL_dopacity, const float* dL_dscales,
                           const float* dL_drotations, uint32_t* count, float* packed, void* stream);

/* gathered: owner r's packed rows at gathered + r * block_stride floats,
 * counts[r] (<= cap) rows, indices into shard r (rows r S + index).  Scatters
 * every owner's rows except `rank`'s into the [P, ...] gradient tensors
 * (zeroed by the caller), or with clear != 0 writes zeros at those rows
 * (undoes an earlier call's scatter, so the tensors need no full re-zeroing). */
int wgsr_sparse_unpack_grads(const float* gathered, int64_t block_stride, const uint32_t* counts, int world,
                             int rank, int64_t cap, int64_t S, int64_t P, int M, float* dL_dmeans3D,
                             float* dL_dsh, float* dL_dopacity, float* dL_dscales, float* dL_drotations,
                             int clear, void* stream);

/* ---- the mapping iteration around the path ----
 * src/mapper.py:1083-1219 per iteration, as fused launches (csrc/mapping.hip;
 * driven by wgsr/mapping.py).  Partial sums are one float (or float pair) per
 * workgroup of wgsr_map_blocks(n) workgroups; callers reduce them in order. */
int wgsr_map_blocks(int64_t n);

/* GaussianModel.get_opacity / get_scaling / get_rotation (gaussian_model.py:
 * sigmoid, exp, F.normalize(eps 1e-12)) of the raw [P,1] / [P,3] / [P,4]
 * parameters, plus iso_partials[wgsr_map_blocks(P)] = per-block sums of
 * sum_k |exp(s_k) - mean_k exp(s_k)| (mapper.py:1167-1169). */
int wgsr_gaussian_activate(int P, const float* opacity_raw, const float* scaling_raw,
                           const float* rotation_raw, float* opacity, float* scales,
                           float* rotations, float* iso_partials, void* stream);

/* Chain rule of wgsr_gaussian_activate back to the raw parameters; adds the
 * gradient of iso_weight * sum |exp(s) - mean_row exp(s)| (iso_weight = 10 /
 * (3 P) for the reference's 10 * isotropic_loss.mean()). */
int wgsr_gaussian_activate_backward(int P, const float* opacity_raw, const float* scaling_raw,
                                    const float* rotation_raw, const float* dL_dopacity,
                                    const float* dL_dscales, const float* dL_drotations,
                                    float iso_weight, float* dL_dopacity_raw,
                                    float* dL_dscaling_raw, float* dL_drotation_raw, void* stream);
/* ... and, in the same pass, wgsr_densification_stats' update of
 * max_radii2D / grad_accum / denom (one launch instead of two).  skip
 * (nullable device word): when non-zero the statistics are left unchanged --
 * pass the capacity-mode forward's overflow word (counts[3]), whose iteration
 * produced no gradient. */
int wgsr_gaussian_activate_backward_stats(int P, const float* opacity_raw, const float* scaling_raw,
                                          const float* rotation_raw, const float* dL_dopacity,
                                          const float* dL_dscales, const float* dL_drotations, float iso_weight,
                                          float* dL_dopacity_raw, float* dL_dscaling_raw, float* dL_drotation_raw,
                                          const int32_t* radii, const float* dL_dmeans2D, float* max_radii2D,
                                          float* grad_accum, float* denom, const uint32_t* skip, void* stream);

/* get_loss_mapping_rgbd (slam_utils.py:107-143) without its SSIM term:
 * image_ab = exp(exposure_a) image + exposure_b ([3,H,W], written for the
 * SSIM kernels); partials[wgsr_map_blocks(H*W)][2] = per-block sums of the
 * boundary-masked rgb L1 (mask: sum_c gt > rgb_threshold) and of the masked
 * depth L1 (gt_depth > 0.01).  exposure_a/b: device scalars. */
int wgsr_mapping_loss_forward(int H, int W, const float* image, const float* gt_image,
                              const float* depth, const float* gt_depth, const float* exposure_a,
                              const float* exposure_b, float rgb_threshold, float* image_ab,
                              float* partials, void* stream);

/* Backward of w_rgb * sum(rgb L1) + w_depth * sum(depth L1) + the SSIM term
 * whose gradient w.r.t. image_ab is ssim_grad ([3,H,W], already scaled; NULL =
 * none): dL_dimage [3,H,W], dL_ddepth [1,H,W] and partials[blocks][2] = per-
 * block sums of dL/dexposure_a and dL/dexposure_b. */
int wgsr_mapping_loss_backward(int H, int W, const float* image, const float* image_ab,
                               const float* gt_image, const float* depth, const float* gt_depth,
                               const float* exposure_a, float rgb_threshold, float w_rgb,
                               float w_depth, const float* ssim_grad, float* dL_dimage,
                               float* dL_ddepth, float* partials, void* stream);

/* ---- The uncertainty-aware mapping loss ---------
 * get_loss_mapping_uncertainty (src/utils/slam_utils.py:146-258) with
 * compute_mapping_loss_components (src/utils/dyn_uncertainty/mapping_utils.py:
 * 206-323): the reference's default mapping loss (uncertainty_params.activate).
 * csrc/uncertainty.hip; driven by wgsr/mapping.py.  Images are [3,H,W] /
 * [1,H,W]; the uncertainty map (the MLP output) is [h,w] (h, w > 2).
 * median_depth: device scalar = ref_depth.median(); the depth threshold is
 * min(10 median, 50).  Partials: per block of wgsr_uncer_blocks(n). */
typedef struct wgsr_uncer_params {
  int H, W;               /* image */
  int h, w;               /* uncertainty map */
  float rgb_threshold;    /* Training.rgb_boundary_threshold */
  float data_rate;        /* 1 + compute_bias_factor(train_frac, 0.8) */
  float ssim_weight;      /* 100 + 900 compute_bias_factor(ssim_frac, 0.8) */
  float opacity_th;       /* uncertainty_params.opacity_th_for_uncer_loss */
  float uncer_depth_mult; /* uncertainty_params.uncer_depth_mult */
  int initialization;     /* 1: no exposure correction */
  int pre_exposed;        /* 1: fuse the mapper's own exposure step: map_opt_online passes
                             exp(a) x + b into the loss (mapper.py:1127-1129), which applies
                             it again (slam_utils.py:179-181).  `image` is the raw render,
                             image_ab = exp(a) (exp(a) x + b) + b, and the image and
                             exposure gradients chain through both applications. */
} wgsr_uncer_params;
int wgsr_uncer_blocks(int64_t n);
/* image_ab = exp(a) image + b (applied twice when pre_exposed); partials[blocks(H*W)][3] = sums of
 * w * masked rgb L1 (over channels), of w, and of the re-weighted depth L1
 * (w where ref_depth < depth + 1), w = the uncertainty weight map. */
int wgsr_uncer_loss_forward(const wgsr_uncer_params* prm, const float* image, const float* gt_image,
                            const float* depth, const float* ref_depth, const float* exposure_a,
                            const float* exposure_b, const float* uncertainty, const float* median_depth,
                            float* image_ab, float* partials, void* stream);
/* The feature-resolution inputs of the uncertainty loss: bilinear downsamples
 * of the opacity image and of clip(opacity ssim_weight (1-l)(1-s)(1-c), 5)
 * (l, c, s: wgsr_ssim_components of (gt, image_ab), full resolution) and the
 * bicubic clipped depth L1, zeroed where the bicubic ref depth > threshold. */
int wgsr_uncer_small_maps(const wgsr_uncer_params* prm, const float* opacity, const float* depth,
                          const float* ref_depth, const float* median_depth, const float* luminance,
                          const float* contrast, const float* structure, float* small_ssim_loss,
                          float* small_depth_loss, float* small_opacity, void* stream);
/* uncertainty_loss (5x5 reflect median of the SSIM loss; zero where the small
 * opacity < opacity_th): loss_map [h,w] (optional), partials[blocks(h*w)],
 * dL_duncertainty = grad_scale * d(loss)/d(uncertainty) (optional; grad_scale
 * = ssim_mult / (h w) for the reference's ssim_mult * mean). */
int wgsr_uncer_loss_small(const wgsr_uncer_params* prm, const float* uncertainty, const float* small_ssim_loss,
                          const float* small_depth_loss, const float* small_opacity, float grad_scale,
                          float* loss_map, float* partials, float* dL_duncertainty, void* stream);
/* The loss epilogue in one launch: fixed-order sums of partials
 * ([blocks(H*W)][3] from wgsr_uncer_loss_forward) and small_partials
 * (wgsr_uncer_loss_small), *loss = alpha rgb + (1 - alpha) depth + ssim_mult
 * mean(uncertainty loss) + extra_weight sum(extra_partials[n_extra]) (e.g. the
 * isotropic term), sums[3] = the three full-resolution sums, ssim_scale[3] =
 * the SSIM backward's per-plane dL/dS (ssim_mean: device scalar from
 * wgsr_ssim_forward; ignored unless ssim_loss). */
int wgsr_uncer_loss_combine(const wgsr_uncer_params* prm, const float* partials, const float* small_partials,
                            const float* ssim_mean, const float* extra_partials, int n_extra, float extra_weight,
                            float alpha, float lambda_dssim, float ssim_mult, int ssim_loss, float* loss,
                            float* sums, float* ssim_scale, void* stream);
/* wgsr_uncer_loss_combine taking the SSIM forward's tile partials
 * (wgsr_ssim_forward_partials of the 3 planes) instead of its mean: the
 * partials are reduced in this launch, in k_ssim_reduce's order (the same
 * mean, bit for bit), and the mean written to ssim_mean (may be NULL). */
int wgsr_uncer_loss_combine_ssim(const wgsr_uncer_params* prm, const float* partials, const float* small_partials,
                                 const float* ssim_partials, float* ssim_mean, const float* extra_partials,
                                 int n_extra, float extra_weight, float alpha, float lambda_dssim, float ssim_mult,
                                 float* loss, float* sums, float* ssim_scale, void* stream);
/* dL_dimage / dL_ddepth of loss_grad x (w_rgb sum(w rgb L1) + w_depth
 * sum(re-weighted depth L1)) + the SSIM term (ssim_grad: its gradient w.r.t.
 * image_ab, already scaled; NULL = none); loss_grad: device scalar (NULL = 1);
 * partials[blocks(H*W)][2] = dL/dexposure_a, _b.  exposure_b is read only
 * when pre_exposed (NULL otherwise allowed). */
int wgsr_uncer_loss_backward(const wgsr_uncer_params* prm, const float* image, const float* image_ab,
                             const float* gt_image, const float* depth, const float* ref_depth,
                             const float* exposure_a, const float* exposure_b, const float* uncertainty, const float* median_depth,
                             float w_rgb, float w_depth, const float* loss_grad, const float* ssim_grad,
                             float* dL_dimage, float* dL_ddepth, float* partials, void* stream);

/* ---- The mapper's pose-refinement loss (tracking) --
 * csrc/tracking.hip; driven by wgsr/tracking.py.
 * wgsr_tracking_loss: get_loss_tracking(..., monocular=True) (src/utils/
 * slam_utils.py:47-82) forward AND backward in one pass: partials[blocks(H*W)]
 * [3] = per-block sums of the opacity-weighted L1 (divide by 3HW for the
 * loss), of dL/dexposure_a and of dL/dexposure_b; dL_dimage [3,H,W] and
 * dL_dopacity [1,H,W] (optional) for dL/dloss = 1.  grad_mask ([1,H,W], the
 * keyframe's Camera.grad_mask) and uncertainty ([H,W], already resized) are
 * optional (NULL: ones / no weights). */
int wgsr_track_blocks(int64_t n);
int wgsr_tracking_loss(int H, int W, const float* image, const float* gt_image, const float* opacity,
                       const float* grad_mask, const float* uncertainty, const float* exposure_a,
                       const float* exposure_b, float rgb_threshold, float* dL_dimage, float* dL_dopacity,
                       float* partials, void* stream);
/* One pose-refinement update (mapper.py:884-906 after loss.backward()): Adam
 * (torch semantics; bias corrections of `step`) over cam_rot_delta (grad =
 * dtau[3:6]), cam_trans_delta (dtau[0:3]), exposure_a / exposure_b (sums of
 * columns 1 / 2 of wgsr_tracking_loss's partials), then update_pose
 * (pose_utils.py:81-98: w2c <- SE3_exp([trans, rot]) w2c, deltas back to 0,
 * *converged = |tau| < threshold) and the next iteration's rasteriser camera
 * (viewmatrix, projmatrix, campos).  state: wgsr_pose_state_floats() floats,
 * layout in csrc/tracking.hip (R, T, exposures, Adam moments, camera).
 * camera_only = 1 only writes the camera fields from the stored (R, T). */
int wgsr_pose_state_floats(void);
int wgsr_pose_step(float* state, const float* dtau, const float* loss_partials, int n_partials,
                   const float* projection_matrix, float lr_rot, float lr_trans, float lr_exposure, float beta1,
                   float beta2, float eps, int step, float converged_threshold, int* converged, int camera_only,
                   void* stream);
/* Camera.compute_grad_mask (src/utils/camera_utils.py:157-180): grad_mask
 * [H,W] of the [3,H,W] image (edge_threshold: Training.edge_threshold).
 * Needs (H/32)(W/32) <= 8192. */
int wgsr_grad_mask(int H, int W, const float* image, float edge_threshold, float* grad_mask, void* stream);

/* ---- The uncertainty MLP ------------------------
 * uncertainty_model.MLPNetwork with its defaults (src/utils/dyn_uncertainty/
 * uncertainty_model.py:5-68): C -> 64 -> 64 -> 1, ReLU, dropout p after each
 * hidden layer, softplus.  csrc/mlp.hip; driven by wgsr/mlp.py.  X [N][C]
 * (C a multiple of 64), weights row-major as torch.nn.Linear keeps them.
 * Forward keeps h1d/h2d ([N][64], post-dropout) and o_pre ([N]) for the
 * backward; dropout masks are a counter hash of (seed, layer, row, column).
 * Backward: grad (wgsr_mlp_grad_floats(C) floats) = dW1 [64][C] | db1 [64] |
 * dW2 [64][64] | db2 [64] | dW3 [64] | db3 [1] for dL_du [N]; scratch:
 * wgsr_mlp_scratch_bytes(N, C). */
size_t wgsr_mlp_scratch_bytes(int N, int C);
int wgsr_mlp_grad_floats(int C);
int wgsr_mlp_forward(int N, int C, const float* X, const float* W1, const float* b1, const float* W2,
                     const float* b2, const float* W3, const float* b3, float dropout_p, uint32_t seed,
                     float* h1d, float* h2d, float* o_pre, float* u, void* stream);
/* wgsr_mlp_forward with the dropout seed read from device memory (a
 * graph-replayed mapping iteration draws a new seed per step). */
int wgsr_mlp_forward_dev_seed(int N, int C, const float* X, const float* W1, const float* b1, const float* W2,
                              const float* b2, const float* W3, const float* b3, float dropout_p,
                              const uint32_t* seed, float* h1d, float* h2d, float* o_pre, float* u, void* stream);
/* keys[i] = 31-bit hash of (seed, i), i < n (seed_dev, when not NULL, holds
 * the seed): sorting the keys gives the DINO term's random sample order. */
int wgsr_random_keys(int64_t n, uint32_t seed, const uint32_t* seed_dev, int32_t* keys, void* stream);
/* perm[0..n) = the stable ascending order of wgsr_random_keys(n, seed) (the
 * DINO term's sample draw) in two launches; keys: n words of scratch.
 * n <= wgsr_random_perm_max(). */
int64_t wgsr_random_perm_max(void);
int wgsr_random_perm(int64_t n, uint32_t seed, const uint32_t* seed_dev, uint32_t* keys, int32_t* perm,
                     void* stream);
/* perm[0..k) = the first k entries of wgsr_random_perm's permutation (the
 * DINO term keeps only n / reg_stride^4 of the draw), in one launch and
 * without a sort of all n; n <= wgsr_random_perm_prefix_max_n(),
 * k <= min(n, wgsr_random_perm_prefix_max_k()). */
int64_t wgsr_random_perm_prefix_max_n(void);
int64_t wgsr_random_perm_prefix_max_k(void);
int wgsr_random_perm_prefix(int64_t n, int64_t k, uint32_t seed, const uint32_t* seed_dev, int32_t* perm,
                            void* stream);
/* Two uncertainty-MLP forwards in one launch (the mapping iteration's
 * keyframe features and the DINO term's sample): rows [0, N1) are X1's with
 * the dropout seed *seed1, rows [N1, N1 + N2) X2's with *seed2 -- each
 * segment's dropout draw is the one its own wgsr_mlp_forward_dev_seed would
 * make; h1d / h2d / o_pre / u hold N1 + N2 rows.  The backward sums both
 * segments' parameter gradients (upstream du1 x du_scale1 and du2 x
 * du_scale2) into grad (added to it with accumulate != 0); scratch:
 * wgsr_mlp_scratch_bytes(N1 + N2, C). */
int wgsr_mlp_forward_seg2(int N1, int N2, int C, const float* X1, const float* X2, const float* W1, const float* b1,
                          const float* W2, const float* b2, const float* W3, const float* b3, float dropout_p,
                          const uint32_t* seed1, const uint32_t* seed2, float* h1d, float* h2d, float* o_pre,
                          float* u, void* stream);
int wgsr_mlp_backward_seg2(int N1, int N2, int C, const float* X1, const float* X2, const float* W2, const float* W3,
                           float dropout_p, const float* h1d, const float* h2d, const float* o_pre, const float* du1,
                           const float* du2, float du_scale1, float du_scale2, int accumulate, float* scratch,
                           float* grad, void* stream);
/* wgsr_mlp_backward with dL_du scaled by du_scale, and with accumulate != 0
 * the gradient ADDED to grad (a second backward into the same parameters,
 * as autograd accumulates). */
int wgsr_mlp_backward_acc(int N, int C, const float* X, const float* W2, const float* W3, float dropout_p,
                          const float* h1d, const float* h2d, const float* o_pre, const float* dL_du, float du_scale,
                          int accumulate, float* scratch, float* grad, void* stream);
int wgsr_mlp_backward(int N, int C, const float* X, const float* W2, const float* W3, float dropout_p,
                      const float* h1d, const float* h2d, const float* o_pre, const float* dL_du,
                      float* scratch, float* grad, void* stream);

/* DINO feature-similarity regulariser: compute_dino_regularization_loss
 * (src/utils/dyn_uncertainty/mapping_utils.py:332-389, replaces its
 * normalize / N x N matmul / topk / gathers on the mapper's uncertainty
 * branch, mapper.py:986-997, 1122-1140).  u [N] uncertainty samples, feat
 * [N, C] features (row-major).  Writes loss[0] = mean_i var_i over the
 * min(top_k, N) most similar samples with cosine similarity > thresh, and
 * grad_u [N] = d loss / d u (zeroed by the call; float atomics, so the
 * order of its adds is not fixed).  Scratch: fn [N, C], sim [N, N], row_var
 * [N].  N <= 16384, thresh > 0.  loss may be NULL: the gradient only (one
 * launch fewer). */
int wgsr_dino_reg(const float* u, const float* feat, int N, int C, int top_k, float thresh, float eps,
                  float* fn_scratch, float* sim_scratch, float* row_var, float* grad_u, float* loss, void* stream);

/* One view's densification bookkeeping (mapper.py:1177-1183,
 * gaussian_model.py:745-749) for Gaussians with radii > 0:
 * max_radii2D = max(max_radii2D, radii); grad_accum += ||dL_dmeans2D[:2]||;
 * denom += 1. */
int wgsr_densification_stats(int P, const int32_t* radii, const float* dL_dmeans2D,
                             float* max_radii2D, float* grad_accum, float* denom, void* stream);

/* Replaces _C.mark_visible: present[i] = (view-space z of point i > 0.2). */
int wgsr_mark_visible(int P, const float* means3D, const float* viewmatrix,
                      const float* projmatrix, uint8_t* present, void* stream);

/* Replaces simple_knn._C.distCUDA2: out[i] = mean of the squared distances
 * to the 3 nearest other points of `points` [P,3] (exact). */
int wgsr_dist_cuda2(int P, const float* points, float* out,
                    wgsr_alloc_fn scratch_alloc, void* alloc_ctx, void* stream);

/* ---- what follows the rasteriser each iteration ---- */

/* One Adam parameter tensor (contiguous fp32, `numel` elements).  The host
 * supplies torch.optim.Adam's per-step scalars: step_size = lr / (1 -
 * beta1^step), bias_correction2_sqrt = sqrt(1 - beta2^step). */
typedef struct wgsr_adam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
  float step_size;
  float bias_correction2_sqrt;
  /* Optional two-rate split (0 = off): element e with e % split_period >=
   * split_len steps with step_size_tail instead of step_size.  Lets one
   * [P,16,3] SH storage carry the reference's f_dc (first 3 floats of each
   * 48, lr 2.5e-3) and f_rest (lr / 20) parameter groups in one tensor. */
  int64_t split_period;
  int64_t split_len;
  float step_size_tail;
} wgsr_adam_tensor;
#define WGSR_ADAM_MAX_TENSORS 16

/* Replaces optimizer.step() of the reference's torch.optim.Adam(param_groups,
 * lr=0.0, eps=1e-15) (gaussian_model.py:309; no weight decay, no amsgrad)
 * for up to WGSR_ADAM_MAX_TENSORS tensors in one launch, element arithmetic
 * in torch's order: exp_avg.lerp_(grad, 1-beta1);
 * exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1-beta2);
 * param.addcdiv_(exp_avg, sqrt(exp_avg_sq)/bias_correction2_sqrt + eps,
 * -step_size).  beta1/beta2/eps are the Python (double) hyper-parameters:
 * 1-beta is formed in double and rounded once, as torch does. */
int wgsr_adam_step(const wgsr_adam_tensor* tensors, int n, double beta1, double beta2, double eps,
                   void* stream);

/* wgsr_adam_step with the per-step scalars in DEVICE memory, for a step
 * replayed from a HIP graph: tensor i uses scalars[3 i + 0..2] = step_size,
 * bias_correction2_sqrt, step_size_tail (its own fields are ignored);
 * skip (or NULL): no update at all when *skip != 0 (a capacity-mode forward
 * that overflowed); weight_decay: torch.optim.Adam's L2 term, the gradient
 * used is grad + weight_decay * param (0: none). */
int wgsr_adam_step_dev(const wgsr_adam_tensor* tensors, int n, double beta1, double beta2, double eps,
                       double weight_decay, const float* scalars, const uint32_t* skip, void* stream);
/* Two optimisers sharing beta1 / beta2 in one launch (the Gaussians' and the
 * uncertainty MLP's in the mapping iteration): tensors [0, n1) step with
 * eps1 / weight_decay1 / scalars1, tensors [n1, n) with eps2 /
 * weight_decay2 / scalars2 (3 floats per tensor, from tensor n1 on). */
int wgsr_adam_step_dev2(const wgsr_adam_tensor* tensors, int n1, int n, double beta1, double beta2, double eps1,
                        double weight_decay1, const float* scalars1, double eps2, double weight_decay2,
                        const float* scalars2, const uint32_t* skip, void* stream);

/* ---- The graph-replayed mapping iteration (wgsr/online_graph.py) -------
 * No reference counterpart: device-side steps that let one captured graph
 * serve every keyframe (mapper.py:1083-1219 per iteration). */
typedef struct wgsr_gather_job {
  const void* src;            /* rows of src_stride_words 32-bit words       */
  void* dst;                  /* nrows contiguous rows of row_words words    */
  int64_t row_words;
  int64_t src_stride_words;   /* >= row_words                                */
  int32_t idx_offset;         /* row r of dst = src row idx[idx_offset + r]  */
  int32_t nrows;
} wgsr_gather_job;
#define WGSR_GATHER_MAX_JOBS 8
/* Every job's rows in one launch (the chosen keyframe's image, depth,
 * features, camera, median depth and exposure, its neighbours' features). */
int wgsr_gather_rows(const wgsr_gather_job* jobs, int n, const int64_t* idx, void* stream);
/* The keyframe exposure optimiser's step (torch.optim.Adam arithmetic, as
 * wgsr_adam_step) on row idx[0] of bank [K][3][2] = (a, b), exp_avg,
 * exp_avg_sq, with grad = the sum of nparts (a, b) rows (the loss
 * backward's per-block partials, added in a fixed order; nparts = 1: the
 * gradient itself) and scalars = (step_size, sqrt(1 - beta2^n)); skipped
 * when *skip_a or *skip_b is non-zero.  With sticky and counts (the
 * capacity-mode forward's, or NULL): sticky[0] += counts[3], sticky[1] =
 * max(sticky[1], counts[0]).  slot_skips (nullable, one word per bank row):
 * slot_skips[idx[0]] += 1 when the step was meant to run (*skip_b == 0) but
 * *skip_a held it back, so the host can roll back that row's step count. */
int wgsr_exposure_step(float* bank, const int64_t* idx, const float* grad, int nparts, const float* scalars,
                       const uint32_t* skip_a, const uint32_t* skip_b, double beta1, double beta2, double eps,
                       int64_t* sticky, const uint32_t* counts, int64_t* slot_skips, void* stream);

/* One row-major tensor for row compaction: rows of `row_bytes` (a multiple
 * of 4) from `src` [P rows]; `dst` receives the kept rows in order. */
typedef struct wgsr_row_tensor {
  const void* src;
  void* dst;
  int64_t row_bytes;
} wgsr_row_tensor;
#define WGSR_COMPACT_MAX_TENSORS 32

/* Replaces prune_points / _prune_optimizer's `t[keep]` (gaussian_model.py:
 * 526-564) over up to WGSR_COMPACT_MAX_TENSORS per-Gaussian tensors at once:
 * dst_i = src_i[keep] for every tensor (keep: [P] bytes, 0/1).  Each dst must
 * hold sum(keep) rows. */
int wgsr_compact_rows(const uint8_t* keep, int64_t P, const wgsr_row_tensor* tensors, int n,
                      wgsr_alloc_fn scratch_alloc, void* alloc_ctx, void* stream);

/* ---- densification on the device (csrc/densify.hip, wgsr/store.py) -------
 * The GaussianModel state lives in a capacity-preallocated SoA of two banks;
 * one bank = the five parameter tensors (xyz [C,3], features [C,M,3],
 * opacity [C,1], scaling [C,3], rotation [C,4]; raw, as GaussianModel's
 * _xyz ... _rotation), their Adam moments in that order, and per-row
 * keyframe ids / observation counts (optional).  Rows are addressed by
 * index; a densify reads one bank and writes the other. */
typedef struct wgsr_gaussian_bank {
  float* xyz;
  float* features;
  float* opacity;
  float* scaling;
  float* rotation;
  float* exp_avg[5];
  float* exp_avg_sq[5];
  int32_t* kf_id;
  int32_t* n_obs;
} wgsr_gaussian_bank;

/* Workgroups of the select / emit kernels over P rows; block_counts holds
 * 4 x (wgsr_densify_blocks(P) + 1) uint32. */
int64_t wgsr_densify_blocks(int64_t P);

/* Replaces the selection of GaussianModel.densify_and_prune(max_grad,
 * min_opacity, extent, max_screen_size) (gaussian_model.py:646-743):
 * grad_threshold = max_grad (> 0), dense_threshold = percent_dense * extent,
 * world_threshold = 0.1 * extent, use_screen_size = bool(max_screen_size).
 * Per row a flag byte (kept original, kept clone, kept split pair, split
 * selected) and, after the built-in scan, block_counts = exclusive per-block
 * offsets of the four regions with the totals (kept originals Ko, kept
 * clones Kc, kept split rows per copy Ks, selected split rows Ns) at
 * [4 * wgsr_densify_blocks(P)].  New row count: Ko + Kc + 2 Ks.
 * With prune_mask (bytes, 1 = prune) instead: prune_points(mask)
 * (gaussian_model.py:548-564) -- only kept originals. */
int wgsr_densify_select(int64_t P, const float* accum, const float* denom, const float* opacity,
                        const float* scaling, const uint8_t* prune_mask, float grad_threshold,
                        float dense_threshold, float min_opacity, float world_threshold, int use_screen_size,
                        float max_screen_size, uint8_t* flags, uint32_t* block_counts, void* stream);

/* Writes the densified / pruned table into bank dst (capacity >= the new row
 * count): kept originals with their moments, then kept clones, kept split
 * copies A and B (zero moments): split xyz = R(q) (z * exp(s)) + xyz with z
 * [2 Ns, 3] standard-normal samples (copy A rows first, by selection rank),
 * split scaling = log(exp(s) / 1.6). */
int wgsr_densify_emit(int64_t P, int M, const uint8_t* flags, const uint32_t* block_counts, const float* z,
                      const wgsr_gaussian_bank* src, const wgsr_gaussian_bank* dst, void* stream);

/* reset_opacity (visible = null, value = inverse_sigmoid(0.01)) and
 * reset_opacity_nonvisible (value = inverse_sigmoid(0.4); visible rows get
 * sigmoid(raw): the reference writes get_opacity[filter] into the raw
 * tensor) (gaussian_model.py:389-402); the opacity moments -> 0. */
int wgsr_reset_opacity(int64_t P, float* opacity_raw, const uint8_t* visible, float value, float* exp_avg,
                       float* exp_avg_sq, void* stream);

/* ---- map deformation (csrc/deform.hip, wgsr/store.py) ---------------------
 * One keyframe's pose / depth update of Mapper._update_mapping_points
 * (src/mapper.py:431-558; caller: _update_keyframes_from_frontend,
 * mapper.py:365-429).  Host-computed, fp32, row-major:
 *   T       = inv(inv(w2c_old) @ w2c_new)                (mapper.py:449 / 530)
 *   q       = rotation_matrix_to_quaternion(T) (w,x,y,z)  (general_utils.py:138-162)
 *   w2c_old, c2w_old = inv(w2c_old), K (the mapper's 3x3 intrinsics), depth /
 *   depth_old ([H,W] device maps) -- the depth-rescale branch (method 1) only. */
typedef struct wgsr_deform_frame {
  int32_t kf_id;
  int32_t method;       /* 0 = "rigid", 1 = depth rescale (method=None)      */
  float T[16];
  float q[4];
  float w2c_old[16];
  float c2w_old[16];
  float K[9];
  int32_t H, W;
  const float* depth;
  const float* depth_old;
} wgsr_deform_frame;

/* Applies every frame of `frames` (DEVICE array of nframes) to the rows of
 * `bank` anchored to its keyframe (lut: DEVICE [lut_size] int32, kf_id ->
 * frame index or -1): xyz, rotation (and scaling for method 1) as the
 * reference does, and -- when any frame has rows -- every row's rotation
 * normalised and the xyz / rotation (and, with a method-1 frame that has rows,
 * scaling) Adam moments zeroed (replace_tensor_to_optimizer,
 * gaussian_model.py:495-508).  flags: DEVICE scratch of 2 uint32. */
int wgsr_deform_points(int64_t P, const wgsr_gaussian_bank* bank, const wgsr_deform_frame* frames, int nframes,
                       const int32_t* lut, int lut_size, uint32_t* flags, void* stream);

/* ---- SSIM for the mapping loss -------------------
 * Images are `planes` contiguous H x W fp32 planes (any leading dims
 * flattened; zero padding at the borders, as F.conv2d(padding=ws//2)).
 * window_size in {3,5,7,9,11}; Gaussian window, sigma 1.5.
 *
 * wgsr_ssim_forward replaces loss_utils.ssim(img1, img2, window_size)
 * (thirdparty/gaussian_splatting/utils/loss_utils.py:61-101): *mean = mean
 * SSIM over all pixels (size_average=True), plane_mean[p] (optional) = per
 * plane mean.  dmap (optional, 3 x planes x H x W floats) receives the
 * per-pixel derivatives the backward needs (dS/dmu1, dS/dE[x^2], dS/dE[xy]).
 * Scratch: wgsr_ssim_scratch_bytes(planes, H, W) through scratch_alloc. */
size_t wgsr_ssim_scratch_bytes(int64_t planes, int H, int W);
int wgsr_ssim_forward(const float* img1, const float* img2, int64_t planes, int H, int W, int window_size,
                      float* dmap, float* plane_mean, float* mean, wgsr_alloc_fn scratch_alloc, void* alloc_ctx,
                      void* stream);
/* The SSIM forward without its reduction launch: per-tile partial sums
 * (wgsr_ssim_tiles(H, W) per plane, plane-major) into `partials`, for a
 * consumer that reduces them itself (wgsr_uncer_loss_combine_ssim). */
int wgsr_ssim_forward_partials(const float* img1, const float* img2, int64_t planes, int H, int W, int window_size,
                               float* dmap, float* partials, void* stream);
int wgsr_ssim_tiles(int H, int W);
/* dL/dimg1 of the forward above given plane_scale[p] = dL/dS for every pixel
 * of plane p (device array; e.g. dL/dmean / (planes*H*W)).  img2 gets no
 * gradient (the reference passes the ground-truth image there). */
int wgsr_ssim_backward(const float* img1, const float* img2, int64_t planes, int H, int W, int window_size,
                       const float* dmap, const float* plane_scale, float* grad_img1, void* stream);
/* compute_ssim_components(img1, img2, window_size) (src/utils/dyn_uncertainty/
 * mapping_utils.py:99-204) for `images` images of `channels` planes each:
 * channel means of the clipped luminance, contrast and structure maps
 * (each images x H x W).  Forward only (the reference detaches them). */
int wgsr_ssim_components(const float* img1, const float* img2, int64_t images, int channels, int H, int W,
                         int window_size, float* luminance, float* contrast, float* structure, void* stream);

/* ---- PLY vertex records ------------------------
 * GaussianModel.save_ply / load_ply (gaussian_model.py:338-493) keep the
 * Gaussians as P fixed-size records of `ncol` float32 properties.  A column
 * set names one contiguous device tensor [P, cols] and, for each of its
 * columns, the record column it maps to.  pack writes records (record
 * columns no set maps -- the reference's zero normals -- become 0); unpack
 * reads them.  Both run on the device (LDS transpose, coalesced on both
 * sides); the host moves only the record block between file and HBM. */
#define WGSR_PLY_MAX_TENSORS 8
#define WGSR_PLY_MAX_COLS 128
typedef struct wgsr_ply_column_set {
  float* data;              /* [P, cols] contiguous fp32 (device) */
  int cols;
  const int* record_col;    /* host array [cols] */
} wgsr_ply_column_set;
int wgsr_ply_pack(const wgsr_ply_column_set* sets, int ntens, int64_t P, int ncol, float* records, void* stream);
int wgsr_ply_unpack(const float* records, int64_t P, int ncol, const wgsr_ply_column_set* sets, int ntens,
                    void* stream);

/* Byte sizes of the forward state buffers (for callers that pre-allocate). */
size_t wgsr_geometry_bytes(int P);
size_t wgsr_binning_bytes(int64_t num_rendered, int W, int H);
size_t wgsr_image_bytes(int W, int H);

/* Optional per-stage timing: HIP events recorded on the caller's stream
 * around each stage (preprocess, depth_sort, offsets_scan, duplicate,
 * tile_sort, ranges, render_fwd, render_bwd, gauss_bwd, dist_cuda2).
 * wgsr_profile_read synchronises on the recorded events and returns the
 * accumulated milliseconds and launch counts per stage (returns the number
 * of stages).  Not thread-safe; meant for benchmarks. */
#define WGSR_NUM_STAGES 10
/* on = 0: off; 1: every stage; (mask << 1) for mask != 0: only the stages
 * whose bit is set (bit i = stage i), e.g. (1 << 7) << 1 times render_bwd
 * alone -- each timed stage adds two event records to the stream. */
void wgsr_profile_enable(int on);
int wgsr_profile_read(double* ms, int64_t* counts, int n, int reset);
const char* wgsr_profile_stage_name(int i);

const char* wgsr_last_error(void);
const char* wgsr_version(void);

/* Byte offset, inside the geometry buffer of this thread's last
 * wgsr_rasterize_forward call, of its depth order: P uint32 Gaussian ids by
 * ascending view-space depth (ties in index order, culled Gaussians last) --
 * the order upstream's (tile | depth) key sort gives every tile list.  Only
 * WGSR_DEPTH_SORT=global (three passes over the visible key range) or =full
 * (four 8-bit passes over the whole keys), or sort bins off, produce one;
 * where it lands varies.  -1 when the last forward had none: by default the
 * entries of every sort bin are ordered by depth after the bin sort. */
int64_t wgsr_depth_order_offset(void);

/* ---- droid_backends (src/lib/droid.cpp:254-266): the tracker-side ops that
 * feed the mapper, and the correlation lookups (csrc/droid.hip,
 * csrc/droid_altcorr.hip).  poses [num, 7] = (tx, ty, tz, qx, qy, qz, qw),
 * world to camera; disps [num, ht, wd] fp32; intrinsics [4] = (fx, fy, cx,
 * cy); all device memory.  projmap has no entry point yet. */

/* Replaces droid_backends.frame_distance (DepthVideo.distance,
 * depth_video.py:205-235): dist[k] = mean induced flow of frame ii[k]'s
 * pixels seen from frame jj[k] (weight beta: full motion, 1 - beta:
 * translation only; depths <= 0.25 do not count), or 1000 when fewer than
 * 0.75 of the weighted terms count.  bidirectional != 0: 0.5 (d(ii, jj) +
 * d(jj, ii)) in the same launch (the reference calls twice).  A pair with an
 * index outside [0, num) reads nothing and gets NaN. */
int wgsr_droid_frame_distance(const float* poses, const float* disps, const float* intrinsics, int num, int ht,
                              int wd, const int64_t* ii, const int64_t* jj, int n, float beta, int bidirectional,
                              float* dist, void* stream);
/* Replaces droid_backends.depth_filter (DepthVideo.update_valid_depth_mask,
 * depth_video.py:407-442): count[b, v, u] = how many of frame inds[b]'s
 * neighbours ix-1, ix-2, ix-3, ix+3, ix+4, ix+5 (those inside [0, num)) see
 * the pixel's point at a depth within thresh[b] of one of the four
 * disparities around its projection.  Every element of count [m, ht, wd] is
 * written (no zero fill needed); a frame index outside [0, num) reads
 * nothing and gets NaN.  m <= 65535. */
int wgsr_droid_depth_filter(const float* poses, const float* disps, const float* intrinsics, int num, int ht, int wd,
                            const int64_t* inds, const float* thresh, int m, float* count, void* stream);
/* Replaces droid_backends.iproj: points [num, ht, wd, 3] = (R(q) X_xyz +
 * d t) / d.  num <= 65535. */
int wgsr_droid_iproj(const float* poses, const float* disps, const float* intrinsics, int num, int ht, int wd,
                     float* points, void* stream);

/* element type of a correlation volume */
#define WGSR_DTYPE_F32 0
#define WGSR_DTYPE_F16 1
/* Replaces droid_backends.corr_index_forward (CorrSampler.forward,
 * corr.py:21-28): corr [n, 2r+1, 2r+1, h1, w1], corr[n, i, j, y, x] = the
 * bilinear sample of the plane volume[n, y, x, :, :] (volume [n, h1, w1, h2,
 * w2]) at (x0 + i - r, y0 + j - r), (x0, y0) = coords[n, :, y, x] (fp32);
 * taps outside the plane are zero.  Accumulated in fp32, rounded once to the
 * volume's type.  radius <= 6. */
int wgsr_droid_corr_index_forward(const void* volume, const float* coords, int dtype, int n, int h1, int w1, int h2,
                                  int w2, int radius, void* corr, void* stream);
/* Replaces droid_backends.corr_index_backward (CorrSampler.backward,
 * corr.py:30-36): volume_grad [n, h1, w1, h2, w2] = the adjoint of the
 * forward applied to corr_grad (the volume's type).  Every element is
 * written, zeros included: the caller needs no memset. */
int wgsr_droid_corr_index_backward(const float* coords, const void* corr_grad, int dtype, int n, int h1, int w1,
                                   int h2, int w2, int radius, void* volume_grad, void* stream);

/* Replaces droid_backends.altcorr_forward (CorrLayer.forward / AltCorrBlock,
 * corr.py:93-159; csrc/droid_altcorr.hip): the lookup above on the all-pairs
 * volume <fmap1[.., y, x, :], fmap2[.., y2, x2, :]>, without the volume.
 * fmap1 [f1, h1, w1, c] and fmap2 [f2, h2, w2, c], channels last, both of
 * type `dtype`; coords [b, n, h1, w1, 2] fp32 (x, y), multiplied by
 * coord_scale (a power of two, so the product is exact: a pyramid level's
 * 2^-i needs no scaled copy).  Entry e reads maps fmap1[ii[e]] and
 * fmap2[jj[e]] (device int64 [b]; a null array: map e, and then b <= f1 / f2);
 * an index outside [0, f) reads nothing and gives that entry NaN.
 * corr[e, m, iy + (2r+1) ix, y, x] (type corr_dtype: fp32, or fp16 with fp16
 * maps) = the bilinear blend, around (x0 + ix - r, y0 + iy - r) with (x0, y0)
 * = coord_scale coords[e, m, y, x], of the taps' dot products; taps outside
 * the plane are zero.  It is written at corr + e corr_stride_b + m
 * corr_stride_n + (channel_offset + iy + (2r+1) ix) h1 w1 + y w1 + x
 * (strides in elements), so one pyramid level lands in its channel slice of
 * [b, n, levels (2r+1)^2, h1, w1].  Each dot product is accumulated in fp32
 * (32-channel partial sums, added in order), the blend in fp32, one rounding
 * to corr_dtype; the weights 1 - dx, 1 - dy are formed as (floor + 1) - x, so
 * each of the four blend weights is accurate relative to itself even for a
 * small negative coordinate.  A centre that is not finite, or whose floor is 1e8 or more
 * in magnitude (compared as a float, before it becomes an int), gives an
 * all-zero window; no coordinate value reads out of bounds.  Every output
 * element is written (no memset), nothing synchronises with the host (the call
 * can be captured in a graph), and the result is bit-reproducible.  c a
 * positive multiple of 32, radius <= 6; 16-byte loads when fmap2 is 16-byte
 * aligned, element loads otherwise.  Anything else: WGSR_EINVAL before a
 * launch. */
int wgsr_droid_altcorr_forward(const void* fmap1, const void* fmap2, const float* coords, const int64_t* ii,
                               const int64_t* jj, int dtype, int corr_dtype, int f1, int f2, int b, int n, int h1,
                               int w1, int h2, int w2, int c, int radius, float coord_scale, void* corr,
                               int64_t corr_stride_b, int64_t corr_stride_n, int channel_offset, void* stream);
/* Replaces droid_backends.altcorr_backward (CorrLayer.backward, corr.py:101-
 * 108): fp32, the plain form (entry e reads maps e, coord_scale 1).  corr_grad
 * [b, n, (2r+1)^2, h1, w1] contiguous.  fmap1_grad [b, h1, w1, c] and
 * fmap2_grad [b, h2, w2, c] = the exact adjoint of the forward's definition;
 * coords_grad [b, n, h1, w1, 2] (may be null) = 0, the reference's contract.
 * Every element of fmap1_grad is written once.  fmap2_grad is zero-filled on
 * the stream by this call and then accumulated with the hardware fp32 atomic
 * add, whose order of arrival varies: fmap2_grad is NOT bit-reproducible from
 * run to run (fmap1_grad is).  No host synchronisation. */
int wgsr_droid_altcorr_backward(const float* fmap1, const float* fmap2, const float* coords, const float* corr_grad,
                                int b, int n, int h1, int w1, int h2, int w2, int c, int radius, float* fmap1_grad,
                                float* fmap2_grad, float* coords_grad, void* stream);

/* ---- The all-pairs correlation pyramid of the frontend and the motion filter
 * (CorrBlock, corr.py:39-90; csrc/droid_corrvol.hip; wgsr.frontend.CorrBlock).
 * The volumes live in a store of `capacity` slots, one device allocation, 16-
 * byte aligned.  A slot holds one edge's `levels` planes back to back: level
 * i is [h, w, h >> i, w >> i] fp16, each level starting on a 16-byte
 * boundary.  levels in [1, 4]; h and w each at least 2^(levels-1).  `dtype`
 * is the volume's element type: only WGSR_DTYPE_F16 is built, and
 * WGSR_DTYPE_F32 is refused with an error that names it.  Neither launch
 * reads anything on the host: both can be captured in a graph. */
/* bytes of one slot (a multiple of 16); -1 (and wgsr_last_error) for shapes
 * the two calls below would refuse */
int64_t wgsr_droid_corr_slot_bytes(int h, int w, int levels);
/* Builds n edges in one launch: fmap1, fmap2 [n, c, h, w] fp16 contiguous
 * (channel-major, as the reference holds them), c a positive multiple of 32;
 * edge e goes to slot slots[e] (device int32 [n]; a slot outside [0, capacity)
 * writes nothing).  Level 0 [p1, p2] = round_fp16(1/16 x the fp32-accumulated
 * dot product of fmap1[:, p1] and fmap2[:, p2]): the reference's matmul of
 * both maps / 4 under autocast.  Level i + 1 = round_fp16 of the mean of the
 * 2 x 2 block of level i's stored fp16 values (avg_pool2d of what was stored,
 * an odd trailing row or column dropped).  The pooled levels come from the
 * workgroup's tile on chip: no plane is read back from memory.  16-byte moves
 * when w is a multiple of 8 and the maps are 16-byte aligned, element moves
 * otherwise.  n <= 65535. */
int wgsr_droid_corr_build(const void* fmap1, const void* fmap2, int dtype, int n, int c, int h, int w, int levels,
                          void* store, int capacity, const int32_t* slots, void* stream);
/* Looks up every level of n edges in one launch: coords [n, h, w, 2] fp32 (x,
 * y) as the caller holds them; corr [n, levels (2r+1)^2, h, w] fp16, channels
 * [i (2r+1)^2, (i+1) (2r+1)^2) = wgsr_droid_corr_index_forward of level i of
 * slot slots[e] at coords / 2^i (the scaling is exact and done in the
 * kernel), bit for bit.  Every output element is written (no zero fill); an
 * edge whose slot lies outside [0, capacity) reads nothing and gets NaN.
 * radius <= 6. */
int wgsr_droid_corr_lookup(const void* store, int capacity, const int32_t* slots, const float* coords, int dtype,
                           int n, int h, int w, int levels, int radius, void* corr, void* stream);

/* ---- droid_backends.ba (csrc/droid_ba.hip): DROID-SLAM's dense bundle
 * adjustment over n_edges edges (ii[e], jj[e]) with targets / weights
 * [n_edges, 2, ht, wd].  Frames [t0, t1) have free poses (P = t1 - t0); the
 * disparities of the K frames kx = sorted({t0..t1-1} u set(ii)) are variables,
 * eta [K, ht, wd] their damping; disps_sens [num, ht, wd] (> 0: a sensor
 * disparity).  A call makes no host round trip and no stream synchronisation
 * and is bit-reproducible.  Its first kernel validates the indices and writes
 * *status (device memory): 0, or WGSR_BA_BAD_* bits, and then every later
 * kernel leaves poses and disps untouched (and dx, dz unwritten). */
#define WGSR_BA_BAD_INDEX 1u /* an ii / jj entry outside [0, num)            */
#define WGSR_BA_BAD_JJ 2u    /* a jj entry >= t1                             */
#define WGSR_BA_BAD_K 4u     /* |kx| differs from K (eta's rows)             */
/* bytes of caller-owned device scratch the two entry points below need
 * (8-byte aligned); -1 (and wgsr_last_error) for sizes they would refuse */
int64_t wgsr_droid_ba_workspace_bytes(int num, int ht, int wd, int n_edges, int t0, int t1, int K);
/* Replaces droid_backends.ba (DepthVideo.ba, depth_video.py:351-373):
 * `iterations` Gauss-Newton steps, each on the state the last one left;
 * poses[t0:t1] and disps[kx] updated in place (motion_only: poses only;
 * depth_only: disparities only).  dx [P, 6] and dz [K, ht * wd] (unused with
 * motion_only) receive the last step.  The reduced system is assembled,
 * damped (D <- D + ep + lm D), factored (Cholesky) and solved in fp64; a
 * failed factorisation gives dx = 0.  The disparity step leaves out the term
 * of pose t0's own update, as the reference does.  Bad sizes, null pointers
 * or a short workspace return WGSR_EINVAL before any launch. */
int wgsr_droid_ba(float* poses, float* disps, const float* intrinsics, const float* disps_sens,
                  const float* targets, const float* weights, const float* eta, const int64_t* ii,
                  const int64_t* jj, int num, int ht, int wd, int n_edges, int K, int t0, int t1, int iterations,
                  float lm, float ep, int motion_only, int depth_only, void* workspace, int64_t workspace_bytes,
                  float* dx, float* dz, uint32_t* status, void* stream);
/* Measurement hook (tools/bench_droid_ba.py): events[0..4] (hipEvent_t, alive
 * until the hook is reset with null) are recorded on the call's stream by
 * every later wgsr_droid_ba / _system call of this thread, in each iteration:
 * before the linearisation, before the reduced system's assembly (Schur
 * complement), before the solve, after it, and after the back-substitution
 * and retractions.  Not for use under stream capture. */
void wgsr_droid_ba_stage_events(void** events);
/* Diagnostic: one linearisation at the current state, nothing updated.  H
 * [6P, 6P] and g [6P] (fp64) = the damped reduced system (A - S, a - s; with
 * motion_only A, a), C and w [K, ht * wd] (fp32; not written, and may be
 * null, with motion_only), dx [P, 6] the solve's result. */
int wgsr_droid_ba_system(const float* poses, const float* disps, const float* intrinsics, const float* disps_sens,
                         const float* targets, const float* weights, const float* eta, const int64_t* ii,
                         const int64_t* jj, int num, int ht, int wd, int n_edges, int K, int t0, int t1, float lm,
                         float ep, int motion_only, void* workspace, int64_t workspace_bytes, double* H, double* g,
                         float* C, float* w, float* dx, uint32_t* status, void* stream);

/* ---- lietorch's SE3 (csrc/lie.hip; python/lietorch).  A group element is 7
 * floats (tx, ty, tz, qx, qy, qz, qw), a tangent vector 6 floats (tau, phi),
 * translation part first; fp32, device memory, inference only. */
#define WGSR_LIE_EXP 0    /* a: tangent [.., 6]            -> element [.., 7]  */
#define WGSR_LIE_LOG 1    /* a: element                    -> tangent [.., 6]  */
#define WGSR_LIE_INV 2    /* a: element                    -> element          */
#define WGSR_LIE_MUL 3    /* a, b: elements                -> a b              */
#define WGSR_LIE_ACT3 4   /* a: element, b: point [.., 3]  -> R b + t          */
#define WGSR_LIE_ACT4 5   /* b: (X, Y, Z, w) [.., 4]       -> (R XYZ + w t, w) */
#define WGSR_LIE_MATRIX 6 /* a: element                    -> 4 x 4 row-major  */
#define WGSR_LIE_ADJ 7    /* b: tangent                    -> Adj b            */
#define WGSR_LIE_ADJT 8   /* b: tangent                    -> Adj^T b          */
#define WGSR_LIE_RETR 9   /* b: tangent                    -> exp(b) a         */
/* One group operation on n output elements, one launch on `stream`, with no
 * allocation and no synchronisation.  Output element e reads a's element
 * e / inner_a and b's element e / inner_b (inner >= 1; b is ignored by the
 * one-operand ops): an operand broadcast over trailing dimensions is passed
 * as it is.  Adj = [[R, [t]x R], [0, R]].  Quaternions are not renormalised;
 * log accepts either sign of q.  exp(0) is exactly (0, 0, 0, 0, 0, 0, 1),
 * log of the identity exactly 0, X * identity exactly X. */
int wgsr_lie_se3(int op, const float* a, int64_t inner_a, const float* b, int64_t inner_b, float* out, int64_t n,
                 void* stream);

#define WGSR_REPROJECT_JACOBIAN 1
#define WGSR_REPROJECT_DEPTH 2
/* projective_ops.projective_transform (DepthVideo.reproject) in one launch:
 * for edge e and pixel (u, v) of frame i = ii[e] with disparity d, X0 =
 * ((u - cx_i) / fx_i, (v - cy_i) / fy_i, 1, d), (X, Y, Z, d) = G_ij X0 with
 * G_ij = G_j G_i^-1 (i == j: the stereo transform t = (-0.1, 0, 0), R = I),
 * coords [n, ht, wd, 2] = (fx_j X / Z' + cx_j, fy_j Y / Z' + cy_j) with Z' =
 * 1 where Z < 0.1 and Z elsewhere; valid [n, ht, wd, 1] = 1.0 where Z > 0.2
 * (the Python's MIN_DEPTH, not the CUDA kernels' 0.25), else 0.0.
 * intrinsics: [num, 4] with per_frame_intrinsics != 0, else one [4].
 * flags & WGSR_REPROJECT_DEPTH: coords is [n, ht, wd, 3] with d / Z' third.
 * flags & WGSR_REPROJECT_JACOBIAN: Jj [n, ht, wd, 2, 6] = d coords / d (left
 * perturbation of G_j), Ji = -Adj^T_Gij applied to Jj's rows, Jz [n, ht, wd,
 * 2, 1] = d coords / d d; without the flag the three must be null.  coords
 * (two-slot form) and Jz 8-byte, Ji and Jj 16-byte aligned.  An edge with an
 * index outside [0, num) reads nothing and gets NaN.  No allocation, no
 * synchronisation; every output element is written. */
int wgsr_droid_reproject(const float* poses, const float* disps, const float* intrinsics, int per_frame_intrinsics,
                         int num, int ht, int wd, const int64_t* ii, const int64_t* jj, int n, int flags,
                         float* coords, float* valid, float* Ji, float* Jj, float* Jz, void* stream);

/* ---- Convex upsampling of the tracker's disparities (cvx_upsample,
 * droid_net.py:23-37; DepthVideo.upsample, depth_video.py:179-183;
 * csrc/droid_upsample.hip; wgsr.frontend.upsample).  With pad the zero-padded
 * coarse map,
 *   up[i, 8y+a, 8x+b, c] = sum_{k=0..8} softmax_k(mask[i, 64k + 8a + b, y, x])
 *                                       * pad[i, y + k/3 - 1, x + k%3 - 1, c]:
 * the softmax in fp32 with the maximum subtracted, the weights never rounded.
 * One launch, no allocation, no synchronisation, no host read.
 * src_index [n] (int64, or null: entry i reads frame i) names the frame of
 * `data` / `disps` [n_src, ht, wd, dim] entry i reads; out_index [n] (or null)
 * the frame of `out` [n_out, 8 ht, 8 wd, dim] it writes: every element of an
 * addressed frame is written, other frames are untouched; the entries of
 * out_index must be distinct.  out must be 16-byte aligned.
 * status (one device word, written by every call): 0, or WGSR_UPSAMPLE_BAD_*
 * when an index lies outside its range -- the call then writes nothing else. */
#define WGSR_UPSAMPLE_BAD_SRC 1u /* a src_index outside [0, n_src) */
#define WGSR_UPSAMPLE_BAD_OUT 2u /* an out_index outside [0, n_out) */
/* mask [n, 576, ht, wd] of mask_dtype (WGSR_DTYPE_F32 or _F16); 1 <= dim <= 4. */
int wgsr_droid_cvx_upsample(const float* data, const int64_t* src_index, const void* mask, int mask_dtype,
                            float* out, const int64_t* out_index, int n, int n_src, int n_out, int ht, int wd,
                            int dim, uint32_t* status, void* stream);
/* The same on dim = 1 with the mask head (GraphAgg.upmask, droid_net.py:61-63:
 * a 1 x 1 convolution) computed inside the launch: feat [n, C, ht, wd] fp16
 * (C a multiple of 32, 16-byte aligned), weight [576, C] fp16 (16-byte
 * aligned), bias [576] fp32.  logit = fp16(fp32 MFMA sum over C + bias): the
 * value the convolution hands on under autocast.  No logit reaches memory. */
int wgsr_droid_upmask_upsample(const void* feat, const void* weight, const float* bias, int C, const float* disps,
                               const int64_t* src_index, float* out, const int64_t* out_index, int n, int n_src,
                               int n_out, int ht, int wd, uint32_t* status, void* stream);

/* ---- The 3 x 3 convolutions after the ConvGRU in the tracker's update
 * operator (UpdateModule.delta / .weight, droid_net.py:102-115, 141-145;
 * GraphAgg.forward up to eta and the input of upmask, droid_net.py:65-77;
 * csrc/droid_conv3x3.hip; wgsr.frontend.update_heads / graph_agg).  One
 * implicit-GEMM kernel: padding 1, stride 1, C_in = 128, maps [*, 128, ht, wd]
 * fp16 contiguous (NCHW), fp16 weights, fp32 accumulation by
 * v_mfma_f32_16x16x32_f16, fp32 bias, the epilogue in fp32.  A value that goes
 * to memory as an activation is rounded to fp16 exactly once (autocast's
 * rounding point); the heads' outputs (delta, weight, eta) are written as fp32
 * and never rounded to fp16, which is more exact than autocast.
 *
 * Packed parameters of a 3 x 3 convolution (a host-side layout, shared with
 * wgsr_droid_gru below; wgsr.frontend.pack_conv3x3_wide builds it,
 * unpack_conv3x3_wide inverts it).  For W [C_out, C_in, 3, 3], C_in a multiple
 * of 32, with KS = C_in / 32 K-steps and R = ceil(C_out / 16) row blocks the
 * packed weights are R x 9 x KS x 64 x 8 fp16 values:
 *   packed[((((rb 9 + tap) KS + ks) 64 + lane) 8 + j)]
 *     = W[16 rb + (lane & 15)][32 ks + 8 (lane >> 4) + j][tap / 3][tap % 3],
 * zero where the row is >= C_out -- the 16 x 32 MFMA A operand of row block
 * rb, tap and K-step ks as a wave reads it, 16 contiguous bytes per lane.  The
 * packed bias is fp32 [16 R], zero past C_out.  Both 16-byte aligned.  The
 * entry points of this section take C_in = 128, KS = 4 (pack_conv3x3 /
 * unpack_conv3x3).
 *
 * Every call: ht x wd < 2^20, at most 65535 maps; launches only -- no
 * allocation, no synchronisation, no host read -- and capturable in a HIP
 * graph.  The LDS a workgroup needs (48976 bytes) is checked against the
 * device's limit before the first launch: an error return, never a launch. */
/* out[n, C_out, ht, wd] fp16 = fp16(ReLU(conv(x) + bias)); C_out a multiple of
 * 128.  Every element of out is written. */
int wgsr_droid_conv3x3_relu(const void* x, const void* w_packed, const float* b_packed, int c_out, void* out, int n,
                            int ht, int wd, void* stream);
/* net [n, 128, ht, wd] fp16.  hidden_w / hidden_b: the packed 256-row stack of
 * delta.0 (rows 0 .. 127) and weight.0 (rows 128 .. 255), both of which read
 * net: one launch into the caller's scratch `hidden` [n, 256, ht, wd] fp16.
 * delta_w / weight_w: the packed second layers (C_out = 2, one 16-row block
 * each).  delta [n, ht, wd, 2] fp32 = conv(hidden[:, :128]) + bias; weight
 * [n, ht, wd, 2] fp32 = sigmoid(conv(hidden[:, 128:]) + bias): the permuted
 * form UpdateModule.forward returns.  Three launches; every element of hidden,
 * delta and weight is written. */
int wgsr_droid_update_heads(const void* net, const void* hidden_w, const float* hidden_b, const void* delta_w,
                            const float* delta_b, const void* weight_w, const float* weight_b, void* hidden,
                            float* delta, float* weight, int n, int ht, int wd, void* stream);
/* net [n, 128, ht, wd] fp16, ix [n] int64: the group (source frame, 0 .. G-1)
 * of each edge.  mean [G, 128, ht, wd] fp16 (the caller's scratch) = the mean
 * over each group's edges, in ascending edge index, of ReLU(conv1(net) +
 * bias), summed in fp32 by one lane per element (no atomics: two runs are
 * bit-identical), x 1 / count, rounded once; a group without an edge gives
 * zeros (scatter_mean).  feat [G, 128, ht, wd] fp16 = fp16(ReLU(conv2(mean) +
 * bias)), what wgsr_droid_upmask_upsample takes; eta [G, ht, wd] fp32 = 0.01
 * softplus(conv_eta(feat) + bias) (softplus(v) = v above 20, as torch).
 * Three launches, the edge lists read from ix inside the first.
 * status (one device word, written by every call): 0, or
 * WGSR_GRAPH_AGG_BAD_IX when an entry of ix lies outside [0, G) -- the call
 * then writes nothing else (mean, feat and eta are untouched). */
#define WGSR_GRAPH_AGG_BAD_IX 1u
int wgsr_droid_graph_agg(const void* net, const int64_t* ix, int n, int G, const void* conv1_w, const float* conv1_b,
                         const void* conv2_w, const float* conv2_b, const void* eta_w, const float* eta_b,
                         void* mean, void* feat, float* eta, int ht, int wd, uint32_t* status, void* stream);

/* ---- The ConvGRU of the update operator (gru.py:34-48, droid_net.py:138;
 * csrc/droid_gru.hip; wgsr.frontend.conv_gru):
 *   glo  = mean over an edge's pixels of sigmoid(w(net)) * net            [n, 128]
 *   z    = sigmoid(convz([net, inp, corr, flow])     + convz_glo(glo))
 *   r    = sigmoid(convr([net, inp, corr, flow])     + convr_glo(glo))
 *   q    = tanh   (convq([r * net, inp, corr, flow]) + convq_glo(glo))
 *   out  = (1 - z) * net + z * q
 * net, corr [n, 128, ht, wd], flow [n, 64, ht, wd], fp16 contiguous.  inp: [n,
 * 128, ht, wd], or with inp_ix [n] int64 the frame buffer [inp_frames, 128,
 * ht, wd] of which edge e reads frame inp_ix[e] (no gathered copy).  The
 * concatenations are never written: the K loop of the convolution runs over
 * the four sources.
 *
 * Packed weights: the layout of the section above with C_in = 448, KS = 14.
 * zr_w: convz (rows 0 .. 127) stacked on convr (rows 128 .. 255), the input
 * channels in the order net, inp, corr, flow; q_w: convq.  (No packed bias:
 * the biases travel in glo_b.)  glo_w, fp16: w [128, 128, 1, 1] packed
 * the same way with its one tap (8 x 4 x 64 x 8 values), then convz_glo,
 * convr_glo, convq_glo as they lie, [384][128].  glo_b, fp32 [896]: w's bias
 * [128], the biases of convz, convr, convq [384], those of convz_glo,
 * convr_glo, convq_glo [384].  All of them and gbias 16-byte aligned.
 *
 * The caller's scratch, readable after the call: gbias [n, 384] fp32,
 *   gbias[e, 128 k + co] = b_k[co] + (W_k_glo glo[e])[co] + b_k_glo[co]
 * (k = z, r, q), z [n, 128, ht, wd] fp16 and rnet = r * net [n, 128, ht, wd]
 * fp16; and glo_part [n, ceil(ht wd / 128), 128] fp32, the sums of the glo
 * term over chunks of 128 pixels.  Four launches (the chunks' sums, gbias, z
 * and rnet, out), fp32 inside each; z, rnet and out are the only values
 * rounded to fp16, once each.  No atomics: two runs give the same bits, and
 * an edge's result does not depend on the other edges.  out, z, rnet, gbias
 * and glo_part must overlap neither each other nor an input (WGSR_EINVAL).
 * Launches only: no allocation, no synchronisation, no host read; n == 0 is a
 * no-op (status 0).  status (one device word, written by every call): 0, or
 * WGSR_GRU_BAD_IX when an entry of inp_ix lies outside [0, inp_frames) -- the
 * call then writes nothing else. */
#define WGSR_GRU_BAD_IX 1u
int wgsr_droid_gru(const void* net, const void* inp, const int64_t* inp_ix, int inp_frames, const void* corr,
                   const void* flow, const void* glo_w, const float* glo_b, const void* zr_w, const void* q_w,
                   float* gbias, float* glo_part, void* z, void* rnet, void* out, int n, int ht, int wd,
                   uint32_t* status, void* stream);

/* ---- The two encoders in front of the ConvGRU (UpdateModule.corr_encoder /
 * .flow_encoder, droid_net.py:88-100, 136-137; csrc/droid_encoders.hip;
 * wgsr.frontend.corr_encoder / flow_encoder), each one launch:
 *   corr [n, 196, ht, wd] fp16 (what wgsr_droid_corr_lookup and
 *        wgsr_droid_altcorr_forward write)
 *        -> Conv2d(196, 128, 1 x 1) ReLU, Conv2d(128, 128, 3 x 3, pad 1) ReLU
 *        -> out [n, 128, ht, wd] fp16
 *   flow [n, 4, ht, wd] fp32 or fp16 (flow_dtype = WGSR_DTYPE_F32 / _F16; fp32
 *        is rounded to fp16, round to nearest even, as it is read: autocast's
 *        cast)
 *        -> Conv2d(4, 128, 7 x 7, pad 3) ReLU, Conv2d(128, 64, 3 x 3, pad 1) ReLU
 *        -> out [n, 64, ht, wd] fp16
 * fp16 weights, fp32 accumulation by v_mfma_f32_16x16x32_f16, fp32 biases.  The
 * hidden layer is fp16(ReLU(first layer + bias)), zero outside the map (the
 * second convolution pads the hidden layer), kept in LDS: it never reaches
 * memory and the ABI takes no scratch for it.  out = fp16(ReLU(second layer +
 * bias)), rounded once; every element is written.  An entry's result does not
 * depend on the other entries; two runs give the same bits.  No channel past
 * 195 of corr is read.
 *
 * Packed first layers (wgsr.frontend.pack_conv1x1_196 / pack_conv7x7_4 build
 * them, unpack_conv1x1_196 / unpack_conv7x7_4 invert them): both have 196
 * products per output, padded to K = 224 = 7 K-steps of 32 with zero weights,
 * and 128 rows = 8 row blocks: 8 x 7 x 64 x 8 fp16 values, fragment (rb, ks) the
 * 16 x 32 MFMA A operand as a wave reads it,
 *   corr: w1[(((rb 7 + ks) 64 + lane) 8 + j)]
 *           = W[16 rb + (lane & 15)][32 ks + 8 (lane >> 4) + j], zero past channel 195
 *   flow: w1[(((rb 7 + ks) 64 + lane) 8 + j)]
 *           = W[16 rb + (lane & 15)][j & 3][ks][2 (lane >> 4) + (j >> 2)], zero where
 *             the last index is 7
 *         (K index 32 ky + 4 kx + ci: one K-step is one kernel row, and a lane's
 *         8 values are the 4 channels of two adjacent pixels),
 * b1 fp32 [128].  w2 / b2: the packed second layer of the section above (C_in =
 * 128, KS = 4; 128 rows for corr, 64 rows = 4 row blocks for flow).  All four
 * 16-byte aligned.
 *
 * ht x wd < 2^20, at most 65535 maps; launches only -- no allocation, no
 * synchronisation, no host read, no atomics -- and capturable in a HIP graph;
 * n == 0 is a no-op.  The LDS a workgroup needs (74896 bytes for corr, 52176 for
 * flow) is checked against the device's limit: an error return, never a
 * launch. */
int wgsr_droid_corr_encoder(const void* corr, const void* w1, const float* b1, const void* w2, const float* b2,
                            void* out, int n, int ht, int wd, void* stream);
int wgsr_droid_flow_encoder(const void* flow, int flow_dtype, const void* w1, const float* b1, const void* w2,
                            const float* b2, void* out, int n, int ht, int wd, void* stream);

/* ---- The tracker's feature and context encoders (DroidNet.fnet / .cnet, the
 * BasicEncoder of extractor.py:75-141; csrc/droid_basic_encoder.hip;
 * wgsr.frontend.feature_encoder / context_encoder), launch by launch:
 *   stem    Conv 7 x 7 stride 2, 3 -> 32; N; ReLU
 *   layer1  2 x block(32 -> 32); layer2  block(32 -> 64, stride 2), block(64 -> 64);
 *   layer3  block(64 -> 128, stride 2), block(128 -> 128); head  Conv 1 x 1, 128 -> out
 *   block(x) = ReLU(x' + ReLU(N(conv2(ReLU(N(conv1(x))))))), with x' = N(Conv 1 x 1
 *   stride 2 (x)) at stride 2, else x; N an instance norm without parameters
 *   (biased variance, eps 1e-5; fnet) or the identity (cnet).  Padding k / 2:
 *   a stride-2 output is ceil(in / 2) pixels.
 *
 * Normalise on read.  A convolution writes its raw output R = fp16(acc + bias)
 * (fp16 operands, fp32 accumulation by v_mfma_f32_16x16x32_f16, fp32 bias) and
 * its consumer applies N, the ReLU and the residual sum while it stages its
 * tile, in fp32 with one rounding to fp16:
 *   A  ReLU(N(R))                      (p null)
 *   B  ReLU(P + ReLU(N(R)))            (p a stored block output, p_stats null)
 *   C  ReLU(N(Rd) + ReLU(N(R)))        (p a downsample's raw output, p_stats its statistics)
 * r_stats null: N is the identity, for r and for p.  A staged pixel outside the
 * map is zero.  side (stride 1 only; or null): [n, c_in, hi, wi] fp16, the
 * staged values of the map's own pixels, the same bits.  r and p are [.., c_in,
 * hi, wi] fp16 with r_frame / p_frame halfs between frames, their statistics
 * [.., c_in, 2] fp32 (mean, rstd) with *_stats_frame floats between frames, so
 * that one half of a stacked output can be a source.
 *
 * wgsr_droid_be_conv computes rows3 rows of a 3 x 3 convolution (w3: the packed
 * layout of the sections above with KS = c_in / 32) and then rows1 rows of a
 * 1 x 1 convolution that reads the centre tap of the same staged tile (w1: that
 * layout with one tap, ((rb KS + ks) 64 + lane) 8 + j; wgsr.frontend.pack_conv1x1):
 * at stride 2 the block's downsample, at stride 1 with rows3 = 0 the head.
 * bias fp32 [rows3 + rows1].  out [n, rows3 + rows1, ho, wo] fp16 with (ho, wo)
 * = (hi, wi), or their halves rounded up at stride 2.  c_in 32 or 64 (rows
 * multiples of c_in), or 128 at stride 1 (multiples of 64).  epilogue
 * WGSR_BE_RAW: out = fp16(acc + bias); WGSR_BE_CNET (c_in 128, rows3 0, rows1
 * 256): out [n, 128, ho, wo] = fp16(tanh(rows 0 .. 127)), out2 [n, 128, ho, wo] =
 * fp16(ReLU(rows 128 .. 255)).
 *
 * Statistics.  part (or null: none) [n, rows, parts, 3] fp32, parts =
 * wgsr_droid_be_parts(ho, wo, stride): (count, mean, M2) of the fp16 values as
 * stored, in-image pixels only, one partial per wave of a tile.
 * wgsr_droid_be_stats merges them in a fixed order with Chan's formula into
 * stats [n, rows, 2] = (mean, 1 / sqrt(M2 / count + 1e-5)): no atomics, two
 * runs give the same bits, a frame does not depend on the others.
 *
 * wgsr_droid_be_stem: image [n, 3, H, W] fp32 or fp16 (image_dtype); with mean /
 * std [3] (both or neither) it reads fp16((x - mean_c) / std_c), computed in
 * fp32, else fp16(x); zero padding after that.  out [n, 32, ceil(H / 2), ceil(W /
 * 2)], part as above with stride 1.  Packed stem (wgsr.frontend.pack_stem7x7):
 * product k = 21 ky + 3 kx + ci, 147 of them padded to K = 160 = 5 K-steps with
 * zero weights, 2 x 5 x 64 x 8 fp16 values,
 *   w[((rb 5 + ks) 64 + lane) 8 + j] = W[16 rb + (lane & 15)][ci][ky][kx],
 *     21 ky + 3 kx + ci = 32 ks + 8 (lane >> 4) + j,
 * bias fp32 [32].  Packed weights and biases 16-byte aligned.
 *
 * Every call: the output map (the stem) or the input map (be_conv) of ht x wd <
 * 2^20 pixels, at most 65535 frames; one launch -- no allocation, no
 * synchronisation, no host read -- capturable in a HIP graph; n == 0 is a
 * no-op.  The LDS a workgroup needs (at most 48960 bytes) is checked against
 * the device's limit: an error return, never a launch. */
#define WGSR_BE_RAW 0
#define WGSR_BE_CNET 1
int wgsr_droid_be_parts(int ho, int wo, int stride);
int wgsr_droid_be_stem(const void* image, int image_dtype, const float* mean, const float* std_dev, const void* w,
                       const float* bias, void* out, float* part, int n, int H, int W, void* stream);
int wgsr_droid_be_conv(const void* r, int64_t r_frame, const float* r_stats, int64_t r_stats_frame, const void* p,
                       int64_t p_frame, const float* p_stats, int64_t p_stats_frame, void* side, int c_in,
                       int stride, const void* w3, int rows3, const void* w1, int rows1, const float* bias,
                       int epilogue, void* out, void* out2, float* part, int n, int hi, int wi, void* stream);
int wgsr_droid_be_stats(const float* part, float* stats, int n, int rows, int parts, void* stream);

/* ---------------------------------------------------------------------------
 * wgsr.frontend.filter_mono_depth (csrc/droid_mono_filter.hip): the tracker's
 * DINO-consistency filter of the metric depth prior,
 * DepthVideo.filter_high_err_mono_depth (depth_video.py:281-349).
 *
 * poses [num, 7], disps_up [num, H, W] fp32 (the metric disparities at full
 * resolution), mask_up [num, H, W] bytes (bool; row idx is updated in place:
 * bytes are only ever cleared), intrinsics [4] = (fx, fy, cx, cy) at 1/8 scale
 * (multiplied by 8 inside), jj [n_ref] the reference frames (device int64; a
 * frame named twice counts twice).  feats: the DINO maps [frames, hd, wd, C]
 * fp32, 16-byte aligned, C a multiple of 4 -- with feats_packed == 0 the whole
 * buffer, frame f at row f (frames >= num); with feats_packed != 0 n_ref + 1
 * rows: the keyframe's, then those of jj[0], jj[1], ...
 *
 * For each reference k and each pixel (x, y) of frame j = jj[k]: X0 = ((x -
 * cx) / fx, (y - cy) / fy, 1), D = disps_up[j, y, x], X1 = R X0 + t D with (R,
 * t) = pose[idx] pose[j]^-1; Z < 0.1 is replaced by 1; u = fx X / Z + cx, v =
 * fy Y / Z + cy, d = D / Z; the target is (round(u), round(v)), half to even,
 * valid inside the image with d > 0 (compared as floats).  The candidate is
 * matched when the cosine between frame j's feature at (x, y) and frame idx's
 * at the target -- both sampled as F.interpolate(mode='bilinear',
 * align_corners=False) from hd x wd to H x W samples them, norms max(|.|,
 * 1e-12) -- exceeds sim_thresh.  Among the matched candidates of one (k,
 * target) the largest source index y W + x wins; with w its d, err = |1 / w - 1
 * / disps_up[idx, target]| w (a zero disparity: inf) adds one to accurate
 * [target] when err < err_thresh, else to inaccurate[target].  mask_up[idx] is
 * cleared where accurate <= 1, inaccurate > 0 and disps_up[idx] > 0.
 * accurate / inaccurate: [H, W] int32, written when non-null.
 *
 * No full-resolution feature map is formed: the cosines are combinations of
 * entries of the cell Gram matrices F_j F_idx^T and F F^T (fp32 MFMA), held in
 * workspace with one 64-bit winner word per (k, target).  workspace: caller-
 * owned device scratch of wgsr_droid_mono_filter_workspace_bytes (-1, and
 * wgsr_last_error, for sizes the call would refuse), 16-byte aligned.
 * Launches only: no allocation, no synchronisation, no host read, no memset
 * node -- capturable in a HIP graph; the winner is chosen by an integer
 * atomic max, so two runs give the same bits.  n_ref == 0 writes zero counts
 * and leaves the mask as it is.  status (one device word, written by every
 * call): 0, or WGSR_MONO_FILTER_BAD_JJ when an entry of jj lies outside [0,
 * num) -- the call then writes neither the mask nor the counts.  Bad sizes,
 * idx outside [0, num), null pointers or a short workspace: WGSR_EINVAL before
 * any launch. */
#define WGSR_MONO_FILTER_BAD_JJ 1u
int64_t wgsr_droid_mono_filter_workspace_bytes(int n_ref, int H, int W, int hd, int wd);
int wgsr_droid_mono_filter(const float* poses, const float* disps_up, uint8_t* mask_up, const float* intrinsics,
                           const float* feats, int feats_packed, const int64_t* jj, int n_ref, int idx, int num,
                           int H, int W, int hd, int wd, int C, float sim_thresh, float err_thresh,
                           int32_t* accurate, int32_t* inaccurate, void* workspace, int64_t workspace_bytes,
                           uint32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WGSR_H */
