/*
 * qed_splat.h -- C ABI of libqed_splat.so, the MI355X (gfx950) native replacement for the
 * render hot path behind qed_splatter/model.py get_outputs() / get_loss_dict().
 *
 * The reference has NO native boundary of its own: its hot path is the single Python call
 *     render, alpha, info = gsplat.rendering.rasterization(...)
 * at /root/reference/qed_splatter/model.py:267-288 (gsplat is a third-party CUDA package, not
 * vendored).  The entry points below are what a native FFI for that call decomposes into
 * (SURVEY.md section 8b); each cites the piece of the reference call path it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless it is named h_*; all float data is fp32
 *   - the caller (PyTorch) owns every buffer: the library never allocates or frees device
 *     memory, never synchronises the stream, reads no environment variable and keeps no global
 *     mutable state besides a thread-local error string -> re-entrant per stream, safe to capture
 *     into a hipGraph
 *   - `stream` is a hipStream_t passed as void*
 *   - return value: 0 = ok, <0 = error (see QED_E_*); qed_last_error() describes it
 *   - C = cameras, N = Gaussians, M = tile/Gaussian intersections, T = tile_w * tile_h
 *   - quaternions are wxyz; pixel centres are at (x + 0.5, y + 0.5); tile size is 16
 */
#ifndef QED_SPLAT_H
#define QED_SPLAT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QED_OK 0
#define QED_E_INVALID_ARG (-1)
#define QED_E_WORKSPACE (-2)
#define QED_E_LAUNCH (-3)
#define QED_E_UNSUPPORTED (-4)

#define QED_TILE 16             /* BLOCK_WIDTH = 16, model.py:243 */
#define QED_SPLAT_FLOATS 12     /* packed per-(camera,Gaussian) record, see qed_project_fwd */
#define QED_METRICS_WS_DOUBLES (10 * 1024)  /* workspace of qed_image_metrics */
#define QED_STEP_METRICS_WS_DOUBLES (16 * 1024)  /* workspace of qed_step_metrics */
#define QED_LOSS_SUMS_FLOATS (8 + 4 * 1024) /* sums workspace of qed_loss_reduce / qed_loss_grad */
#define QED_VSPLAT_FLOATS 16    /* packed per-(camera,Gaussian) gradient row, see qed_composite_bwd */
#define QED_SH_JAC_FLOATS 10    /* per-(camera,Gaussian) floats of qed_project_fwd's sh_jac hand-over */

/* flags of qed_project_fwd / qed_project_bwd */
#define QED_F_ANTIALIASED 1u    /* rasterize_mode == "antialiased": opacity *= compensation */
#define QED_F_LOG_SCALES 2u     /* `scales` holds log-scales: fuse torch.exp        (model.py:270) */
#define QED_F_LOGIT_OPAC 4u     /* `opacities` holds logits:  fuse torch.sigmoid    (model.py:271) */
#define QED_F_DEPTH_CHANNEL 8u  /* render_mode "RGB+D": depth is colour channel 3   (model.py:256-259) */
#define QED_F_SIGMOID_COLORS 16u /* sh_degree None path: fuse torch.sigmoid(colors) (model.py:264) */
#define QED_F_SH_GRAD_COMPACT 64u /* qed_project_bwd (one camera): v_sh0 receives the clamp-masked colour gradient
                                    (3 floats) instead of b_0 v, v_shN is not written; qed_sh_grad_from_views
                                    rebuilds all coefficient gradients from the views' colour gradients */
#define QED_F_TIGHT_TILES 32u   /* list only the tiles of the 3-sigma square that can reach alpha >= 1/255 (the
                                   rectangle of that ellipse; with qed_project_fwd's tile_masks exactly the tiles in
                                   which some pixel can): tiles_per_gauss / the sorted list become subsets of gsplat's,
                                   images and gradients are unchanged (pass `splats` -- and the masks -- to
                                   qed_bin_tiles) */
#define QED_F_CAMERA_C2W 128u   /* qed_project_fwd: `viewmats` holds camera-to-world matrices c2w[C,3,4] (OpenGL) and `Ks`
                                   the intrinsics [C,4] = (fx, fy, cx, cy); the kernel derives view matrix and K itself
                                   (get_viewmat, model.py:22-38: what qed_camera_setup does in a launch of its own) and
                                   writes them to viewmats_out[C,4,4] / Ks_out[C,3,3] for the kernels that follow */

/* Version of this C ABI: bumped whenever an entry point's argument list or a buffer layout changes incompatibly.
 *   1  rounds 1-3.
 *   2  round 4: qed_composite_fwd / qed_composite_bwd gained `t_final` in the middle of their argument lists; the row of
 *      the compact data-parallel message grew from 3 N + 16 to 3 N + 20 floats (still reported as 1 by that round's
 *      library).  A caller built against another version must not call further: the pointers would be shifted.
 *   3  round 5: qed_composite_fwd gained `tile_order` behind `tile_cost`.
 *   4  qed_adam_tick_t carries beta1 / beta2 as doubles (they were floats): the device-resident bias corrections are
 *      formed at double precision, as the host-state path forms them.
 * New entry points change nothing a caller of version 4 relies on and keep the number (the latest: qed_gaussian_normals,
 * qed_normal_maps, qed_depth_normals, qed_angular_error; qed_normal_loss, qed_gaussian_normals_bwd, qed_normal_rows_merge;
 * qed_normal_consistency, qed_normal_rows_merge_depth; qed_depth_loss; qed_relative_depth_loss; qed_depth_spread_fwd,
 * qed_depth_spread_bwd, qed_depth_distortion_loss; qed_features_fwd, qed_features_bwd, qed_label_loss, qed_label_confusion,
 * qed_label_present). */
#define QED_ABI_VERSION 4
int qed_version(void);   /* == QED_ABI_VERSION of the header the library was built from */
const char* qed_last_error(void);

/* Device-side address of a pinned, mapped host allocation (hipHostGetDevicePointer): what qed_bin_tiles' host_words must
 * be given.  Host code, no launch. */
int qed_host_device_pointer(void* host, void** device);
/* size in bytes of the error/overflow status word block a caller passes as `status` (int32[4]):
 * [0] != 0 -> intersection buffer capacity exceeded (value = required M),
 * [1] != 0 -> radix-sort look-back watchdog fired. */
#define QED_STATUS_WORDS 4

/* ---- a1/a3: camera setup in one launch --------------------------------------------------------
 * get_viewmat (model.py:22-38): c2w[C,3,4] (OpenGL) -> viewmats[C,4,4] = rigid inverse after flipping
 * the y/z columns of R; intrinsics[C,4] = (fx, fy, cx, cy) -> Ks[C,3,3] (model.py:247). */
int qed_camera_setup(int32_t C, const float* c2w, const float* intrinsics, float* viewmats, float* Ks,
                     void* stream);

/* ---- K1+K2: projection + SH colour, fused ------------------------------------------------
 * Replaces, inside rasterization() (model.py:267-288): world->camera, 3D covariance from
 * quat+scale, EWA 2D covariance + eps2d blur, conic, radius, near/far/frustum culling
 * (near_plane=0.01, far_plane=1e10: model.py:279-280), SH evaluation to degree sh_degree
 * (model.py:261-262, 282) with +0.5 and clamp, and the per-Gaussian tile count.
 *
 * means[N,3] quats[N,4] scales[N,3] opacities[N] viewmats[C,4,4] Ks[C,3,3] (row major).
 * sh0 / shN: degree-0 coefficient [.,3] and higher coefficients [.,K-1,3] with row strides
 * (in floats) sh0_stride / shN_stride -- `colors[N,K,3]` is (colors, 3K, colors+3, 3K);
 * features_dc / features_rest (model.py:241) can be passed without the torch.cat.
 * sh_degree < 0: sh0 holds ready colours [N,3] (model.py:263-265).
 *
 * outputs: radii[C,N] i32, means2d[C,N,2], depths[C,N], conics[C,N,3], opac_out[C,N],
 *   colors_out[C,N,3], tiles_per_gauss[C,N] i32 and the packed record splats[C*N][12] =
 *   {x, y, conic_a, conic_b | conic_c, opacity, r, g | b, depth, ln(255 opacity), 0} read by the
 *   compositing kernels; block_sums[ceil(C*N/256)] i32 = tile counts summed per 256
 *   consecutive (camera,Gaussian) slots (input of qed_isect_scan).
 * Culled Gaussians get radius 0 and zeros everywhere.
 * tile_masks (may be NULL; with QED_F_TIGHT_TILES only): u64[C*N][2], 16-byte aligned.  Exact tile lists: word 1 of a slot
 *   is a mask whose bit l says whether tile l (row-major) of the rectangle in record slot 11 can be reached -- whether ANY
 *   pixel centre of the tile can have alpha >= 1/255, the rectangle test the compositing kernels apply to a tile's
 *   quadrants, applied to the tile; tiles_per_gauss then counts the set bits.  A rectangle of more than 64 tiles keeps
 *   every tile (mask ~0).  Word 0 repeats the count (low half) and the packed rectangle (high half), so that the emit
 *   pass reads ONE 16-byte descriptor per slot.  Hand the array to qed_bin_tiles together with `splats`.  Images and
 *   gradients do not change; the list loses ~18 % at config B.
 * sh_jac (may be NULL; used with sh_degree >= 0): QED_SH_JAC_FLOATS planes of C*N floats that the backward pass takes
 *   instead of the coefficients -- planes 0..8 = d colour_ch / d unit direction_axis at [3 axis + ch] (sum over k of
 *   d b_k / d axis * c_k,ch, before the clamp), plane 9 = the clamp mask as an integer (bit ch: colour_ch + 0.5 >= 0).
 *   Written for visible (camera, Gaussian) slots only.  With it qed_project_bwd reads 40 B per slot where it would
 *   re-read all 3 K coefficients (192 B at degree 3) and rebuild the basis derivatives beside the projection state. */
int qed_project_fwd(int32_t N, int32_t C, const float* means, const float* quats, const float* scales,
                    const float* opacities, const float* sh0, int32_t sh0_stride, const float* shN,
                    int32_t shN_stride, int32_t sh_degree, const float* viewmats, const float* Ks,
                    int32_t width, int32_t height, int32_t tile_w, int32_t tile_h, float eps2d,
                    float near_plane, float far_plane, float radius_clip, uint32_t flags,
                    int32_t* radii, float* means2d, float* depths, float* conics, float* opac_out,
                    float* colors_out, float* splats, int32_t* tiles_per_gauss, uint64_t* tile_masks,
                    int32_t* block_sums, float* viewmats_out, float* Ks_out, float* sh_jac, void* stream);

/* Backward of qed_project_fwd (autograd backward of the projection + SH part of model.py:267-288).
 * vsplat[C*N][16] = packed gradient row written by qed_composite_bwd:
 *   {v_x, v_y, |v_x|, |v_y|, v_conic_a, v_conic_b, v_conic_c, v_opacity, v_r, v_g, v_b, v_depth, 0,0,0,0}
 * Outputs (overwritten, summed over cameras): v_means[N,3] v_quats[N,4] v_scales[N,3]
 * v_opacities[N] v_sh0 (stride v_sh0_stride) v_shN (stride v_shN_stride); with
 * QED_F_LOG_SCALES / QED_F_LOGIT_OPAC / QED_F_SIGMOID_COLORS the exp / sigmoid Jacobians are
 * applied so the gradients are w.r.t. the raw parameters.  v_viewmats[C,4,4] (nullable) is
 * accumulated with atomics and must be zeroed by the caller (camera optimiser, model.py:212).
 * sh_jac (may be NULL): the planes qed_project_fwd wrote for the SAME inputs; when given (and sh_degree >= 0) sh0 / shN
 * are not read and may be NULL.  Same gradients either way (the sums run in the same order). */
int qed_project_bwd(int32_t N, int32_t C, const float* means, const float* quats, const float* scales,
                    const float* opacities, const float* sh0, int32_t sh0_stride, const float* shN,
                    int32_t shN_stride, int32_t sh_degree, const float* viewmats, const float* Ks,
                    int32_t width, int32_t height, float eps2d, uint32_t flags, const int32_t* radii,
                    const float* vsplat, float* v_means, float* v_quats, float* v_scales,
                    float* v_opacities, float* v_sh0, int32_t v_sh0_stride, float* v_shN,
                    int32_t v_shN_stride, float* v_viewmats, const float* sh_jac, void* stream);

/* ---- data-parallel exchange of the SH gradients -----------------------------------------
 * d L / d sh_k = sum over views of b_k(dir_view) * v_view (b_k the real SH basis, dir = mean - camera
 * position, v_view the clamp-masked colour gradient written by qed_project_bwd with
 * QED_F_SH_GRAD_COMPACT).  View c's colour gradients are v_views + c * view_stride ([N,3]; a view that
 * does not see a Gaussian holds zeros) and its 4x4 view matrix viewmats + c * viewmat_stride (strides in
 * floats, so that one all-gathered buffer can carry both); v_sh0 / v_shN receive scale * the sums
 * (scale = 1/n_views averages). */
/* The same clamp-masked colour gradient BEFORE qed_project_bwd has run: out[total,3] = vsplat row slots 8..10 (what
 * qed_composite_bwd accumulated) under the clamp mask qed_project_fwd kept in plane 9 of sh_jac (total = C * N slots, one
 * camera per rank in the exchange).  Lets the all-gather of the colour gradients start ahead of the projection backward. */
int qed_pack_color_grad(int32_t total, const float* vsplat, const float* sh_jac, float* out, void* stream);

int qed_sh_grad_from_views(int32_t N, int32_t n_views, const float* means, const float* viewmats,
                           int64_t viewmat_stride, const float* v_views, int64_t view_stride,
                           int32_t sh_degree, float scale, float* v_sh0, int32_t v_sh0_stride,
                           float* v_shN, int32_t v_shN_stride, void* stream);

/* ---- K3: tile intersection ------------------------------------------------------------------
 * qed_isect_scan: exclusive scan of block_sums -> block_offsets[n_blocks] and the total
 * M -> n_isect[0] (device int32).  If M > capacity, status[0] = M (emit/sort then do nothing).
 * qed_isect_emit: for every (camera,Gaussian) with radius > 0 writes one (key,value) per touched
 * tile: key = (cam << tile_bits | tile_id) << 32 | float_bits(depth), value = cam*N + n, in
 * Gaussian-index then row-major tile order (gsplat isect_tiles, behind model.py:267-288). */
int qed_isect_scan(const int32_t* block_sums, int32_t n_blocks, int32_t* block_offsets,
                   int32_t* n_isect, int64_t capacity, int32_t* status, void* stream);
int qed_isect_emit(int32_t N, int32_t C, const float* means2d, const int32_t* radii, const float* depths,
                   const int32_t* tiles_per_gauss, const int32_t* block_offsets, int32_t tile_w,
                   int32_t tile_h, int32_t tile_bits, const int32_t* n_isect, int64_t capacity,
                   uint64_t* keys, int32_t* vals, void* stream);

/* ---- K4: device radix sort of (u64 key, i32 value) pairs, LSD, 8-bit digits, stable ------------
 * Sorts the first *n_dev (device int32, <= capacity) pairs on key bits [0, end_bit).  Ping-pongs
 * between (keys,vals) and (keys_alt,vals_alt); returns 0 if the sorted result is in (keys,vals),
 * 1 if it is in (keys_alt,vals_alt), <0 on error.  `workspace` needs
 * qed_sort_workspace_bytes(capacity) bytes. */
int64_t qed_sort_workspace_bytes(int64_t capacity);
int qed_sort_pairs(uint64_t* keys, int32_t* vals, uint64_t* keys_alt, int32_t* vals_alt,
                   const int32_t* n_dev, int64_t capacity, int32_t end_bit, void* workspace,
                   int64_t workspace_bytes, int32_t* status, void* stream);

/* ---- K3+K4+K5 in one call: two-stage tile binning (what rasterization() uses) ---------------------
 * Produces exactly the sorted list of qed_isect_emit + qed_sort_pairs + qed_tile_offsets (same
 * order, ties included) with ~3x less sort traffic: (A) the C*N (camera,Gaussian) slots are radix
 * sorted by their 32 depth bits, (B) intersections are emitted in that order with the 32-bit key
 * cam|tile and STABLY sorted on the tile bits only (2 passes at 1080p instead of 6 on 64-bit keys).
 * Outputs: flatten_ids[capacity] (first M valid), offsets[C*T+1] (offsets[C*T] = M), n_isect[1],
 * and, if isect_ids != NULL, the 64-bit keys (cam|tile) << 32 | depth_bits of the sorted list.
 * Overflow (M > capacity) sets status[0] = M and leaves M = 0.  workspace: qed_bin_workspace_bytes.
 * splats (may be NULL): the records of qed_project_fwd; when given, each Gaussian's tile rectangle is
 * taken from record slot 11 (the rectangle project_fwd counted) instead of being recomputed from
 * means2d / radii -- REQUIRED when project_fwd ran with QED_F_TIGHT_TILES.
 * tile_masks (may be NULL; needs splats): qed_project_fwd's per-slot masks -- REQUIRED when project_fwd wrote them
 * (tiles_per_gauss then counts the set bits, not the rectangle).
 * mode: QED_BIN_TWO_STAGE is the pipeline above.  QED_BIN_TILE_SORT gives the same list another way: entries
 * are emitted in slot order and stably sorted on the tile bits, then one workgroup per tile sorts its run by
 * the 32 depth bits (stable, in LDS for runs of <= 2048 entries, through global scratch beyond) -- no global
 * sort of the C*N slots, 10 launches instead of 23, faster while the runs are short.  QED_BIN_BUCKET gives the
 * same list in 6 launches: emit in slot order, ONE stable radix pass on the top <= 8 key bits (buckets of 2^s
 * consecutive cam|tile keys), one workgroup per bucket that stably orders it by the low s bits and writes its tiles'
 * offsets, then the per-tile depth sort of QED_BIN_TILE_SORT; keys of more than 16 cam|tile bits run the tile-sort
 * pipeline.  QED_BIN_AUTO picks by capacity per tile: the bucket pipeline for short runs, two-stage for long ones.  block_sums (may be NULL): qed_project_fwd's per-256-slot sums of tiles_per_gauss, which
 * save the tile-sort pipeline one counting launch.
 * host_words (may be NULL): int32[4], 16-byte aligned, in HOST-MAPPED memory (hipHostMalloc / a pinned torch tensor);
 * the call's last list kernel stores {M, status[0], status[1], 0} there in ONE 16-byte store.  A caller that wants the
 * count without blocking sets word 0 to -1 before the call and looks at it later (M >= 0 once the store has landed):
 * neither a device-to-host copy nor an event enters the stream. */
#define QED_BIN_AUTO 0
#define QED_BIN_TWO_STAGE 1
#define QED_BIN_TILE_SORT 2
#define QED_BIN_BUCKET 3
int64_t qed_bin_workspace_bytes(int64_t n_slots, int64_t capacity);
int qed_bin_tiles(int32_t N, int32_t C, const float* means2d, const int32_t* radii, const float* depths,
                  const int32_t* tiles_per_gauss, const float* splats, const uint64_t* tile_masks,
                  const int32_t* block_sums, int32_t tile_w, int32_t tile_h, int64_t capacity, int32_t mode,
                  int32_t* flatten_ids,
                  int32_t* offsets, int32_t* n_isect, uint64_t* isect_ids, void* workspace,
                  int64_t workspace_bytes, int32_t* status, int32_t* host_words, void* stream);

/* ---- K5: tile offsets --------------------------------------------------------------------------
 * offsets[C*T + 1]: offsets[t] = first sorted index whose (cam,tile) >= t; offsets[C*T] = M. */
int qed_tile_offsets(const uint64_t* sorted_keys, const int32_t* n_dev, int64_t capacity, int32_t C,
                     int32_t n_tiles, int32_t tile_bits, int32_t* offsets, void* stream);

/* ---- K6: alpha compositing forward -------------------------------------------------------------
 * One workgroup per 16x16 tile; front-to-back over the tile's run of the sorted list:
 * sigma = .5(a dx^2 + c dy^2) + b dx dy, alpha = min(.999, o e^-sigma), skip if sigma < 0 or
 * alpha < 1/255, stop (Gaussian not applied) when T(1-alpha) <= 1e-4.
 * channels = 3 (RGB) or 4 (RGB+D).  backgrounds[C,channels] may be NULL (model.py:267-288 passes
 * none).  Outputs render[C,H,W,channels], alpha[C,H,W], last_ids[C,H,W] i32.
 * t_final (may be NULL; [C,H,W]): receives every pixel's final transmittance T itself.  alpha = 1 - T loses up to
 * 3e-8 / T of it (a saturated pixel's alpha sits just below 1), and every gradient term of a pixel scales with its T:
 * qed_composite_bwd, given this image, reconstructs the transmittances from T instead of from 1 - alpha.
 * launch_flags: 0 in production.  One wave composites a whole tile, or one 8x8 quadrant of it for the
 * last tiles of a launch (finer work items fill the end of the launch); QED_CL_TILE_WAVES / _QUADRANT_WAVES
 * / _HALF_AND_HALF force one shape and QED_CL_NO_CULL turns the per-quadrant culling off -- results must
 * not change (parity tests).
 * tile_cost (may be NULL; [C*tiles][4] i32): receives, per tile and quadrant wave, the number of (Gaussian, quadrant)
 * visits + a staging term per batch -- the work predictor qed_composite_bwd orders its launch by.
 * tile_order (may be NULL; [C * tiles + 1]): a launch order for THIS kernel -- the order_ws an ordering job (qed_ssim_fwd_step,
 * or qed_composite_bwd's own) produced for an EARLIER frame of the same camera and tile grid.  The forward kernel cannot
 * know its tiles' costs in advance (the list length does not predict them), an earlier frame's counts do: heaviest tiles
 * first, 114-117 us against 122-126 at config B.  Must be a permutation of the tiles as those jobs write it (any valid
 * order gives the same image; a poor predictor only costs time).  NULL: raster order with a tail of quadrant waves. */
/* get_outputs' post-processing (model.py:295-297, 304-306) folded into the compositing kernels -- the reference-shaped route
 * then has no pass of its own over the image between the rasterizer and the loss, in either direction:
 *   qed_post_t (forward, may be NULL): rgb[C,H,W,3] = clamp(render[..., :3] + (1 - alpha) background[3], 0, 1) is written by
 *     the compositing kernel beside render; with a depth channel, depth[C,H,W] = alpha > 0 ? render[..., 3] : max render[..., 3]
 *     (one extra pass over alpha that patches the empty pixels; tile_dmax: C * tiles * 4 floats of scratch);
 *   qed_post_grad_t (backward, may be NULL): v_render / v_alpha are derived per pixel from v_rgb[C,H,W,3] and v_depth[C,H,W]
 *     (either may be NULL = no gradient) in the tile prologue: pass NULL for v_render and v_alpha; render = the forward
 *     pass's output.  Same arithmetic as qed_post_process_fwd / _bwd. */
typedef struct {
    const float* background;
    float* rgb;
    float* depth;
    float* tile_dmax;
} qed_post_t;
typedef struct {
    const float* background;
    const float* render;
    const float* v_rgb;
    const float* v_depth;
} qed_post_grad_t;
#define QED_CL_TILE_WAVES 1
#define QED_CL_QUADRANT_WAVES 2
#define QED_CL_HALF_AND_HALF 3
#define QED_CL_NO_CULL 4
#define QED_CL_ORDER_READY 8    /* qed_composite_bwd: order_ws already holds the launch order of this tile_cost
                                   (qed_ssim_fwd_step wrote it): no ordering launch in front of the kernel */
int qed_composite_fwd(int32_t C, int32_t N, const float* splats, const int32_t* flatten_ids,
                      const int32_t* offsets, int32_t width, int32_t height, int32_t tile_w,
                      int32_t tile_h, int32_t channels, const float* backgrounds, float* render,
                      float* alpha, float* t_final, int32_t* last_ids, int32_t* tile_cost,
                      const int32_t* tile_order, const qed_post_t* post, int32_t launch_flags, void* stream);

/* ---- K7: alpha compositing backward ------------------------------------------------------------
 * Back-to-front replay from last_ids; per-pixel gradients are reduced across each 64-wide wave
 * (one permlane level, the rest through LDS) and added once per (tile,Gaussian) to the
 * 64-byte row vsplat[C*N][16] (layout at qed_project_bwd; includes absgrad, model.py:284).
 * vsplat must be zeroed by the caller.
 * t_final (may be NULL; [C,H,W]): qed_composite_fwd's image of the final transmittances; with it render_alpha is not read
 * (1 - t_final is that alpha bit for bit).  NULL: T_final = 1 - render_alpha, as gsplat's backward pass forms it.
 * tile_cost (may be NULL; [C*tiles][4] i32, 16-byte aligned): what qed_composite_fwd wrote for the same list -- the
 * tiles are then handed out costliest first (greedy longest-processing-time scheduling of the launch; tiles heavier than
 * the average wave slot's whole share are dealt as four quadrant waves), ordered by one extra one-workgroup launch into
 * order_ws (C*tiles + 1 ints of scratch).  Same gradients up to the order of the float atomics. */
int qed_composite_bwd(int32_t C, int32_t N, const float* splats, const int32_t* flatten_ids,
                      const int32_t* offsets, int32_t width, int32_t height, int32_t tile_w,
                      int32_t tile_h, int32_t channels, const float* backgrounds,
                      const float* render_alpha, const float* t_final, const int32_t* last_ids,
                      const float* v_render, const float* v_alpha, float* vsplat, const int32_t* tile_cost, int32_t* order_ws,
                      const qed_post_grad_t* post, int32_t launch_flags, void* stream);

/* ---- blending contribution of every Gaussian over a view (pruning; importance.hip) ---------------
 * The walk of qed_composite_fwd over the same records, ids and offsets (same argument checks; flatten_ids may be NULL
 * when the list is empty) without colours and without per-pixel outputs.  At a pixel that is inside the image and
 * whose pixel_mask[C,H,W] byte (may be NULL = all set) is not 0, Gaussian i CONTRIBUTES where the forward pass applies
 * it: it passes the alpha test (sigma >= 0, alpha = min(.999, o e^-sigma) >= 1/255), the pixel has not terminated and
 * T (1 - alpha) > 1e-4; its weight is w = alpha T_before.  The Gaussian that terminates a pixel is not applied by the
 * renderer and has w = 0 there.  Records c * N + n of every camera c land on row n of three [N] buffers that
 * ACCUMULATE across calls (the caller zeroes them once):
 *   max_weight  the bit pattern of a non-negative float: max w (an unsigned integer max is the float max)
 *   sum_weight  unsigned 64-bit fixed point with 32 fractional bits: sum w.  Capacity 2^32 units of weight per
 *               Gaussian (every pixel of 2 000 views at 1920x1080 at alpha 0.999); not guarded
 *   hits        #{(view, pixel) : w > 0}
 * All three are integers updated with order-independent atomics (the sum of one (tile, Gaussian) is formed in a fixed
 * lane order in float and converted once, round to nearest): the same bits on every run, for any order of views.
 * N == 0 or an empty list leaves the buffers untouched.  launch_flags: QED_CL_NO_CULL is honoured (identical results);
 * the launch-shape bits are ignored (always one wave per tile). */
int qed_contribution(int32_t C, int32_t N, const float* splats, const int32_t* flatten_ids, const int32_t* offsets,
                     int32_t width, int32_t height, int32_t tile_w, int32_t tile_h, const uint8_t* pixel_mask /* [C,H,W] or NULL */,
                     uint32_t* max_weight, uint64_t* sum_weight, uint32_t* hits, int32_t launch_flags, void* stream);

/* Keep flags and slots of a prune, in the form qed_densify_emit reads: row i is kept when score[i] > min_score, or
 * score[i] == min_score and i < tie_below (ties by row index; a NaN score is never kept).  flags[N] receives 4 (keep the
 * old row) or 0, pos (qed_densify_pos_ints(N) ints) the slot of every kept row in column 1, totals[4] = {0, K, 0, 0}. */
int qed_prune_classify(int32_t N, const double* score, double min_score, int32_t tie_below, uint8_t* flags,
                       int32_t* pos, int32_t* totals, void* stream);

/* ---- K8: fused image-space loss + gradient ------------------------------------------------------
 * Collapses model.py:295-297 (background composite + clamp), :304-306 (depth fix-up), :87-116
 * (masked depth-L1, depth_lambda) and the L1 part of the parent's RGB loss into one pass.
 * Pass 1 (qed_loss_reduce) fills per-workgroup partials in sums[QED_LOSS_SUMS_FLOATS] (only {n_valid,
 * max depth} are needed before gradients; the two loss sums are accumulated by pass 2, which leaves
 * sums[0..3] = {sum|rgb-gt|, sum|d-dgt|, n_valid, max depth}); pass 2 (qed_loss_grad) writes v_render[H,W,channels] and v_alpha[H,W] for
 *   loss = rgb_weight * mean|rgb - gt| + depth_lambda * sum|d - dgt| / n_valid
 * and the scalar losses -> losses[0..2] = {rgb term, depth term, their sum}.  mask[H,W] may be
 * NULL; when given it multiplies the rendered AND the ground-truth image before the L1 (and the SSIM)
 * term, as the parent's get_loss_dict does behind model.py:83-85, and both depths (model.py:93-97).
 * An additional term on the same clamped colour (the SSIM part of the
 * parent's loss, qed_ssim_* below) enters through v_rgb_extra[H,W,3] = its gradient w.r.t. rgb and
 * extra_sum[extra_n] (qed_ssim_fwd's per-workgroup partials): losses[0] += extra_offset + extra_scale * sum(extra_sum);
 * both pointers may be NULL. */
int qed_loss_reduce(int32_t n_pix, int32_t channels, const float* render, const float* alpha,
                    const float* background, const float* gt_rgb, const float* gt_depth,
                    const float* mask, float* sums, void* stream);
int qed_loss_grad(int32_t n_pix, int32_t channels, const float* render, const float* alpha,
                  const float* background, const float* gt_rgb, const float* gt_depth,
                  const float* mask, const float* sums, float rgb_weight, float depth_lambda,
                  float* v_render, float* v_alpha, float* losses, const float* v_rgb_extra,
                  const float* extra_sum, int32_t extra_n, float extra_scale, float extra_offset, void* stream);

/* ---- SSIM term of the parent's RGB loss (reached from model.py:83-85) ----------
 * pytorch_msssim semantics: data_range 1, 11-tap Gaussian window (sigma 1.5) applied separably with
 * no padding, K = (0.01, 0.03), mean over the (H-10) x (W-10) map and 3 channels.
 * pred is either a plain [H,W,3] image (alpha == NULL) or the compositor's render[H,W,channels]
 * together with alpha[H,W] and background[3], in which case the colour clamp(render + (1-alpha) bg)
 * of model.py:296-297 is formed on the fly.  qed_ssim_fwd writes one partial sum of the SSIM map per workgroup into
 * ssim_sum[qed_ssim_sum_floats(H, W)] (SSIM = sum of them / (3 (H-10)(W-10)); nothing to zero, no same-address
 * atomics) and, unless maps == NULL (value only: the rgb_ssim metric), the
 * coefficient maps (qed_ssim_maps_floats floats) that
 * qed_ssim_bwd turns into v_pred[H,W,3] = scale * (scale_dev ? scale_dev[0] : 1) * d ssim_sum / d colour
 * (scale_dev: an upstream gradient that lives in device memory).  mask[H,W] (may be NULL) multiplies
 * both images before the SSIM, as the parent's loss does; v_pred is the gradient w.r.t. the colour
 * BEFORE that multiply. */
int64_t qed_ssim_maps_floats(int32_t height, int32_t width);
int64_t qed_ssim_sum_floats(int32_t height, int32_t width);
int qed_ssim_fwd(int32_t height, int32_t width, int32_t channels, const float* pred, const float* alpha,
                 const float* background, const float* gt_rgb, const float* mask, float* maps,
                 float* ssim_sum, void* stream);
int qed_ssim_bwd(int32_t height, int32_t width, int32_t channels, const float* pred, const float* alpha,
                 const float* background, const float* gt_rgb, const float* mask, const float* maps,
                 float scale, const float* scale_dev, float* v_pred, void* stream);
/* qed_ssim_fwd of the fused training step, with two optional PASSENGERS riding in the same launch instead of in launches of
 * their own on the step's critical chain:
 *  - tile_cost != NULL: one extra workgroup sorts the tiles of the compositing backward that follows by the cost
 *    qed_composite_fwd counted (tile_cost[n_tiles][4], n_tiles = C * tile_w * tile_h) and leaves the launch order in
 *    order_ws[n_tiles + 1] -- pass that order_ws to qed_composite_bwd with QED_CL_ORDER_READY;
 *  - sums != NULL: pass 1 of the image loss, exactly qed_loss_reduce(height * width, channels, render, ..., gt_depth, mask,
 *    sums), as extra workgroups (no separate qed_loss_reduce call then).
 * render / alpha / background as in qed_ssim_fwd's composite mode (alpha must be given). */
int qed_ssim_fwd_step(int32_t height, int32_t width, int32_t channels, const float* render, const float* alpha,
                      const float* background, const float* gt_rgb, const float* mask, float* maps,
                      float* ssim_sum, const int32_t* tile_cost, int64_t n_tiles, int32_t* order_ws,
                      const float* gt_depth, float* sums, void* stream);

/* qed_ssim_bwd and qed_loss_grad in ONE launch (the fused training step), after qed_ssim_fwd and qed_loss_reduce on
 * the same buffers: every thread of the SSIM backward pass finishes its pixels on the spot -- SSIM gradient (scale
 * ssim_scale = -ssim_lambda / (3 (H-10)(W-10))) + L1 gradient through the clamp and the background composite
 * (model.py:296-297) -> v_render[H,W,channels] / v_alpha[H,W], depth-L1 gradient (model.py:87-116, :304-306) into channel
 * 3 -- instead of handing v_pred to a second pass that re-reads render, alpha and the ground truth (116 MB at 1080p).
 * losses[0..2] as qed_loss_grad with extra_sum = ssim_sum, extra_scale = ssim_scale, extra_offset = ssim_offset (=
 * ssim_lambda); sums is qed_loss_reduce's workspace (which also zeroes the slots this pass adds its loss sums to).
 * zero_buf (may be NULL; 16-byte aligned, zero_floats a multiple of 4): a buffer the same launch zeroes -- the vsplat
 * accumulator qed_composite_bwd needs zeroed, which saves the fill launch in front of that kernel.
 * tick (may be NULL): the optimiser's device-resident step state is advanced by the one-workgroup fold launch of this call
 * (what qed_adam_step_dev / qed_adam_step_sh otherwise do in a one-thread launch of their own: this call sits between
 * the previous step's Adam launches and this step's); follow with qed_adam_step_sh(parts | QED_ADAM_PART_TICKED). */
typedef struct {
    float* dev_state;        /* as qed_adam_step_dev */
    double beta1, beta2;     /* doubles, as the Adam entry points take them: the bias corrections are formed in double */
    float* dev_lr_slot;     /* NULL, or &dev_lr[scheduled group]: receives the exponential decay of qed_lr_exp_decay_dev */
    float lr_init, lr_final;
    int32_t max_steps;
    const int32_t* skip_flag; /* NULL, or as qed_adam_step's: non-zero -> the state is not advanced */
} qed_adam_tick_t;
int qed_loss_grad_ssim(int32_t height, int32_t width, int32_t channels, const float* render, const float* alpha,
                       const float* background, const float* gt_rgb, const float* gt_depth, const float* mask,
                       const float* maps, float* sums, float rgb_weight, float depth_lambda, float ssim_scale,
                       float* v_render, float* v_alpha, float* losses, const float* ssim_sum,
                       int32_t ssim_sum_n, float ssim_offset, float* zero_buf, int64_t zero_floats,
                       const qed_adam_tick_t* tick, void* stream);

/* qed_ssim_bwd and qed_image_losses_bwd in ONE launch (get_loss_dict's backward): v_rgb[H,W,3] = g_main[0] * d main_loss /
 * d rgb (the L1 term joins the SSIM term inside the SSIM backward pass, which has the pixel's colours at hand) and
 * v_depth[H,W] (may be NULL) = g_depth[0] * d depth_loss / d depth.  sums: qed_image_losses_fwd's; maps: qed_ssim_fwd's;
 * ssim_scale = -ssim_lambda / (3 (H-10)(W-10)); g_depth may be NULL (no upstream gradient: zeros).  zero_buf (may be
 * NULL): as qed_loss_grad_ssim's -- the accumulator the compositing backward that follows adds into. */
int qed_image_losses_ssim_bwd(int32_t height, int32_t width, const float* rgb, const float* depth,
                              const float* gt_rgb, const float* gt_depth, const float* mask, const float* maps,
                              const float* sums, float rgb_weight, float depth_lambda, float ssim_scale,
                              const float* g_main, const float* g_depth, float* v_rgb, float* v_depth,
                              float* zero_buf, int64_t zero_floats, void* stream);

/* ---- the same arithmetic behind the reference's OWN call sequence --------------------------------
 * get_outputs() returns images and get_loss_dict() turns them into a dict of scalar losses that the
 * trainer sums and differentiates; each half is one autograd node on the host side.
 *
 * qed_post_process_fwd/bwd = model.py:295-297 + 304-306:
 *   rgb[H,W,3] = clamp(render[..., :3] + (1 - alpha) background, 0, 1)
 *   depth[H,W] = alpha > 0 ? render[..., 3] : max(render[..., 3])      (channels == 4; max is detached)
 * workspace: QED_LOSS_SUMS_FLOATS floats.  bwd: v_rgb / v_depth (either may be NULL) -> v_render, v_alpha.
 *
 * qed_image_losses_fwd/bwd = the parent's main loss (behind model.py:83-85) + the depth term (:87-116):
 *   losses[0] = rgb_weight * mean|m rgb - m gt| + extra_offset + extra_scale * sum(extra_sum[0 .. extra_n))
 *   losses[1] = depth_lambda * sum|m d - m dgt| / n_valid   (finite & dgt > 0; 0 when nothing is valid)
 * with extra_* the SSIM term (qed_ssim_fwd on the same images).  depth / gt_depth / mask may be NULL.
 * sums: QED_LOSS_SUMS_FLOATS floats, kept for the backward.  bwd: v_rgb = g_main[0] * d losses[0] / d rgb
 * (accumulate != 0: added to what qed_ssim_bwd left there), v_depth = g_depth[0] * d losses[1] / d depth;
 * g_main / g_depth are DEVICE scalars (NULL = 0): the trainer may weight or scale each term. */
int qed_post_process_fwd(int32_t n_pix, int32_t channels, const float* render, const float* alpha,
                         const float* background, float* rgb, float* depth, float* workspace, void* stream);
int qed_post_process_bwd(int32_t n_pix, int32_t channels, const float* render, const float* alpha,
                         const float* background, const float* v_rgb, const float* v_depth,
                         float* v_render, float* v_alpha, void* stream);
int qed_image_losses_fwd(int32_t n_pix, const float* rgb, const float* depth, const float* gt_rgb,
                         const float* gt_depth, const float* mask, float rgb_weight, float depth_lambda,
                         const float* extra_sum, int32_t extra_n, float extra_scale, float extra_offset,
                         float* sums, float* losses, void* stream);
int qed_image_losses_bwd(int32_t n_pix, const float* rgb, const float* depth, const float* gt_rgb,
                         const float* gt_depth, const float* mask, const float* sums, float rgb_weight,
                         float depth_lambda, const float* g_main, const float* g_depth, int32_t accumulate,
                         float* v_rgb, float* v_depth, void* stream);

/* ---- per-step evaluation metrics (model.py:120-197, metrics.py:84-156) ----------
 * One streaming pass, results left in DEVICE memory (the reference synchronises ~12 times per step
 * with .item()).  out[10] = {rgb_mse, rgb_psnr, depth_abs_rel, depth_sq_rel, depth_rmse,
 * depth_rmse_log, depth_a1, depth_a2, depth_a3, n_valid_depth}; the depth entries are NaN when no
 * pixel is valid (metrics.py:134-143) or when pred_depth/gt_depth are NULL; the rgb entries are NaN
 * when pred_rgb/gt_rgb are NULL.  pred_rgb, gt_rgb: [n_pix,3]; depths: [n_pix]; valid depth =
 * finite(pred) & finite(gt) & gt > tolerance (0.1 in the reference).  workspace: QED_METRICS_WS_DOUBLES
 * doubles (per-workgroup partial sums; no zeroing needed).
 * rgb_ssim is qed_ssim_fwd's value; rgb_lpips is the qed_lpips_* entry points' (weights are supplied by the caller). */
int qed_image_metrics(int32_t n_pix, const float* pred_rgb, const float* gt_rgb, const float* pred_depth,
                      const float* gt_depth, float tolerance, double* workspace, float* out, void* stream);
/* Everything get_metrics_dict (model.py:120-197) needs from one training step's images in ONE streaming pass + ONE fold,
 * with what get_loss_dict (model.py:73-118) needs from the same images riding along -- two launches instead of the eight
 * short ones of qed_image_metrics + the SSIM map's sum + qed_nanmean_exp + qed_image_losses_fwd:
 *   out[0..9]  as qed_image_metrics;
 *   out[10]    rgb_ssim = ssim_norm * sum(ssim_sum[0 .. ssim_n))  (qed_ssim_fwd's partials; ssim_norm = 1 / (3 (H-10)(W-10));
 *              NaN when ssim_sum is NULL);
 *   out[11]    avg_min_scale = nanmean_i exp(scales[i * scale_stride]), i < n_scales (model.py:192-194; NaN when NULL);
 *   losses[3], loss_sums[QED_LOSS_SUMS_FLOATS] (both may be NULL): exactly what qed_image_losses_fwd(rgb_weight,
 *              depth_lambda, extra = the SSIM term with weight ssim_lambda, mask = loss_mask) would write for the same
 *              images -- get_loss_dict then launches nothing in its forward pass.
 * workspace: QED_STEP_METRICS_WS_DOUBLES doubles. */
int qed_step_metrics(int32_t n_pix, const float* pred_rgb, const float* gt_rgb, const float* pred_depth,
                     const float* gt_depth, float tolerance, const float* ssim_sum, int32_t ssim_n, float ssim_norm,
                     const float* scales, int32_t n_scales, int32_t scale_stride, const float* loss_mask,
                     float rgb_weight, float depth_lambda, float ssim_lambda, float* loss_sums, float* losses,
                     double* workspace, float* out, void* stream);
/* out[0] = nanmean_i exp(x[i * stride]), i < n (NaN when nothing is left) -- the "avg_min_scale" entry of
 * get_metrics_dict (model.py:192-194).  workspace: QED_METRICS_WS_DOUBLES doubles. */
int qed_nanmean_exp(int32_t n, const float* x, int32_t stride, double* workspace, float* out, void* stream);

/* ---- LPIPS (AlexNet) from user-supplied weights: the rgb_lpips entry (metrics.py:83-112) ------------------------------
 * The two images travel as a batch of two; feature maps are NHWC, float32[2][h][w][C].  Layers l = 0..4:
 *   Cin -> Cout  3 -> 64, 64 -> 192, 192 -> 384, 384 -> 256, 256 -> 256;  kernel 11, 5, 3, 3, 3;  stride 4, 1, 1, 1, 1;
 *   padding 2, 2, 1, 1, 1.  Output size of a layer: (in + 2 pad - kernel) / stride + 1.
 * qed_lpips_conv: out[2][ho][wo][Cout] = relu(bias + conv(in)), in0 / in1 = the two inputs [in_h][in_w][Cin] (for l > 0
 *   the two halves of the previous map).  l = 0 applies the input scaling (x - shift) / scale to the taps inside the
 *   image; a padded tap is 0.  weights: the layer's filters packed as [Kp][Np], row k = (kh * kernel + kw) * Cin + c,
 *   column = output channel, Kp = K rounded up to QED_LPIPS_TILE_K, Np = Cout rounded up to QED_LPIPS_TILE_N, zero in the
 *   padding (qed_lpips_packed_floats(l) = Kp * Np; host arithmetic).  float32 in, float32 accumulation in the order
 *   k = 0, 1, 2, ... (the f32-input matrix instruction): the same input gives the same bits.
 * qed_lpips_pool: 3x3 max-pool, stride 2, no padding, floor, of in[2][in_h][in_w][channels]; in front of l = 1 and l = 2.
 * qed_lpips_distance: layer l's map feat[2][height][width][Cout] and its lin[Cout] -> per-workgroup partial sums of
 *   sum_c lin[c] (f0[c] / sqrt(eps + |f0|^2) - f1[c] / sqrt(eps + |f1|^2))^2, eps = 1e-8, in its fifth of `workspace`
 *   (QED_LPIPS_WS_DOUBLES doubles, no zeroing needed).
 * qed_lpips_finalize: after the five distance launches; n_pix0..4 = height * width of the five maps.  out[6] (device) =
 *   {the LPIPS value, the five per-layer means}; folded in float64 in a fixed order, no atomics, no host synchronisation.
 * Refused on the host: a layer outside 0..4, sizes below the window or beyond 32768, null buffers. */
#define QED_LPIPS_TILE_K 16
#define QED_LPIPS_TILE_N 64
#define QED_LPIPS_WS_DOUBLES (5 * 256)
int64_t qed_lpips_packed_floats(int32_t layer);
int qed_lpips_conv(int32_t layer, int32_t in_h, int32_t in_w, const float* in0, const float* in1, const float* weights,
                   const float* bias, float* out, void* stream);
int qed_lpips_pool(int32_t channels, int32_t in_h, int32_t in_w, const float* in, float* out, void* stream);
int qed_lpips_distance(int32_t layer, int32_t height, int32_t width, const float* feat, const float* lin,
                       double* workspace, void* stream);
int qed_lpips_finalize(int64_t n_pix0, int64_t n_pix1, int64_t n_pix2, int64_t n_pix3, int64_t n_pix4,
                       const double* workspace, float* out, void* stream);

/* ---- densification / culling ---------------------------------------------------
 * GPU side of the parent class's callbacks that consume model.py:249,289-292 (self.xys.absgrad,
 * self.radii, self.last_size): SplatfactoModel.after_train / refinement_after / split_gaussians /
 * dup_gaussians / cull_gaussians / dup_in_all_optim / remove_from_all_optim, restated in
 * oracle/densify_oracle.py.  All buffers are the flat [means | scales | quats | opacities |
 * features_dc | features_rest] layout of this package.
 *
 * qed_densify_accumulate (every step): for radii > 0: vis_counts += 1, xys_grad_norm +=
 *   |absgrad| (absgrad = [N] rows of 2 floats, stride_floats apart), max_2Dsize = max(., radii *
 *   inv_max_dim) with inv_max_dim = 1 / max(H, W).
 * qed_densify_classify: flags[N] (bit0 split, bit1 duplicate, bit2 keep old, bit3 keep children,
 *   bit4 keep duplicate), pos[4][N] exclusive scans {split rank, kept-old slot, kept-children slot,
 *   kept-duplicate slot} followed by 4 * ceil(N/256) ints of scratch (qed_densify_pos_ints), totals[4] = {n_split, K_old, K_child, K_dup} (device).  densify = 0 is the
 *   cull-only pass after stop_split_at.  Negative split_screen_size / cull_scale_thresh /
 *   cull_screen_size switch the corresponding test off (step-dependent in the reference).
 * qed_densify_emit: writes the N' = K_old + n_samples * K_child + K_dup rows of the new parameter and
 *   Adam-moment buffers in the reference's order [kept old | children (sample-major) | duplicates];
 *   children: mean + R(q/|q|) (exp(scale) * samples[s * n_split + split_rank]), scale = log(exp(s)/1.6),
 *   zero moments.  h_totals = totals copied to the host (the caller needs N' to allocate).
 * qed_densify_reset_opacity: opacities = min(opacities, max_logit), opacity moments = 0. */
int qed_densify_accumulate(int32_t N, const float* absgrad, int32_t stride_floats, const int32_t* radii,
                           float inv_max_dim, float* xys_grad_norm, float* vis_counts, float* max_2Dsize,
                           void* stream);
int64_t qed_densify_pos_ints(int32_t N);
int qed_densify_classify(int32_t N, const float* scales, const float* opacities, const float* xys_grad_norm,
                         const float* vis_counts, const float* max_2Dsize, int32_t densify,
                         float half_max_dim, float densify_grad_thresh, float densify_size_thresh,
                         float split_screen_size, float cull_alpha_thresh, float cull_scale_thresh,
                         float cull_screen_size, uint8_t* flags, int32_t* pos, int32_t* totals, void* stream);
int qed_densify_emit(int32_t N, int32_t n_samples, const uint8_t* flags, const int32_t* pos,
                     const int32_t* h_totals, const float* samples, const float* old_params,
                     const float* old_exp_avg, const float* old_exp_avg_sq, const int64_t* h_old_begin,
                     float* new_params, float* new_exp_avg, float* new_exp_avg_sq,
                     const int64_t* h_new_begin, void* stream);
int qed_densify_reset_opacity(int32_t N, float* opacities, float* exp_avg, float* exp_avg_sq,
                              float max_logit, void* stream);

/* ---- depth back-projection for the initial point cloud --------------------------
 * Geometry of qed-init-pc's backproject_frame (create_init_pointcloud.py:148-196): every stride-th pixel
 * (u, v) with a finite depth 0 < d < depth_max becomes the world point c2w * ((u-cx) d/fx, (v-cy) d/fy, d)
 * (Open3D create_from_depth_image with depth_scale 1).  h_c2w_opengl: HOST pointer to the OpenGL
 * camera-to-world pose, row-major with row stride 4 (a 3x4 or 4x4 matrix); the OpenCV flip of
 * _opengl_c2w_to_opencv_w2c (:61-70) is applied inside.  points[capacity,3] receives the points in
 * row-major pixel order, n_points[1] their number; more than `capacity` sets status[0] to the number
 * needed and n_points to 0.  workspace: qed_backproject_workspace_ints ints. */
int64_t qed_backproject_workspace_ints(int32_t height, int32_t width, int32_t stride);
int qed_backproject_depth(int32_t height, int32_t width, const float* depth, float fx, float fy, float cx,
                          float cy, const float* h_c2w_opengl, float depth_max, int32_t stride,
                          int64_t capacity, float* points, int32_t* n_points, int32_t* workspace,
                          int32_t* status, void* stream);

/* ---- colouring the initial point cloud (qed-init-pc --colorize; create_init_pointcloud.py:264-390) --------
 * qed_colorize_accumulate: one batch of F >= 1 frames of one size height x width against N points.
 *   points[N,3] float; depth[F,H,W] float, the RAW file values: the kernel multiplies by depth_unit_scale_factor in
 *   fp32 and treats non-finite / <= 0 as "no measurement" (:310-312); color[F,H,W,3] uint8.
 *   h_c2w_opengl: HOST pointer to F OpenGL camera-to-world poses as 4x4 row-major DOUBLES (transforms.json's
 *   transform_matrix); the OpenCV world-to-camera matrix of _opengl_c2w_to_opencv_w2c (:59-68) is formed on the host
 *   by flipping columns 1, 2 and inverting the 4x4 generally in float64, then cast to fp32 (a singular pose is refused).
 *   h_intrinsics: HOST pointer to F x (fx, fy, cx, cy).
 *   Per (point, frame): p = w2c [x y z 1] in fp32; z = p.z must be finite and > 1e-6; u = fx (p.x / z) + cx, v
 *   likewise; finite u, v, z <= depth_max, -0.5 <= u < W - 0.5, -0.5 <= v < H - 0.5; ui = rint(u) (half to even), vi
 *   likewise; measured = depth[vi, ui]; hit iff measured > 0 && |measured - z| <= max(depth_tolerance,
 *   depth_tolerance_rel z).  A hit adds float(c / 255) per channel to color_sum[N,3] (float64) and 1 to
 *   color_count[N] (int32); the caller zeroes both before the first batch.  Each point owns its accumulator and the
 *   frames are taken in order, so any split of a frame sequence into batches gives bit-identical sums.
 * qed_colorize_finalize: colors[N,3] uint8 = (uint8) clip(sum / count * 255, 0, 255) in float64, TRUNCATED as
 *   NumPy's astype(uint8) does (:378-383); points never hit stay (0,0,0); n_colored[1] = number of points with count > 0.
 * No allocation, no sync; capturable. */
int qed_colorize_accumulate(int32_t N, const float* points, int32_t F, int32_t height, int32_t width,
                            const float* depth, float depth_unit_scale_factor, const uint8_t* color,
                            const double* h_c2w_opengl, const float* h_intrinsics, float depth_max,
                            float depth_tolerance, float depth_tolerance_rel, double* color_sum,
                            int32_t* color_count, void* stream);
int qed_colorize_finalize(int32_t N, const double* color_sum, const int32_t* color_count, uint8_t* colors,
                          int32_t* n_colored, void* stream);

/* ---- voxel down-sampling of a point cloud (qed-init-pc step 1: per frame, per merge, at the end) ------------
 * One output point per occupied voxel: the mean of its members.  Voxel of a point = (floorf(x / v), floorf(y / v),
 * floorf(z / v)) with v = voxel_size and a correctly rounded fp32 division; sums in float64, rounded to fp32 once.
 * out_points[n,3] receives the means in ascending (ix, iy, iz) order, n_out[1] (device) their number.  The result
 * is a pure function of the input (no floating-point atomics; a fixed combination order): bit-identical between
 * calls, streams and occupancies.  A point with a non-finite coordinate is dropped.
 * status[QED_STATUS_WORDS] (device): [0] = 1 when an axis spans more than 2^21 voxels (62 km at 3 cm): refused,
 * n_out = 0; [1] = points dropped as non-finite; [2] = the widest axis span in voxels.
 * Refused on the host: voxel_size not finite or <= 0, n < 0 or >= 2^30, null buffers, a workspace smaller than
 * qed_voxel_workspace_bytes(n) (8-byte aligned).  n == 0 gives n_out = 0.  No allocation, no sync. */
int64_t qed_voxel_workspace_bytes(int64_t n);
int qed_voxel_down_sample(int32_t n, const float* points, float voxel_size, float* out_points, int32_t* n_out,
                          void* workspace, int64_t workspace_bytes, int32_t* status, void* stream);
/* The same down-sampling carrying n_attrs (1 to QED_VOXEL_MAX_ATTRS) float attribute columns and a weight per point:
 * points[n,3], attrs[n,n_attrs], weights[n] or NULL (every weight 1).  Per occupied voxel, with the sums over its members i:
 *   out_points = Sum w_i p_i / Sum w_i,  out_attrs = Sum w_i a_i / Sum w_i,  out_weights = Sum w_i,
 * products and sums in float64, each result rounded to fp32 once.  Voxel membership, the ascending key order, the fixed
 * combination order and the status words are qed_voxel_down_sample's; with weights == NULL out_points equals its
 * out_points bit for bit and out_weights holds the member counts.  A point with a non-finite coordinate, attribute or
 * weight, or with a weight <= 0, is dropped and counted in status[1].  No floating-point atomics: the same input gives
 * the same bits.  The mean of a voxel's members lies in that voxel, so with ONE voxel size the weighted merge of clouds
 * that were down-sampled already equals down-sampling their concatenation once, up to rounding.
 * Refused on the host: as qed_voxel_down_sample, and n_attrs outside 1 .. QED_VOXEL_MAX_ATTRS; workspace:
 * qed_voxel_attr_workspace_bytes(n, n_attrs) (8-byte aligned). */
#define QED_VOXEL_MAX_ATTRS 8
int64_t qed_voxel_attr_workspace_bytes(int64_t n, int32_t n_attrs);
int qed_voxel_down_sample_attr(int32_t n, const float* points, int32_t n_attrs, const float* attrs, const float* weights,
                               float voxel_size, float* out_points, float* out_attrs, float* out_weights, int32_t* n_out,
                               void* workspace, int64_t workspace_bytes, int32_t* status, void* stream);

/* ---- exact nearest neighbours between two point clouds, and PDMetrics' reductions (metrics.py:9-63) -------------
 * For every query point: the distance to, and the row of, the nearest point of the target cloud (what cKDTree.query
 * returns with k = 1).  Points are [n,3] fp32 and finite (the caller checks: a non-finite coordinate makes that row's
 * result unspecified, though every access stays in bounds; status[1] of qed_nn_build counts the target's).
 * The result is defined once: d2 = fma(dz, dz, fma(dy, dy, dx * dx)) on fp32 differences target - query, distance =
 * sqrtf(d2), and among targets of equal fp32 d2 the smallest row wins.  The grid path and the brute-force path both
 * return exactly that, bit for bit, whatever the cell size, max_rings, the order of the queries or of the launches'
 * workgroups (integer min only; no floating-point atomics).
 * qed_nn_build: a sparse uniform grid over the target in `workspace` (qed_nn_workspace_bytes(n_target,
 *   n_query_capacity) bytes, 16-byte aligned; it also holds the scratch of qed_nn_query for up to n_query_capacity
 *   queries).  cell_size > 0, or flags = QED_NN_AUTO_CELL: chosen on the device so that an occupied cell holds a
 *   handful of points (cell_size is then ignored).  A cell size that would need more than 2^20 cells on an axis is
 *   enlarged: no finite cloud is refused.  status[QED_STATUS_WORDS] (device): [1] = non-finite target points.
 * qed_nn_query: the grid search.  Shells of cells of growing Chebyshev radius around the query's cell until the best
 *   distance cannot be beaten from outside the visited box (exact).  A query not finished after max_rings shells is
 *   NOT written; its row goes to fallback[1 ..], fallback[0] (device) = their number (fallback: 1 + n_query int32).
 *   Pass that list to qed_nn_brute with the same dist / idx.  `target` is not needed: the index holds a copy.
 *   flags: QED_NN_NATURAL_ORDER takes the queries in row order instead of the order of their cell in the target's grid.
 * qed_nn_brute: every target against the rows of `rows` (rows[0] = count on the device, rows[1 ..] = row ids; the
 *   other rows of dist / idx are left alone) or, rows == NULL, against all n_query rows.  workspace: 8 n_query bytes.
 * qed_pd_reduce: count_under[0] (device int64) = number of dist[i] whose float64 value is < threshold; order_stats[2]
 *   (device) = the k0-th and the min(k0 + 1, n - 1)-th smallest distance (0-based): the two NumPy's "linear" percentile
 *   reads at k0 = floor((n - 1) p / 100).  workspace: qed_pd_workspace_bytes(n).
 * Refused on the host: counts out of range (n_target < 1, n < 1, negative or >= 2^30), cell_size not finite or <= 0
 * without QED_NN_AUTO_CELL, max_rings outside [0, 64], unknown flags, null buffers, a short workspace.
 * No allocation, no sync. */
#define QED_NN_NATURAL_ORDER 1
#define QED_NN_AUTO_CELL 2
int64_t qed_nn_workspace_bytes(int64_t n_target, int64_t n_query_capacity);
int qed_nn_build(int32_t n_target, const float* target, float cell_size, int32_t flags, void* workspace,
                 int64_t workspace_bytes, int64_t n_query_capacity, int32_t* status, void* stream);
int qed_nn_query(int32_t n_query, const float* query, int32_t n_target, void* workspace, int64_t workspace_bytes,
                 int64_t n_query_capacity, int32_t max_rings, int32_t flags, float* dist, int32_t* idx,
                 int32_t* fallback, void* stream);
int qed_nn_brute(int32_t n_query, const float* query, int32_t n_target, const float* target, const int32_t* rows,
                 float* dist, int32_t* idx, void* workspace, int64_t workspace_bytes, void* stream);
int64_t qed_pd_workspace_bytes(int64_t n);
int qed_pd_reduce(int32_t n, const float* dist, double threshold, int64_t k0, int64_t* count_under,
                  float* order_stats, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- exact k nearest neighbours on the index of qed_nn_build, and the seed initialisation of the Gaussians ----------
 * Definition (the k = 1 definition above, applied k times): a candidate is the packed word bits(d2) << 32 | row with
 * d2 = fma(dz, dz, fma(dy, dy, dx * dx)) on fp32 differences target - query; the answer of a query is its k smallest
 * candidates in ascending order of the packed word (ascending d2, among equal d2 ascending row).  It is a pure
 * function of the two fp32 clouds, bit for bit: it does not depend on the cell size, max_rings, the order of the
 * queries (QED_NN_NATURAL_ORDER), the order of the workgroups or the path (grid or brute force).
 * dist[n_query, k] = sqrtf(d2) and idx[n_query, k] (int32), row-major.  1 <= k <= 8.
 * flags: QED_KNN_SKIP_FIRST computes the k + 1 smallest and drops the smallest (k_nearest_sklearn's [:, 1:]): for a cloud
 *   queried against itself that removes the point itself, for duplicated points one of the zeros.
 * qed_knn_query: the shell walk of qed_nn_query on the same workspace (built by qed_nn_build, same sizes); a query
 *   stops once its list is full and its largest entry is closer than everything outside the visited box.  A query
 *   not finished after max_rings shells is NOT written; its row goes to fallback[1 ..] as for qed_nn_query.
 *   flags may also hold QED_NN_NATURAL_ORDER.
 * qed_knn_brute: every target against the rows of `rows` (same convention as qed_nn_brute), one wave per query; no
 *   workspace.
 * Refused on the host: k outside [1, 8], n_target < k (k + 1 with QED_KNN_SKIP_FIRST), and what qed_nn_query /
 * qed_nn_brute refuse (counts, max_rings, unknown flags, null buffers, a short workspace).
 *
 * qed_seed_gaussians: splatfacto's initialisation of five parameter groups from dist[n, k] (qed_knn_query on the cloud
 *   itself with QED_KNN_SKIP_FIRST), one launch, written straight into the caller's (views of the flat) buffers:
 *   scales[n,3] = logf(max(mean_j dist[i,j], min_distance)) in all three columns; quats[n,4] = (sqrt(1-u) sin 2 pi v,
 *   sqrt(1-u) cos 2 pi v, sqrt(u) sin 2 pi w, sqrt(u) cos 2 pi w) with u, v, w in [0, 1) a function of (seed, row);
 *   opacities[n] = logit(0.1); features_dc[n,3] = (c / 255 - 0.5) / 0.28209479177387814 for sh_coeffs > 1,
 *   logit(c / 255, eps = 1e-10) for sh_coeffs == 1 (both in float64, rounded once), uniform [0, 1) for colors_u8 ==
 *   NULL; features_rest[n, sh_coeffs - 1, 3] = 0 (may be NULL for sh_coeffs == 1).  status[QED_STATUS_WORDS]
 *   (device, zeroed by the call): [0] = rows whose mean distance was below min_distance.  flags: 0.
 * qed_seed_random_points: points[n,3] = (uniform [0, 1) - 0.5) * scale, a function of (seed, element).
 * Refused on the host: n negative or >= 2^30, k outside [1, 8], sh_coeffs outside [1, 16], min_distance negative or not
 * finite, unknown flags, null buffers.  No allocation, no sync. */
#define QED_KNN_SKIP_FIRST 4
int qed_knn_query(int32_t n_query, const float* query, int32_t n_target, void* workspace, int64_t workspace_bytes,
                  int64_t n_query_capacity, int32_t k, int32_t max_rings, int32_t flags, float* dist, int32_t* idx,
                  int32_t* fallback, void* stream);
int qed_knn_brute(int32_t n_query, const float* query, int32_t n_target, const float* target, const int32_t* rows,
                  int32_t k, int32_t flags, float* dist, int32_t* idx, void* stream);
int qed_seed_gaussians(int32_t n, const float* dist, int32_t k, const uint8_t* colors_u8, int32_t sh_coeffs,
                       uint64_t seed, float min_distance, int32_t flags, float* scales, float* quats, float* opacities,
                       float* features_dc, float* features_rest, int32_t* status, void* stream);
int qed_seed_random_points(int32_t n, uint64_t seed, float scale, float* points, void* stream);

/* ---- fused multi-tensor Adam over one flat parameter buffer (config.py:44-68) --
 * n_groups contiguous segments; segment g covers elements [h_group_begin[g], h_group_begin[g+1])
 * and uses learning rate h_lr[g].  bias corrections use `step` (1-based).  The betas are doubles: 1 - beta is
 * formed in double and rounded once, as torch.optim.Adam's Python scalars are (exp_avg_sq then agrees to 1e-6).
 * skip_flag (may be NULL; all three Adam entry points and qed_adam_tick_t): a DEVICE word; when it is non-zero
 * the launch updates nothing.  Pass qed_bin_tiles' status[0]: a frame whose intersection list overflowed its
 * buffer renders empty, and a step enqueued behind it without a host round trip must not train on it. */
int qed_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                  int32_t n_groups, const int64_t* h_group_begin, const float* h_lr, double beta1,
                  double beta2, float eps, int32_t step, const int32_t* skip_flag, void* stream);

/* Same update with the step state and learning rates in DEVICE memory, so that a captured hipGraph
 * can be replayed: dev_state[3] = {step, 1/(1-beta1^step), 1/sqrt(1-beta2^step)} is advanced by one
 * (zero it before the first step), dev_lr[8] holds the per-group learning rates.  Both factors are formed from the
 * double betas at double precision and rounded once: they agree with qed_adam_step's to float rounding at every step. */
int qed_adam_step_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                      int32_t n_groups, const int64_t* h_group_begin, const float* dev_lr, double beta1,
                      double beta2, float eps, float* dev_state, const int32_t* skip_flag, void* stream);

/* Adam step that never materialises the SH-coefficient gradients.  Every group is [N, width]; the LAST
 * two must be features_dc [N,3] and features_rest [N,KR,3].  Their gradient is the rank-1 product
 *   g[n][k][c] = scale * sum_{view} b_k(direction of Gaussian n from that view's camera) * v_views[view][n][c]
 * (what qed_sh_grad_from_views would write), evaluated on the fly from the 3 N clamp-masked colour
 * gradients qed_project_bwd leaves with QED_F_SH_GRAD_COMPACT; `grads` is read for the other groups only
 * (v_views may point into it).  `means` are the positions the views were rendered with (normally the
 * means group of `params`: the SH launch, which reads them, precedes the launch that updates them).
 * State: either device (dev_state + dev_lr as qed_adam_step_dev; h_lr and step ignored; with
 * sched_group >= 0 the same tick launch first sets dev_lr[sched_group] to the exponential decay of
 * qed_lr_exp_decay_dev for the step about to be taken) or host (h_lr + 1-based step; dev_* NULL,
 * sched_group < 0).  Saves, for one camera per step at 500 k Gaussians, 96 MB written + 96 MB read; for
 * data-parallel steps also the rebuild pass.
 * `parts`: QED_ADAM_PART_SH (the tick + the two SH groups: needs the gathered views only), QED_ADAM_PART_LEADING
 * (the other groups: needs `grads`), or both (3).  A data-parallel step issues the SH part while the all-reduce of
 * the leading groups' gradients is still on the wire, then the leading part -- in that order (see `means`), with the
 * same `step`; with device state only the SH part advances it. */
#define QED_ADAM_PART_SH 1
#define QED_ADAM_PART_LEADING 2
#define QED_ADAM_PART_TICKED 4   /* device state already advanced for this step (qed_loss_grad_ssim's tick) */
int qed_adam_step_sh(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                     int32_t n_groups, const int64_t* h_group_begin, const float* h_lr, float* dev_lr,
                     double beta1, double beta2, float eps, int32_t step, float* dev_state,
                     int32_t sched_group, float sched_lr_init, float sched_lr_final,
                     int32_t sched_max_steps, int32_t N, int32_t sh_degree, const float* means,
                     int32_t n_views, const float* viewmats, int64_t viewmat_stride,
                     const float* v_views, int64_t view_stride, float scale, int32_t parts,
                     const int32_t* skip_flag, void* stream);

/* ExponentialDecayScheduler of one group (the reference schedules "means": 1.6e-4 -> 1.6e-6 over
 * 30000 steps, config.py:46-51) from the device step counter, for graph replay: dev_lr_slot[0] =
 * exp((1-t) log lr_init + t log lr_final), t = clip(dev_state[0] / max_steps, 0, 1).  Call it before
 * qed_adam_step_dev (dev_state[0] is then the 0-based index of the step about to be taken). */
int qed_lr_exp_decay_dev(float* dev_lr_slot, const float* dev_state, float lr_init, float lr_final,
                         int32_t max_steps, void* stream);

/* ---- bilateral grid (the reference's use_bilateral_grid, model.py:299-302; nerfstudio 1.1.x lib_bilagrid) ---------
 * One slab grid[12, L, Y, X] per training image: a 3x4 affine colour transform (row-major) at every lattice vertex;
 * grid_shape (X, Y, L) = splatfacto's (16, 16, 8) by default, every extent >= 2.
 * qed_bilagrid_slice_fwd: out[H,W,3] = A[:, :3] rgb + A[:, 3], A = the slab trilinearly sliced at
 *   x = j (X-1)/(W-1), y = i (Y-1)/(H-1), z = (0.299 r + 0.587 g + 0.114 b)(L-1)  (clipped to [0, L-1]),
 * i.e. F.grid_sample(align_corners=True, padding_mode="border") at linspace coordinates and guidance 2 gray - 1.
 * qed_bilagrid_slice_bwd: v_out[H,W,3] -> v_rgb[H,W,3] (A^T v_out plus the term through the guidance, 0 where the
 * clipped z sits at or beyond either end) and v_grid[12,L,Y,X] (written, not accumulated; float atomics: the last bits
 * may differ from run to run).  workspace: 12 L Y X floats (cleared by the call).
 * qed_bilagrid_tv_fwd: out[0] = (1/N) sum over d in {L, Y, X} of sum((g[d+1] - g[d])^2) / numel(difference along d) of
 * grids[N,12,L,Y,X] (block partials, fixed-order fold: deterministic).  workspace: QED_BILAGRID_TV_WS_DOUBLES doubles.
 * qed_bilagrid_tv_bwd: v_grids[N,12,L,Y,X] = v_tv[0] * d tv / d grids (written; v_tv is a DEVICE scalar). */
#define QED_BILAGRID_TV_WS_DOUBLES 1024
int qed_bilagrid_slice_fwd(int32_t height, int32_t width, const float* rgb, const float* grid, int32_t gx, int32_t gy,
                           int32_t gl, float* out, void* stream);
int qed_bilagrid_slice_bwd(int32_t height, int32_t width, const float* rgb, const float* grid, int32_t gx, int32_t gy,
                           int32_t gl, const float* v_out, float* v_rgb, float* v_grid, float* workspace, void* stream);
int qed_bilagrid_tv_fwd(int32_t n_grids, const float* grids, int32_t gx, int32_t gy, int32_t gl, float* out,
                        double* workspace, void* stream);
int qed_bilagrid_tv_bwd(int32_t n_grids, const float* grids, int32_t gx, int32_t gy, int32_t gl, const float* v_tv,
                        float* v_grids, void* stream);

/* The fused training route's grid group (bilagrid.BilateralGridOptimizer).
 * qed_bilagrid_slice_bwd_acc: qed_bilagrid_slice_bwd's kernel alone -- v_rgb[H,W,3] written, the slab's gradient ADDED
 *   into slab_ws[Y][X][L][12] (channel-last, the caller's persistent buffer; neither cleared nor re-laid-out here).
 * qed_bilagrid_step: ONE launch over grids[N,12,L,Y,X]: g = tv_weight * d tv / d grids (qed_bilagrid_tv_bwd's
 *   definition and weights, from the values the grids hold before the launch) + for grid `row` (-1: none) slab_ws,
 *   then torch.optim.Adam's update in place on grids / exp_avg / exp_avg_sq (the arithmetic of qed_adam_step; `step`
 *   is 1-based).  slab_ws is zeroed after it is read.  skip_flag (may be NULL): a device word; non-zero leaves grids and
 *   moments untouched (slab_ws is zeroed all the same; grad_out is then not written).  grad_out[N,12,L,Y,X] (may be
 *   NULL): the gradient used.  One workgroup per (grid, channel) volume, staged in LDS: L * Y * X <= 16384. */
#define QED_BILAGRID_STEP_MAX_VOLUME 16384
int qed_bilagrid_slice_bwd_acc(int32_t height, int32_t width, const float* rgb, const float* grid, int32_t gx, int32_t gy,
                               int32_t gl, const float* v_out, float* v_rgb, float* slab_ws, void* stream);
int qed_bilagrid_step(int32_t n_grids, float* grids, float* exp_avg, float* exp_avg_sq, int32_t gx, int32_t gy,
                      int32_t gl, float tv_weight, int32_t row, float* slab_ws, float lr, double beta1, double beta2,
                      float eps, int32_t step, float* grad_out, const int32_t* skip_flag, void* stream);

/* ---- MCMC densification (splatfacto strategy="mcmc"; gsplat MCMCStrategy) -------------------------------------------
 * Flat buffers as qed_densify_emit's: six groups means, scales (log), quats, opacities (logit), features_dc,
 * features_rest, each [N, width], h_*begin[7] their element offsets (+ end), starting at 0.  sigma = sigmoid(logit).
 * Draws are proportional to sigma over the rows with sigma > min_opacity: weights sigma 2^32 rounded (>= 1) and their
 * exact uint64 prefix, searched with an integer uniform.  Every random number is a function of (seed, counter, row) --
 * of (seed, step, row) for the noise -- so equal arguments give bit-identical results.  workspace: device memory of
 * qed_mcmc_workspace_bytes(N, n_draws) bytes (n_draws = N for qed_mcmc_relocate, n_add for qed_mcmc_add).
 * qed_mcmc_sample: out_idx[n_draws] = rows drawn with replacement (a zero total weight draws row k mod N).
 * qed_mcmc_relocate (in place, no host read-back): the dead rows D = {sigma <= min_opacity} draw one live source each
 *   (or take sources[i], i in D: a live row; other entries are not read).  Per source drawn c times, ratio =
 *   min(c + 1, 51): sigma' = 1 - (1 - sigma)^(1/ratio) clamped to [min_opacity, 1 - 2^-23], scales *= sigma /
 *   sum_{j=1..ratio} C(ratio,j) (-1)^(j-1) sigma'^j / sqrt(j) (fp64), both Adam moments of the source zeroed in every
 *   group; then every group of each dead row <- its source.  The dead rows' moments are left as they were.  n_dead
 *   (may be NULL): device int32, |D|.
 * qed_mcmc_add: n_add draws over all rows with sigma > 0 (or sources[n_add], in [0, N)); the sources are updated as
 *   above with ratio = 1 + times drawn, IN PLACE in `params`; the new buffers [N + n_add rows] hold the N rows (moments
 *   kept) followed by one copy of each draw with zero moments.
 * qed_mcmc_noise: means += Sigma (eps gate lr noise_lr), Sigma = R diag(s^2) R^T (R of the normalised wxyz quaternion),
 *   gate = sigmoid(100 ((1 - sigma) - 0.995)), eps = noise[N,3] or standard normals of (seed, step, row).  dev_lr /
 *   dev_state (may be NULL) replace lr / step by dev_lr[0] / dev_state[0] (qed_adam_step_dev's state: the launch can
 *   then be replayed from a hipGraph).  skip_flag: as the Adam entry points' (non-zero: no update).
 * qed_mcmc_reg: out (may be NULL) = {lo mean(sigma), ls mean(exp(scales)) over 3N, their sum} from a fixed-order fold of
 *   block partials (deterministic; workspace QED_MCMC_REG_WS_DOUBLES doubles); grad_opacities[N] += lo sigma(1-sigma)/N
 *   and grad_scales[N,3] += ls exp(scale)/(3N), each times *v_*_reg (DEVICE scalars; NULL = 1), when given. */
#define QED_MCMC_REG_WS_DOUBLES 2048
int64_t qed_mcmc_workspace_bytes(int32_t N, int64_t n_draws);
int qed_mcmc_sample(int32_t N, const float* opacities, float min_opacity, int64_t n_draws, uint64_t seed,
                    uint64_t counter, int32_t* out_idx, void* workspace, int64_t workspace_bytes, void* stream);
int qed_mcmc_relocate(int32_t N, float* params, float* exp_avg, float* exp_avg_sq, const int64_t* h_group_begin,
                      float min_opacity, const int32_t* sources, uint64_t seed, uint64_t counter, int32_t* n_dead,
                      void* workspace, int64_t workspace_bytes, void* stream);
int qed_mcmc_add(int32_t N, int32_t n_add, float* params, const float* exp_avg, const float* exp_avg_sq,
                 const int64_t* h_old_begin, float min_opacity, const int32_t* sources, uint64_t seed, uint64_t counter,
                 float* new_params, float* new_exp_avg, float* new_exp_avg_sq, const int64_t* h_new_begin,
                 void* workspace, int64_t workspace_bytes, void* stream);
int qed_mcmc_noise(int32_t N, float* means, const float* scales, const float* quats, const float* opacities,
                   const float* noise, float lr, const float* dev_lr, float noise_lr, int64_t step,
                   const float* dev_state, uint64_t seed, const int32_t* skip_flag, void* stream);
int qed_mcmc_reg(int32_t N, const float* scales, const float* opacities, float opacity_reg, float scale_reg,
                 float* out, float* grad_scales, float* grad_opacities, const float* v_opacity_reg,
                 const float* v_scale_reg, double* workspace, void* stream);

/* ---- the ground truth of one training frame, from a cached dataset frame (csrc/ingest.hip) ------------------------
 * What the parent's get_gt_img + composite_with_background and the loss mask (model.py:88-97) make of batch["image"],
 * batch["depth_image"] and batch["mask"], in ONE launch: d x d box means (d in 1..8; Ho = height / d, Wo = width / d,
 * the remainder rows and columns dropped).
 *   image  [height,width,channels], channels 3 or 4: uint8 (scaled by 1/255) or, with image_is_f32, float32
 *   depth  [height,width]: uint16 (times depth_scale) or, with depth_is_f32, float32 (depth_scale is not read); NULL:
 *          no depth plane (gt_depth is not written)
 *   mask   [height,width] bytes, non-zero = 1, or NULL;  background[3] floats
 *   gt_rgb [Ho,Wo,3]: the channel means, with 4 channels composited AFTER averaging: a rgb + (1 - a) background
 *   gt_depth [Ho,Wo]: the mean, zeros included;  gt_mask [Ho,Wo] (NULL without mask): the mean of 0 / 1
 * Integer inputs are summed exactly and scaled once (uint8: sum * (1.0f / (255 d^2)); uint16: sum * (depth_scale / d^2));
 * float inputs are summed in row-major block order and multiplied by 1 / d^2.  At d = 1 float inputs pass through.
 * Refused on the host: d outside 1..8, channels not 3 or 4, an empty output, NULL buffers.  No allocation, no sync. */
int qed_ingest_ground_truth(int32_t height, int32_t width, int32_t d, const void* image, int32_t channels,
                            int32_t image_is_f32, const void* depth, int32_t depth_is_f32, float depth_scale,
                            const uint8_t* mask, const float* background, float* gt_rgb, float* gt_depth,
                            float* gt_mask, void* stream);

/* ---- a distorted dataset frame resampled to a pinhole (csrc/undistort.hip) -----------------------------------------
 * What nerfstudio's datamanager does on the CPU to every frame of a camera with distortion, while the image cache is
 * filled: ONE launch over all planes of a frame.  The definitions are written out in qed_splatter_amd/undistort.py.
 * Per output pixel (j, i): x = (j + 0.5 - cx') / fx', y likewise under new_K; (xd, yd) = distort(x, y);
 * (u, v) = (fx xd + cx, fy yd + cy) under src_K -- evaluated in float64 from the float32 parameters, the blend in float32.
 *   model  0: OPENCV  rad = 1 + k1 r2 + k2 r2^2 + k3 r2^3, xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2),
 *             yd = y rad + p1 (r2 + 2 y^2) + 2 p2 x y  (k4 must be 0)
 *          1: OPENCV_FISHEYE  t = atan(r), td = t (1 + k1 t^2 + k2 t^4 + k3 t^6 + k4 t^8), (xd, yd) = (td / r)(x, y),
 *             the identity at r = 0  (p1, p2 must be 0)
 *   src_K[4], new_K[4] = (fx, fy, cx, cy), dist[6] = (k1, k2, k3, k4, p1, p2): HOST arrays, read during the call and
 *          passed to the kernel by value
 *   image  [height,width,channels] uint8, channels 3 or 4 -> out_image, same shape: bilinear at (u - 0.5, v - 0.5),
 *          taps outside the source read 0, floor(value + 0.5); alpha is interpolated like any channel
 *   depth  [height,width] uint16 or, with depth_is_f32, float32 -> out_depth, same type: the nearest tap
 *          (floor(u), floor(v)), 0 outside the source; both NULL: no depth plane
 *   mask   [height,width] bytes -> out_mask, 0 / 1 bytes: (nearest tap != 0), 0 outside; both NULL: no mask
 *   out_coords [height,width,2] float32 = (u, v), or NULL (for tests and diagnosis)
 * Outputs must not alias inputs.  Refused on the host: channels not 3 or 4, a frame smaller than 2 x 2 or larger than
 * qed_ingest_ground_truth's limit, an unknown model, coefficients the model does not have, non-positive focal lengths,
 * NULL buffers.  No allocation, no sync, nothing is read back. */
int qed_undistort_frame(int32_t height, int32_t width, const uint8_t* image, int32_t channels, const void* depth,
                        int32_t depth_is_f32, const uint8_t* mask, const float* src_K, const float* new_K,
                        const float* dist, int32_t model, uint8_t* out_image, void* out_depth, uint8_t* out_mask,
                        float* out_coords, void* stream);

/* ---- trained Gaussians to and from the rows of a 3DGS PLY file (csrc/export.hip) -------------------------------------
 * The file format is stated in qed_splatter_amd/gaussian_ply.py.  A row of color_mode 0 (sh_coeffs) is 17 + 3 K floats,
 * K = (sh_degree + 1)^2 - 1:  x y z  nx ny nz (zeros)  f_dc[3]  f_rest[3 K] (channel-major: features_rest[N,K,3]
 * transposed)  opacity (logit)  scale[3] (log)  rot[4] (wxyz, as stored).  A row of color_mode 1 (rgb) is 59 bytes: the
 * three colour bytes clamp(SH_C0 f_dc + 0.5, 0, 1) * 255 truncated (sh_degree 0: the sigmoid of f_dc) stand where f_dc
 * and f_rest stood, and features_rest is not read.
 * qed_pack_gaussians drops a row if one of its values (rgb mode: f_dc instead of the bytes) is not finite, else if its
 * opacity is below -5.5373f = logit(1 / 255); the rows kept are written to `rows` in input order without gaps.
 *   counts[3] (device): rows written, dropped as non-finite, dropped as transparent
 *   rows      16-byte aligned, room for N rows; bytes behind the last kept row are not written
 *   workspace qed_pack_workspace_bytes(N)
 * Three launches (count, scan of the per-workgroup counts, pack): a row's position does not depend on scheduling.
 * qed_unpack_gaussians reads N rows of row_bytes bytes each: h_offsets[14 + 3 K] (HOST) holds the byte offset inside a
 * row of every float32 column, in the order means[3] scales[3] quats[4] opacity f_dc[3] features_rest[K][3] -- the
 * caller finds the columns by name, so a file may order them freely and carry others.  At least 4 readable bytes behind
 * every offset; no alignment is asked of rows, row_bytes or the offsets.
 * Both take an optional similarity p' = s (R p + t): h_similarity[17] (HOST doubles) = R (row-major), t, s, the
 * quaternion of R (wxyz), and h_sh[83] = the band matrices of R, 3 x 3, 5 x 5 and 7 x 7 row-major, for which
 * c'_band = D_band c_band.  Means go through the map, log-scales get + log s, quaternions are left-multiplied, the
 * coefficients of bands 1-3 are multiplied per channel; each new value is accumulated in float64 and rounded once.
 * Both NULL: every value is moved bit for bit.  (pack classifies the values AFTER the map.)
 * Refused on the host: N < 1, sh_degree outside 0..3, NULL buffers, a scale that is not positive and finite, an offset
 * outside the row.  No allocation, no sync, nothing is read back. */
int64_t qed_pack_workspace_bytes(int64_t N);
int qed_pack_gaussians(int32_t N, int32_t sh_degree, int32_t color_mode, const float* means, const float* scales,
                       const float* quats, const float* opacities, const float* features_dc, const float* features_rest,
                       const double* h_similarity, const double* h_sh, uint8_t* rows, int32_t* counts, void* workspace,
                       int64_t workspace_bytes, void* stream);
int qed_unpack_gaussians(int32_t N, int32_t sh_degree, const uint8_t* rows, int64_t row_bytes, const int32_t* h_offsets,
                         const double* h_similarity, const double* h_sh, float* means, float* scales, float* quats,
                         float* opacities, float* features_dc, float* features_rest, void* stream);

/* ---- a rendered frame finished for image files (csrc/present.hip) --------------------------------------------------
 * get_outputs' float planes of one frame -- rgb [height,width,3], depth [height,width], alpha [height,width] (the
 * accumulation) -- turned into the integer planes an image writer stores.  A pixel is VALID when alpha > 0 and its depth
 * is finite and > 0.  clamp(x, 0, 1) = fminf(fmaxf(x, 0), 1), which sends NaN to 0; fmaf is ONE rounding.
 *
 * qed_present_range writes (min, max) of the depth over the valid pixels into range_out (device float[2]); (0, 0) if no
 * pixel is valid.  It zeroes range_out itself (a memset on `stream`) and combines the workgroups of its one launch through
 * integer atomics on the bit patterns of the positive floats: the result does not depend on the order.
 *
 * qed_present_frame writes, in one launch, every plane whose pointer is not NULL:
 *   out_rgb8 [height,width,3]      floor(fmaf(clamp(x, 0, 1), 255, 0.5)).  NaN gives 0.
 *   out_alpha8 [height,width]      the same rule on alpha.
 *   out_depth16 [height,width]     uint16, little-endian.  0 where alpha <= 0 or the depth is not finite or <= 0 (0 is the
 *                                  dataset's "no measurement", as qed_ingest_ground_truth's readers take it); otherwise
 *                                  min(65535, floor(fmaf(depth, inv_depth_unit, 0.5))).  inv_depth_unit is a float32 the
 *                                  host computes in float64 as 1 / (dataparser_scale * depth_unit_scale_factor).
 *   out_depthmap8 [height,width,3] t = clamp((depth - lo) * inv_span, 0, 1), where (lo, hi) = range_dev[0], range_dev[1]
 *                                  if range_dev (device float[2], qed_present_range's result, never read back) is not
 *                                  NULL, else the host's near, far; inv_span = 1 / (hi - lo) in float32, or 0 when
 *                                  hi <= lo.  k = min(255, (int)(t * 255)) (truncation, as Nerfstudio's
 *                                  apply_depth_colormap indexes its table).  c = fmaf(alpha_c, lut[k][ch] - 255, 255)
 *                                  with alpha_c = clamp(alpha, 0, 1): the colour over white by accumulation.  The stored
 *                                  byte is floor(c + 0.5f).  Pixels that are not valid are white.
 *   lut                            device uint8[256][3], any alignment.
 * The fast path (a lane owns four consecutive pixels, every store is a whole dword) needs rgb, depth and alpha 16-byte
 * aligned and the outputs dword-aligned; any other alignment takes a per-pixel path with the same results.
 * Refused on the host: an empty or too large frame, NULL alpha, no output at all, an output whose input is NULL
 * (out_rgb8: rgb; out_depth16: depth; out_depthmap8: depth and lut), an inv_depth_unit that is not positive and finite
 * when out_depth16 is asked for, NaN near / far when they are read, misaligned element pointers.  No allocation, no sync,
 * nothing is read back. */
int qed_present_range(int32_t height, int32_t width, const float* depth, const float* alpha, float* range_out,
                      void* stream);
int qed_present_frame(int32_t height, int32_t width, const float* rgb, const float* depth, const float* alpha,
                      float inv_depth_unit, const float* range_dev, float near, float far, const uint8_t* lut,
                      uint8_t* out_rgb8, uint16_t* out_depth16, uint8_t* out_depthmap8, uint8_t* out_alpha8, void* stream);

/* ---- camera pose optimiser: Nerfstudio's CameraOptimizer, mode SO3xR3 (csrc/pose.hip) -------------------------------
 * pose_adjustment[n_rows, 6], one row per training camera: columns 0:3 the translation d, 3:6 the rotation vector w.
 *   a = sqrt(max(|w|^2, 1e-4));  R = I + (sin a / a) K + ((1 - cos a) / a^2) K^2,  K = skew(w)
 *   c2w_opt[3,4] = c2w[3,4] [[R, d], [0, 0, 0, 1]]            (R_opt = R0 R, t_opt = R0 d + t0)
 * Below the clamp (|w| < 0.01) the angle is held at 0.01 and passes no gradient, as upstream.  sinf / cosf are the precise
 * ones.  Camera c of a call uses row rows[c] (device int32) or, with rows == NULL, row0 + c (a batch of all rows: C =
 * n_rows, row0 = 0); a rows[c] outside [0, n_rows) gives NaN outputs.  The regulariser is
 *   trans_l2_penalty * mean_rows |d| + rot_l2_penalty * mean_rows |w|     (gradient 0 at a zero row).
 *
 * qed_pose_apply: c2w_out[C,3,4] from c2w_in[C,3,4], one launch; reg_out (device float, may be NULL) receives the
 *   regulariser's value over ALL rows.
 * qed_pose_apply_bwd: v_rows[C,6] = the gradient of each camera's row for the gradient v_c2w[C,3,4] of c2w_out.
 * qed_pose_step: everything a training step does for the poses after qed_project_bwd, in one one-workgroup launch.
 *   v_viewmats[1,4,4] is the buffer qed_project_bwd accumulated for the view matrix rendered from qed_pose_apply's result
 *   for row `row` of c2w_in[1,3,4]; it is read and ZEROED for the next step.  The gradient goes back through get_viewmat
 *   (flip of the y / z columns, rigid inverse: the chain rule of those statements) and through the composition to the row;
 *   the regulariser's gradient is added to every row; torch.optim.Adam's update (no weight decay, no amsgrad; `step`
 *   1-based, betas doubles as for qed_adam_step) runs over all n_rows x 6 elements with rate lr.  raw_grad[n_rows,6]
 *   (may be NULL) receives the gradient the update used, reg_out (may be NULL) the regulariser's value BEFORE the update.
 *   row = -1: no camera this step (c2w_in may be NULL).  skip_flag as qed_adam_step's: non-zero -> the buffer is zeroed,
 *   nothing else is written but reg_out.
 * Refused on the host: null buffers, n_rows outside [1, 2^24), rows outside pose_adjustment, step < 1.  No allocation, no
 * sync. */
int qed_pose_apply(int32_t C, int32_t n_rows, const float* pose_adjustment, const int32_t* rows, int32_t row0,
                   const float* c2w_in, float* c2w_out, float trans_l2_penalty, float rot_l2_penalty, float* reg_out,
                   void* stream);
int qed_pose_apply_bwd(int32_t C, int32_t n_rows, const float* pose_adjustment, const int32_t* rows, int32_t row0,
                       const float* c2w_in, const float* v_c2w, float* v_rows, void* stream);
int qed_pose_step(int32_t n_rows, int32_t row, float* pose_adjustment, float* exp_avg, float* exp_avg_sq,
                  const float* c2w_in, float* v_viewmats, float trans_l2_penalty, float rot_l2_penalty, float lr,
                  double beta1, double beta2, float eps, int32_t step, float* raw_grad, float* reg_out,
                  const int32_t* skip_flag, void* stream);

/* ---- colour correction of an evaluation render against its ground truth (csrc/color_correct.hip) --------------------
 * nerfstudio's lib_bilagrid.color_correct (a port of multinerf's), what SplatfactoModelConfig.color_corrected_metrics
 * applies before cc_psnr / cc_ssim / cc_lpips.  With x = img, r = ref ([n_pix,3], values in [0,1]),
 * unclipped(z) = (z >= eps) & (z <= 1 - eps) and mask0 = unclipped(img), num_iters times:
 *   a(x) = (rr, rg, rb, gg, gb, bb, r, g, b, 1);  m_c = mask0[c] & unclipped(x[c]) & unclipped(r[c]);
 *   w_c = the least-squares solution of (m_c a) w = m_c r[c];  x <- clip(a(x) [w_0 w_1 w_2], 0, 1) on ALL pixels.
 * out[n_pix,3] receives the last x (num_iters == 0: img itself).  warps_out (device double[num_iters][3][10], may be
 * NULL) receives every iteration's w_c, [iteration][channel][feature]; the pixels are warped with these values rounded to
 * float32, in float32.  The sums of the normal equations are carried in double and solved in double by Cholesky with
 * diagonal pivoting: a column whose remaining pivot is <= 1e-10 x the largest original diagonal entry is dropped and its
 * coefficient is 0 (upstream's lstsq returns the minimum-norm solution instead; the fitted values on the pixels of the
 * fit are the same).  A channel without an unmasked pixel gets w = 0.  A pixel with a non-finite value in img or ref
 * takes part in no fit, for every eps; where it is warped its non-finite values are read as 0, and with num_iters >= 1 out
 * holds no NaN (num_iters == 0 copies img bit for bit, non-finite values included).  2 num_iters + 1 launches, no allocation, nothing is read back, no floating-point atomics: the same input gives
 * the same bits.  workspace: QED_COLOR_CORRECT_WS_DOUBLES doubles (no zeroing needed).  Rejected: num_iters outside
 * [0, QED_COLOR_CORRECT_MAX_ITERS], eps outside [0, 0.5), NULL or misaligned pointers. */
#define QED_COLOR_CORRECT_MAX_ITERS 8
#define QED_COLOR_CORRECT_MAX_GRID 512        /* workgroups of the summing pass */
#define QED_COLOR_CORRECT_SUMS_STRIDE 196     /* doubles per workgroup: 3 x (55 + 10) sums, padded */
#define QED_COLOR_CORRECT_WS_DOUBLES (QED_COLOR_CORRECT_MAX_GRID * QED_COLOR_CORRECT_SUMS_STRIDE + 120)
int qed_color_correct(int32_t n_pix, const float* img, const float* ref, int32_t num_iters, float eps,
                      double* workspace, double* warps_out, float* out, void* stream);

/* ---- normal maps at evaluation / rendering time (csrc/normals.hip) ----------------------------------------------------
 * A Gaussian's normal, one (camera, Gaussian) slot per thread.  means[N,3], RAW quats[N,4] (wxyz), scales[N,3] (with
 * QED_F_LOG_SCALES in `flags`: logarithms), viewmats[C,4,4]:
 *   k = the index of the smallest scale (lowest index on an exact tie);  n_w = column k of R(q / |q|) (a zero quaternion:
 *   n_w = 0, never NaN);  o = -R_v^T t the camera origin of the view matrix;  n_w is negated where dot(n_w, mean - o) > 0,
 *   so it faces the camera;  the result is n_w (QED_NORMALS_WORLD) or R_v n_w (QED_NORMALS_CAMERA: the OpenCV frame of
 *   `viewmats`, x right, y down, z forward -- a surface facing the camera has n_z < 0).
 * normals_out[C,N,3] (may be NULL).  splats / splats_out (both may be NULL): splats_out[C*N][12] receives the record of
 * qed_project_fwd with slots 6, 7, 8 (r, g, b) replaced by the normal and every other slot copied bit for bit (culled
 * slots and the packed rectangle of slot 11 included); 16-byte aligned, must not overlap `splats`.  ONE call of
 * qed_composite_fwd with channels = 3, splats_out, the colour pass's own flatten_ids / offsets and no background then
 * gives the accumulated normal A(p) = Sum_i alpha_i T_i n_i with the weights of the colour image: no second projection, no
 * second binning.  N == 0 or C == 0 launches nothing. */
#define QED_NORMALS_WORLD 0
#define QED_NORMALS_CAMERA 1
int qed_gaussian_normals(int32_t N, int32_t C, const float* means, const float* quats, const float* scales,
                         const float* viewmats, const float* splats, int32_t frame, uint32_t flags,
                         float* normals_out, float* splats_out, void* stream);
/* One pass over an image.  accum[H,W,3] = A, alpha[H,W], depth = the accumulated depth D, read at depth[p * depth_stride]
 * (1: a plain [H,W] map; 4: channel 3 of an RGB+D render, passed as render + 3):
 *   normal[H,W,3] = A / |A| where alpha >= min_alpha and |A| > 1e-8, else 0;
 *   surface depth z = D / alpha where alpha >= min_alpha (alpha == NULL: z = D); invalid where not finite or <= 0;
 *   P(x,y) = ((x + .5 - cx) / fx z, (y + .5 - cy) / fy z, z);  dx = P(x+1,y) - P(x-1,y), dy = P(x,y+1) - P(x,y-1);
 *   depth_normal[H,W,3] = normalize(dy x dx) -- (0, 0, -1) for a fronto-parallel plane -- and 0 at every border pixel (so
 *   everywhere in an image under 3 x 3), where the pixel or one of its four neighbours is invalid, and where
 *   |dy x dx| <= 1e-20.  The stencil is evaluated in double from the float32 inputs.
 *   valid[H,W] u8: QED_NV_NORMAL | QED_NV_DEPTH_NORMAL.  rgb8 (may be NULL; [H,W,3] u8): the usual colouring for files,
 *   round(255 (.5 + .5 (n_x, -n_y, -n_z))), a facing surface blue-violet, black = undefined -- of `normal` in
 *   qed_normal_maps (of the depth normal when accum == NULL), of the depth normal in qed_depth_normals.
 * accum / normal may be NULL (bit 0 stays clear), depth_normal may be NULL.  qed_depth_normals is the alpha-free half with
 * the same body, for a sensor depth map. */
#define QED_NV_NORMAL 1
#define QED_NV_DEPTH_NORMAL 2
int qed_normal_maps(int32_t height, int32_t width, const float* accum, const float* alpha, const float* depth,
                    int32_t depth_stride, float fx, float fy, float cx, float cy, float min_alpha, float* normal,
                    float* depth_normal, uint8_t* valid, uint8_t* rgb8, void* stream);
int qed_depth_normals(int32_t height, int32_t width, const float* depth, int32_t depth_stride, float fx, float fy,
                      float cx, float cy, float* depth_normal, uint8_t* valid, uint8_t* rgb8, void* stream);
/* Angular error between two normal images a, b [n_pix,3] (unit vectors where valid).  A pixel counts where
 * (valid_a[i] & bits_a) and (valid_b[i] & bits_b) are non-zero and mask (u8, may be NULL) is non-zero.  Its angle is
 * atan2(|a x b|, a . b) in radians (well conditioned at 0 and pi, where acos of a float32 dot product is not).
 * angle[n_pix] (may be NULL) receives it, NaN where the pixel does not count.  out[5] (device doubles) = {sum of angles,
 * count, count of angles < t0, < t1, < t2} (the first n_thresholds of them, 0 to 3; radians).  Sums are carried in double
 * and folded in a fixed order (2 launches, no floating-point atomics): the same input gives the same bits.
 * workspace: QED_ANGULAR_WS_DOUBLES doubles (no zeroing needed). */
#define QED_ANGULAR_WS_DOUBLES (5 * 1024)
int qed_angular_error(int32_t n_pix, const float* a, const float* b, const uint8_t* valid_a, uint32_t bits_a,
                      const uint8_t* valid_b, uint32_t bits_b, const uint8_t* mask, int32_t n_thresholds, float t0,
                      float t1, float t2, double* workspace, float* angle, double* out, void* stream);

/* ---- normal supervision in training (csrc/normal_loss.hip) ---------------------------------------------------------------
 * The loss is dn-splatter's normal loss RESTATED FROM MEMORY of that project, not checked against it.  Per pixel p:
 *   n^(p) = A(p) / |A(p)| where alpha(p) >= min_alpha and |A(p)| > 1e-8 (qed_normal_maps' rule), undefined elsewhere;
 *   g(p)  = the target, a unit normal in the OpenCV camera frame of the view matrix, valid where target_valid[p] & valid_bits
 *           (qed_depth_normals' plane with QED_NV_DEPTH_NORMAL, or any u8 plane);
 *   V     = the pixels where n^ is defined, g is valid and mask (float32, may be NULL) is non-zero.
 *   normal_loss = normal_lambda * [ mean over V and the 3 channels of |n^_c - g_c|
 *                                   + (use_cosine ? mean over V of (1 - n^ . g) : 0) ],   0 with zero gradients when V is empty.
 * Gradients flow through A (d n^ / d A = (I - n^ n^T) / |A|), through every alpha_i T_i (qed_composite_bwd on the normal
 * records, then qed_project_bwd, both unchanged) and through every n_i = +-R_v column k of R(q / |q|) to the RAW quaternion,
 * normalisation Jacobian included (a zero quaternion: 0, never NaN).  The axis k and the facing sign are piecewise constant
 * and carry no gradient; the direct dependence of n_i on the view rotation R_v is NOT differentiated (the host layers refuse
 * a camera optimiser beside this loss).  Stated deviation from gsplat's absgrad (the sum over pixels of the absolute
 * per-pixel gradient of the TOTAL loss, which two separate compositing passes cannot form): the normal pass adds to the
 * signed 2-D mean gradient and NOT to the absgrad slots, which stay those of the colour and depth loss.
 *
 * qed_normal_loss: accum[n_pix,3] = A, alpha[n_pix], target[n_pix,3].  v_accum[n_pix,3] receives the UNSCALED per-pixel
 *   d l / d A of l(p) = mean_c |n^_c - g_c| (+ 1 - n^ . g), zero outside V: d loss / d A = normal_lambda / max(|V|, 1) times
 *   it, and since the compositing backward is linear in its upstream gradient that factor may be applied later, per row
 *   (`scale` below), without a second pass over the image or a host read-back.  out[4] (device doubles) = {normal_loss,
 *   the L1 mean, the cosine mean (0 without use_cosine), |V|}; out_f[2] (device floats, may be NULL) = {normal_loss,
 *   normal_lambda / max(|V|, 1)}.  The per-pixel arithmetic is double from the float32 inputs; sums are carried in double
 *   and folded in a fixed order (2 launches, no floating-point atomics): the same input gives the same bits.
 *   workspace: QED_NORMAL_LOSS_WS_DOUBLES doubles (no zeroing needed).  n_pix == 0 writes zeros to out.
 * qed_gaussian_normals_bwd: one thread per Gaussian, looping over the C cameras (no atomics).  normal_rows[C*N][16] = the
 *   accumulator qed_composite_bwd filled for the records of qed_gaussian_normals(QED_NORMALS_CAMERA): slots 8..10 are
 *   d L / d n_i in the camera frame.  means / quats / scales / viewmats / flags as qed_gaussian_normals, whose k, sign and
 *   frame rules are applied to the same float32 inputs.  radii[C,N] (may be NULL): slots with radius <= 0 (culled) contribute
 *   nothing.  scale (device float, may be NULL = 1) multiplies the result.  v_quats[N,4] is overwritten (add == 0) or added
 *   to (add != 0).  normal_rows 16-byte aligned; quats / v_quats need float alignment only.
 * qed_normal_rows_merge: rows[r][s] += scale * normal_rows[r][s] for slots s = 0, 1 (2-D mean) and 4..7 (conic, opacity)
 *   of `total` rows of 16 floats, in place; slots 2, 3 (absgrad), 8..10 (colour), 11 (depth) and 12..15 of `rows` keep
 *   their bits.  scale: device float, may be NULL = 1.  Both 16-byte aligned; one row per thread, 16-byte accesses. */
#define QED_NORMAL_LOSS_WS_DOUBLES (3 * 1024)
int qed_normal_loss(int32_t n_pix, const float* accum, const float* alpha, const float* target,
                    const uint8_t* target_valid, uint32_t valid_bits, const float* mask, float min_alpha,
                    int32_t use_cosine, float normal_lambda, double* workspace, float* v_accum, double* out,
                    float* out_f, void* stream);
int qed_gaussian_normals_bwd(int32_t N, int32_t C, const float* means, const float* quats, const float* scales,
                             const float* viewmats, const int32_t* radii, const float* normal_rows, const float* scale,
                             uint32_t flags, int32_t add, float* v_quats, void* stream);
int qed_normal_rows_merge(int64_t total, const float* normal_rows, const float* scale, float* rows, void* stream);

/* ---- normal consistency and normal smoothness in training (csrc/normal_consistency.hip) ------------------------------------
 * Two regularisers on the rendered normal that need no sensor normals.  The consistency term is the rendered-normal to
 * rendered-depth-normal term of 2DGS / PGSR / dn-splatter, the smoothness term dn-splatter's total variation on the predicted
 * normal restricted to defined pairs -- both RESTATED FROM MEMORY of those projects, not checked against them.  Per pixel p of
 * one camera's step, with A the accumulated normal, alpha the accumulation and D the ACCUMULATED depth:
 *   n^(p) = A / |A| where alpha >= min_alpha and |A| > 1e-8 (qed_normal_maps' rule);
 *   N(p)  = qed_normal_maps' depth normal, exactly: z = D / alpha where alpha >= min_alpha, invalid where not finite or <= 0;
 *           P = ((x + .5 - cx) z / fx, (y + .5 - cy) z / fy, z); dx = P(x+1,y) - P(x-1,y), dy = P(x,y+1) - P(x,y-1),
 *           N = normalize(dy x dx); undefined on the border, where the pixel or a 4-neighbour is invalid and where
 *           |dy x dx| <= 1e-20; evaluated in double from the float32 inputs;
 *   V_c   = the pixels where n^ and N are both defined and mask (float32, may be NULL) is non-zero;
 *   normal_consistency_loss = lambda_c * mean over V_c of (1 - n^ . N),   0 with zero gradients when V_c is empty;
 *   E_x   = the horizontal neighbour pairs (p, p + x) with n^ defined and the mask non-zero at both ends, E_y the vertical ones;
 *   normal_tv_loss = lambda_tv * [ mean over E_x and the 3 channels of |n^(p + x) - n^(p)|
 *                                  + mean over E_y and the 3 channels of |n^(p + y) - n^(p)| ],  each mean 0 on an empty set;
 *           the derivative of |t| at exactly t == 0 is 0.
 * Gradients flow to A from both terms; from the consistency term also through N to z at the FOUR NEIGHBOURS (the centre's own
 * z does not enter N: a pixel gets a depth gradient only as a neighbour of other pixels), and from z to D and alpha:
 * d z / d D = 1 / alpha, d z / d alpha = -D / alpha^2.  Every validity decision, the 1e-20 test and the intrinsics are constants.
 *
 * qed_normal_consistency: one image.  A(p) = accum[p * accum_stride + 0..2] (accum_stride >= 3: an [H,W,4] = [A, D] image has
 *   stride 4), alpha[H,W], D(p) = depth[p * depth_stride] (as qed_normal_maps; NULL allowed without QED_NC_CONSISTENCY).
 *   flags: the terms QED_NC_CONSISTENCY, QED_NC_TV (a term that is off has value 0 and no gradient) and the passes
 *   QED_NC_REDUCE (one streaming launch and a one-workgroup fold: out[8] (device doubles) = {consistency loss, mean of
 *   1 - n^ . N, |V_c|, tv loss, x mean, y mean, |E_x|, |E_y|}, out_f[2] (device floats, may be NULL) = {consistency loss,
 *   tv loss}) and QED_NC_GRAD (one launch, after a reduce pass on the same inputs -- in the same call or an earlier one --
 *   whose `out` it READS: the two terms have different denominators, which therefore never reach the host).  The gradient
 *   pass writes the FULLY SCALED d (g_c loss_c + g_tv loss_tv) / d . : v_accum(p) at v_accum[p * v_accum_stride + 0..2],
 *   v_depth(p) at v_depth[p * v_depth_stride] and v_alpha[H,W] (either may be NULL), zero where nothing arrives.  g_c, g_tv:
 *   the upstream gradients, device floats, NULL = 1.  nl_v_accum (may be NULL; [H,W,3]): qed_normal_loss' UNSCALED image,
 *   added to v_accum times nl_scale[0] (its out_f[1]) times g_nl[0] (NULL = 1), so that with all three normal terms one
 *   image carries the sum.  No floating-point atomics: the depth gradient of a pixel is GATHERED, in a fixed order, from the
 *   stencils centred on its four neighbours; sums are carried in double and folded in a fixed order -- the same input gives
 *   the same bits.  workspace: QED_NORMAL_CONSISTENCY_WS_DOUBLES doubles (no zeroing needed; the reduce pass only).
 *   height * width == 0 writes zeros to out; an image under 3 x 3 has no depth normal (its TV pairs exist).
 * qed_normal_rows_merge_depth: qed_normal_rows_merge for the rows of a 4-channel normal pass: slots 0, 1, 4..7 AND 11 (depth)
 *   are added, times the device scale (NULL = 1); slots 2, 3 (absgrad), 8..10 (colour) and 12..15 of `rows` keep their bits. */
#define QED_NORMAL_CONSISTENCY_WS_DOUBLES (6 * 1024)
#define QED_NC_CONSISTENCY 1u
#define QED_NC_TV 2u
#define QED_NC_REDUCE 4u
#define QED_NC_GRAD 8u
int qed_normal_consistency(int32_t height, int32_t width, const float* accum, int32_t accum_stride, const float* alpha,
                           const float* depth, int32_t depth_stride, float fx, float fy, float cx, float cy, float min_alpha,
                           const float* mask, float lambda_c, float lambda_tv, uint32_t flags, const float* g_c,
                           const float* g_tv, const float* nl_v_accum, const float* nl_scale, const float* g_nl,
                           double* workspace, float* v_accum, int32_t v_accum_stride, float* v_depth, int32_t v_depth_stride,
                           float* v_alpha, double* out, float* out_f, void* stream);
int qed_normal_rows_merge_depth(int64_t total, const float* normal_rows, const float* scale, float* rows, void* stream);

/* ---- robust depth losses and depth smoothness in training (csrc/depth_loss.hip) ------------------------------------------------
 * A family of data terms and an edge-aware smoothness term on the rendered depth.  THIS PROJECT'S definitions, in the spirit of
 * DN-Splatter's depth losses, not checked against it and not in the reference (which keeps the L1 term of qed_loss_grad).
 * Per pixel p = (i, j) of one camera's step, everything in the model's units (after the dataparser's scale):
 *   d(p)  = the depth get_outputs returns: the accumulated depth channel and, where alpha == 0, the channel's maximum,
 *           detached (qed_loss_grad's dmax: fmaxf over the channel, so a NaN is skipped);
 *   g(p)  = the sensor depth, m(p) = the float mask (1 without one), I = the ground-truth colour [H,W,3];
 *   a = d m, b = g m, V = {p : finite(a), finite(b), b > 0} (the reference's validity), r = |a - b|;
 *   gx(p) = mean over c of |I(i, j+1, c) - I(i, j, c)|, gy(p) = mean over c of |I(i+1, j, c) - I(i, j, c)|: forward
 *           differences, 0 in the last column / row;
 *   depth_loss = depth_lambda * sum over V of w(p) rho(r) / max(|V|, 1), 0 when V is empty, with
 *           QED_DL_L1 rho = r | QED_DL_MSE r^2 | QED_DL_LOGL1 log1p(r) | QED_DL_HUBER r^2 / (2 delta) for r <= delta, else
 *           r - delta / 2 (a FIXED delta) | QED_DL_EDGE_LOGL1 log1p(r) with w = (exp(-gx) + exp(-gy)) / 2; w = 1 otherwise;
 *   d depth_loss / d d(p) = depth_lambda w rho'(r) sign(a - b) m / |V| on V, exactly 0 elsewhere; sign(0) = 0; with
 *           QED_DL_FIXUP also exactly 0 where alpha == 0 (the maximum is detached);
 *   an x-pair (p, p + x) exists for j < W - 1 and is valid iff both pixels have alpha > 0, a finite d and m != 0;
 *   E_x = sum over the valid x-pairs of omega_x(p) |d(p + x) - d(p)|, omega_x = exp(-gx(p)) with QED_DL_TV_EDGE, else 1;
 *           N_x their number; E_y, omega_y, N_y the same along y;
 *   depth_tv_loss = tv_lambda * (E_x / max(N_x, 1) + E_y / max(N_y, 1)): on d, not d m, and without the sensor depth.
 * alpha, g, m and I are constants.
 *
 * qed_depth_loss: one image.  d is read at depth[p * depth_stride] (channel 3 of an [H,W,4] render has stride 4).  With
 *   QED_DL_FIXUP `depth` is the raw channel and the entry forms d itself from alpha[H,W] and the maximum -- dmax[0] (device;
 *   qed_loss_grad's sums[3]) or, with dmax NULL, one more launch of its own; without it `depth` is d as get_outputs returned
 *   it.  alpha may be NULL without the fix-up and QED_DL_TV; gt_rgb without an edge-aware term; gt_depth without QED_DL_DATA.
 *   flags: the terms QED_DL_DATA, QED_DL_TV (+ QED_DL_TV_EDGE) -- a term that is off has value 0 and no gradient -- and the
 *   passes.  QED_DL_REDUCE: one streaming launch leaves per-workgroup sums in `workspace` (QED_DEPTH_LOSS_WS_DOUBLES doubles,
 *   no zeroing needed); alone it is followed by a one-workgroup fold that writes out[8] (device doubles) = {depth_loss,
 *   depth_tv_loss, |V|, N_x, N_y, E_x, E_y, the maximum used (0 without the fix-up)} and out_f[3] (device floats, may be NULL)
 *   = {depth_loss, depth_tv_loss, loss_base[0] + their sum} (loss_base: a device float, NULL = 0: the fused step's total rides
 *   along without a launch of its own).  QED_DL_GRAD: one launch, after a reduce pass on the same inputs and the SAME
 *   workspace -- in the same call or an earlier one --; every workgroup folds the workspace itself, so the denominators never
 *   reach the host, and with both passes in one call the gradient launch writes out / out_f too (two launches in all).
 *   It writes the FULLY SCALED d (g_data depth_loss + g_tv depth_tv_loss) / d d(p) to v_depth[p * v_depth_stride], every
 *   pixel, zero where nothing arrives.  g_data, g_tv: the upstream gradients, device floats, NULL = 1.
 *   No floating-point atomics: a pixel's smoothness gradient is gathered, in a fixed order, from the up to four pairs it
 *   belongs to; sums are carried in double and folded in a fixed order -- the same input gives the same bits.
 *   height * width == 0 writes zeros to out. */
#define QED_DEPTH_LOSS_WS_DOUBLES (6 * 256 + 136)
#define QED_DL_L1 0
#define QED_DL_MSE 1
#define QED_DL_LOGL1 2
#define QED_DL_HUBER 3
#define QED_DL_EDGE_LOGL1 4
#define QED_DL_DATA 1u
#define QED_DL_TV 2u
#define QED_DL_TV_EDGE 4u
#define QED_DL_FIXUP 8u
#define QED_DL_REDUCE 16u
#define QED_DL_GRAD 32u
int qed_depth_loss(int32_t height, int32_t width, const float* depth, int32_t depth_stride, const float* alpha,
                   const float* dmax, const float* gt_depth, const float* mask, const float* gt_rgb, int32_t type,
                   float depth_lambda, float huber_delta, float tv_lambda, uint32_t flags, const float* g_data,
                   const float* g_tv, const float* loss_base, double* workspace, float* v_depth, int32_t v_depth_stride,
                   double* out, float* out_f, void* stream);

/* ---- relative-depth supervision in training (csrc/relative_depth.hip) ---------------------------------------------------------
 * Three terms between the rendered depth and a PRIOR known only up to an unknown scale and shift -- a monocular network's depth
 * or inverse depth -- for datasets without a depth sensor.  THIS PROJECT'S definitions, in the spirit of FSGS, SparseGS (the
 * Pearson terms) and MiDaS (the scale-and-shift aligned L1), restated from memory, not checked against them and not in the
 * reference.  Per pixel p = (i, j) of one camera's step:
 *   d(p)  = the depth, read at depth[p * depth_stride]: channel 3 of an [H,W,4] render (stride 4) or the depth get_outputs
 *           returns (stride 1) -- pixels with alpha == 0 are outside V, so the raw channel and the fixed-up depth give the same
 *           bits and the entry needs neither the channel's maximum nor the fix-up;
 *   alpha = the accumulation, g(p) = the prior, m(p) = an optional float mask (NULL = 1).  The mask only selects: nothing is
 *           multiplied by it;
 *   V = {p : alpha > 0, m != 0, finite(d), finite(g), g > 0}, with QED_RD_INVERSE also d > 0;
 *   x = d, or x = 1 / d with QED_RD_INVERSE (dx/dd = 1, or -1 / d^2);
 *   over a set S of valid pixels: n = |S|, the means mx, mg, the BIASED moments vx, vg, cov, rho = cov / sqrt(vx vg).
 *   S is DEGENERATE when n < 2, or vx <= 1e-12 mean(x^2), or vg <= 1e-12 mean(g^2): its value is 0, its gradient exactly zero.
 * QED_RD_PEARSON, S = V:
 *   loss = lambda (1 - rho);  d loss / d x_p = -lambda / (n sqrt(vx vg)) [(g_p - mg) - rho sqrt(vg / vx) (x_p - mx)], times dx/dd.
 * QED_RD_SCALE_SHIFT_L1, S = V:
 *   s = cov / vg, t = mx - s mg: the least-squares fit of the prior to the render, CONSTANTS (not differentiated);
 *   r = x - (s g + t);  loss = lambda sum over V of |r| / n;  d loss / d x_p = lambda sign(r) / n, sign(0) = 0, times dx/dd.
 * QED_RD_PATCH_PEARSON: boxes of P x P pixels, P = `patch` a power of two from 8 to 128; the box of pixel (i, j) is
 *   (floor((i + offset_y) / P), floor((j + offset_x) / P)) with 0 <= offset_x, offset_y < P; partial boxes at the borders
 *   count.  A box CONTRIBUTES iff its valid count n_b >= K = max(2, ceil(min_valid * P * P)), min_valid in (0, 1], and it is
 *   not degenerate; B = the number of contributing boxes;
 *   loss = lambda / B * sum over the contributing boxes of (1 - rho_b), 0 when B == 0; a pixel of V in a contributing box gets
 *   its box's Pearson gradient (lambda = 1) times lambda / B, every other pixel exactly 0.
 * alpha, g and m are constants.  Every sum is carried in double from the float32 inputs (raw one-pass moments) and folded in a
 * fixed order, the per-pixel arithmetic (x, r, the bracket) is double, and there are no floating-point atomics: the same input
 * gives the same bits on every run.
 *
 * qed_relative_depth_loss: one image.  flags: QED_RD_INVERSE; the passes QED_RD_REDUCE and QED_RD_GRAD, as in qed_depth_loss --
 *   the reduce pass leaves its sums in `workspace` (QED_RELATIVE_DEPTH_WS_DOUBLES(height, width, patch) doubles; patch = 0 for
 *   the two whole-image types; no zeroing needed) and writes out / out_f; a gradient pass, in the same call or a later one on
 *   the same inputs and the SAME workspace, folds what it needs itself, so nothing reaches the host; QED_RD_ACCUMULATE: the
 *   gradient pass ADDS to v_depth[p * v_depth_stride] (a plane that qed_depth_loss' smoothness term or a zero fill has written)
 *   where without it the pass writes every element, zero where nothing arrives.
 *   Launches: Pearson one streaming reduce and one gradient launch (a one-workgroup fold follows a reduce pass that runs
 *   alone); ScaleShiftL1 one further streaming launch for sum |r|; PatchPearson one workgroup per box (patch <= 16: one wave per box,
 *   four boxes per workgroup), which leaves the box's
 *   moments and gradient coefficients in its row of a table in the workspace, a one-workgroup fold over the rows, and the
 *   gradient launch, which reads its pixel's row.
 *   out[8] (device doubles) = {loss, |V|, rho of the whole image, s, t (both of the whole image; 0 for a degenerate V), B, the
 *   mean of rho_b over the contributing boxes (B and the mean 0 for the whole-image types), 0}; out_f[2] (device floats, may
 *   be NULL) = {loss, loss_base[0] + loss} (loss_base: a device float, NULL = 0).  g_up: the upstream gradient, a device float,
 *   NULL = 1.  height * width == 0 writes zeros.  Refused (QED_E_INVALID_ARG, qed_last_error): an unknown type or flag, no
 *   pass flag, a negative or non-finite lambda and, for QED_RD_PATCH_PEARSON, a patch outside {8, 16, 32, 64, 128}, offsets
 *   outside [0, patch), min_valid outside (0, 1]. */
#define QED_RD_WS_HEAD_DOUBLES (8 * 512)
#define QED_RD_BOX_DOUBLES 12
#define QED_RELATIVE_DEPTH_WS_DOUBLES(H, W, P)                                                                         \
    (QED_RD_WS_HEAD_DOUBLES + ((P) > 0 ? QED_RD_BOX_DOUBLES * ((((int64_t)(H)) + 2 * (P) - 2) / (P)) *                  \
                                             ((((int64_t)(W)) + 2 * (P) - 2) / (P))                                      \
                                       : 0))
#define QED_RD_PEARSON 0
#define QED_RD_PATCH_PEARSON 1
#define QED_RD_SCALE_SHIFT_L1 2
#define QED_RD_INVERSE 1u
#define QED_RD_REDUCE 2u
#define QED_RD_GRAD 4u
#define QED_RD_ACCUMULATE 8u
int qed_relative_depth_loss(int32_t height, int32_t width, const float* depth, int32_t depth_stride, const float* alpha,
                            const float* prior, const float* mask, int32_t type, float lambda, int32_t patch,
                            int32_t offset_x, int32_t offset_y, float min_valid, uint32_t flags, const float* g_up,
                            const float* loss_base, double* workspace, float* v_depth, int32_t v_depth_stride, double* out,
                            float* out_f, void* stream);

/* ---- oriented surface samples of one rendered view (csrc/surface.hip) -------------------------------------------------------
 * The planes get_outputs returns in evaluation mode with output_normals, back-projected into a compact list of world points
 * with normals and colours; no intermediate image.  The filters are THIS PROJECT'S definitions, in the spirit of
 * DN-Splatter's back-projection, not checked against it and not in the reference.
 * rgb[H,W,3]; depth = the ACCUMULATED depth D, read at depth[p * depth_stride] (as qed_normal_maps); alpha[H,W];
 * normal[H,W,3] and depth_normal[H,W,3] in the OpenCV camera frame; valid[H,W] u8 with the QED_NV_* bits; mask[H,W] u8 (may
 * be NULL); viewmat[4,4]: the OpenCV world-to-camera matrix [R | t], row-major, on the DEVICE.
 * For every stride-th pixel (x, y) in x and y, IN THIS ORDER (the order is the contract):
 *   1. alpha >= min_alpha and (mask == NULL or mask != 0), else the pixel is dropped;
 *   2. z = D / alpha must be finite with depth_min <= z <= depth_max;
 *   3. the chosen normal n -- `normal` (QED_SURFACE_NORMAL_RENDERED) or `depth_normal` (QED_SURFACE_NORMAL_DEPTH) -- must
 *      carry its bit in `valid`;
 *   4. agreement filter, on where cos_max_normal_angle > -1: where BOTH bits are set, dot(normal, depth_normal) >=
 *      cos_max_normal_angle; a pixel with only one valid normal passes;
 *   5. P = ((x + .5 - cx) z / fx, (y + .5 - cy) z / fy, z): the renderer's pixel centres (qed_normal_maps' convention, NOT
 *      Open3D's integer pixels of qed_backproject_depth);
 *   6. grazing filter, on where min_view_cos > 0: -(n_x P_x / |P| + n_y P_y / |P| + n_z P_z / |P|) >= min_view_cos;
 *   7. world point = R^T (P - t), world normal = R^T n (not renormalised).
 * All of it in double from the float32 inputs (the thresholds are float32 values, compared in double), rounded to float32
 * once.  points / normals / colors[capacity,3] receive the kept pixels in row-major pixel order (colors: rgb's values),
 * n_out[1] (device) their number.  More than `capacity`: status[0] = the number needed, n_out = 0, nothing is written.
 * Deterministic (count / scan / write, no atomic counter): two calls give the same bits.  status[QED_STATUS_WORDS] is
 * zeroed by the call.  workspace: qed_surface_workspace_ints(height, width, stride) int32.  No allocation, no sync;
 * height * width == 0 launches nothing (n_out and status are then left as they are).
 * Refused on the host: null required buffers, stride < 1, depth_stride < 1, non-finite intrinsics, fx or fy == 0,
 * depth_min > depth_max (or either NaN), an unknown normal_source, a negative capacity; a short workspace returns
 * QED_E_WORKSPACE. */
#define QED_SURFACE_NORMAL_RENDERED 0
#define QED_SURFACE_NORMAL_DEPTH 1
int64_t qed_surface_workspace_ints(int32_t height, int32_t width, int32_t stride);
int qed_surface_samples(int32_t height, int32_t width, const float* rgb, const float* depth, int32_t depth_stride,
                        const float* alpha, const float* normal, const float* depth_normal, const uint8_t* valid,
                        const uint8_t* mask, float fx, float fy, float cx, float cy, const float* viewmat, int32_t stride,
                        float min_alpha, float depth_min, float depth_max, int32_t normal_source,
                        float cos_max_normal_angle, float min_view_cos, int64_t capacity, float* points, float* normals,
                        float* colors, int32_t* n_out, int32_t* workspace, int64_t workspace_ints, int32_t* status,
                        void* stream);

/* ---- growing Gaussians from sensor depth (csrc/depth_grow.hip) -------------------------------------------------------------
 * Where one view's render misses the surface its depth image measures, new Gaussians are proposed at the measured points and
 * appended to the flat buffers.  The rules are THIS PROJECT'S definitions, in the spirit of SplaTAM's densification (seed where
 * the accumulated alpha is low or the rendered depth lies behind the measured one), restated from memory; they are not checked
 * against it and are not in the reference.
 *
 * qed_depth_grow_candidates, one view.  gt_rgb[H,W,3] and gt_depth[H,W] (model units): the frame's ground truth as float
 * planes at the render's size; mask[H,W] u8 (may be NULL); depth = the ACCUMULATED depth D, read at depth[p * depth_stride] (as
 * qed_surface_samples); alpha[H,W]; viewmat[4,4]: the OpenCV world-to-camera matrix [R | t], row-major, on the DEVICE.
 * For every stride-th pixel (x, y) in x and y, in row-major order (the order is the contract), with d = gt_depth, the pixel
 * is a CANDIDATE when
 *   1. it has a measurement: d finite, d > 0, depth_min <= d <= depth_max, and (mask == NULL or mask != 0); and
 *   2. it is a HOLE, alpha < hole_alpha, or -- only where alpha >= hole_alpha and z = D / alpha is finite -- the render lies
 *      BEHIND the measurement, z > d + max(depth_tol, depth_tol_rel * d).  The hole test comes first: alpha == 0 never
 *      divides.  (depth_tol = depth_tol_rel = +inf: holes only.)
 * All comparisons in double on the float32 inputs (the thresholds are float32 values).  K = the number of candidates (it stays
 * on the device); cap = capacity, the most rows this view may add.  K <= cap: candidate j (0-based, pixel order) goes to row
 * j.  K > cap: candidate j is kept iff floor((j + 1) cap / K) > floor(j cap / K) and goes to row floor(j cap / K), in 64-bit
 * integers: exactly cap candidates, spread evenly in pixel order.  Per kept candidate, in double, rounded to float32 once:
 *   P = ((x + .5 - cx) d / fx, (y + .5 - cy) d / fy, d)   the renderer's pixel centres, as qed_surface_samples;
 *   points[row] = R^T (P - t);
 *   log_scale[row] = log(scale_factor * stride * d / (0.5 (fx + fy)))   one sampled pixel's footprint at that depth;
 *   colors[row] = gt_rgb at the pixel.
 * points / colors[capacity,3], log_scale[capacity]; rows from min(K, cap) on are not written.  n_out[1] (device) = min(K, cap);
 * status[QED_STATUS_WORDS] is written by the call: [0] = K, [1] = the hole candidates, [2] = the behind candidates, the rest 0.
 * Deterministic (count / scan / write, no atomic counter, no host read-back): two calls give the same bits.  workspace:
 * qed_depth_grow_workspace_ints(height, width, stride) int32.  No allocation, no sync; height * width == 0 launches nothing
 * (n_out and status are then left as they are).
 * Refused on the host: null required buffers, stride < 1, depth_stride < 1, non-finite intrinsics, fx or fy == 0, depth_min >
 * depth_max (or either NaN), a negative (or NaN) tolerance, a NaN hole_alpha, a scale_factor that is not positive and finite,
 * a negative capacity; a short workspace returns QED_E_WORKSPACE.
 *
 * qed_grow_append: old flat parameters and both Adam moments of n Gaussians (begins h_old_begin[7], host, as
 * qed_densify_emit) and k candidate rows -> the buffers of n + k Gaussians (begins h_new_begin[7]), one launch.  Rows [0, n)
 * of every group are copied bit for bit, in params, exp_avg and exp_avg_sq.  Rows [n, n + k): means = points; scales =
 * log_scale in all three columns; quats = (1, 0, 0, 0); opacities = logit(init_opacity); features_dc = (c - 0.5) /
 * 0.28209479177387814 for sh_coeffs > 1 and logit(c, eps = 1e-10) for sh_coeffs == 1 (sh_coeffs from the width of
 * features_rest), in double, rounded once, as qed_seed_gaussians; features_rest = 0; both moments 0.  k is a HOST value (the
 * caller has read n_out: the one sync of a growth); k == 0 is a plain copy, n == 0 is legal, n + k == 0 launches nothing.
 * Refused on the host: n or k negative or n + k >= 2^30, a layout whose groups are not width x rows in the order means,
 * scales, quats, opacities, features_dc, features_rest, init_opacity outside (0, 1), null buffers that would be read or
 * written. */
int64_t qed_depth_grow_workspace_ints(int32_t height, int32_t width, int32_t stride);
int qed_depth_grow_candidates(int32_t height, int32_t width, const float* gt_rgb, const float* gt_depth, const uint8_t* mask,
                              const float* depth, int32_t depth_stride, const float* alpha, float fx, float fy, float cx,
                              float cy, const float* viewmat, int32_t stride, float hole_alpha, float depth_tol,
                              float depth_tol_rel, float depth_min, float depth_max, float scale_factor, int64_t capacity,
                              float* points, float* log_scale, float* colors, int32_t* n_out, int32_t* workspace,
                              int64_t workspace_ints, int32_t* status, void* stream);
int qed_grow_append(int32_t n, int32_t k, const float* old_params, const float* old_exp_avg, const float* old_exp_avg_sq,
                    const int64_t* h_old_begin, const float* points, const float* log_scale, const float* colors,
                    float init_opacity, float* new_params, float* new_exp_avg, float* new_exp_avg_sq,
                    const int64_t* h_new_begin, void* stream);

/* ---- depth spread along the ray and the depth distortion loss (csrc/depth_spread.hip) ---------------------------------------
 * How the blending weights of a pixel are spread in depth: Mip-NeRF 360's distortion loss in the squared form 2DGS uses for
 * splats, RESTATED FROM MEMORY of those papers, not checked against their code and not in the reference.
 * Per pixel, over the Gaussians the colour pass applied there -- the same records, ids and offsets, the same accept / skip /
 * terminate decisions as qed_composite_fwd (and qed_contribution) -- with the weights w_i = alpha_i T_i and the depths z_i =
 * slot 9 of the record:
 *   A = sum w_i,   m = sum w_i z_i / A,   S = sum w_i (z_i - m)^2
 *   spread     L = A S = sum_{i<j} w_i w_j (z_i - z_j)^2
 *   depth_std    = sqrt(S / A)                  the weighted standard deviation of the depth along the ray (0 where A == 0)
 * Both are in the model's units (after the dataparser's scale) and exactly 0 where one Gaussian contributes.
 *
 * qed_depth_spread_fwd writes four planes [C,H,W]: spread; mean_u = m - z_ref, the mean ANCHORED at z_ref = the depth of the
 * tile's first list entry (0 where A == 0); acc = A; depth_std (may be NULL).  The sums run in float32 by the weighted Welford
 * update on u_i = z_i - z_ref (L from the raw moments A sum w z^2 - (sum w z)^2 cancels on a thin surface); pixels of empty
 * tiles get zeros; N == 0 or flatten_ids == NULL (an empty list) zero the planes.  launch_flags: QED_CL_NO_CULL is honoured
 * (bit-identical planes); the launch-shape bits are ignored (always one wave per tile).
 *
 * qed_depth_spread_bwd: the gradient of sum_p v_p L_p for a per-pixel factor image v[C,H,W], walked back to front from the
 * colour pass's last_ids with its t_final (both required, [C,H,W]) and the three planes of the forward call:
 *   d / d w_i     = v_p (S + A (z_i - m)^2) = g_i
 *   d / d z_i     = 2 v_p A w_i (z_i - m)                                 -> slot 11 of the row
 *   d / d alpha_i = T_i g_i - (sum_{j>i} w_j g_j) / (1 - alpha_i)         then qed_composite_bwd's own chain to the opacity
 *                   (slot 7), the conic (4..6) and the 2-D mean (0, 1); a clamped alpha passes nothing.
 * One add per (tile, Gaussian) and value into rows[C*N][16], qed_project_bwd's layout, which the caller zeroes; the absgrad
 * slots 2, 3, the colour slots 8..10 and the padding are not touched.  tile_cost / order_ws / QED_CL_ORDER_READY: as
 * qed_composite_bwd (costliest tiles first; every tile stays one whole-tile wave); QED_CL_NO_CULL is honoured; a forced
 * launch shape only selects the plain tile order.  Same gradients up to the order of the float atomics.
 *
 * qed_depth_distortion_loss: loss[1] = lambda * mean of spread over the n_pix pixels whose mask (float, may be NULL = all) is
 * not 0, or 0 when there is none, and -- with v (may be NULL) -- v[n_pix] = lambda / count at those pixels, 0 elsewhere: the
 * factor image of qed_depth_spread_bwd for an upstream gradient of 1.  Sum and count are doubles, folded in a fixed order:
 * no float atomics, no host read-back, the same bits on every run.  workspace: QED_DEPTH_DISTORTION_WS_DOUBLES doubles; its
 * last two hold the sum and the count afterwards.  Refused on the host: a negative or non-finite lambda. */
#define QED_DEPTH_DISTORTION_WS_DOUBLES (2 * 256 + 2)
int qed_depth_spread_fwd(int32_t C, int32_t N, const float* splats, const int32_t* flatten_ids, const int32_t* offsets,
                         int32_t width, int32_t height, int32_t tile_w, int32_t tile_h, float* spread, float* mean_u,
                         float* acc, float* depth_std, int32_t launch_flags, void* stream);
int qed_depth_spread_bwd(int32_t C, int32_t N, const float* splats, const int32_t* flatten_ids, const int32_t* offsets,
                         int32_t width, int32_t height, int32_t tile_w, int32_t tile_h, const float* t_final,
                         const int32_t* last_ids, const float* spread, const float* mean_u, const float* acc, const float* v,
                         float* rows, const int32_t* tile_cost, int32_t* order_ws, int32_t launch_flags, void* stream);
int qed_depth_distortion_loss(int64_t n_pix, const float* spread, const float* mask, float lambda, double* workspace,
                              float* v, float* loss, void* stream);

/* ---- label fields on frozen Gaussians: K-channel compositing and the label kernels (csrc/semantic.hip) -----------------------
 * A table features[N,K] (class logits, one row per Gaussian) composited with the render's own blending weights, LangSplat's /
 * Feature-3DGS's route RESTATED FROM MEMORY of those papers, not checked against their code and not in the reference.  The
 * geometry is frozen: nothing here produces a gradient to the records.
 *
 * qed_features_fwd: out[c,p,k] = sum_i w_i(p) features[n_i,k] over the Gaussians the colour pass applied at pixel p -- the
 * same records, ids and offsets, the same accept / skip / terminate decisions as qed_composite_fwd (and qed_contribution: a
 * Gaussian contributes where it passes the alpha test, the pixel has not terminated and T (1 - alpha) > 1e-4; the one that
 * terminates a pixel is not applied), w_i = alpha_i T_i.  Records c * N + n of every camera c read row n of the one table.
 * 1 <= K <= QED_FEATURES_MAX.  Every entry of features (and of v_out) must be FINITE: a lane that did not accept a Gaussian adds
 * weight 0 times its row, so a non-finite entry reaches every pixel of an 8x8 quadrant in which some pixel accepted that
 * Gaussian, and "the same bits with the cull off" holds for finite tables only.  out is [C,H,W,K]; every pixel inside the image is written (zeros in empty tiles and where
 * nothing contributed) and nothing outside it; N == 0 or flatten_ids == NULL (an empty list) zero out.  The sum of one (pixel,
 * channel) runs in list order in float32 whatever the kernel's channel chunk, and no value depends on the launch order of the
 * tiles.  launch_flags: QED_CL_NO_CULL is honoured (bit-identical out); the launch-shape bits are ignored (always one wave per
 * tile and channel chunk).
 *
 * qed_features_bwd: v_features[n,k] += sum over cameras and pixels of w_i(p) v_out[c,p,k] for n = n_i: a FORWARD walk again
 * (no last_ids, no t_final, no suffix sums).  The caller zeroes v_features [N,K]; calls accumulate.  One float atomic add per
 * (tile, contributing Gaussian, channel) -- the tile's sum is formed in a fixed lane order first -- and none for a Gaussian that
 * contributed to no pixel of the tile: its row keeps its bits.  Same values up to the order of those adds.  N == 0 or an empty
 * list: nothing is done.
 *
 * Both refuse on the host: bad extents, K outside 1..QED_FEATURES_MAX, a tile grid that does not match the image, NULL
 * buffers, features / out / v_out not 16-byte aligned.
 *
 * qed_label_loss: loss[1] = sum_p cw[y_p] nll_p / sum_p cw[y_p] over the LABELLED pixels p -- labels[p] = y_p is not
 * ignore_label and < K (a label >= K counts as ignored) -- with nll_p = logsumexp(logits[p,:]) - logits[p,y_p] taken about
 * the row maximum and cw = class_weight[K] (NULL: all 1): torch.nn.functional.cross_entropy(logits, labels, weight=cw,
 * ignore_index=ignore_label, reduction="mean").  With v_logits (may be NULL): v_logits[p,k] = cw[y_p] (softmax_k - [k == y_p])
 * / sum cw at the labelled pixels, 0 at the others.  Loss and gradient are 0 when no pixel is labelled (or the weights of the
 * labelled pixels sum to 0).  The two sums are doubles, folded in a fixed order: no float atomics, no host read-back, the same
 * bits on every run.  workspace: QED_LABEL_LOSS_WS_DOUBLES doubles; its last two hold sum cw nll and sum cw afterwards.
 *
 * qed_label_confusion ADDS, for every labelled pixel, 1 to confusion[y_p][pred_p] of a [K][K + 1] table of unsigned 64-bit
 * counts (row = label, column = prediction; ONE layout, with or without acc): pred_p = the first maximum of logits[p,:] (ties
 * go to the lower index, a NaN never wins), or K -- "no prediction", the last column -- when acc (float [n_pix], may be NULL) is
 * given and acc[p] >= min_alpha does not hold.  Integer atomics only: the same bits for any order of views.  The caller
 * zeroes the table once.
 *
 * qed_label_present: the planes an image writer stores.  out_label[p] (uint8, may be NULL) = pred_p, or QED_LABEL_NONE where
 * acc[p] >= min_alpha does not hold; out_rgb[p] (uint8 [n_pix,3], may be NULL) = palette[pred_p] of a uint8 [K + 1][3] palette
 * whose last row colours the pixels without a prediction.
 * The three refuse a class count outside 1..QED_FEATURES_MAX, NULL buffers and a NaN min_alpha.  No function of this section
 * allocates, synchronises or reads anything back. */
#define QED_FEATURES_MAX 32
#define QED_LABEL_NONE 255
#define QED_LABEL_LOSS_WS_DOUBLES (2 * 256 + 2)
int qed_features_fwd(int32_t C, int32_t N, int32_t K, const float* splats, const int32_t* flatten_ids, const int32_t* offsets,
                     int32_t width, int32_t height, int32_t tile_w, int32_t tile_h, const float* features, float* out,
                     int32_t launch_flags, void* stream);
int qed_features_bwd(int32_t C, int32_t N, int32_t K, const float* splats, const int32_t* flatten_ids, const int32_t* offsets,
                     int32_t width, int32_t height, int32_t tile_w, int32_t tile_h, const float* v_out, float* v_features,
                     int32_t launch_flags, void* stream);
int qed_label_loss(int64_t n_pix, int32_t K, const float* logits, const uint8_t* labels, int32_t ignore_label,
                   const float* class_weight, double* workspace, float* v_logits, float* loss, void* stream);
int qed_label_confusion(int64_t n_pix, int32_t K, const float* logits, const uint8_t* labels, int32_t ignore_label,
                        const float* acc, float min_alpha, uint64_t* confusion, void* stream);
int qed_label_present(int64_t n_pix, int32_t K, const float* logits, const float* acc, float min_alpha, const uint8_t* palette,
                      uint8_t* out_label, uint8_t* out_rgb, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QED_SPLAT_H */
