/* manus_hip.h — C ABI of libmanus_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the one hot path of brown-ivl/manus that this project
 * accelerates.  Every entry point is `extern "C"`, takes plain device pointers,
 * sizes and a hipStream_t (passed as void*), and returns 0 or a negative MGR_E*.
 * No torch types appear here; the Python shims in manus_amd/ bind these with
 * ctypes, and INTEGRATION.md shows the binding a MANUS maintainer would add.
 *
 * Reference interfaces replaced (paths relative to the brown-ivl/manus tree):
 *   mgr_raster_forward / mgr_raster_backward
 *       diff_gaussian_rasterization._C.rasterize_gaussians{,_backward}, called by
 *       GaussianRasterizer at src/utils/gaussian_utils.py:393-416 (installed by
 *       setup_env.sh:6; colors_precomp + cov3D_precomp variant only — the one
 *       MANUS uses).
 *   mgr_knn3_mean_dist2
 *       simple_knn._C.distCUDA2, src/models/gaussian.py:4,110.
 *   mgr_skin_weights_fwd/bwd
 *       skinning_weights_from_voxel_grid, src/utils/gaussian_utils.py:167-196
 *       (via HandGaussianModel.get_skin_weights, src/models/hand_gaussian.py:65-76).
 *   mgr_lbs_cov_fwd/bwd
 *       TrainingModule.forward LBS block, src/modules/hand_dynamic.py:106-127, with
 *       GaussianModel.get_covariance, src/models/gaussian.py:49-53,84-93 and
 *       build_rotation/build_scaling_rotation, src/utils/gaussian_utils.py:279-314.
 *   mgr_sh_color_fwd/bwd
 *       calculate_colors_from_sh, src/utils/gaussian_utils.py:431-449 with
 *       eval_sh, src/utils/sh_utils.py:57-104.
 *   mgr_project_points
 *       project_points, src/utils/transforms.py:304-311.
 *   mgr_dilate_mask, mgr_points_outside_mask
 *       dilate_mask / get_points_outside_mask, src/utils/gaussian_utils.py:35-47,101-147.
 *
 * Conventions
 *   - All pointers are DEVICE pointers unless the name ends in _host.
 *   - All tensors are dense fp32 / int32, caller-owned; outputs are fully
 *     written (no zero-initialisation needed) unless stated.
 *   - "V" = number of camera views batched in one call, "N" = Gaussians.
 *     Per-Gaussian inputs take a view stride in ELEMENTS (floats); 0 means the
 *     same array is shared by every view.
 *   - Cameras: a device array of V records of MGR_CAM_FLOATS floats:
 *       [0] tanfovx [1] tanfovy [2..17] viewmatrix [18..33] projmatrix
 *       [34..36] campos [37..39] unused
 *     with the matrices exactly as MANUS stores them
 *     (`world_view_transform`, `full_proj_transform`, src/utils/cam_utils.py:58-63:
 *     row-major storage of the transposed matrix == column-major math matrix,
 *     element (row r, col c) at [4*c + r]).
 *   - Launches are asynchronous on `stream`; the only host synchronisation is in
 *     the *_sync helpers.  No library-owned device memory.  What the library does
 *     own, all of it host-side:
 *       * a process-wide call counter (the epoch that tags gradient records) and
 *         the profiling switch of mgr_profile_*;
 *       * per device: the "function attributes set" flag (dynamic LDS above 64 KB
 *         is requested on the first forward that runs on a device);
 *       * per (host thread, device), created on first use and only by the per-tile
 *         sort route of the forward (MGR_BINNING=sorted, or a tile grid too large
 *         for the depth-ordered route): ONE non-blocking side stream with a fork
 *         and a join event.  It forks from `stream` and joins it again inside the
 *         call, so the caller sees plain stream order.  The default route, and every
 *         other entry point, launches on `stream` only.
 *     Calls on different devices from different host threads do not share any of
 *     the per-device state (one process per GPU, or one thread per GPU, both work).
 */
#ifndef MANUS_HIP_H
#define MANUS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGR_VERSION 100
#define MGR_CAM_FLOATS 40
#define MGR_TILE 16
#define MGR_MAX_BONES 32

enum {
    MGR_OK = 0,
    MGR_EINVAL = -1,   /* bad argument */
    MGR_ENOMEM = -2,   /* workspace too small (see mgr_raster_workspace_bytes) */
    MGR_EHIP = -3,     /* a HIP call failed; text in mgr_last_error() */
    MGR_EOVERFLOW = -4, /* pair capacity exceeded (reported by mgr_raster_status_sync) */
    MGR_ECUT = -6,      /* a forward run with the depth cut (MGR_FWD_DEPTH_CUT) met a scene its hints no longer fit: its image is
                           incomplete; run it again without the flag (reported by mgr_raster_status_sync) */
    MGR_ETIER = -7,     /* a forward told to skip binning launches (MGR_FWD_SKIP_*) had a view that needed one: its image
                           is incomplete; run it again without those flags */
    MGR_ESTATE = -8     /* the workspace does not hold what the call needs (mgr_raster_blend_features: no complete forward
                           of these sizes, or one whose tile lists are cut short or clipped) */
};

/* `flags` of mgr_raster_forward / mgr_views_forward, OR-ed together (0 = none); spelt out at mgr_raster_forward. */
#define MGR_FWD_CHECK 1              /* synchronise and check after every kernel (upstream's `debug=True`) */
#define MGR_FWD_NO_BLEND 2           /* stop before the blend */
#define MGR_FWD_BLEND_ONLY 4         /* the blend only */
#define MGR_FWD_DEPTH_CUT 8          /* mgr_views_forward only: apply the depth-cut hints */
#define MGR_FWD_SKIP_BOX_LARGE 16    /* skip the binning launches for tile boxes of more than 2048 tiles */
#define MGR_FWD_SKIP_BOX_MID 32      /* skip the binning launch for tile boxes of 1537..2048 tiles */
#define MGR_FWD_SKIP_SORT_BEHIND 128 /* skip the radix launch behind the instance sort (k_dbin_rank) */
#define MGR_FWD_RANK_LARGE 256       /* k_dbin_rank's instantiation for items of up to 3072 keys */
#define MGR_FWD_IMAGE_KEPT 1024      /* the caller vouches that out_color is the kept image (see below mgr_views_backward) */
#define MGR_FWD_REPAIR 2048          /* with MGR_FWD_DEPTH_CUT: repair depth-cut tiles on the device instead of flagging */
#define MGR_FWD_SPREAD 4096          /* k_bin_scatter's lane-spreading instantiation */

/* `flags` of mgr_raster_backward / mgr_views_backward / mgr_views_backward_pose. */
#define MGR_BWD_CHECK 1              /* synchronise and check after every kernel */
#define MGR_BWD_OUTPUTS_KEPT 512     /* mgr_views_backward*: the caller vouches for the leaf-gradient buffers (see there) */

/* The overflow word of a forward (mgr_raster_status_sync, word 1 of the status mirror): non-zero = the image is incomplete. */
#define MGR_OVF_PAIRS 1u   /* the pair capacity was exceeded: lists clipped, image and gradients incomplete (MGR_EOVERFLOW) */
#define MGR_OVF_CUT 2u     /* a tile's depth-cut list ran out of entries with a pixel still unsaturated (MGR_ECUT) */
#define MGR_OVF_TIER 4u    /* a view needed a binning launch the caller had asked to skip, MGR_FWD_SKIP_* (MGR_ETIER) */
#define MGR_OVF_FLAGS_MASK 0xFFFF  /* the status mirror's word carries, above the flags, ... */
#define MGR_OVF_REPAIRED_SHIFT 16  /* ... the number of (tile, quadrant) units the forward repaired on the device */

/* The tiers word of a forward (mgr_raster_status_tiers_sync, word 2 of the status mirror): what its views needed. */
#define MGR_TIERS_BOX_LARGE 1          /* a view's tile box had more than 2048 tiles: do not pass MGR_FWD_SKIP_BOX_LARGE */
#define MGR_TIERS_BOX_MID 2            /* one had 1537..2048 tiles: do not pass MGR_FWD_SKIP_BOX_MID */
#define MGR_TIERS_WIDE_RECT 4          /* rectangles of more than 64 tiles were met: pass MGR_FWD_SPREAD */
#define MGR_TIERS_NEAR_SMALL_SHIFT 8   /* bits 8..15: items of the instance sort beyond 13/16 of k_dbin_rank's 2048 keys ... */
#define MGR_TIERS_NEAR_LARGE_SHIFT 16  /* bits 16..23: ... and of the 3072 keys of MGR_FWD_RANK_LARGE (both capped at 255) */
#define MGR_TIERS_NEAR_MASK 0xFF
#define MGR_TIERS_BEYOND_SMALL_SHIFT 24 /* bits 24..30: items beyond 2048 keys (capped at 127): pass MGR_FWD_RANK_LARGE */
#define MGR_TIERS_BEYOND_SMALL_MASK 0x7F

int mgr_version(void);
/* 0 for the product build.  Non-zero when the library was compiled with one of the instrumentation macros of tools/instr
 * (never by manus_amd.build's defaults): bit 0 = a knock-out that CHANGES RESULTS (BWD_KO, FWD_KO_DEEP: cost bounds
 * only), bit 1 = counters / clocks inside the kernels (MGR_STATS, MGR_TIMELINE, *_PROF: results unchanged, timings
 * perturbed), bit 2 = an alternative code path selected at compile time (FWD_PF1, FWD_LDS_PIPE1, BWD_WLAST_REDUCE, a
 * non-default MGR_BIN_BLOCK: results unchanged).  bench.py labels such a run and refuses to call it the headline; the parity
 * block does not run on a library that reports bit 0. */
int mgr_build_variant(void);
/* Tiles per view (ceil(W/16) * ceil(H/16)) up to which the depth cut's on-device repair (mgr_views_forward with MGR_FWD_REPAIR) is
 * used; on a larger grid a depth-cut tile that runs out flags the forward (MGR_ECUT) and the caller runs it again uncut. */
int mgr_raster_repair_max_tiles(void);
/* Thread-local text of the last error returned on this host thread. */
const char* mgr_last_error(void);

/* ------------------------------------------------------------------------
 * Rasterizer (tile binning, per-tile depth sort, alpha compositing, backward)
 * ------------------------------------------------------------------------ */

/* Bytes of workspace needed for V views of N Gaussians at W x H with room for
 * `pair_capacity` (Gaussian, tile) pairs summed over all views.  The workspace
 * must be zero-filled once when (re)allocated, and again before it is reused
 * with a different (V, N, W, H, pair_capacity): it carries counters, tags and
 * per-tile state from one call to the next (a forward leaves its tile counters
 * zeroed for the following one instead of clearing them per call); otherwise it
 * is opaque state that links a forward call to its backward call. */
size_t mgr_raster_workspace_bytes(int V, int N, int W, int H, int64_t pair_capacity);

/* Forward.  out_color: (V,3,H,W).  radii: (V,N) int32.  bg: 3 floats.
 * means3D (N,3), cov3D (N,6) packed [xx,xy,xz,yy,yz,zz], colors (N,3),
 * opacity (N) — each with its per-view stride.
 * If the number of pairs exceeds pair_capacity the image is still written but
 * is incomplete and the overflow flag is raised: check with
 * mgr_raster_status_sync and retry with a larger workspace.
 * flags (here and in mgr_views_forward): MGR_FWD_* OR-ed together.  The tile lists come from the depth-ordered binning
 * whatever the flags; MGR_BINNING=sorted in the environment selects the per-tile sorts instead (identical lists).
 *   MGR_FWD_CHECK  synchronise and check after every kernel (upstream's `debug=True`).
 *   MGR_FWD_NO_BLEND  stop before the blend (projection and binning only): radii, the pair total and the tile lists are
 *     final, out_color is not written.
 *   MGR_FWD_BLEND_ONLY  the blend only, after a call with MGR_FWD_NO_BLEND on the same workspace and arguments.  The pair lets
 *     a caller put work that needs the tile lists but not the image next to the blend (the image loss's span list,
 *     mgr_image_loss_tiles_list).
 *   MGR_FWD_DEPTH_CUT  (mgr_views_forward only) depth cut.  Every forward leaves, per tile whose pixels all saturated, the
 *     depth in front of which they had all stopped plus a margin; with this flag the next forward on the same workspace leaves
 *     the instances behind that depth out of the tile's list (they lie behind every pixel's stop: image, n_contrib and
 *     gradients are bit for bit those of the full lists, but the binning handles a fraction of the pairs).  Only valid when
 *     that previous forward rendered the SAME views (camera + pose) of a model that has moved little since; if a cut list
 *     runs out under a pixel that has not saturated the forward raises MGR_OVF_CUT (mgr_raster_status_sync: MGR_ECUT) and
 *     the caller runs it again without the flag.  Pass it to both calls of a forward split with MGR_FWD_NO_BLEND /
 *     MGR_FWD_BLEND_ONLY.  No counterpart upstream (the reference renders one view per step and re-bins everything).
 *   MGR_FWD_REPAIR  (with MGR_FWD_DEPTH_CUT) repair on the device.  A tile whose cut list runs out under an unsaturated pixel
 *     is completed by two kernels behind the blend instead of flagging the forward: the instances the cut dropped from that
 *     tile are found (one pass over the view's rectangles), sorted by (depth, index) -- the tail of the tile's full list --,
 *     appended behind the regular lists, and the walks of the tile's unsaturated quadrants continue from their saved state;
 *     the backward's work items of such a tile point at the appended entries / checkpoints.  Image, n_contrib and gradients
 *     stay bit for bit those of the full lists and NO re-run is needed; MGR_OVF_CUT is only raised when a capacity of the
 *     repair is exceeded (repaired quadrants, 256 tiles per view, 8192 entries behind the cut of one tile, the appended
 *     entries: all sized from pair_capacity), or when a hinted tile ends up with no list at all.  A tile that ran out gets no
 *     hint for the next mgr_raster_set_cut_penalty forwards (the same few tiles at the rim of the saturating region otherwise
 *     run out step after step under a moving model).  The status mirror's overflow word carries the number of repaired
 *     quadrants of the forward above MGR_OVF_REPAIRED_SHIFT.
 *   MGR_FWD_SKIP_BOX_LARGE, MGR_FWD_SKIP_BOX_MID  skip the binning launches that only serve views whose box of non-empty
 *     tiles has more than 2048 / has 1537..2048 tiles (they hold more LDS per workgroup; three launches of ~6 us each that do
 *     nothing for smaller boxes).  mgr_raster_status_tiers_sync reports which of them a forward needed (MGR_TIERS_BOX_LARGE /
 *     MGR_TIERS_BOX_MID); pass the flags for the tiers the previous forward did not need.  A view that needs a skipped launch
 *     raises MGR_OVF_TIER (MGR_ETIER).
 *   MGR_FWD_SKIP_SORT_BEHIND  skip the launch behind the instance sort.  Since round 6 the (depth, index) keys of a view are
 *     sorted in items of ~768 keys, one workgroup each (k_dbin_rank: depth buckets uniform over the depth range of the view's
 *     visible instances in this forward); an item of more than 2048 keys -- a dense depth slice -- is left to a radix launch
 *     behind, which returns at once when there is none.  The flag omits that launch (mgr_raster_status_tiers_sync reported no
 *     item near the limit for the previous forward: the tiers word's field at MGR_TIERS_NEAR_SMALL_SHIFT for the usual
 *     instantiation, at MGR_TIERS_NEAR_LARGE_SHIFT for the one MGR_FWD_RANK_LARGE asks for); an item that needs it then raises
 *     MGR_OVF_TIER (MGR_ETIER: run the forward again without the flag), like a skipped tile-box tier.
 *   MGR_FWD_RANK_LARGE  k_dbin_rank's instantiation for items of up to 3072 keys (the previous forward met items of more than
 *     2048: the tiers word's field at MGR_TIERS_BEYOND_SMALL_SHIFT) -- ~4 us slower for all its items, but the dense slice no
 *     longer waits for the launch behind (33 us).
 *   MGR_FWD_SPREAD  k_bin_scatter's lane-spreading instantiation (the previous forward met rectangles of more than 64 tiles:
 *     MGR_TIERS_WIDE_RECT): a batch that holds such a rectangle is spread over lanes, one row piece per lane, instead of going
 *     instance by instance (correct either way; cameras close to the hand: 1.2 -> 0.87 ms).  Without the flag the producer is
 *     the plain one of round 5.  (MGR_FWD_IMAGE_KEPT: see below mgr_views_backward.) */
int mgr_raster_forward(int V, int N, int W, int H, const float* cams, const float* bg,
                       const float* means3D, int64_t stride_means3D, const float* cov3D,
                       int64_t stride_cov3D, const float* colors, int64_t stride_colors,
                       const float* opacity, int64_t stride_opacity, float* out_color,
                       int32_t* radii, void* workspace, size_t workspace_bytes,
                       int64_t pair_capacity, int flags, void* stream);

/* Backward of the forward that last used `workspace` (same inputs again, plus the
 * image that forward produced: out_color (V,3,H,W)).
 * dL_dcolor: (V,3,H,W).  Outputs, all fully written:
 * dL_dmeans3D (V,N,3), dL_dmeans2D (V,N,3) (z = 0; x,y in NDC-scaled pixel units
 * 0.5*W, 0.5*H as the reference's densification statistic expects,
 * src/models/gaussian.py:335-338), dL_dcolors (V,N,3), dL_dopacity (V,N),
 * dL_dcov3D (V,N,6) (off-diagonals carry the factor 2 of the symmetric pack). */
int mgr_raster_backward(int V, int N, int W, int H, const float* cams, const float* bg,
                        const float* means3D, int64_t stride_means3D, const float* cov3D,
                        int64_t stride_cov3D, const float* colors, int64_t stride_colors,
                        const float* opacity, int64_t stride_opacity, const float* out_color,
                        const float* dL_dcolor, float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dcolors,
                        float* dL_dopacity, float* dL_dcov3D, void* workspace,
                        size_t workspace_bytes, int64_t pair_capacity, int flags, void* stream);

/* Feature render: composite C caller channels, and optionally expected depth and accumulated opacity, over the tile lists
 * the LAST FORWARD left in `workspace` -- no projection, no sort, no binning.  (Its gradients:
 * mgr_raster_blend_features_backward below.)
 *   out_feat[v, c, y, x] = sum_i w_i features[v, gid_i, c] + T_final bg_feat[c],   w_i = alpha_i T_i
 * with exactly the (pixel, entry) contributions of that forward's image: the same alpha arithmetic and keep rule
 * (alpha >= 1/255, clamped to 0.99), the same stop rule (an entry that would bring T below 1e-4 ends the pixel's walk and
 * contributes nothing), the same list order.  Rendering the forward's colours as features reproduces its image up to the
 * rounding of the sums.
 * features: (N, C) rows shared by the views (stride_features = 0) or (V, N, C) with a view stride in floats (>= N * C); a row
 * may start at any 4-byte alignment.  0 <= C <= 32; C = 0 is allowed when with_depth is set or out_alpha is given.
 * bg_feat: C floats, NULL = zeros.
 * out_feat: (V, C + (with_depth ? 1 : 0), H, W), every element written.  With with_depth the LAST channel is the EXPECTED
 * depth sum_i w_i z_i, z = the view-space depth the forward sorted by: it is not divided by the accumulated opacity and its
 * background is 0 (divide by out_alpha for a normalised depth).  out_alpha: (V, H, W) = 1 - T_final, or NULL.
 * Pixels of tiles without a list get bg_feat, depth 0, alpha 0.
 * Valid between a complete forward on `workspace` (mgr_raster_forward or mgr_views_forward, same V, N, W, H and
 * pair_capacity) and the next forward on it.  A backward in between is fine: mgr_raster_backward / mgr_views_backward write
 * the pair-gradient records and tags, the per-instance gradient rows and the header's backward counters, none of which this
 * call reads (it reads the queue records, the sorted lists, the geometry half of the per-(view, Gaussian) records and the
 * depths).  The workspace is only read.  One blocking read of its header decides, before anything is launched, whether the
 * lists are usable; MGR_ESTATE (text in mgr_last_error) when
 *   - no forward has run on the workspace, or the last one stopped before its blend (MGR_FWD_NO_BLEND),
 *   - the last forward applied the depth cut (mgr_views_forward with MGR_FWD_DEPTH_CUT: lists cut short, repaired entries
 *     behind the regular ones),
 *   - the last forward raised an MGR_OVF_* bit (pair capacity, depth cut, skipped binning tier),
 *   - the last forward was made for another V, N, W, H or pair_capacity.
 * The depth-cut refusal reads what the call that ran the blend was given: a forward split with MGR_FWD_NO_BLEND / MGR_FWD_BLEND_ONLY must pass
 * MGR_FWD_DEPTH_CUT to BOTH calls (as the forward's own comment asks) -- a blend-only call without it stamps lists cut by the first call
 * as uncut.
 * A tile's list is walked once per group of up to 8 channels (groups of 8, 4 or 2 accumulators per lane; the depth is the
 * last group's last slot, out_alpha is written by the first group). */
int mgr_raster_blend_features(int V, int N, int C, int W, int H, const float* features, int64_t stride_features,
                              const float* bg_feat, int with_depth, float* out_feat, float* out_alpha,
                              const void* workspace, size_t workspace_bytes, int64_t pair_capacity, void* stream);

/* Backward of the feature render: gradients of a loss on the maps of the mgr_raster_blend_features call described by the same
 * V, N, C, W, H, features, with_depth, through the tile lists of the SAME forward (still the last one on `workspace`).
 * out_feat (V, C + (with_depth ? 1 : 0), H, W) and out_alpha (V, H, W) are what that call produced (each needed only where
 * its gradient is given; bg_feat is accepted for symmetry and not read: the background's share is in out_feat).
 * dL_dout_feat: (V, C + (with_depth ? 1 : 0), H, W) or NULL; dL_dalpha: (V, H, W) or NULL; both NULL is MGR_EINVAL.
 * Per pixel, with g the upstream gradients and s_i = f_i . g (the depth a channel f = z, the alpha a channel f = 1, both on
 * background 0):  dL/df_ic = w_i g_c,  dL/dz_i = w_i g_depth,  dL/dalpha_i = T_i s_i - (suffix_i . g) / (1 - alpha_i) -- the
 * conventions of mgr_raster_backward: the forward's keep and stop rules and list order, the gradient passes through the 0.99
 * clamp, the sort order is not differentiated.  From dL/dalpha the path is mgr_raster_backward's (conic, mean2D, opacity,
 * then the projection's backward); the depth adds dL/dz times the z row of the view matrix to dL_dmeans3D.
 * Outputs, every element written (zero rows for culled Gaussians and Gaussians without a contributing pair):
 * dL_dmeans3D (V,N,3), dL_dmeans2D (V,N,3; units and z = 0 as mgr_raster_backward), dL_dopacity (V,N), dL_dcov3D (V,N,6),
 * dL_dfeatures (V,N,C) per view (NULL when C = 0).  cams, means3D, cov3D and their strides are the forward's.
 * The workspace is ONLY READ: a colour backward before, between or after changes nothing, and the two backwards of one
 * forward may run in either order.  All temporary state lives in the caller's `scratch` of at least
 * mgr_raster_feat_backward_workspace_bytes bytes (MGR_ENOMEM below that); its contents need not be initialised and mean nothing
 * after the call.  Deterministic: one record per (tile, Gaussian) pair in the pair's private slot, summed per (view, Gaussian)
 * in slot order; no atomics.  Channels go in the forward's groups of up to 8, one walk of the lists per group.
 * Refusals before anything is launched: the MGR_ESTATE cases of mgr_raster_blend_features (one blocking read of the header).
 * flags: MGR_BWD_CHECK synchronises and checks after every launch. */
size_t mgr_raster_feat_backward_workspace_bytes(int V, int N, int C, int W, int H, int64_t pair_capacity);
int mgr_raster_blend_features_backward(int V, int N, int C, int W, int H, const float* cams, const float* means3D,
                                       int64_t stride_means3D, const float* cov3D, int64_t stride_cov3D, const float* features,
                                       int64_t stride_features, const float* bg_feat, int with_depth, const float* out_feat,
                                       const float* out_alpha, const float* dL_dout_feat, const float* dL_dalpha,
                                       float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dopacity, float* dL_dcov3D,
                                       float* dL_dfeatures, const void* workspace, size_t workspace_bytes, int64_t pair_capacity,
                                       void* scratch, size_t scratch_bytes, int flags, void* stream);

/* Sequence number of the last forward binned on `workspace` (0: none yet), one blocking read on `stream`.  A caller that comes
 * back to a forward's lists later notes it behind the forward and compares before it calls the backward below. */
int mgr_raster_forward_seq_sync(const void* workspace, uint32_t* seq, void* stream);

/* ------------------------------------------------------------------------
 * Fused articulated path (training engine): canonical parameters in, image out.
 * One launch chain per V views = mgr_lbs_cov_fwd + mgr_sh_color_fwd + sigmoid +
 * mgr_raster_forward, without writing posed means / covariances / transforms /
 * colours to HBM; the backward returns the leaf gradients of the six MANUS
 * parameter tensors (src/models/gaussian.py:34-39) summed over the views, the
 * skin-weight gradient (feed it to mgr_skin_weights_bwd), and the densification
 * statistics of src/models/gaussian.py:335-338 / src/utils/gaussian_utils.py:469-471.
 *   xyz (N,3), log_scale (N,3) = _scaling, rot (N,4) = _rotation (raw),
 *   opacity_logit (N) = _opacity, f_dc (N,1,3) = _features_dc, f_rest (N,15,3) = _features_rest,
 *   skin_w (n_articulated,B) or NULL (static object), transforms (V,B,16): one pose per view.
 *   n_articulated <= N: the first n_articulated Gaussians are skinned, the rest are static (identity
 *   transform, no skin-weight row): the hand+object concatenation of src/modules/composite.py:50-59.
 *   d_skin_w is (n_articulated,B).
 *   sh_half != 0: f_rest points to the fp16 storage copy of _features_rest made by mgr_sh_to_half -- (N,48) halves,
 *   16-byte aligned rows, 45 used (BASELINE config 5 "fp16 SH coeffs"; the reference has no counterpart, everything
 *   there is fp32).  Arithmetic and d_f_rest stay fp32 (N,15,3); the optimizer owns the fp32 master copy.
 * stat_grad2d (N): sum over views of ||dL/dmeans2D[:, :2]|| * grad2d_scale,
 * stat_vis (N): number of views with radius > 0, stat_radii (N): max radius (any may be NULL).
 * ------------------------------------------------------------------------ */
int mgr_views_forward(int V, int N, int B, int n_articulated, int sh_half, int W, int H, const float* cams, const float* bg,
                      const float* xyz, const float* log_scale, const float* rot,
                      const float* opacity_logit, const float* f_dc, const float* f_rest,
                      const float* skin_w, const float* transforms, float* out_color, int32_t* radii,
                      void* workspace, size_t workspace_bytes, int64_t pair_capacity, int flags,
                      void* stream);
int mgr_views_backward(int V, int N, int B, int n_articulated, int sh_half, int W, int H, const float* cams, const float* bg,
                       const float* xyz, const float* log_scale, const float* rot,
                       const float* opacity_logit, const float* f_dc, const float* f_rest,
                       const float* skin_w, const float* transforms, const int32_t* radii,
                       const float* out_color, const float* dL_dcolor, float grad2d_scale, float* d_xyz,
                       float* d_log_scale, float* d_rot, float* d_opacity_logit, float* d_f_dc,
                       float* d_f_rest, float* d_skin_w, float* stat_grad2d, float* stat_vis,
                       int32_t* stat_radii, void* workspace, size_t workspace_bytes,
                       int64_t pair_capacity, int flags, void* stream);

/* MGR_FWD_IMAGE_KEPT of mgr_views_forward / mgr_raster_forward = "image kept": the caller vouches that out_color is the image the
 * previous complete forward on this workspace wrote, untouched since.  A tile that held the background colour then and is
 * empty again is not written again (85 % of the tiles of a capture-like frame are empty: 170 MB of stores at eight 1080p
 * views); the image is identical.  Honoured only when the header says so: that forward was the last one binned on this
 * workspace, wrote this very buffer, with this background colour -- otherwise every empty tile is written as without the flag.
 * (Without the flag the background of the empty tiles is written by extra workgroups of the instance sort's launch when the
 * depth-ordered binning runs, by the blend otherwise; MANUS_BG_FILL=blend in the environment: always by the blend.) */

/* flags of mgr_views_backward: MGR_BWD_CHECK as in the forward.  MGR_BWD_OUTPUTS_KEPT = "outputs kept": the caller vouches that the leaf-gradient buffers
 * (d_xyz ... d_skin_w, stat_grad2d) are the ones the previous mgr_views_backward on this workspace wrote, untouched since
 * (persistent .grad-like tensors).  The backward then zeroes only the rows that call wrote and this one does not, instead
 * of every row of every buffer (97 MB of stores on the bench step); the results are identical.  Honoured only when the
 * workspace's row state is that previous call's and describes these very buffers (the library checks a call counter and
 * d_xyz; V <= 8, 3..8 views, run lists on) -- otherwise every row is zeroed as without the flag. */

/* mgr_views_backward plus the gradient of the loss with respect to the pose: d_transforms (V,B,16), row-major 4x4 per
 * (view, transform), d_transforms[v][b][r][c] = sum_n skin_w[n][b] * dL/d(blended transform of Gaussian n in view v)[r][c]
 * for r < 3; row 3 is written as zero; the background (identity) transform is a row like any other.  No reference
 * counterpart: the reference names a pose optimizer (config/model/pose_optimizer.yaml -> src.models.pose_optimizer) that
 * was never released.  Needs articulated rows (skin_w, n_articulated > 0); the static rows of a composite contribute nothing.
 * d_transforms is always fully written (all-zero rows for a view in which nothing was visible), whatever `flags` says about
 * the leaf buffers; every other output is exactly that of mgr_views_backward.  The workspace keeps its layout and everything a
 * later forward or backward reads, with one difference: the `inst_grad` slots (mgr_raster_layout) of the lanes that held records
 * end up holding those lanes' dL/d(blended transform) (12 floats) instead of their nine gathered sums -- every gather rewrites
 * the slots before a backward reads them, but a tool that inspects `inst_grad` after the call sees other contents.
 * No float atomics, bit-reproducible: the per-instance backward leaves every lane's dL/d(blended transform) in the workspace
 * slot it read its sums from (its order of work is that of the gather's atomics and differs from run to run, so nothing is
 * summed there); at most 1024 workgroups then walk the slots in Gaussian order, each reducing its chunks of 256 / Gv Gaussians in
 * a fixed order in LDS and writing one partial of Gv x B x 12 floats (Gv = views per lane group: 1, 2, 4 or 8) into
 * pose_workspace; a fold kernel adds the partials in a fixed order.  With V > 8 every group of eight views writes its own rows.
 * pose_workspace_bytes >= mgr_views_pose_workspace_bytes(V, N, B) = min(1024, ceil(N / (256 / Gv))) x Gv x B x 12 x 4 bytes of
 * partials (at most 12.6 MB; 8.3 MB at 21 transforms and 8 views) + N x Gv flag bytes (2.4 MB at 300 k Gaussians). */
size_t mgr_views_pose_workspace_bytes(int V, int N, int B);
int mgr_views_backward_pose(int V, int N, int B, int n_articulated, int sh_half, int W, int H, const float* cams, const float* bg,
                            const float* xyz, const float* log_scale, const float* rot,
                            const float* opacity_logit, const float* f_dc, const float* f_rest,
                            const float* skin_w, const float* transforms, const int32_t* radii,
                            const float* out_color, const float* dL_dcolor, float grad2d_scale, float* d_xyz,
                            float* d_log_scale, float* d_rot, float* d_opacity_logit, float* d_f_dc,
                            float* d_f_rest, float* d_skin_w, float* stat_grad2d, float* stat_vis,
                            int32_t* stat_radii, void* workspace, size_t workspace_bytes,
                            int64_t pair_capacity, int flags, float* d_transforms, void* pose_workspace,
                            size_t pose_workspace_bytes, void* stream);

/* Map backward of the fused route: gradients of a loss on the accumulated-opacity and expected-depth maps that
 * mgr_raster_blend_features (C = 0) rendered over the lists of the last mgr_views_forward on `workspace`, carried to the
 * canonical leaves.  The leading arguments are those of mgr_views_backward without the SH tensors.  No reference counterpart
 * (the reference uses its masks for pruning only).
 *   out_alpha, dL_dalpha   (V,H,W) the alpha map of that render and its upstream gradient, or both NULL
 *   out_depth, dL_ddepth   (V,H,W) the depth map (with_depth = 1, C = 0) and its upstream gradient, or both NULL
 *                          (both gradients NULL: MGR_EINVAL)
 *   accumulate             0: every row of every output is written, zeros where no view holds a contribution;
 *                          1: rows with a contribution are added to, every other row is left bit for bit as it was
 *   d_xyz (N,3) d_log_scale (N,3) d_rot (N,4) d_opacity_logit (N) d_skin_w (n_articulated,B; NULL without skin_w)
 * One walk of the lists (the feature backward's kernel, one 64-byte record per (tile, Gaussian) pair into `scratch`), then one
 * launch per group of up to eight views that sums a Gaussian's records in slot order, recomputes its posed mean and covariance
 * from the canonical parameters as the forward did, and runs the projection, depth, LBS, quaternion and sigmoid backward in
 * registers; views are summed in ascending order over a fixed tree, groups in group order.  No atomics: bit-reproducible.
 * Gaussians >= n_articulated take the identity transform; skin_w == NULL (or n_articulated == 0): a static object.
 * The workspace is only read.  scratch_bytes >= mgr_views_maps_backward_workspace_bytes (68 bytes per pair of capacity); its
 * contents need not be initialised.  flags: MGR_BWD_CHECK.
 * Refused with nothing launched and no output touched: MGR_ESTATE as mgr_raster_blend_features (no complete forward on the
 * workspace, a depth-cut forward, an overflow bit, other sizes), MGR_ENOMEM below either size. */
size_t mgr_views_maps_backward_workspace_bytes(int V, int N, int W, int H, int64_t pair_capacity);
int mgr_views_maps_backward(int V, int N, int B, int n_articulated, int W, int H, const float* cams, const float* xyz,
                            const float* log_scale, const float* rot, const float* opacity_logit, const float* skin_w,
                            const float* transforms, const float* out_alpha, const float* out_depth, const float* dL_dalpha,
                            const float* dL_ddepth, int accumulate, float* d_xyz, float* d_log_scale, float* d_rot,
                            float* d_opacity_logit, float* d_skin_w, const void* workspace, size_t workspace_bytes,
                            int64_t pair_capacity, void* scratch, size_t scratch_bytes, int flags, void* stream);

/* mgr_views_maps_backward plus the map terms' gradient with respect to the pose: d_transforms (V,B,16) in the layout and
 * conventions of mgr_views_backward_pose -- d_transforms[v][b][r][c] = sum_n skin_w[n][b] * dL/d(blended transform of Gaussian
 * n in view v)[r][c] for r < 3, row 3 zero, the background transform a row like any other, the static rows of a composite
 * contributing nothing.  The leading arguments are those of mgr_views_maps_backward, in its order.
 *   accumulate_pose        0: every element of d_transforms is written (row 3 as zero; all-zero rows for a view in which
 *                             nothing held a record);
 *                          1: the result is added, as the last addition, to rows 0 .. 2 of what d_transforms holds and row 3 is
 *                             left as it is -- on top of the d_transforms mgr_views_backward_pose wrote for the colour term
 * Every other output is bit for bit that of mgr_views_maps_backward with the same arguments (they are written by the same
 * kernels with the same arguments); the workspace is only read; the scratch contract is unchanged.  Behind the gather of every
 * group of up to eight views one more kernel runs over the articulated Gaussians in the gather's lane layout: at most 1024
 * workgroups, each taking the chunks x, x + gridDim.x, ... (gridDim.x = min(1024, chunks)) of 256 / Gv Gaussians (Gv = views per lane group: 1, 2, 4 or 8); a lane
 * sums the records of its (view, Gaussian) again, recomputes dL/d(blended transform) in registers and parks it in LDS, the
 * workgroup reduces the chunk in a fixed order and writes ONE partial of Gv x B x 12 floats into pose_workspace, and a fold kernel
 * adds the partials in slot order.  No float atomics, bit-reproducible, nothing kept per (Gaussian, view).  With V > 8 every
 * group of eight views writes (or adds to) its own rows.
 * pose_workspace_bytes >= mgr_views_maps_pose_workspace_bytes(V, N, B) = min(1024, ceil(N / (256 / Gv))) x Gv x B x 12 x 4 bytes
 * rounded up to 256 (at most 12.6 MB); 0 for non-positive sizes.  Its contents need not be initialised.
 * Refused as mgr_views_maps_backward, and: MGR_EINVAL for skin_w == NULL or n_articulated <= 0 (nothing to differentiate) and for
 * d_transforms or pose_workspace NULL; MGR_ENOMEM for a pose workspace below the size function.  On any refusal nothing is
 * launched and no output is touched. */
size_t mgr_views_maps_pose_workspace_bytes(int V, int N, int B);
int mgr_views_maps_backward_pose(int V, int N, int B, int n_articulated, int W, int H, const float* cams, const float* xyz,
                                 const float* log_scale, const float* rot, const float* opacity_logit, const float* skin_w,
                                 const float* transforms, const float* out_alpha, const float* out_depth, const float* dL_dalpha,
                                 const float* dL_ddepth, int accumulate, float* d_xyz, float* d_log_scale, float* d_rot,
                                 float* d_opacity_logit, float* d_skin_w, const void* workspace, size_t workspace_bytes,
                                 int64_t pair_capacity, void* scratch, size_t scratch_bytes, int flags, int accumulate_pose,
                                 float* d_transforms, void* pose_workspace, size_t pose_workspace_bytes, void* stream);

/* Device pointers (into the workspace) to the compacted list of Gaussians that received a gradient in the last
 * mgr_views_backward and to its length; V <= 8. */
int mgr_views_active_list(void* workspace, int V, int N, int W, int H, int64_t pair_capacity, const uint32_t** list,
                          const uint32_t** count);

/* Lane layout of the fused per-instance backward at 3..8 views per group (lane groups of four or eight; process-wide; returns
 * the previous setting).
 * on (default; MANUS_INST_RUNS=0 in the environment starts with it off): an active Gaussian takes 8 / 4 / 2 lanes by the
 * number of its views that hold pair-gradient records (41 % of the (active Gaussian, view) lanes did on the bench step), and
 * the gather walks a compacted list of the instances with records;
 * off: always one lane per view.  The per-view contributions are summed in ascending view order either way, over a tree of
 * the views with records (on) or of all views (off): the results agree to rounding (tests/test_gpu_fused.py), each is
 * bit-reproducible.  No reference counterpart (there, autograd accumulates the views' contributions into .grad). */
int mgr_views_backward_run_lists(int on);

/* f_rest (N,45) fp32 -> out_half (N,48) fp16 (round to nearest even, 3 halves of zero padding per row). */
int mgr_sh_to_half(int N, const float* f_rest, void* out_half, void* stream);

/* Debug/test: byte offsets of the workspace regions, in the order header, grec, depth, rect,
 * alive, pair_off, tile_count, tile_start, tile_cursor, tile_done, tile_queue, chunk_start, items,
 * ckpt, keys, sorted_gid, final_T (reserved, not written), n_contrib, pair_tag, pair_grad, total, inst_grad
 * (fused backward: per (Gaussian, view-lane) the 9 gathered blend sums, 12 floats each, then the active list),
 * inst_tag, db_nvis (per view: instances with at least one non-null tile), db_bbox (per view: ushort4 x0, y0, w, h of the
 * non-empty tiles), db_order (per view: those instances in (depth, index) order) -- these three belong to the
 * depth-ordered binning --, tile_zcut, tile_zused, tile_qend (depth cut: hint of the next forward / applied / end of the
 * tile's walks), tile_rep, rep_unit, rep_cnt (repair of depth-cut tiles: owner unit + 1 per tile, the 64-byte unit records,
 * entries found behind the cut per owner unit).  Returns the count. */
int mgr_raster_layout(int V, int N, int W, int H, int64_t pair_capacity, size_t* out, int n_out);
/* Debug/test: stride in bytes of the per-(view, Gaussian) records of the workspace's `grec` region (x, y, conic A B C, opacity,
 * r g b, pair-slot base, rectangle width: twelve 4-byte words, then padding to the stride). */
int mgr_raster_record_bytes(void);

/* Blocking read-back of the workspace header after a forward: total number of
 * (Gaussian, tile) pairs (`num_rendered`, summed over views) and the overflow
 * flag.  Returns MGR_EOVERFLOW when the flag is set. */
/* Margins of the depth-cut hints the forwards of this host thread leave (MGR_FWD_DEPTH_CUT): a tile keeps the entries its walks
 * used plus max(min_entries, frac_entries x that many), and at least the depth of the last one plus depth_range_frac of the
 * walked depth range plus depth_rel of that depth.  interior_only: hints only for tiles whose eight neighbours saturated
 * too (a silhouette tile stops saturating when an edge moves by a fraction of a pixel).  Defaults 0.125, 64, 0.0625, 2e-4, 0.
 * Wider margins: more pairs binned, fewer forwards flagged MGR_ECUT when the model moves between two forwards of a view. */
int mgr_raster_set_cut_margin(float frac_entries, int min_entries, float depth_range_frac, float depth_rel, int interior_only);
/* Forwards (of this host thread) for which a tile whose cut list ran out receives no hint; default 16, 0 = none. */
int mgr_raster_set_cut_penalty(int forwards);
/* Status without a copy: `host_words` points to 4 uint32 of host memory the device can write (hipHostMalloc / pinned
 * memory); the next forward that runs the blend on `workspace` writes (pair total, overflow word, binning tiers, 1) there
 * from its last kernel.  An event recorded behind that forward then tells the host when the words are valid -- no
 * device-to-host copy, no host synchronisation of the stream.  One shot per call; nullptr withdraws a pending mirror.  The
 * caller zeroes word 3 beforehand and keeps the memory alive until it has read it.  (The reference's rasterizer returns
 * num_rendered through a blocking read-back, SURVEY App. A.) */
int mgr_raster_set_status_mirror(const void* workspace, void* host_words);
/* mgr_raster_status_sync plus `tiers`: the MGR_TIERS_* word, from which the caller picks the next forward's MGR_FWD_SKIP_*,
 * MGR_FWD_RANK_LARGE and MGR_FWD_SPREAD. */
int mgr_raster_status_tiers_sync(const void* workspace, int64_t* num_pairs, int32_t* overflow, int32_t* tiers,
                                 void* stream);
int mgr_raster_status_sync(const void* workspace, int64_t* num_pairs, int32_t* overflow,
                           void* stream);

/* Debug/test access to the binning state of view v after a forward (blocking):
 * tile_ranges_host (tiles,2) int32 [start,end) into the global sorted list,
 * point_list_host up to `max_pairs` Gaussian indices in blend order. */
int mgr_raster_debug_binning_sync(const void* workspace, int V, int N, int W, int H,
                                  int64_t pair_capacity, int view, int32_t* tile_ranges_host,
                                  int32_t* point_list_host, int64_t max_pairs, void* stream);

/* Debug/test: the blend kernels' own evaluation of alpha for n (Gaussian record, pixel) pairs -- the device function
 * both blend kernels call, exp through v_exp_f32 in the log2 domain.  rec (n,6) = pixel centre x, y, conic A, B, C,
 * opacity; px, py (n) pixel coordinates; out: alpha (n) and valid (n) = 1 when the pair passes the kernels' tests
 * (power <= 0 and alpha >= 1/255).  Lets a parity test decide which side of the threshold the
 * kernels took for pairs that sit within rounding of it.  All pointers are device pointers. */
int mgr_debug_pair_alpha(int n, const float* rec, const int32_t* px, const int32_t* py, float* alpha, int32_t* valid,
                         void* stream);

/* ------------------------------------------------------------------------
 * Articulation: skin weights, LBS of means + covariances, SH colour
 * ------------------------------------------------------------------------ */

/* Trilinear sample (align_corners=True, zero padding) of a channel-last grid
 * (D,H,W,B) at u = (xyz - center)/scale, u=(x,y,z) indexing (W,H,D), then
 * w /= sum(w) without epsilon (0/0 -> NaN exactly like the reference).
 * out_w: (N,B).  B <= MGR_MAX_BONES.  grid_stride = floats per voxel: B (the
 * reference layout) or 24 (channels zero-padded to 24, 16-byte aligned base: the
 * fast path with float4 gathers; needs B <= 24). */
int mgr_skin_weights_fwd(int N, const float* xyz, const float* grid, int D, int H, int W, int B,
                         int grid_stride, const float* center3, const float* scale3, float* out_w,
                         void* stream);
/* dL_dxyz (N,3) written, or added to when accumulate != 0 (the training engine adds the skin-weight path
 * to the gradient mgr_views_backward has already written for the same xyz leaf). */
int mgr_skin_weights_bwd(int N, const float* xyz, const float* grid, int D, int H, int W, int B,
                         int grid_stride, const float* center3, const float* scale3,
                         const float* dL_dw, float* dL_dxyz, int accumulate, void* stream);
/* The same for the Gaussians index[0 .. *index_count) only (device list + device count <= max_count, e.g. the active
 * list of mgr_views_active_list: rows of dL_dw that received nothing are zero and contribute nothing); entries >= N
 * (static Gaussians of a composite) are skipped; always accumulates. */
int mgr_skin_weights_bwd_indexed(int N, const float* xyz, const float* grid, int D, int H, int W, int B,
                                 int grid_stride, const float* center3, const float* scale3, const float* dL_dw,
                                 float* dL_dxyz, const uint32_t* index, const uint32_t* index_count, int max_count,
                                 void* stream);

/* dL/d(grid): the half of the chain rule mgr_skin_weights_bwd drops, as a SPARSE gradient.  No reference kernel counterpart:
 * the reference gets it from autograd through F.grid_sample (src/utils/gaussian_utils.py:173) once grid_weights requires grad.
 * For every processed Gaussian n (all N when index is NULL -- max_count is then taken as N --, else index[0 .. min(*index_count,
 * max_count)), entries >= N skipped as in mgr_skin_weights_bwd_indexed): corner weights t_c, raw samples s_b = sum_c t_c g[c][b],
 * S = sum_b s_b, a = dL_dw[n], r_b = (a_b - sum_k a_k s_k / S) / S, and G[voxel(c)][b] += t_c r_b for every corner inside the
 * grid (zero padding: an outside corner receives nothing).
 *   out_voxel[0 .. *out_count)  linear indices (z*H + y)*W + x, strictly ascending: every in-bounds corner of every contributing
 *                               Gaussian, nothing else
 *   out_grad                    row i: grid_stride floats, channels >= B written as zero
 * Entries beyond *out_count are left untouched.  capacity (rows of out_voxel / out_grad) >= min(8 * max_count, D*H*W) is
 * required, so nothing can overflow and there is no overflow flag.
 * A Gaussian whose S is zero or not finite (every corner outside, or every in-bounds corner zero) contributes nothing and lists
 * nothing -- a stated deviation from autograd, which would write 0/0 into a leaf every Gaussian shares; the forward still
 * returns NaN weights for it.
 * No float atomics: a voxel's contributions are added in an order fixed by the Gaussian indices, never by positions in `index`,
 * so the result is bit-identical for any permutation of the same list.
 * grid_stride as in mgr_skin_weights_fwd.  D*H*W < 2^31, max_count < 2^27.  workspace_bytes >=
 * mgr_skin_grid_bwd_workspace_bytes(D, H, W, max_count): 4 bytes per voxel + 292 per list entry.
 * MGR_EINVAL (nothing launched, outputs untouched): B > MGR_MAX_BONES, grid_stride neither B nor 24, the padded layout on a base
 * that is not 16-byte aligned, capacity too small, max_count < 0; MGR_ENOMEM: workspace too small. */
size_t mgr_skin_grid_bwd_workspace_bytes(int D, int H, int W, int max_count);
int mgr_skin_grid_bwd(int N, const float* xyz, const float* grid, int D, int H, int W, int B, int grid_stride,
                      const float* center3, const float* scale3, const float* dL_dw,
                      const uint32_t* index, const uint32_t* index_count, int max_count,
                      int32_t* out_voxel, float* out_grad, uint32_t* out_count, int capacity,
                      void* workspace, size_t workspace_bytes, void* stream);
/* Row Adam on such a list, torch.optim.SparseAdam's semantics: the moments (laid out like the grid) are updated and the grid is
 * stepped on the rows voxel[0 .. min(*count, capacity)) only, channels < B (pad channels stay zero); the bias correction uses
 * the global `step` (>= 1).  The hyper-parameters are doubles, as in mgr_adam_step: 1 - beta2 taken from a float 0.999 is off by
 * 1e-5 of itself.  clamp != 0: x = max(x, clamp_min) afterwards (weights below zero make S cancel). */
int mgr_skin_grid_adam(const int32_t* voxel, const float* grad, const uint32_t* count, int capacity,
                       float* grid, int grid_stride, int B, float* exp_avg, float* exp_avg_sq,
                       double lr, double beta1, double beta2, double eps, int step, int clamp, float clamp_min,
                       void* stream);
/* Refinement step of the grid on such a list: prior gradient, the row Adam above, clamp, projection of the row back onto sum 1
 * and the prior's value, in ONE pass over the listed rows (k_sg_refine: 32 lanes per row, 8 rows per workgroup).  The reference
 * (HandGaussianModel.optimizing_skin_weights) would use a dense Adam on the whole grid and keeps grid_weights_init beside
 * grid_weights for such a prior; it has no kernel of its own.  For every listed row r < min(*count, capacity), v = voxel[r],
 * channels b < B:
 *   1. x = grid[v][b]; prior_weight != 0: d = x - grid0[v][b], g = grad[r][b] + w2 * d with w2 = (float)(2 * prior_weight);
 *      prior_weight == 0: g = grad[r][b], no prior arithmetic at all, grid0 and prior_value may be NULL
 *   2. Adam with the expressions and roundings of mgr_skin_grid_adam (one device function serves both): with prior_weight == 0
 *      and project == 0 the grid and both moments come out bit for bit as mgr_skin_grid_adam leaves them
 *   3. clamp != 0: x' = max(x', clamp_min) (fmaxf: a NaN x' becomes clamp_min, as in mgr_skin_grid_adam; the moments keep the NaN)
 *   4. project != 0: S = sum_b x'_b in fp32 in a fixed order (a butterfly over the row's 32 lanes); S > min_sum -- false for a
 *      NaN -- : x'_b = x'_b / S, a true division; otherwise the row stays as clamped.  The division never creates a NaN.
 *   5. *prior_value = prior_weight * sum_rows sum_b (double)d * (double)d: the prior ON THE GRID BEFORE THE STEP (the grid its
 *      gradient was taken on), over the LISTED rows only, added in fp64 in a tree fixed by the count alone -- no atomics, the same
 *      bits from run to run and for every capacity >= the count.  Written as 0 when prior_weight == 0 and the pointer is given.
 * The forward divides every sample by its raw sum, so a row's scale is a gauge: without the projection Adam drifts along it.
 * Pad channels (b >= B) of grid and moments are not touched, rows behind the count are not read, unlisted voxels stay bitwise
 * as they are.  The list is mgr_skin_grid_bwd's, strictly ascending; a voxel listed twice is UNDEFINED (two half-waves would
 * step the same row).  voxel entries are trusted to lie inside the grid, as in mgr_skin_grid_adam.
 * workspace_bytes >= mgr_skin_grid_refine_workspace_bytes(capacity): one double per 8 rows of capacity.
 * MGR_EINVAL (nothing launched, nothing written, prior_value included): B outside 1 .. MGR_MAX_BONES, grid_stride neither B nor
 * 24 (or 24 below B), capacity < 0, step < 1, prior_weight negative or not finite, prior_weight != 0 with grid0 or prior_value
 * NULL, min_sum < 0 (or NaN), a null voxel / grad / count / grid / moment pointer with capacity > 0; MGR_ENOMEM: a short
 * workspace.  capacity == 0: MGR_OK, prior_value (if given) written 0. */
size_t mgr_skin_grid_refine_workspace_bytes(int capacity);
int mgr_skin_grid_refine(const int32_t* voxel, const float* grad, const uint32_t* count, int capacity,
                         float* grid, const float* grid0, int grid_stride, int B,
                         float* exp_avg, float* exp_avg_sq,
                         double lr, double beta1, double beta2, double eps, int step,
                         int clamp, float clamp_min,
                         double prior_weight, int project, float min_sum,
                         double* prior_value, void* workspace, size_t workspace_bytes, void* stream);
/* mask[i] = 1 where row i of dL_dw (n,B) holds an entry != 0 (a NaN counts), else 0; every mask[0 .. n) is written.  With
 * mgr_exchange_index behind it: the ascending list of the non-zero rows of a skin-weight gradient, the `index` of mgr_skin_grid_bwd
 * where more than one backward added into dL_dw.  MGR_EINVAL (nothing launched): n < 0, B outside 1 .. MGR_MAX_BONES, a null
 * pointer with n > 0. */
int mgr_skin_rows_mask(int n, int B, const float* dL_dw, uint8_t* mask, void* stream);

/* LBS for P poses. transforms: (P,B,16) row-major 4x4 bone transforms
 * T_b = posed_b * inv(rest_b) (+ identity background).  skin_w (N,B) or NULL for
 * the static-object path (identity transform: posed = xyz, cov = Sigma).
 * Outputs: posed_xyz (P,N,3), posed_cov (P,N,6), tf (P,N,12) = rows 0..2 of the
 * blended 4x4 (may be NULL). */
int mgr_lbs_cov_fwd(int P, int N, int B, const float* xyz, const float* log_scale,
                    const float* rot, const float* skin_w, const float* transforms,
                    float* posed_xyz, float* posed_cov, float* tf, void* stream);
/* Backward.  dL_dtf (P,N,12) may be NULL.  Outputs fully written, summed over
 * poses: dL_dxyz (N,3) (direct path only — the skin-weight path is dL_dw),
 * dL_dlog_scale (N,3), dL_drot (N,4), dL_dw (N,B) (NULL when skin_w is NULL). */
int mgr_lbs_cov_bwd(int P, int N, int B, const float* xyz, const float* log_scale,
                    const float* rot, const float* skin_w, const float* transforms,
                    const float* dL_dposed_xyz, const float* dL_dposed_cov, const float* dL_dtf,
                    float* dL_dxyz, float* dL_dlog_scale, float* dL_drot, float* dL_dw,
                    void* stream);

/* SH degree-3 colour for V views.  sh: (N,16,3).  If tf != NULL (V,N,12 with
 * stride_tf floats per view, 0 = shared) the camera is pulled back to canonical
 * space: dir = xyz - inv(tf)*campos; else dir = xyz - campos, where xyz has
 * stride_xyz floats per view.  colors (V,N,3) = max(sh2rgb + 0.5, 0). */
int mgr_sh_color_fwd(int V, int N, const float* sh, const float* xyz, int64_t stride_xyz,
                     const float* tf, int64_t stride_tf, const float* cams, float* colors,
                     void* stream);
/* Outputs fully written: dL_dsh (N,16,3) summed over views, dL_dxyz (V,N,3) per
 * view, dL_dtf (V,N,12) per view (NULL when tf is NULL). */
int mgr_sh_color_bwd(int V, int N, const float* sh, const float* xyz, int64_t stride_xyz,
                     const float* tf, int64_t stride_tf, const float* cams,
                     const float* dL_dcolors, float* dL_dsh, float* dL_dxyz, float* dL_dtf,
                     void* stream);

/* The same four with the rows of tf / dL_dtf `tf_row_floats` apart: 12 (as above) or 16 = the reference's (N,4,4) layout
 * (TrainingModule.forward returns the blended transforms as 4x4, src/modules/hand_dynamic.py:128-137, and render_gaussians
 * takes them as such, src/utils/gaussian_utils.py:431-449): mgr_lbs_cov_fwd_rows then writes the constant last row
 * (0,0,0,1) too, mgr_sh_color_bwd_rows writes zeros into the last row of dL_dtf, the readers skip it -- no torch.cat /
 * slice copy between the two operators and none in their backward (round 6). */
int mgr_lbs_cov_fwd_rows(int P, int N, int B, const float* xyz, const float* log_scale,
                         const float* rot, const float* skin_w, const float* transforms,
                         float* posed_xyz, float* posed_cov, float* tf, int tf_row_floats, void* stream);
int mgr_lbs_cov_bwd_rows(int P, int N, int B, const float* xyz, const float* log_scale,
                         const float* rot, const float* skin_w, const float* transforms,
                         const float* dL_dposed_xyz, const float* dL_dposed_cov, const float* dL_dtf, int tf_row_floats,
                         float* dL_dxyz, float* dL_dlog_scale, float* dL_drot, float* dL_dw, void* stream);
/* Pose gradient of the modular route: what mgr_lbs_cov_bwd_rows leaves out.  dL_dtransforms (P,B,16):
 * dL_dtransforms[p][b][r][c] = sum_n skin_w[n][b] * G[p][n][r][c] for r < 3, where G is the dL/d(blended transform) that
 * backward forms per Gaussian before it contracts it with T_b (dL_dposed_xyz (x) [xyz, 1], the covariance path into columns
 * 0..2, plus the incoming dL_dtf, which may be NULL); row 3 is written as zero, the background transform is a row like any
 * other, the output is fully written.  No reference counterpart (config/model/pose_optimizer.yaml names
 * src.models.pose_optimizer, which was never released).  B <= MGR_MAX_BONES, tf_row_floats 12 or 16; skin_w == NULL is an
 * error (a static object has no transforms).  Two stages, no float atomics, bit-reproducible: min(1024, ceil(N / 256))
 * workgroups per pose reduce their chunks of 256 Gaussians in a fixed order and write one partial each, a fold kernel adds
 * the partials in a fixed order.  workspace_bytes >= mgr_lbs_pose_workspace_bytes(P, N, B) =
 * min(1024, ceil(N / 256)) x P x B x 12 x 4 bytes. */
size_t mgr_lbs_pose_workspace_bytes(int P, int N, int B);
int mgr_lbs_pose_bwd(int P, int N, int B, const float* xyz, const float* log_scale, const float* rot,
                     const float* skin_w, const float* transforms, const float* dL_dposed_xyz,
                     const float* dL_dposed_cov, const float* dL_dtf, int tf_row_floats, float* dL_dtransforms,
                     void* workspace, size_t workspace_bytes, void* stream);
int mgr_sh_color_fwd_rows(int V, int N, const float* sh, const float* xyz, int64_t stride_xyz,
                          const float* tf, int64_t stride_tf, int tf_row_floats, const float* cams, float* colors,
                          void* stream);
int mgr_sh_color_bwd_rows(int V, int N, const float* sh, const float* xyz, int64_t stride_xyz,
                          const float* tf, int64_t stride_tf, int tf_row_floats, const float* cams,
                          const float* dL_dcolors, float* dL_dsh, float* dL_dxyz, float* dL_dtf,
                          void* stream);

/* Host glue of the reference-shaped route, one launch each (no reference kernel counterpart: the reference does both with
 * a dozen small torch ops per step).
 * mgr_pack_camera: the (MGR_CAM_FLOATS = 40)-float camera row every kernel here reads, from the fields of
 *   GaussianRasterizationSettings (src/utils/gaussian_utils.py:378-391): [tanfovx, tanfovy, viewmatrix 16, projmatrix 16,
 *   campos 3, 0 0 0]; the matrices as the reference stores them (row-major of the transposed = column-major float[16],
 *   SURVEY App. A).  view16 / proj16 / campos3 are DEVICE pointers and may be NULL (zeros); the scalars travel as kernel
 *   arguments, so no host-to-device copy is made.
 * mgr_bone_transforms: T_b = posed_b @ inv(rest_b) for B bones (4x4 row-major each), + one identity row when
 *   `background` (src/modules/hand_dynamic.py:93-102); out (B + background, 4, 4). */
int mgr_pack_camera(float tanfovx, float tanfovy, const float* view16, const float* proj16, const float* campos3,
                    float* out40, void* stream);
int mgr_bone_transforms(int B, int background, const float* posed, const float* rest, float* out, void* stream);

/* Pose chain on the device (csrc/pose.hip; manus_amd/pose.py: PoseRefiner).  No reference counterpart: the reference's
 * config names src.models.pose_optimizer, which was never released.  A per-frame, per-bone correction rotvec / trans (F,B,3)
 * of the posed bone matrices, in the bone's local frame:
 *     T[v,b] = (posed[v,b] @ [[exp(rotvec[f,b]), trans[f,b]], [0,0,0,1]]) @ inv(rest[b])
 * exp = Rodrigues, R = I + a K + b K^2 with a = sin(th)/th, b = (1 - cos th)/th^2, and for t = |r|^2 < 1e-6 the series
 * a = 1 - t/6 + t^2/120, b = 1/2 - t/24 (pose._exp_so3).  The inverse and the last product are those of mgr_bone_transforms
 * (same elimination, same summation order): a zero correction, or no correction, gives its bits.  fp32, one thread per small
 * matrix, one or two workgroups per launch, no workspace, no atomics.  All pointers are DEVICE pointers; posed is
 * (V_all,B,4,4) and transforms (V_all,B+1,4,4), the tables of all views, rest (B,4,4); view_rows[k] (int32) is the row of
 * those tables the step's position k shows, frame_of_view[k] (int32) its row of rotvec / trans -- outside [0,F) (-1 for
 * validation views): no correction.  The caller vouches for view_rows lying inside the tables.
 * Every entry refuses, before any launch and with mgr_last_error() naming it: a NULL pointer (gathered alone may be NULL),
 * V, B or U below 1, B > MGR_MAX_BONES, F < 1.
 *
 * mgr_pose_apply: T of the positions k < V into transforms[view_rows[k], 0..B-1], the identity into row B; the same B+1
 *   rows into gathered[k] (V,B+1,4,4), the contiguous copy the fused kernels read, when it is given.  Rows of views not
 *   listed are not touched.
 * mgr_pose_backward: d_transforms (V,B+1,4,4) by position (the step's "d_transforms").  Per position and bone
 *   dC = posed[v,b]^T dT inv(rest[b])^T; d_trans = dC[:3,3]; d_rotvec = the vector-Jacobian product of exp at rotvec[f,b]
 *   with dC[:3,:3], the series branch differentiated as a series (da/dt = -1/6 + t/60, db/dt = -1/24).  Row u of d_rotvec /
 *   d_trans (U,B,3) is the sum over the positions with frame_of_view[k] == frames_listed[u], in ascending k by ONE thread per
 *   (u, bone): deterministic.  A listed frame without a view (or outside [0,F)) gets zeros; positions whose frame is not
 *   listed contribute nothing.
 * mgr_pose_adam: the row Adam of mgr_skin_grid_adam (torch.optim.SparseAdam: parameters and moments of the listed rows only,
 *   bias correction of the global `step` >= 1) on the rows frames_listed[u] (distinct, inside the tables: the caller's to
 *   ensure; negative entries are skipped) of rotvec / trans and their moments m_r, v_r, m_t, v_t (F,B,3), from d_rotvec /
 *   d_trans (U,B,3).  Separate learning rates, no clamp.
 * mgr_pose_backward_prior: mgr_pose_backward (one kernel body instantiated twice: the same sums in the same order; the two
 *   instantiations may differ in the last bit of the chain gradient, as the compiler fuses other products) with priors.  For
 *   x = rotvec or trans, each with its own pair of weights (finite, >= 0),
 *       E = w_mag sum_f |x_f|^2 + w_smooth sum_edges |x_f - x_next(f)|^2
 *   where neighbours (F,2) int32 gives (prev, next) of every frame row, -1 = none (an index outside [-1,F) is read as -1; the
 *   caller keeps the table symmetric: next(prev(f)) = f).  Row u of d_rotvec / d_trans gains the true dE/dx_f of f =
 *   frames_listed[u], 2 w_mag x_f + 2 w_smooth ((x_f - x_prev) + (x_f - x_next)), formed in fp32 in that order -- the
 *   differences, their sum prev first, the two products, then the addition to the chain gradient -- uncontracted.  Neighbours
 *   that are not listed are read, never written: the tables are read-only here, and mgr_pose_adam behind this entry is what
 *   moves the listed rows, so every prior gradient of a step is taken at the tables before the step.  *prior_value (double,
 *   device) = the part of E that touches the listed rows, each term once: their magnitude terms, every edge (f, next(f)) of
 *   a listed f, and every edge (prev(f), f) of a listed f whose prev is NOT listed (found by walking frames_listed, which may
 *   be in any order).  The differences are the gradient's fp32 ones, squared and added in fp64: one share per (u, bone)
 *   thread in the workspace (mgr_pose_prior_workspace_bytes(U, B) bytes), folded by one workgroup in a fixed order -- no
 *   float atomics, equal bits run to run.  With all four weights zero this is mgr_pose_backward's own launch (equal bits),
 *   neighbours / workspace may be NULL, and *prior_value, if given, is set to 0.  Refused before any launch, nothing written:
 *   all of mgr_pose_backward's conditions; a negative or non-finite weight; NULL neighbours with a smoothness weight
 *   non-zero; NULL prior_value or workspace with any weight non-zero; a short workspace (MGR_ENOMEM). */
int mgr_pose_apply(int V, int B, int F, const int32_t* view_rows, const int32_t* frame_of_view, const float* posed,
                   const float* rest, const float* rotvec, const float* trans, float* transforms, float* gathered, void* stream);
int mgr_pose_backward(int V, int B, int F, int U, const int32_t* frames_listed, const int32_t* view_rows,
                      const int32_t* frame_of_view, const float* posed, const float* rest, const float* rotvec,
                      const float* trans, const float* d_transforms, float* d_rotvec, float* d_trans, void* stream);
int mgr_pose_adam(int U, int B, const int32_t* frames_listed, const float* d_rotvec, const float* d_trans, float* rotvec,
                  float* trans, float* m_r, float* v_r, float* m_t, float* v_t, double lr_rot, double lr_trans, double beta1,
                  double beta2, double eps, int step, void* stream);
size_t mgr_pose_prior_workspace_bytes(int U, int B);
int mgr_pose_backward_prior(int V, int B, int F, int U, const int32_t* frames_listed, const int32_t* view_rows,
                            const int32_t* frame_of_view, const float* posed, const float* rest, const float* rotvec,
                            const float* trans, const float* d_transforms, float* d_rotvec, float* d_trans,
                            const int32_t* neighbours, double w_mag_rot, double w_smooth_rot, double w_mag_trans,
                            double w_smooth_trans, double* prior_value, void* workspace, size_t workspace_bytes, void* stream);

/* Kinematic pose chain on the device (csrc/fk.hip; manus_amd/pose.py: KinematicPoseRefiner): joint angles through forward
 * kinematics instead of a free correction per bone.  The reference's config/model/pose_optimizer.yaml names this
 * parametrisation (num_pose_parameters: 23, optimize_global_R / optimize_global_T) and src/utils/transforms.py carries its
 * host machinery (euler_angles_to_armature_space, apply_constraints_to_poses, apply_limits_to_poses); the optimizer itself was
 * never released.  J bones, parents[i] (int32) in {-1} u [0, i) -- several roots are allowed; an entry outside that set is
 * READ AS -1 by the kernels, so no list can make them index outside their tables (the Python class refuses such a list).
 * theta (F, J+2, 3) per frame row: row 0 the global Euler angles g, rows 1..J the bones' Euler angles e_i, row J+1 the global
 * translation t.  E(e) = Rz(e2) Ry(e1) Rx(e0) (transforms.euler_angles_to_matrix(e, "XYZ", intrinsic=True)), H(R) its
 * homogeneous 4x4.  Constants, built once by the caller in fp64 and stored in fp32: local (J,4,4) = inv(rest_parent(i)) rest_i,
 * rest_i for a root; base (F,4,4), a fixed left transform per frame from armature to world.
 *     A_f = base_f [[E(g), t], [0,0,0,1]]
 *     M_i = (A_f for a root, M_parent(i) otherwise) local_i H(E(e_i))
 *     T[v,i] = M_i inv(rest_i)                                             f = the frame view v shows
 * The inverse and the last product are those of mgr_bone_transforms (bone_math.h).  fp32, row-major 4x4, one workgroup of one
 * wave per view / per listed frame; the tree is walked sequentially in index order (four threads, one matrix row each), every
 * sum in a fixed order, no atomics, no workspace: two runs give equal bits.  All pointers are DEVICE pointers; posed
 * (V_all,J,4,4), transforms (V_all,J+1,4,4), view_rows, frame_of_view and frames_listed as for the pose chain above.
 * Every entry refuses with MGR_EINVAL, before any launch and with nothing written: J outside 1 .. MGR_MAX_BONES, V, U or F
 * below 1, a NULL pointer other than gathered / posed_out, and (mgr_fk_adam) step < 1 or a non-finite rate.
 *
 * mgr_fk_apply: T of the positions k < V into transforms[view_rows[k], 0..J-1], the identity into row J, and the same J+1 rows
 *   into gathered[k] (V,J+1,4,4) when it is given -- the background row and the gathered copy exactly as mgr_pose_apply
 *   writes them.  posed_out (V,J,4,4), when given, receives the M_i by position.  A position whose frame lies outside [0,F)
 *   (-1: a validation view) gets the bits of mgr_bone_transforms on its row of posed (and that row in posed_out); rows of
 *   views not listed are not touched.
 * mgr_fk_backward: d_transforms (V,J+1,4,4) by position.  Per listed frame f: G_i = the sum, in ascending position, over the
 *   positions showing f of dT[k,i] inv(rest_i)^T; bones in descending index pass G_i (local_i H(E(e_i)))^T up to their parent
 *   (a root: into dA); dL/dE(e_i) is the 3x3 block of (M_parent local_i)^T G_i (A_f in place of M_parent for a root), dL/de_i
 *   its contraction with the three analytic partials of Rz Ry Rx (no division: finite at e_1 = pi/2); dL/dg and dL/dt come
 *   from base_f^T dA in the same way.  Row u of d_theta (U,J+2,3) is that gradient of frames_listed[u], every element taken
 *   times mask (J+2,3) of 0 / 1 -- an element with mask 0 is exactly 0, whatever the sums hold.  A listed frame that no position
 *   shows (or outside [0,F)) gets zeros; rows behind U are not touched.
 * mgr_fk_adam: mgr_pose_adam's row Adam (the same device function) on the rows frames_listed[u] of theta and its moments m, v
 *   (F,J+2,3) from d_theta (U,J+2,3): rows 0..J at lr_rot, row J+1 at lr_trans; the stepped value is then clamped to
 *   [lo, hi] (J+2,3), +-inf: no limit.  Elements with mask 0 and frames not listed (negative entries are skipped) keep their
 *   bits, moments included. */
int mgr_fk_apply(int V, int J, int F, const int32_t* view_rows, const int32_t* frame_of_view, const float* posed, const float* rest,
                 const float* local, const int32_t* parents, const float* base, const float* theta, float* transforms,
                 float* gathered, float* posed_out, void* stream);
int mgr_fk_backward(int V, int J, int F, int U, const int32_t* frames_listed, const int32_t* view_rows,
                    const int32_t* frame_of_view, const float* rest, const float* local, const int32_t* parents, const float* base,
                    const float* theta, const float* mask, const float* d_transforms, float* d_theta, void* stream);
int mgr_fk_adam(int U, int J, const int32_t* frames_listed, const float* d_theta, float* theta, float* m, float* v,
                const float* mask, const float* lo, const float* hi, double lr_rot, double lr_trans, double beta1, double beta2,
                double eps, int step, void* stream);

/* mgr_fk_backward_terms: mgr_fk_backward with three opt-in terms on the angles of the listed frames (another
 * instantiation of mgr_fk_backward's kernel template: one body, the same order of every sum, and that entry's bits).  Rows 0..J
 * of theta take the "rot" weights, row J+1 the "trans" weights; all five weights finite and >= 0.
 *     E_dev    = sum_f sum_{r,c: mask != 0} w_dev(r)    (theta_f[r,c] - theta_ref_f[r,c])^2
 *     E_smooth = sum_{edges (f, next f)} sum_{r,c: mask != 0} w_smooth(r) (theta_f[r,c] - theta_next[r,c])^2
 *     E_kp     = w_kp sum_f sum_{k<K} c[f,k] |p_k(theta_f) - y[f,k]|^2,   p_k = (M_{bone[k]}(theta_f) [o_k; 1])[:3]
 *   theta_ref (F,J+2,3); neighbours (F,2) int32 = (prev, next) of every frame row, -1 = none (outside [-1,F): read as -1; the caller
 *   keeps it symmetric), differences plain, without an angle wrap; kp_bone (K) int32, kp_offset (K,3) in the bone's own frame,
 *   kp_target (F,K,3), kp_weight (F,K), K 1 .. MGR_FK_MAX_KEYPOINTS.  A keypoint is SKIPPED -- exactly 0 in gradient and value,
 *   whatever its target holds -- unless its weight is > 0 (zero, negative, NaN: skipped) and its bone lies in [0,J).
 *   Gradient: row u of d_theta gains the true dE/dtheta_f of f = frames_listed[u], everything at the tables before the step
 *   (mgr_fk_adam is the launch behind: Jacobi; unlisted neighbours are read, never written).  Per element the prior part is
 *   2 w_dev (x - x_ref) + 2 w_smooth ((x - x_prev) + (x - x_next)) in fp32, uncontracted: the differences, their sum prev first,
 *   the two products ((float)(2 w) each), their sum, the addition to the chain gradient, then the mask (mask 0: exactly 0).
 *   The keypoint part goes through the tree: with r_k = p_k - y and g_k = ((float)(2 w_kp) c) r_k, rows 0..2 of G_bone[k] gain
 *   g_k (x) [o_k; 1] behind the view sum, in ascending k, by the one thread that owns the bone -- no atomics --, and the upward
 *   pass and the angle partials of mgr_fk_backward follow unchanged.  The terms do not depend on views: a listed frame inside
 *   [0,F) that no position shows gets the terms' gradient on a zero chain part; a listed frame outside [0,F) gets zeros.
 *   values (4 doubles, device) = E_dev, E_smooth, E_kp and their sum, each the part that touches the listed rows, each term
 *   once: every edge (f, next f) of a listed f and every edge (prev f, f) of a listed f whose prev is NOT listed (found by
 *   walking frames_listed, in any order).  The gradient's fp32 differences and residuals are squared and added in fp64; one
 *   share per listed frame and term in the workspace (mgr_fk_terms_workspace_bytes(U, J, K) bytes), folded by one workgroup in
 *   list order: no float atomics, equal bits run to run.
 *   All five weights zero: mgr_fk_backward's own launch (equal bits); theta_ref, neighbours, the keypoint pointers and the
 *   workspace may be NULL; values, if given, is set to zeros.  Any weight non-zero: d_transforms may be NULL -- the chain part
 *   is zero, view_rows / frame_of_view are not read and V may be 0.
 *   Refused before any launch, nothing written: all of mgr_fk_backward's conditions but those relaxed above; a negative or
 *   non-finite weight; NULL theta_ref with a dev weight on; NULL neighbours with a smooth weight on; w_kp != 0 with K outside
 *   1 .. MGR_FK_MAX_KEYPOINTS or a NULL keypoint pointer; NULL values or workspace with any weight on; a short workspace
 *   (MGR_ENOMEM). */
#define MGR_FK_MAX_KEYPOINTS 64
size_t mgr_fk_terms_workspace_bytes(int U, int J, int K);
int mgr_fk_backward_terms(int V, int J, int F, int U, const int32_t* frames_listed, const int32_t* view_rows,
                          const int32_t* frame_of_view, const float* rest, const float* local, const int32_t* parents, const float* base,
                          const float* theta, const float* mask, const float* d_transforms, float* d_theta,
                          const float* theta_ref, const int32_t* neighbours,
                          double w_dev_rot, double w_smooth_rot, double w_dev_trans, double w_smooth_trans,
                          int K, const int32_t* kp_bone, const float* kp_offset, const float* kp_target, const float* kp_weight, double w_kp,
                          double* values, void* workspace, size_t workspace_bytes, void* stream);

/* mgr_fk_backward_terms2d: mgr_fk_backward_terms with a fourth opt-in term, the multi-view 2-D reprojection of the same keypoints
 * (a third instantiation of the same kernel template: the other two entries keep their bits).  All of
 * mgr_fk_backward_terms' arguments, and behind w_kp: C cameras, kp2d_proj (C,3,4) the projections P_c (for pixels K_c E_c[:3,:4],
 * mgr_project_points' convention; formed by the caller in fp64, stored in fp32), kp2d_target (F,C,K,2), kp2d_weight (F,C,K),
 * w_kp2d, delta (the Huber radius; 0: the plain square), z_min and kp2d_dist (U,C,K), which may be NULL.
 *     q = P_c [p_k(theta_f); 1],   u = q[:2] / q[2],   r = u - t[f,c,k],   d = |r|
 *     rho(d) = d^2 where delta == 0 or d <= delta,   2 delta d - delta^2 otherwise
 *     E_kp2d = w_kp2d sum_f sum_{c<C} sum_{k<K} s[f,c,k] rho(d[f,c,k])
 *   with p_k, kp_bone and kp_offset those of E_kp.  Units are the caller's: P and the targets may be pre-scaled, w_kp2d and delta
 *   are then in that unit.  A detection is SKIPPED -- exactly 0 in gradient and value, NaN in kp2d_dist, whatever its target
 *   holds -- unless its weight is > 0 (zero, negative, NaN: skipped), its bone lies in [0,J) and q[2] > (float)z_min.
 *   Gradient, fp32 and uncontracted: g_u = (((float)(2 w_kp2d) s) h) r with h = 1 inside delta (or delta == 0) and delta / d
 *   outside; dE/dq = [g_u0 / q2, g_u1 / q2, -(g_u0 u0 + g_u1 u1) / q2]; dE/dp = P_c[:, :3]^T dE/dq.  Per keypoint the cameras'
 *   dE/dp are added over a fixed tree of camera slices: lane group g of the wave's 64 / K groups adds the cameras g, g + 64 / K, ...
 *   in ascending index, and the keypoint's thread adds the groups' sums in ascending g -- an order that depends on C and K alone;
 *   cameras are read from global memory and nothing is sized by C.  That sum is added to the 3-D term's g_k (the 3-D part first, 0
 *   when w_kp == 0); g_k (x) [o_k; 1] then
 *   enters rows 0..2 of G_bone[k] exactly as for E_kp and the upward pass follows unchanged.  Row u of d_theta depends on the inputs
 *   of frame frames_listed[u] alone: not on U, the order of the list or the other frames listed.  The term needs no view.
 *   values (5 doubles, device) = E_dev, E_smooth, E_kp, the sum of all four terms, E_kp2d: values[3] = ((v0 + v1) + v2) + v4.  The
 *   fp32 residuals and distances of the active detections are weighted and added in fp64, one share per listed frame and term in
 *   the workspace (mgr_fk_terms2d_workspace_bytes(U, J, K, C) bytes), folded by one workgroup in list order.
 *   kp2d_dist, when given, receives d of every detection of the listed frames (NaN where skipped, and for a listed frame outside
 *   [0,F)), also for a listed frame no view shows.  kp_target / kp_weight may be NULL when w_kp == 0; d_transforms may be NULL.
 *   w_kp2d == 0: mgr_fk_backward_terms' own path on the first 31 arguments (its refusals, its launches, equal bits); values[4] = 0
 *   when values is given, kp2d_dist (when given, with C and K >= 1) all NaN, and every 2-D pointer may be NULL.
 *   Refused before any launch, nothing written: a negative or non-finite w_kp2d or delta; z_min not finite or not > 0; and with
 *   w_kp2d != 0: all of mgr_fk_backward_terms' conditions for a call with a term on; C < 1; K outside 1 .. MGR_FK_MAX_KEYPOINTS; a
 *   NULL kp_bone, kp_offset, kp2d_proj, kp2d_target or kp2d_weight; w_kp != 0 with a NULL kp_target or kp_weight; NULL values or
 *   workspace; a short workspace (MGR_ENOMEM). */
size_t mgr_fk_terms2d_workspace_bytes(int U, int J, int K, int C);
int mgr_fk_backward_terms2d(int V, int J, int F, int U, const int32_t* frames_listed, const int32_t* view_rows,
                            const int32_t* frame_of_view, const float* rest, const float* local, const int32_t* parents, const float* base,
                            const float* theta, const float* mask, const float* d_transforms, float* d_theta,
                            const float* theta_ref, const int32_t* neighbours,
                            double w_dev_rot, double w_smooth_rot, double w_dev_trans, double w_smooth_trans,
                            int K, const int32_t* kp_bone, const float* kp_offset, const float* kp_target, const float* kp_weight, double w_kp,
                            int C, const float* kp2d_proj, const float* kp2d_target, const float* kp2d_weight,
                            double w_kp2d, double delta, double z_min, float* kp2d_dist,
                            double* values, void* workspace, size_t workspace_bytes, void* stream);

/* mgr_triangulate: robust multi-view triangulation of F * K independent (frame, keypoint) problems -- the input side of the two
 * keypoint terms above.  proj (C,3,4), targets (F,C,K,2) and weights (F,C,K) in the layouts of mgr_fk_backward_terms2d's kp2d_*
 * tables; C <= MGR_TRI_MAX_CAMERAS (a camera is a lane of the problem's wave, a set of cameras one ballot).  Deterministic, no
 * sampling; the full definition stands above the entry in csrc/triangulate.hip.  In short, per problem:
 *   active     s > (float)min_conf (NaN: not), both target coordinates finite, both plane norms finite and > 0
 *   planes     a_u = t_x P2 - P0, a_v = t_y P2 - P1, each divided by the norm of its first three components -> (n, d), fp32
 *   solve      N = sum w (n_u n_u^T + n_v n_v^T), b = -sum w (d_u n_u + d_v n_v); accepted iff det N > det_min (tr N / 3)^3;
 *              X = adj(N) b / det N in closed form
 *   inlier     active, q[2] > (float)z_min and |q[:2] / q[2] - t| < (float)tau with q = P_c [X; 1], fp32
 *   seed       the pairs a < b of active cameras in lexicographic order, X_ab = solve({a,b}, 1) in fp32, accepted only with both
 *              cameras' own depths above z_min; the FIRST pair with the most inliers; none accepted: invalid
 *   refit      refit_rounds times: S = inliers(X); |S| < 2 or a rejected solve: invalid; X = solve(S, s), products and sums in fp64
 *              over the cameras in ascending order, X rounded to fp32.  Then S = inliers(X), the final set
 *   polish     gn_iters Gauss-Newton steps on sum_S s |u(X) - t|^2 over the fixed S: residuals and Jacobians fp32, H and g in fp64,
 *              the same determinant test on H; a rejected H ends the polish and keeps X
 * Outputs: xyz (F,K,3) = X after the polish; conf (F,K) = sum_S s / |S|; n_inliers (F,K) = |S|; inliers (F,C,K) bytes 0 / 1 = S, the
 * set the fit used, classified BEFORE the polish; dist (F,C,K) = the pixel distance at the final X, AFTER the polish, for active
 * cameras with q[2] > z_min there, NaN otherwise.  inliers and dist may be NULL.  A problem that is invalid by the rules above,
 * or whose |S| < min_views, gives xyz = NaN, conf = 0, n_inliers = 0, inliers = 0, dist = NaN and nothing else.  No atomics, no
 * workspace: equal bits run to run, and a problem's bits do not depend on the other problems of the call.
 * Refused before any launch, nothing written: F, C or K < 1; C > MGR_TRI_MAX_CAMERAS; a NULL proj, targets, weights, xyz, conf or
 * n_inliers; tau, z_min or det_min not finite or not > 0; min_conf negative or not finite; min_views < 2; refit_rounds < 1;
 * gn_iters < 0; F * K above 2^30. */
#define MGR_TRI_MAX_CAMERAS 64
int mgr_triangulate(int F, int C, int K, const float* proj, const float* targets, const float* weights,
                    double tau, double min_conf, int min_views, double z_min, double det_min,
                    int refit_rounds, int gn_iters,
                    float* xyz, float* conf, int32_t* n_inliers, uint8_t* inliers, float* dist, void* stream);

/* uv =(K*E*[x;1])[:2]/z for N points; K (3,3), E (3,4) row-major. */
int mgr_project_points(int N, const float* xyz, const float* K9, const float* E12, float* uv,
                       void* stream);

/* Segmentation-mask pruning test of on_after_backward (src/modules/hand_dynamic.py:193-209,
 * src/modules/object.py:66-72).
 * mgr_dilate_mask: dilate_mask, src/utils/gaussian_utils.py:35-47 (conv2d with a kernel_size^2 box of
 *   ones, zero padding, > 0) on a (H,W) byte mask (non-zero = set); scratch and out are (H,W) bytes.
 * mgr_points_outside_mask: get_points_outside_mask, src/utils/gaussian_utils.py:101-147:
 *   out[i] = !mask[int(clamp(v_i, 0, H-1))][int(clamp(u_i, 0, W-1))] with (u,v) = project_points(xyz_i);
 *   when any of the n_keypoints keypoints (may be 0 / NULL) lands outside the mask, all out[i] = 0
 *   (:125-131).  mask: the (already dilated, when the caller asks for dilate=True) (H,W) byte mask. */
int mgr_dilate_mask(int H, int W, int kernel_size, const uint8_t* mask, uint8_t* scratch, uint8_t* out,
                    void* stream);
int mgr_points_outside_mask(int N, const float* xyz, const float* K9, const float* E12, int H, int W,
                            const uint8_t* mask, int n_keypoints, const float* keypoints, uint8_t* out,
                            void* stream);
/* out[i] = mean_k |xyz_i - keypoint_k| > thresh: the keypoint-distance pruning test,
 * src/modules/hand_dynamic.py:210-218 (torch.cdist(posed_xyz, keypoints).mean(1) > 0.2). */
int mgr_keypoint_far_mask(int N, const float* xyz, int n_keypoints, const float* keypoints, float thresh,
                          uint8_t* out, void* stream);

/* ------------------------------------------------------------------------
 * simple-knn: mean squared distance to the 3 nearest other points
 * ------------------------------------------------------------------------ */
size_t mgr_knn3_workspace_bytes(int N);
int mgr_knn3_mean_dist2(int N, const float* xyz, float* out, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Exact k nearest neighbours of every point among the points themselves (knn_k.hip).
 *
 * xyz (N,3) device floats, 1 <= k <= MGR_KNN_MAX_K.  The squared distance is fp32, (dx*dx + dy*dy) + dz*dz with no
 * contraction (mgr_contact_dist's rule).  The neighbours of i are the points j with the smallest keys (d2, j): the lower
 * index wins a tie.  include_self = 1 keeps i itself (d2 = 0: what a kd-tree query at a stored point returns);
 * include_self = 0 excludes i by index, not by distance.  A point with a non-finite coordinate is nobody's neighbour and
 * has no neighbours; n_i = min(k, number of finite candidates).
 *   out_idx (N,k) int32, out_d2 (N,k)   row i in ascending key order; slots beyond n_i hold -1 / +inf
 *   out_sigma (N)    sqrtf((float)(S / n_i)), S the fp64 sum of the row's d2 taken in an order that is a function of the
 *                    sorted row alone (every 64th entry from each of 64 starts, nearest first, then a fixed butterfly of the
 *                    64 partial sums); NaN for n_i = 0
 *   out_count (N)    int32 n_i
 * Every output may be NULL.  N = 0 is valid (nothing is launched); N < k, N = k and N = k + 1 are ordinary cases.
 * Results are the same bits run to run: nothing depends on the order the grid's cells were filled in.
 * workspace_bytes >= mgr_knn_self_workspace_bytes(N, k) (a grid of at most max(N, 64) cells and 16 bytes per point).
 * Refused before any launch, outputs untouched: MGR_EINVAL for N < 0, k out of range, a NULL xyz with N > 0; MGR_ENOMEM for a
 * NULL or short workspace.
 * The cell edge follows k: about max(MGR_KNN_CELL_MIN_POINTS, k / MGR_KNN_CELL_K_DIV) points per cell over the bounding box.
 * ------------------------------------------------------------------------ */
#define MGR_KNN_MAX_K 512
#ifndef MGR_KNN_CELL_K_DIV            /* (-DMGR_KNN_CELL_K_DIV=... builds a library with another cell size: a measurement aid) */
#define MGR_KNN_CELL_K_DIV 16.0f
#endif
#define MGR_KNN_CELL_MIN_POINTS 2.0f
size_t mgr_knn_self_workspace_bytes(int N, int k);
int mgr_knn_self(int N, const float* xyz, int k, int include_self, float* out_d2, int32_t* out_idx, float* out_sigma,
                 int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Local Outlier Probability (LoOP; Kriegel, Kroeger, Schubert, Zimek, CIKM 2009) of every point, on the neighbourhoods of
 * mgr_knn_self: the filter behind the reference's update_mask_based_on_outliers (src/utils/gaussian_utils.py:557-568 calls
 * MeshLab's compute_selection_point_cloud_outliers through pymeshlab).  MeshLab's own constants (its erf approximation,
 * whether it counts the query point) cannot be pinned without it; every such choice is an argument or a constant here.
 *
 * With S_i the neighbour set of i above (n_i members) and lambda = MGR_LOOP_LAMBDA = 1:
 *   sigma_i = as out_sigma of mgr_knn_self
 *   den_i   = (float)((fp64 sum over j in S_i of sigma_j, in the order of sigma's own sum) / n_i)
 *   plof_i  = sigma_i / den_i - 1                      (0 where den_i == 0)
 *   nplof   = lambda * sqrt(mean over the valid points of plof_i^2)     (fp64: one partial per workgroup, then a fixed-order
 *             fold; no float atomics; 0 when no point is valid)
 *   score_i = max(0, erff(plof_i / (nplof * sqrt(2)))) (0 for every valid point when nplof == 0)
 *   mask_i  = score_i > prob                           (a NaN score gives 0)
 * A point with n_i = 0 (non-finite, or alone with include_self = 0) has NaN sigma, plof and score and is left out of the mean.
 *   out_score (N) required; out_mask (N) uint8, out_sigma (N), out_plof (N) or NULL
 *   out_stats       3 device doubles [nplof, n_valid, n_flagged] or NULL
 * Nothing is read back to the host.  Equal bits run to run.  The second pass reads the neighbour indices the first stored in
 * the workspace: workspace_bytes >= mgr_outlier_scores_workspace_bytes(N, k) = the search's + 4 N k + 28 N bytes, rounded.
 * Refused before any launch, outputs untouched: MGR_EINVAL for N < 0, k out of range, a NULL xyz or out_score with N > 0;
 * MGR_ENOMEM for a NULL or short workspace.  N = 0: out_stats (if given) becomes [0, 0, 0].
 * ------------------------------------------------------------------------ */
#define MGR_LOOP_LAMBDA 1.0f
#define MGR_LOOP_SQRT2 1.41421356237309505f
size_t mgr_outlier_scores_workspace_bytes(int N, int k);
int mgr_outlier_scores(int N, const float* xyz, int k, int include_self, float prob, float* out_score, uint8_t* out_mask,
                       float* out_sigma, float* out_plof, double* out_stats, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ------------------------------------------------------------------------
 * Image loss used by the benchmark step: L = mean|a-b| over (V,3,H,W);
 * writes dL/da = sign(a-b) * scale and accumulates sum|a-b| into loss_sum[0].
 * (src/utils/loss_utils.py:22-27 with src/modules/base.py:329-331.)
 * ------------------------------------------------------------------------ */
int mgr_l1_loss_grad(int64_t count, const float* a, const float* b, float scale, float* dL_da,
                     float* loss_sum, void* stream);

/* ------------------------------------------------------------------------
 * Training image loss, forward + backward in one pass:
 *   L = grad-scaled  w_l1 * sum|pred - target|  +  w_ssim * (- sum ssim_map)
 * over images in the rasterizer's (V,3,H,W) layout.  Replaces l1_loss
 * (src/utils/loss_utils.py:22-27) and ssim (src/utils/loss_utils.py:57-97) as
 * called by loss_func (src/modules/base.py:323-365) together with their
 * autograd backward.  The reference evaluates ssim() on HWC tensors, so its
 * 11x11 window runs over the (W,3) plane of every image row (groups = H,
 * loss_utils.py:58); that is the statistic computed here.
 *   dL_dpred (V,3,H,W) = grad_scale * (w_l1 * sign(pred - target) - w_ssim * d(sum ssim_map)/dpred)
 *   sums[0] = sum|pred - target|, sums[1] = sum of the ssim map (both over V*3*H*W values),
 *   sums[2] = grad_scale * (w_l1 * sums[0] - w_ssim * sums[1]) + loss_offset  (the loss value whose
 *             gradient dL_dpred is; loss_offset carries the constant of "1 - ssim"),
 * so mean L1 = sums[0]/(V*3*H*W) and the reference's ssim(...) of one view = sums[1]/(3*H*W).
 * workspace: mgr_image_loss_workspace_bytes(V,H,W) bytes of scratch (per-workgroup sums).
 * ------------------------------------------------------------------------ */
size_t mgr_image_loss_workspace_bytes(int V, int H, int W);
int mgr_image_loss(int V, int H, int W, const float* pred, const float* target, float w_l1, float w_ssim,
                   float grad_scale, float loss_offset, float* dL_dpred, float* sums, void* workspace,
                   size_t workspace_bytes, void* stream);
/* The same loss when `pred` is the image mgr_raster_forward / mgr_views_forward has just rendered with background bg3
 * and tile_start points at that forward's tile-list offsets (workspace + mgr_raster_layout()[7]; V * T + 1 words,
 * T = ceil(W/16) * ceil(H/16)).  Where every tile under a span of the loss holds no Gaussian the rendered pixels ARE
 * the background colour, so the span only has to be compared with the target's background: the rendered image is not
 * read there, and no zero gradient is written.  sums are those of mgr_image_loss.  dL_dpred is written wherever a tile
 * holds a Gaussian (everywhere the backward pass reads it) and wherever the target differs from the background; it is
 * left untouched under empty tiles whose target is background. */
int mgr_image_loss_tiles(int V, int H, int W, const float* pred, const float* target, const float* bg3,
                         const uint32_t* tile_start, float w_l1, float w_ssim, float grad_scale, float loss_offset,
                         float* dL_dpred, float* sums, void* workspace, size_t workspace_bytes, void* stream);
/* mgr_image_loss_tiles in two calls.  _list builds the span list: it needs the forward's tile offsets but not its
 * image, so it can run on another stream while the forward blend runs (mgr_views_forward / mgr_raster_forward with
 * MGR_FWD_NO_BLEND, then MGR_FWD_BLEND_ONLY).  _finish does the rest on that list (same
 * workspace; the caller orders it after both the list and the blend). */
int mgr_image_loss_tiles_list(int V, int H, int W, const float* target, const float* bg3, const uint32_t* tile_start,
                              void* workspace, size_t workspace_bytes, void* stream);
/* The span list without reading the targets.  mgr_image_loss_target_map computes, once per set of target images and
 * background colour, the column masks the list is derived from (mgr_image_loss_target_map_words(V,H,W) uint32);
 * mgr_image_loss_tiles_list_mapped then builds the list of mgr_image_loss_tiles_list from those masks and the forward's tile
 * offsets.  Same list, same sums and gradients; a target image is a constant of its view (the reference reads it from the
 * dataset every step, src/modules/base.py:323-365). */
size_t mgr_image_loss_target_map_words(int V, int H, int W);
int mgr_image_loss_target_map(int V, int H, int W, const float* target, const float* bg3, uint32_t* map, void* stream);
int mgr_image_loss_tiles_list_mapped(int V, int H, int W, const uint32_t* map, const float* bg3, const uint32_t* tile_start,
                                     void* workspace, size_t workspace_bytes, int workspace_kept, void* stream);
/* workspace_kept != 0: the workspace was zero-filled when allocated and has only been used by list / finish pairs since (the
 * finish pass leaves its list counter zero): the 4-byte memset per call is skipped. */
/* The same list built by the forward itself: attached to `raster_workspace`, the next forward (mgr_views_forward /
 * mgr_raster_forward) that runs its blend on that workspace builds the list in extra workgroups of its last kernel, from
 * its own tile offsets (one shot, like mgr_raster_set_status_mirror; map == NULL withdraws a pending attachment).
 * `loss_workspace` must be a kept one (zero-filled once, only ever used by list / finish pairs: nothing is cleared here);
 * mgr_image_loss_tiles_finish follows as after mgr_image_loss_tiles_list_mapped.  V, H, W must be the forward's.  (Round 6:
 * as a launch of its own the list was 8 us in the chain of small kernels between the forward blend and the loss.) */
int mgr_views_forward_attach_loss_list(const void* raster_workspace, int V, int H, int W, const uint32_t* map,
                                       void* loss_workspace, size_t loss_workspace_bytes);
int mgr_image_loss_tiles_finish(int V, int H, int W, const float* pred, const float* target, float w_l1, float w_ssim,
                                float grad_scale, float loss_offset, float* dL_dpred, float* sums, void* workspace,
                                size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Spatial image loss: L1 + the STANDARD 2-D SSIM, forward + backward in one pass (csrc/ssim2d.hip).  Opt-in; mgr_image_loss
 * above stays the reference's statistic.  Here the 11x11 Gaussian window (sigma 1.5; G = g g^T with the fp32 g of
 * mgr_image_loss) slides over H x W of every colour channel separately, zero padding 5 -- what the reference's ssim() computes
 * when it is handed CHW images, as upstream 3DGS does.  pred, target (V,3,H,W) fp32; mask (V,H,W) fp32, possibly fractional, or
 * NULL: x = pred * mask, y = target * mask at load, the same map for the three channels.  Per channel
 *   E_s = G * s for s in {x, y, xx, yy, xy} (zero outside the image),
 *   S = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s11 + s22 + C2)),  C1 = 1e-4, C2 = 9e-4.
 *   sums[0] = sum|x - y|, sums[1] = sum S (both over V*3*H*W values), sums[2] = grad_scale * (w_l1 * sums[0] - w_ssim * sums[1])
 *             + loss_offset: the meaning they have in mgr_image_loss;
 *   view_sums (V,2) or NULL: the two sums of every view;
 *   dL_dpred (V,3,H,W) = grad_scale * mask * (w_l1 * sign(x - y) - w_ssim * d(sum S)/dx); NULL = forward only (the same sums,
 *             bit for bit).
 * Blocks: the image is cut into blocks of mgr_image_loss2d_block() = (block_w << 16) | block_h pixels.  A block is SETTLED when
 * x - y == 0 in fp32 (tested on the difference: NaN and Inf never count as equal) over the block dilated by 10 px and clipped to
 * the image -- exact: a pixel's gradient reaches 5 px to the derivative maps and those 5 px to the statistics.  A settled block
 * contributes exactly its value count to sum S and 0 to sum L1, gets zeros as its gradient, and does not run the heavy kernel.
 * flags & MGR_IL2D_DENSE: every block runs it.
 * The sums are accumulated as 64-bit fixed point (2^-32) per view: independent of the order the blocks ran in (two calls give
 * equal bits) and of the other views of the call.  A view whose inputs hold a NaN, or whose block sums leave the fixed-point
 * range (|sum over a block| beyond 2^31 / blocks of a view), reports NaN for its two sums, and so does `sums`; the other views'
 * view_sums keep their bits.
 * Refusals (MGR_EINVAL / MGR_ENOMEM, nothing touched): sizes <= 0, NULL pred / target / sums / workspace, H or V > 65535,
 * 3 H W >= 2^31, an unknown flag, workspace_bytes below mgr_image_loss2d_workspace_bytes(V,H,W) (sum slots, one bit per pixel,
 * the list of blocks; 0 for sizes <= 0).
 * ------------------------------------------------------------------------ */
#define MGR_IL2D_DENSE 1
size_t mgr_image_loss2d_workspace_bytes(int V, int H, int W);
int mgr_image_loss2d_block(void);
int mgr_image_loss2d(int V, int H, int W, const float* pred, const float* target, const float* mask, float w_l1, float w_ssim,
                     float grad_scale, float loss_offset, float* dL_dpred, float* sums, float* view_sums, int flags,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Silhouette and depth terms on the maps of mgr_raster_blend_features, value and gradient in one pass.  No reference
 * counterpart.
 *   L_mask  = mean over V H W of |alpha - mask|               mask (V,H,W) fp32 in [0,1]
 *   L_depth = mean over V H W of mask |depth - depth_target|  (depth: the expected, un-normalised depth; term off when depth,
 *                                                              depth_target and dL_ddepth are NULL -- all three or none)
 *   dL_dalpha = fp32(grad_scale w_mask / (V H W)) sign(alpha - mask), every element written (sign(0) = 0)
 *   dL_ddepth = (fp32(grad_scale w_depth / (V H W)) mask) sign(depth - depth_target), every element written
 *   sums[0] = L_mask, sums[1] = L_depth (0 with the term off), sums[2] = w_mask L_mask + w_depth L_depth (without grad_scale)
 * The sums are fp64 over a fixed two-stage tree (4096 elements per workgroup in a fixed assignment, then one workgroup over
 * the partials): no atomics, bit-reproducible; a term that is not finite makes its sum and sums[2] NaN.
 * workspace_bytes >= mgr_map_loss_workspace_bytes (16 bytes per 4096 elements); contents need not be initialised. */
size_t mgr_map_loss_workspace_bytes(int V, int H, int W);
int mgr_map_loss(int V, int H, int W, const float* alpha, const float* mask, const float* depth, const float* depth_target,
                 float w_mask, float w_depth, float grad_scale, float* dL_dalpha, float* dL_ddepth, float* sums,
                 void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Per-camera exposure: a learnt affine colour transform between the render and the image terms of the loss (csrc/exposure.hip).
 * No reference counterpart; the definition is the per-image 3x4 transform of upstream 3DGS' exposure option.
 *
 *   E (C,3,4) fp32, one row per camera, A = E[:,:,:3], b = E[:,:,3].  cam_of_view (V) int32 gives the row r of the view at
 *   position k; r outside [0,C) means "no correction".  img / out / g_in / g_out are planar (V,3,H,W) fp32.
 *     out[k,c,p]   = ((A[r,c,0] img[k,0,p] + A[r,c,1] img[k,1,p]) + A[r,c,2] img[k,2,p]) + b[r,c]       every pixel, background too
 *     g_out[k,j,p] = (A[r,0,j] g_in[k,0,p] + A[r,1,j] g_in[k,1,p]) + A[r,2,j] g_in[k,2,p]
 *     dE[k,c,j]    = sum_p g_in[k,c,p] img[k,j,p]  (j < 3),     dE[k,c,3] = sum_p g_in[k,c,p]            dE (V,3,4) by position
 *   in fp32, in that order, uncontracted.  A view without correction: out[k] = img[k] and g_out[k] = g_in[k] bit for bit,
 *   dE[k] = 0.  With the identity row out = img and g_out = g_in for finite inputs.
 *
 * mgr_exposure_apply: out may not alias img.  One grid row per view, mgr_exposure_block() pixels per workgroup; 16-byte
 *   accesses when H W is a multiple of 4 and both buffers are 16-byte aligned, single floats otherwise; nothing beyond H W is
 *   read or written.
 * mgr_exposure_backward: one pass reads img and g_in and writes g_out; g_out == g_in (in place) is allowed and gives the bits of
 *   the out-of-place call; g_out may not alias img.  The same pass forms the sums: products in fp32, added in fp64 -- per
 *   thread in ascending pixel order, across the wave and the workgroup in a fixed tree, one record of 12 doubles per workgroup
 *   in the workspace, folded per view by one workgroup in a fixed order.  No atomics: equal bits run to run.  A term that is
 *   not finite makes all of dE[k] NaN; the other views keep the bits of a run without it.  workspace_bytes >=
 *   mgr_exposure_workspace_bytes(V, H, W) (96 bytes per mgr_exposure_block() pixels of a view); contents need not be initialised.
 * mgr_exposure_block: the pixels of one workgroup of the two image kernels (a constant of the build).
 * mgr_exposure_adam: mgr_pose_adam's row Adam (the same device function; torch.optim.SparseAdam, bias correction of the
 *   global `step` >= 1, no clamp) on the rows cams_listed[u] (U entries, distinct: the caller's to ensure) of E and its moments
 *   m, v (C,3,4).  The gradient of row cams_listed[u] is the sum of dE[k] over the positions k < V with cam_of_view[k] ==
 *   cams_listed[u], in ascending k by one thread per (u, element) -- several views of a step may share a camera; a listed
 *   camera without a view steps on a zero gradient.  Rows that are not listed, and entries outside [0,C), keep their bits,
 *   moments included.
 * Refused before any launch, nothing written, mgr_last_error() naming the cause: a NULL pointer; V, H, W, C or U below 1; more
 *   than 65535 views or H W beyond 2^31; aliasing as above; a short workspace (MGR_ENOMEM); step < 1 or a non-finite rate. */
int mgr_exposure_block(void);
size_t mgr_exposure_workspace_bytes(int V, int H, int W);
int mgr_exposure_apply(int V, int H, int W, int C, const int32_t* cam_of_view, const float* E, const float* img, float* out,
                       void* stream);
int mgr_exposure_backward(int V, int H, int W, int C, const int32_t* cam_of_view, const float* E, const float* img,
                          const float* g_in, float* g_out, float* dE, void* workspace, size_t workspace_bytes, void* stream);
int mgr_exposure_adam(int C, int U, const int32_t* cams_listed, int V, const int32_t* cam_of_view, const float* dE, float* E,
                      float* m, float* v, double lr, double beta1, double beta2, double eps, int step, void* stream);

/* ------------------------------------------------------------------------
 * LPIPS: the reference's fourth loss term, lpips.LPIPS(net="vgg") from start_lpips_iter on (base.py:333-341), and the
 * LPIPS-AlexNet column of its validation CSV (loss_utils.py:111-117).  csrc/lpips.hip; convolutions on the fp32 matrix pipe, or
 * (the *_op entries with operands = MGR_LPIPS_BF16) on the bf16 matrix pipe.
 *
 *   x' = x mask (optional)   x'' = 2 x' - 1 (normalize != 0; the reference never passes it)   in = (x'' - shift) / scale
 *   f_k: the five taps of the frozen backbone (net 0: VGG16 relu1_2, 2_2, 3_3, 4_3, 5_3; net 1: AlexNet's five ReLUs)
 *   fh = f / (sqrt(sum_c f^2) + 1e-10)   s_k = mean_hw sum_c lin_k[c] (fh0 - fh1)^2   values[v] = sum_k s_k
 * One deviation from autograd: a pixel whose tap features are all zero contributes a zero gradient (autograd: 0 * inf = NaN),
 * the skip rule of a zero skin-weight sum above.
 *
 * Weights are user-supplied and frozen (no weight gradient): mgr_lpips_net_pack lays them out once into a caller-owned blob of
 * mgr_lpips_net_bytes(net) bytes.  conv_w / conv_b / lin_w are HOST arrays of DEVICE pointers in layer order (13 or 5
 * convolutions in torch's [Cout][Cin][KH][KW] layout, their biases, the 5 lin vectors of C_k floats).
 *
 * mgr_lpips: value and gradient in one pass, like mgr_map_loss.  pred / target (V,3,H,W), mask (V,H,W) or NULL (multiplies BOTH
 * images), values (V).  dL_dpred (V,3,H,W) or NULL: the gradient of grad_scale * sum_v values[v] w.r.t. pred, written
 * (accumulate = 0) or added to what is there (accumulate = 1); net 0 only.  Views run one after another on a workspace sized
 * for one view (mgr_lpips_workspace_bytes; contents need not be initialised).  Spatial means are fp64 over a fixed tree, there
 * are no float atomics: results are bit-reproducible, and V views equal V calls of one view bit for bit.
 *
 * mgr_lpips_layout: byte offsets into the workspace of, in order, pred's convolution outputs (post-ReLU; 13 / 5), the target's
 * five taps, the two scratch buffers, the fp64 partials, and the total: n_conv + 9 entries; returns that count.  All are (C,h,w)
 * fp32 of the LAST view of a call.
 *
 * Refused on the host, before any launch (-1 and mgr_last_error): net not 0 / 1, sizes at which the deepest tap has no pixel
 * (or above 2^24 pixels), null pointers, blob_bytes != mgr_lpips_net_bytes, workspace too small (-2), net 1 with dL_dpred. */
size_t mgr_lpips_net_bytes(int net);
int mgr_lpips_net_pack(int net, const float* const* conv_w, const float* const* conv_b, const float* const* lin_w, void* blob,
                       size_t blob_bytes, void* stream);
size_t mgr_lpips_workspace_bytes(int net, int H, int W, int need_grad);
int mgr_lpips_layout(int net, int H, int W, int need_grad, size_t* offsets, int n);
int mgr_lpips(int net, int V, int H, int W, const float* pred, const float* target, const float* mask, const void* blob,
              size_t blob_bytes, int normalize, float grad_scale, float* values, float* dL_dpred, int accumulate,
              void* workspace, size_t workspace_bytes, void* stream);
/* One convolution of the LPIPS backbones on its own (tests, tools/measure_lpips.py; loss_utils.py:111-117 runs them inside the
 * package): y = [relu](conv(x [gate > 0], w) + bias), w in torch's layout, packed into `scratch` (mgr_lpips_conv_scratch_bytes)
 * on every call.  transposed != 0 runs the layer's data gradient instead: x and gate have Cout channels, y gets Cin (stride 1,
 * 2 pad = K - 1, no bias).  Square kernels only. */
size_t mgr_lpips_conv_scratch_bytes(int Cin, int Cout, int KH, int KW);
int mgr_lpips_conv(int Cin, int Cout, int H, int W, int KH, int KW, int stride, int pad, const float* x, const float* gate,
                   const float* w, const float* bias, int relu, int transposed, float* y, void* scratch, size_t scratch_bytes,
                   void* stream);
/* The operand mode: the entries above with a trailing `operands`.  MGR_LPIPS_F32 is the entries above, bit for bit (they are
 * calls of these).  MGR_LPIPS_BF16: in every convolution of the call, forward and data gradient, the two matrix operands --
 * the input value AFTER the ReLU gate and the zero padding, and the weight -- are rounded to bf16 (round to nearest even) and
 * their products are summed in fp32 on v_mfma_f32_32x32x16_bf16.  Everything else is as above: fp32 bias, ReLU, fp32 stored
 * activations (the gates of the data gradient come from them), the workspace and mgr_lpips_layout (neither depends on the
 * mode), scaling layer, pools, heads, fp64 spatial means, accumulate, grad_scale.  The summation order inside a bf16 MFMA is
 * the hardware's, so this mode promises no k-ordered chain; it keeps the rest: no atomics, results depend on the sizes alone,
 * two runs give equal bits, V views equal V calls of one view.  The packed blob differs in size and layout between the modes:
 * a blob packed for one is refused by the other (blob_bytes).  Also refused on the host: operands other than 0 / 1 (the *_bytes
 * entries return 0), and everything the entries above refuse. */
enum { MGR_LPIPS_F32 = 0, MGR_LPIPS_BF16 = 1 };
size_t mgr_lpips_net_bytes_op(int net, int operands);
int mgr_lpips_net_pack_op(int net, const float* const* conv_w, const float* const* conv_b, const float* const* lin_w, void* blob,
                          size_t blob_bytes, void* stream, int operands);
int mgr_lpips_op(int net, int V, int H, int W, const float* pred, const float* target, const float* mask, const void* blob,
                 size_t blob_bytes, int normalize, float grad_scale, float* values, float* dL_dpred, int accumulate,
                 void* workspace, size_t workspace_bytes, void* stream, int operands);
size_t mgr_lpips_conv_scratch_bytes_op(int Cin, int Cout, int KH, int KW, int operands);
int mgr_lpips_conv_op(int Cin, int Cout, int H, int W, int KH, int KW, int stride, int pad, const float* x, const float* gate,
                      const float* w, const float* bias, int relu, int transposed, float* y, void* scratch, size_t scratch_bytes,
                      void* stream, int operands);

/* LPIPS on a per-view window (the mgr_lpips_roi* entries).  The windowed distance of view v with the rectangle rects[v] =
 * (x0, y0, w, h) in frame pixels is the LPIPS OF THE TWO CROPS: mgr_lpips_op on contiguous (3,h,w) copies of that rectangle of
 * pred and target (and of mask), with the crop's own zero padding at its edges and its own spatial means, bit for bit.  It is
 * NOT the full-frame value restricted to a region (no halo).  The scaling kernels read and write the rectangle of the pitched
 * frame directly; the convolutions run on (h, w).  Gradient: inside the rectangle the crop's gradient, written or (accumulate
 * = 1) added with one fp32 add; outside it 0 (accumulate = 0, the same launch writes the whole frame) or untouched (accumulate
 * = 1).  A rectangle with w == 0 or h == 0 is an empty view: value 0, no gradient, a zero-filled frame with accumulate = 0.
 *
 * rects: HOST (V,4) ints.  grad_scales: HOST array of V floats, one per view (may be NULL without dL_dpred).  pred / target
 * (V,3,H,W), mask (V,H,W) or NULL: the frames.  target_taps: NULL, or a HOST array of V DEVICE pointers, each NULL ("compute
 * this view's target") or mgr_lpips_taps_bytes(net, h, w) bytes that mgr_lpips_roi_taps_op filled for that view's rectangle,
 * target, mask, normalize and operand mode: the view's target forward is skipped and the result is bit for bit the call
 * without (the taps are the same kernels' output).  With taps for every non-empty view, target may be NULL.  The workspace is
 * the largest view's: mgr_lpips_roi_workspace_bytes = the maximum of mgr_lpips_workspace_bytes over the non-empty rectangles
 * (0 where one is refused).  mgr_lpips_roi_taps_op: the target forward of ONE view's window (target_v (3,H,W), mask_v (H,W) or
 * NULL) into taps_out: the five taps (C_k,h_k,w_k) fp32, each at a multiple of 256 bytes, in tap order; its workspace is
 * mgr_lpips_workspace_bytes(net, h, w, 0).
 *
 * Refused on the host before any launch (outputs untouched): a rectangle not inside the frame, negative sizes, a non-empty
 * rectangle at which the deepest tap has no pixel (what mgr_lpips refuses for an image of that size), null pointers (a
 * non-empty view with neither target nor taps included), net 1 with dL_dpred, wrong blob_bytes, a workspace too small (-2),
 * H above 65535. */
size_t mgr_lpips_roi_workspace_bytes(int net, int V, const int* rects, int need_grad);
size_t mgr_lpips_taps_bytes(int net, int h, int w);
int mgr_lpips_roi_taps_op(int net, int H, int W, const int* rect, const float* target_v, const float* mask_v, const void* blob,
                          size_t blob_bytes, int normalize, float* taps_out, void* workspace, size_t workspace_bytes, void* stream,
                          int operands);
int mgr_lpips_roi_op(int net, int V, int H, int W, const int* rects, const float* pred, const float* target, const float* mask,
                     const void* blob, size_t blob_bytes, int normalize, const float* grad_scales, float* values, float* dL_dpred,
                     int accumulate, const float* const* target_taps, void* workspace, size_t workspace_bytes, void* stream,
                     int operands);
int mgr_lpips_roi(int net, int V, int H, int W, const int* rects, const float* pred, const float* target, const float* mask,
                  const void* blob, size_t blob_bytes, int normalize, const float* grad_scales, float* values, float* dL_dpred,
                  int accumulate, const float* const* target_taps, void* workspace, size_t workspace_bytes, void* stream);

/* A step's equal-size windows in one batched call (the mgr_lpips_roi*_batch* entries).  mgr_lpips_roi_batch_op batches
 * mgr_lpips_roi_op: the same arguments and a trailing max_batch, the same refusals, and bit for bit the same values and
 * gradient frames -- in every kernel an output depends on the sizes alone, so the batch coordinate changes no sum.  On the host,
 * before the first launch, the non-empty views are grouped by (w, h) in ascending view order and every group is cut into chunks
 * of at most min(max_batch, LP_MAX_BATCH) views; the chunks run in the order of their first view, and a chunk of G views is ONE
 * chain of launches: the convolutions carry (batch, output-channel block) in blockIdx.z, the scaling kernels a per-launch
 * table of (view, x0, y0), the head one grid row and the fold one workgroup per view.  Empty views are handled as in
 * mgr_lpips_roi_op.  A chunk's target tower runs, batched among themselves, for those of its views that have no cached taps.
 *
 * Workspace of a chunk of G views: the one-view layout (mgr_lpips_layout) with every region G times as long, batch-major --
 * view b of a buffer of e elements sits at b e.  mgr_lpips_roi_batch_workspace_bytes is the largest chunk's; with max_batch = 1
 * it is mgr_lpips_roi_workspace_bytes and the call is the sequential one.
 *
 * mgr_lpips_roi_taps_batch_op batches mgr_lpips_roi_taps_op over the V views of a call: target (V,3,H,W), mask (V,H,W) or NULL,
 * rects HOST (V,4), taps_out a HOST array of V DEVICE pointers (mgr_lpips_taps_bytes(net, h, w) bytes each; ignored, and
 * normally NULL, for an empty view).  Every view's buffer ends up exactly as mgr_lpips_roi_taps_op leaves it.  Its workspace is
 * mgr_lpips_roi_batch_workspace_bytes(net, V, rects, 0, max_batch).
 *
 * Refused in addition to what the sequential entries refuse, on the host before any launch (no buffer touched): max_batch < 1
 * (-1; the size query returns 0), a workspace below the batched size (-2), a non-empty view of the taps build without a buffer. */
#define LP_MAX_BATCH 16 /* the most views of one launch: keeps the per-launch tables well inside the kernel-argument space */
size_t mgr_lpips_roi_batch_workspace_bytes(int net, int V, const int* rects, int need_grad, int max_batch);
int mgr_lpips_roi_taps_batch_op(int net, int V, int H, int W, const int* rects, const float* target, const float* mask, const void* blob,
                                size_t blob_bytes, int normalize, float* const* taps_out, int max_batch, void* workspace,
                                size_t workspace_bytes, void* stream, int operands);
int mgr_lpips_roi_batch_op(int net, int V, int H, int W, const int* rects, const float* pred, const float* target, const float* mask,
                           const void* blob, size_t blob_bytes, int normalize, const float* grad_scales, float* values, float* dL_dpred,
                           int accumulate, const float* const* target_taps, void* workspace, size_t workspace_bytes, void* stream,
                           int operands, int max_batch);
int mgr_lpips_roi_batch(int net, int V, int H, int W, const int* rects, const float* pred, const float* target, const float* mask,
                        const void* blob, size_t blob_bytes, int normalize, const float* grad_scales, float* values, float* dL_dpred,
                        int accumulate, const float* const* target_taps, void* workspace, size_t workspace_bytes, void* stream,
                        int max_batch);

/* The storage mode (the *_st entries): each is its base entry with trailing storage arguments.  MGR_LPIPS_STORE_F32 is the
 * base entry, bit for bit (the base entries are calls of these).  MGR_LPIPS_STORE_BF16, valid with MGR_LPIPS_BF16 operands only:
 *
 *   layout     every tensor of the chain -- pred's 13 (AlexNet 5) convolution outputs, the target's taps and non-tap outputs,
 *              every pool output, every gradient buffer -- is bf16 as [ceil(C/8)][h][w][8]: 16 bytes per (pixel, block of 8
 *              channels), channel c at block c / 8, lane c % 8; pad lanes are written as zero.  Batch-major as before: view b
 *              of a buffer sits at b times the bytes of one view.  The image-side pair stays (3,h,w) fp32 planar: the scaled
 *              image and dL/d(scaled image), so windows and the frame-side bits are those of fp32 storage's scaling kernels.
 *   conv       the operand mode's chunking, MFMA sequence, fp32 accumulation, fp32 bias and ReLU, then ONE round to nearest
 *              even at the store.  A stored value is the next MFMA's operand as it is (no second rounding); the gate of a
 *              data gradient is `stored value > 0`.
 *   pool       the maximum of the stored values (exact); the winner is the FIRST maximum in row-major window order among the
 *              STORED values, forward and backward -- ties that the rounding creates go to the first position.
 *   head       reads the taps exactly (bf16 -> fp32), arithmetic as in fp32 storage (fp32, fp64 partials); its gradient is
 *              rounded once at the store, with a deeper gradient present fp32(stored g) + t is rounded once.  The fold is
 *              unchanged.
 *   as before  no atomics (two runs give equal bits); V views equal V calls of one view; a batched call equals the
 *              sequential one; a window equals the call on contiguous crops; d(x, x) and its gradient are exactly 0; a pixel
 *              with all-zero tap features contributes no gradient.
 *
 * Sizes: mgr_lpips_workspace_bytes_st / mgr_lpips_layout_st / mgr_lpips_taps_bytes_st /
 * mgr_lpips_roi_batch_workspace_bytes_st -- an act or tap region is mgr_align(2 G pad8(C) h w) bytes, the partials are
 * unchanged.  The weight blob is the bf16 operand mode's, unchanged.  mgr_lpips_roi_batch_st with max_batch = 1 is the sequential
 * windowed call; mgr_lpips_roi_taps_batch_st with max_batch = 1 builds the taps view by view.  mgr_lpips_conv_st (tests,
 * tools/measure_lpips.py): x_storage is the storage of x and gate, y_storage that of y; any Cin and Cout, blocked tensors
 * padded to 8 channels.
 *
 * Refused on the host before any launch (no buffer touched): a storage other than 0 / 1 (-1; the size queries return 0),
 * MGR_LPIPS_STORE_BF16 with MGR_LPIPS_F32 operands (-1), and everything the base entries refuse.  A taps buffer built under the
 * other storage cannot be told apart here: the Python layer (TargetTaps.matches) refuses it. */
enum { MGR_LPIPS_STORE_F32 = 0, MGR_LPIPS_STORE_BF16 = 1 };
size_t mgr_lpips_workspace_bytes_st(int net, int H, int W, int need_grad, int storage);
int mgr_lpips_layout_st(int net, int H, int W, int need_grad, size_t* offsets, int n, int storage);
size_t mgr_lpips_taps_bytes_st(int net, int h, int w, int storage);
size_t mgr_lpips_roi_batch_workspace_bytes_st(int net, int V, const int* rects, int need_grad, int max_batch, int storage);
int mgr_lpips_st(int net, int V, int H, int W, const float* pred, const float* target, const float* mask, const void* blob,
                 size_t blob_bytes, int normalize, float grad_scale, float* values, float* dL_dpred, int accumulate, void* workspace,
                 size_t workspace_bytes, void* stream, int operands, int storage);
int mgr_lpips_roi_batch_st(int net, int V, int H, int W, const int* rects, const float* pred, const float* target, const float* mask,
                           const void* blob, size_t blob_bytes, int normalize, const float* grad_scales, float* values, float* dL_dpred,
                           int accumulate, const float* const* target_taps, void* workspace, size_t workspace_bytes, void* stream,
                           int operands, int max_batch, int storage);
int mgr_lpips_roi_taps_batch_st(int net, int V, int H, int W, const int* rects, const float* target, const float* mask, const void* blob,
                                size_t blob_bytes, int normalize, float* const* taps_out, int max_batch, void* workspace,
                                size_t workspace_bytes, void* stream, int operands, int storage);
int mgr_lpips_conv_st(int Cin, int Cout, int H, int W, int KH, int KW, int stride, int pad, const float* x, const float* gate,
                      const float* w, const float* bias, int relu, int transposed, float* y, void* scratch, size_t scratch_bytes,
                      void* stream, int operands, int x_storage, int y_storage);

/* ------------------------------------------------------------------------
 * Device frame store: the stored uint8 RGBA crops of a capture decoded into the float targets and masks of a step
 * (manus_amd/frames.py; SequenceDataset.fetch_images, brics_dynamic.py:343-373, restated bit for bit).
 *
 * A target image is a constant of its view only on a still frame; a sequence draws new (action, frame, camera) items every
 * step.  The crops of all items live in one device pool (`pool`, rows packed, each crop at a multiple of 16 bytes) and one
 * call rewrites the rows `slot` of the caller's tables from them:
 *   source pixel  the crop's value inside its bbox, (0,0,0,0) outside; the source frame is (H k) x (W k)
 *   block mean    per channel the integer sum s of the k x k block, m = (2 s + k k) / (2 k k) in integers (numpy's
 *                 floor(mean + 0.5), cv2's INTER_AREA for the factor 1/k on uint8)
 *   composite     c' = m_c / 255.0, a' = m_a / 255.0 in fp64 (a table of constants: no division on the device),
 *                 target = fp32(c' a' + bg (1.0 - a')), products and sum rounded one by one (no fma), mask = fp32(a')
 * Only the rectangle (rx0, ry0, rx1, ry1) of OUTPUT pixels of a view is written: the whole image, or the union of the boxes of
 * the old and the new crop when the caller knows what the slot held before (same background).  `views_host` is HOST memory:
 * the records travel as kernel arguments, MGR_FRAMES_MAX_VIEWS per launch (a larger V is a loop over chunks).  No copy, no
 * allocation on the device, no synchronisation.  masks may be NULL.  An empty crop (x1 == x0 or y1 == y0) gives background
 * and a zero mask.
 * MGR_EINVAL, before anything is launched: k < 1; a bbox outside [0, W k] x [0, H k] or reversed; an offset that is no multiple
 * of 16; offset + crop bytes > pool_bytes; a rectangle outside the image; a slot outside [0, n_slots); two views of the call
 * with one slot; a NULL pool with a non-empty crop. */
#define MGR_FRAMES_MAX_VIEWS 16
typedef struct {
    int64_t offset;             /* byte offset of the crop in the pool, a multiple of 16 */
    int32_t x0, y0, x1, y1;     /* bbox in SOURCE pixels; the crop is (y1 - y0, x1 - x0, 4) uint8 RGBA, rows packed */
    int32_t rx0, ry0, rx1, ry1; /* rectangle of OUTPUT pixels to write */
    float bg[3];                /* background colour */
    int32_t slot;               /* row of targets / masks to write */
} MgrFrameView;
int mgr_frames_decode(int V, int H, int W, int k, const uint8_t* pool, int64_t pool_bytes, const MgrFrameView* views_host,
                      float* targets /* (n_slots,3,H,W) */, float* masks /* (n_slots,H,W) or NULL */, int64_t n_slots, void* stream);

/* ------------------------------------------------------------------------
 * Optimizer step and densification of the Gaussian parameter model
 * (src/models/gaussian.py:128-338).
 *
 * mgr_adam_step: one torch.optim.Adam update (betas, eps as given; no weight
 * decay, no amsgrad; the reference uses Adam(l, lr=0, eps=1e-15),
 * gaussian.py:142) of `n_groups` <= 8 parameter groups in one launch.
 * counts / lrs are host arrays; params, grads, exp_avg, exp_avg_sq are host
 * arrays of device pointers (fp32, counts[k] elements each).  `step` is the
 * 1-based step number of this update (bias correction).
 *
 * mgr_reset_opacity: reset_opacity, gaussian.py:148-165 (opacity <-
 * inverse_sigmoid(min(sigmoid(opacity), 0.01)), both moments zeroed).  The fp32 expression of
 * the reference, edge rows included: a NaN logit stays NaN (torch.min propagates it), -inf stays
 * -inf, +inf is clamped like any logit above log(0.01 / 0.99), and a logit below about -88.7
 * becomes -inf (exp(-x) overflows in fp32, so sigmoid is 0 there in torch's fp32 too).
 *
 * mgr_densify_plan + mgr_densify_apply: densify_and_prune, gaussian.py:310-333
 * (clone :288-308, split with N=2 :254-286, prune :183-200, optimizer-state
 * surgery :148-252).  plan classifies the N Gaussians from the densification
 * statistics (grad = accum / denom, NaN -> 0), scans, builds the source map in
 * `workspace` and returns (blocking) counts_host[5] = {kept originals, kept
 * clones, split-selected, kept split parents, M = new number of Gaussians}.
 * apply writes the M new rows of the six leaves in group order (xyz 3, f_dc 3,
 * f_rest 45, opacity 1, scaling 3, rotation 4), of both Adam moments (zero for
 * new rows) and of the skin weights (N,B) (may be NULL), in the reference's
 * order [kept originals | clones | split copies 0 | split copies 1].
 * noise: standard normals (2 * n_selected, 3), row c * n_selected + j for copy c
 * of the j-th split-selected Gaussian (torch.normal(mean=0, std) / std of :264-266).
 * max_screen_size: the reference's `if max_screen_size:` (:316); 0 = None.  When set, Gaussians
 * whose largest world-space scale exceeds 0.1 * extent are pruned (big_points_ws, :318); the
 * screen-size half (max_radii2D > max_screen_size, :317) can never fire -- densification_postfix
 * has just zeroed max_radii2D (:249-251) -- so max_radii2D is not an input.  When 0, only the
 * opacity test (and NaN scales, :328-329) prunes.
 *
 * mgr_adam_step_groups: the same update with one step count per group (steps[k] <= 0 skips
 * group k): torch.optim.Adam keeps state["step"] per parameter, and the reference replaces
 * leaves (reset_opacity / densify / prune run in on_after_backward, hand_dynamic.py:193-224)
 * before optimizer.step(), which then skips the gradient-less new nn.Parameter.
 *
 * mgr_prune_plan: prune_points(mask), gaussian.py:185-203 (the mask_to_prune branch of
 * density_update, gaussian_utils.py:454-459): prune_mask (N) bytes, non-zero = remove.  Builds the
 * same source map as mgr_densify_plan (counts_host[0] = counts_host[4] = survivors); the rows are
 * then written by mgr_densify_apply(N, M, 0, ..., noise = NULL).
 *
 * mgr_gather_rows: dst[o,:] = src[map[o],:] for the M rows of the plan in `workspace`, rows of
 * `width` 4-byte words: the per-Gaussian statistics (xyz_gradient_accum, denom, max_radii2D,
 * gaussian.py:199-203) and any other per-Gaussian side array.
 * ------------------------------------------------------------------------ */
int mgr_adam_step(int n_groups, const int64_t* counts, float* const* params, const float* const* grads,
                  float* const* exp_avg, float* const* exp_avg_sq, const double* lrs, int64_t step, double beta1,
                  double beta2, double eps, void* stream);
int mgr_adam_step_groups(int n_groups, const int64_t* counts, float* const* params, const float* const* grads,
                         float* const* exp_avg, float* const* exp_avg_sq, const double* lrs, const int64_t* steps,
                         double beta1, double beta2, double eps, void* stream);
int mgr_reset_opacity(int N, float* opacity_logit, float* exp_avg, float* exp_avg_sq, void* stream);
/* add_densification_stats, gaussian.py:335-338 (xyz_gradient_accum += the step's sum over views of ||dL/dmeans2D[:, :2]||,
 * denom += the number of views that saw the Gaussian) and the max_radii2D update of density_update,
 * gaussian_utils.py:470-473 (max_radii2D = max(max_radii2D, radii)), in one launch.  grad2d_sum / vis_count: (N,) fp32,
 * radii_max: (N,) int32 -- the statistics outputs of mgr_views_backward; the three accumulators (N,) fp32, in place. */
int mgr_add_densification_stats(int N, const float* grad2d_sum, const float* vis_count, const int32_t* radii_max,
                                float* xyz_gradient_accum, float* denom, float* max_radii2D, void* stream);
size_t mgr_densify_workspace_bytes(int N);
int mgr_densify_plan(int N, const float* grad_accum, const float* denom, const float* log_scale,
                     const float* opacity_logit, float max_grad, float min_opacity, float extent, float percent_dense,
                     float max_screen_size, void* workspace, size_t workspace_bytes, int64_t* counts_host,
                     void* stream);
int mgr_prune_plan(int N, const uint8_t* prune_mask, void* workspace, size_t workspace_bytes, int64_t* counts_host,
                   void* stream);
int mgr_gather_rows(int N, int64_t M, const void* workspace, const void* src, void* dst, int width, void* stream);
/* The prune tests of densify_and_prune (gaussian.py:315-320) on rows as they are, in mgr_densify_plan's own fp32 expressions:
 * out_mask[i] = sigmoid(opacity_logit[i]) < min_opacity, or max_j exp(log_scale[i,j]) > 0.1 * extent (only with
 * max_screen_size > 0), or a NaN log scale.  On the rows a plan with the tests disabled (min_opacity = -inf,
 * max_screen_size = 0) produced, this is the mask the plan with the tests enabled would have applied, row for row: the
 * pruning half of densify_and_prune taken after clone and split, where an outlier mask can be ORed in.
 * MGR_EINVAL: N < 0 or a NULL pointer with N > 0. */
int mgr_prune_tests(int N, const float* log_scale, const float* opacity_logit, float min_opacity, float extent,
                    float max_screen_size, uint8_t* out_mask, void* stream);
int mgr_densify_apply(int N, int64_t M, int64_t n_selected, const void* workspace, const float* const* params,
                      const float* const* exp_avg, const float* const* exp_avg_sq, float* const* new_params,
                      float* const* new_exp_avg, float* const* new_exp_avg_sq, const float* skin, float* new_skin, int B,
                      const float* noise, void* stream);

/* Isotropic regulariser of loss_func (src/modules/base.py:349-356):
 *   loss[0] = weight * mean_n (min_j s_nj / (max_j s_nj + 1e-8) - condition_number)^2, s = exp(log_scale (N,3));
 *   d_log_scale (N,3) = its gradient (added to the existing content when accumulate != 0).
 * workspace: mgr_isotropic_reg_workspace_bytes(N). */
size_t mgr_isotropic_reg_workspace_bytes(int N);
int mgr_isotropic_reg(int N, const float* log_scale, float condition_number, float weight, float* d_log_scale,
                      int accumulate, float* loss, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Contact distance: for each of the N1 points of pt1
 * (N1,3) the fp32 distance to its nearest point of pt2 (N2,3) and that point's
 * index.  Replaces get_contact_dist (taichi kernel, src/utils/gaussian_utils.py:
 * 521-549) and get_contact_map (chunked torch.cdist().min(), :514-518).  Same
 * loop semantics: dist = sqrt(dx^2+dy^2+dz^2), strict '<' on the rooted
 * distance (lowest index wins a tie), initial minimum 1e9 (N2 = 0 -> 1e9, index 0).
 * out_idx (int32) may be NULL.
 * ------------------------------------------------------------------------ */
size_t mgr_contact_workspace_bytes(int N1, int N2);
int mgr_contact_dist(int N1, const float* pt1, int N2, const float* pt2, float* out_dist, int32_t* out_idx,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Contact maps: near search, value formula and colour epilogue.  Together they replace get_cmap
 * (src/utils/gaussian_utils.py:571-577), get_colors_from_cmap (src/utils/vis_util.py:22-25: a device -> numpy ->
 * matplotlib -> device round trip per render) and the colour blends of Composite.render_contacts
 * (src/modules/composite.py:143-214).
 *
 * mgr_contact_near: for each of the N1 points of pt1 the nearest point of pt2 WITHIN RADIUS c_thresh (> 0), with the
 *   arithmetic and tie rule of mgr_contact_dist (fp32, (dx^2+dy^2)+dz^2 without contraction, correctly rounded root,
 *   strict '<' on the rooted distance, lowest index wins a tie).  pt2 is counting-sorted on the device into a hashed
 *   uniform grid of cell edge just above c_thresh whose table is sized from N2 (a far outlier costs nothing); a point
 *   of pt1 visits at most 27 cells.  Contract:
 *     out_value (N1)  = 1 - clamp(dist, 0, c_thresh) / c_thresh, fp32 in that order with an IEEE division, of the
 *                       brute-force distance, bit for bit, for every point (get_cmap lines 573-574);
 *     out_idx (N1)    = the brute-force index wherever out_value > 0, -1 elsewhere (the reference only reads indices
 *                       under the mask dist > 0, composite.py:190-196);
 *     out_dist (N1)   = (may be NULL) the brute-force distance where out_value > 0, 1e9 (the loop's initial minimum)
 *                       elsewhere.
 *   N1 = 0 and N2 = 0 (all values 0, indices -1) are valid; coincident and duplicated points follow the tie rule; a
 *   point with a NaN coordinate is nobody's neighbour and has value 0 (the strict '<' of the reference loop).
 *   workspace: mgr_contact_near_workspace_bytes(N1, N2).  No host read-back, everything on `stream`.
 * mgr_contact_values: out_value (N) = the same formula applied to distances some other search produced.
 * mgr_contact_colors: per point, out (N,3) =
 *     table == NULL:  c = lut[k] (lut (256,3) fp32), k = min(int(value * 256.0f), 255), 0 for value < 0, 255 for
 *                     value >= 1 (+inf included), c = (0,0,0) for NaN -- matplotlib's Colormap.__call__ on a float32
 *                     array; then c itself (base == NULL) or base[n] * alpha + one_minus_alpha * c (base (N,3)), two
 *                     rounded products and one rounded sum like rgb_colors * alpha + (1 - alpha) * cmap.  The caller
 *                     passes one_minus_alpha = (float)(1.0 - alpha_as_double), which is what the reference multiplies by.
 *     table != NULL:  value[n] > 0 ? table[idx_nn ? idx_nn[n] : n] : (0,0,0)   (table (M,3); the NOCS renders,
 *                     composite.py:165-183; an index outside [0, M) gives black).
 * ------------------------------------------------------------------------ */
size_t mgr_contact_near_workspace_bytes(int N1, int N2);
int mgr_contact_near(int N1, const float* pt1, int N2, const float* pt2, float c_thresh, float* out_value, int32_t* out_idx,
                     float* out_dist, void* workspace, size_t workspace_bytes, void* stream);
int mgr_contact_values(int N, const float* dist, float c_thresh, float* out_value, void* stream);
int mgr_contact_colors(int N, const float* value, const float* lut, const float* base, float alpha, float one_minus_alpha,
                       const float* table, int M, const int32_t* idx_nn, float* out, void* stream);

/* ------------------------------------------------------------------------
 * Validation pass (eval.hip): the metrics and the triptych of BaseTrainingModule.validation_step /
 * on_validation_epoch_end (src/modules/base.py:112-188) with psnr of src/utils/loss_utils.py:100-108, for V views kept in
 * the rasterizer's layout.  Forward only; everything on `stream`, no host read-back, no float atomics: two calls on the
 * same inputs give bit-equal outputs, and a view's outputs depend on that view's pixels only.
 *
 * mgr_eval_views: pred, target (V,3,H,W) fp32; mask (V,H,W) fp32, possibly fractional, NULL = ones.  Per view v:
 *     sq_sum[v]   = sum over all 3*H*W elements of (pred*mask - target*mask)^2, the two products and the difference each
 *                   rounded to fp32 (`render * mask`, `gt * mask`, `inputs - targets`); masked-out pixels count in the mean
 *                   like in the reference: psnr = -10 log10(sq_sum / (3*H*W)), +inf for equal masked images (sq_sum == 0);
 *     ssim_sum[v] = sum of the reference's SSIM map of the two masked images in the HWC form it computes (the 11x11 window
 *                   over the (W,3) plane of every row, zero padded -- the statistic of mgr_image_loss); ssim = / (3*H*W);
 *     gt_max[v]   = maximum of the unmasked target (NaN if it holds one, as ndarray.max), for dump_image's rule below;
 *     flags[v]    = (may be NULL) 1 when the view's pred / target / mask hold a NaN or Inf or a total is not finite: sq_sum
 *                   and ssim_sum of THAT view are then NaN; 0 otherwise.
 *   Per-workgroup partial sums are folded per view in fp64 by a second kernel.  workspace: mgr_eval_workspace_bytes(V,H,W).
 *   Limits as mgr_image_loss: H, V <= 65535, W <= 16384.
 * mgr_eval_triptych: out (V,3H,W,3) uint8 = three HWC panels stacked along the rows (concat_img_array, axis 0):
 *     rows [0,H)    uint8(clamp(pred,0,1) * 255.0f), truncating, of the UNMASKED render (base.py:116-117);
 *     rows [H,2H)   dump_image(gt): uint8(target * 255.0f) when gt_max[v] <= 1.0, else uint8(target) (extra.py:153-160);
 *     rows [2H,3H)  diff_table[gt_byte * 256 + render_byte]: the reference's uint8((gt/255.0 - img/255.0) * 255.0) in float64
 *                   (base.py:124-127) is a function of the two bytes; the caller builds the 256x256 table with that very
 *                   numpy expression (manus_amd.validation.diff_table) and passes it on the device.
 *   A NaN pixel gives byte 0 in its panel (this library's definition: numpy's cast of NaN is not defined); finite values
 *   outside the byte range wrap like numpy's cast on x86-64 (truncate toward zero, low eight bits).
 * ------------------------------------------------------------------------ */
size_t mgr_eval_workspace_bytes(int V, int H, int W);
int mgr_eval_views(int V, int H, int W, const float* pred, const float* target, const float* mask, float* sq_sum,
                   float* ssim_sum, float* gt_max, int32_t* flags, void* workspace, size_t workspace_bytes, void* stream);
int mgr_eval_triptych(int V, int H, int W, const float* pred, const float* target, const float* gt_max,
                      const uint8_t* diff_table, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------
 * Contact evaluation (contact_eval.hip): the IoU / F1 scripts scripts/process/get_iou_ours.py and get_iou.py, for V
 * evaluation cameras of one H x W per launch chain.  All images are uint8 and row-major; everything runs on `stream`
 * without a host read-back; there are no float atomics, two calls on the same inputs give the same bytes, and a view's
 * outputs depend on that view's images only.  H, W <= 16384, V <= 65535.  One workspace of
 * mgr_ceval_workspace_bytes(V,H,W) serves labels -> fill -> counts.
 *
 * mgr_ceval_masks (get_iou_ours.py:313-322): frame (V,H,2W,3) = the 'acc_gt_eval' render, left half the skin-weight
 *   colours, right half the grey contact map (the reference hard-codes the split at column 1080; here it is W), as
 *   uint8, or (frame_is_f32) as the fp32 render, converted like test_step does (src/modules/base.py:245-246:
 *   uint8(clamp(x,0,1) * 255) with the product in fp32, truncating; NaN -> 0) and ALSO written to frame_u8 (V,H,2W,3)
 *   (required then, unused otherwise).  gt_seg (V,H,W,3), gt_rgba (V,H,W,4).  One byte (0/1) per pixel:
 *     pred = every channel of the right half in [128,255]    (cv2.inRange(our_mask, (128,)*3, (255,)*3))
 *     gt   = the same test on gt_seg
 *     hand = alpha of gt_rgba > 128.
 * mgr_ceval_labels (get_skin_mask, :74-138): frame (V,H,row_px,3) whose first W pixels of a row are the skin-weight
 *   render in RGB (row_px = 2W: the whole frame; W: the half on its own).  labels (V,H,W): 0 when no palette mask holds
 *   the pixel, else 1 + the index of the FIRST of the 16 palette masks that does (np.argmax over [background, m1..m16]);
 *   mask i = "every channel within +-10 of colour i, inclusive" (cv2.inRange), eroded and then dilated with the 3x3
 *   MORPH_ELLIPSE element = the 4-neighbour cross, OpenCV's default borders (outside the image: set for the erosion,
 *   unset for the dilation).  hand (V,H,W) or NULL (= all ones): labels outside it are 0 (all_masks * gt_mask).  The
 *   kernel also leaves in the workspace what mgr_ceval_fill reads: per 16x16 tile the bitmap of its labelled pixels,
 *   the tile bounding box of the view's labelled pixels and the list of RESIDUAL pixels (hand != 0, label 0).
 * mgr_ceval_fill (:136-144 and get_contact_dist, :44-71): in place, every residual pixel takes the label of its nearest
 *   labelled pixel: Euclidean distance on integer (row, col), among equals the one that comes first in row-major order
 *   (the reference scans np.argwhere order with a strict '<' on fp32 roots; below 2^11 distinct integer squared
 *   distances have distinct fp32 roots) -- computed exactly as min over (d^2, row * W + col) by a ring search over the
 *   tile bitmaps, never as the N_res x N_skin scan.  `workspace` is the one mgr_ceval_labels just filled for the SAME
 *   labels.  flags (V) int32: 1 for a view with residual pixels and no labelled pixel at all (the reference raises an
 *   IndexError there; such a view's labels are left as they are), 0 otherwise.
 * mgr_ceval_counts (cal_iou and the f1_score inputs of evaluate_metric / calculate_per_bone_iou, :162-232): counts
 *   (V,17,3) int64 = [I, A, B] = [|gt & pred|, |gt|, |pred|] restricted to labels == i for rows i = 0..15 (0 is "no
 *   label"; label 16 is never scored -- the reference's range(16)) and unrestricted in row 16.  Per-workgroup records,
 *   folded per view by a second kernel.
 * mgr_ceval_collage (blend_masks / combine_images, :269-291): out (V,H,(1+M)W,3) = [photo on white | photo blended with
 *   mask 0 in (0,128,0) | ... mask M-1]; masks (M,V,H,W) bytes (non-zero = set), 0 <= M <= 16.  Every output byte is
 *   table[((photo_byte * 3 + kind) * 2 + alpha_bit) * 3 + channel], kind 0 = the plain panel, 1 / 2 = blended with a
 *   clear / set mask pixel; the caller builds the 256x3x2x3 table with the reference's float64 numpy expression
 *   (manus_amd.contact_eval.collage_table).
 * ------------------------------------------------------------------------ */
size_t mgr_ceval_workspace_bytes(int V, int H, int W);
int mgr_ceval_masks(int V, int H, int W, const void* frame, int frame_is_f32, const uint8_t* gt_seg, const uint8_t* gt_rgba,
                    uint8_t* frame_u8, uint8_t* pred, uint8_t* gt, uint8_t* hand, void* stream);
int mgr_ceval_labels(int V, int H, int W, const uint8_t* frame, int row_px, const uint8_t* hand, uint8_t* labels,
                     void* workspace, size_t workspace_bytes, void* stream);
int mgr_ceval_fill(int V, int H, int W, uint8_t* labels, int32_t* flags, void* workspace, size_t workspace_bytes, void* stream);
int mgr_ceval_counts(int V, int H, int W, const uint8_t* pred, const uint8_t* gt, const uint8_t* labels, int64_t* counts,
                     void* workspace, size_t workspace_bytes, void* stream);
int mgr_ceval_collage(int V, int H, int W, int M, const uint8_t* gt_rgba, const uint8_t* masks, const uint8_t* table,
                      uint8_t* out, void* stream);

/* ------------------------------------------------------------------------
 * Skin-weight initialisation from the MANO rest mesh (model-initialisation side of the
 * dataloader): the device half of init_mano_weights (src/utils/train_utils.py:48-89) as called by
 * Dataset.build_voxel_grid / Dataset.sample_gaussians_on_bones (src/datasets/brics_dynamic.py:69-144).
 *
 * mgr_knn_mean_rows: for each of the n points (n,3) its k nearest of the m reference points (m,3) by squared Euclidean
 *   distance (replaces torch.cdist(points, mano_verts).topk(k, largest=False), train_utils.py:70-72; ties keep the lower
 *   index), out (n,C) = mean of rows[idx] (m,C) added nearest first in fp32 (np.mean(init_weights[indices], axis=1),
 *   :73), out_idx (n,k) int32 the indices (nearest first; -1 beyond m).  Either output may be NULL.  1 <= k <= 32.
 *   A neighbour is a reference whose fp32 squared distance is below 3e38; the mean is over the neighbours there are, and a
 *   point without any (a non-finite coordinate, every squared distance overflowing, m = 0 -- refs and rows may then be
 *   NULL) gets indices -1 and a NaN mean.
 * mgr_mesh_sdf: signed distance (n,) of the points to the triangle mesh verts (nv,3) / faces (nf,3) int32, positive
 *   inside (replaces pysdf.SDF(verts, faces)(points), train_utils.py:55-58; pysdf is an external package that is not in
 *   this image: parity unpinned).  |distance| is the exact point-triangle minimum; the sign comes from the generalised
 *   winding number (|sum of solid angles| / 4 pi > 1/2), also written to out_winding (n,) when not NULL.  A mesh
 *   without faces (nf = 0) gives -sqrt(3e38) and winding 0 for every point.
 * ------------------------------------------------------------------------ */
int mgr_knn_mean_rows(int n, const float* points, int m, const float* refs, const float* rows, int C, int k, float* out,
                      int32_t* out_idx, void* stream);
int mgr_mesh_sdf(int n, const float* points, int nv, const float* verts, int nf, const int32_t* faces, float* out_sdf,
                 float* out_winding, void* stream);

/* ------------------------------------------------------------------------
 * Row-compacted gradient exchange of the view-sharded step (no reference counterpart: the reference trains
 * on one GPU, /root/reference/main.py:84-87).  The step buffer `flat` holds nseg segments of N rows (segment k: widths[k]
 * floats per row, first float at offs[k]), the visibility counts (N floats at vis_off) and (loss, overflow) at tail_off.
 * Between two SUM all-reduces issued by the host (torch.distributed / RCCL):
 *   mgr_exchange_mask    small[0:N] = 1 where the row may be non-zero -- from the rows themselves, or (active_list /
 *                        active_count: device pointers of mgr_views_active_list) from the fused backward's list of the
 *                        Gaussians that received a gradient --, small[N:2N] = the visibility counts as bytes
 *   mgr_exchange_index   idx = the rows with mask != 0 in ascending order, *count (device) their number
 *   mgr_exchange_pack    buf = [segment 0 rows (n x widths[0]) | segment 1 rows | ... | loss, overflow]
 *   mgr_exchange_unpack  the inverse into `flat` (rows outside idx untouched) and, when small_vis is given, the visibility
 *                        counts back as floats
 * ------------------------------------------------------------------------ */
int mgr_exchange_mask(int N, const float* flat, int nseg, const int64_t* offs, const int* widths, int64_t vis_off,
                      const uint32_t* active_list, const uint32_t* active_count, uint8_t* small, void* stream);
size_t mgr_exchange_index_workspace_bytes(int N);
int mgr_exchange_index(int N, const uint8_t* mask, uint32_t* idx, uint32_t* count, void* workspace, size_t workspace_bytes,
                       void* stream);
int mgr_exchange_pack(int N, int n, const uint32_t* idx, const float* flat, int nseg, const int64_t* offs, const int* widths,
                      int64_t tail_off, float* buf, void* stream);
int mgr_exchange_unpack(int N, int n, const uint32_t* idx, float* flat, int nseg, const int64_t* offs, const int* widths,
                        int64_t tail_off, const float* buf, const uint8_t* small_vis, int64_t vis_off, void* stream);
/* The same two with the row count read FROM THE DEVICE (`count`: the word mgr_exchange_index wrote) and a row capacity
 * `cap_rows` <= N chosen by the host beforehand -- the second collective (cap_rows x columns + 2 floats, segment k at
 * cap_rows x its first column) is sized without a host read in the middle of the step.  Rows [min(*count, cap_rows), cap_rows)
 * are packed as zeros and ignored by the unpack; *count > cap_rows adds 1 to the packed overflow word (buf's last float), which
 * the all-reduce sums and the unpack writes back: the caller runs the step again with a larger capacity. */
int mgr_exchange_pack_rows(int N, int cap_rows, const uint32_t* count, const uint32_t* idx, const float* flat, int nseg, const int64_t* offs,
                           const int* widths, int64_t tail_off, float* buf, void* stream);
int mgr_exchange_unpack_rows(int N, int cap_rows, const uint32_t* count, const uint32_t* idx, float* flat, int nseg, const int64_t* offs,
                             const int* widths, int64_t tail_off, const float* buf, const uint8_t* small_vis, int64_t vis_off, void* stream);

/* ------------------------------------------------------------------------
 * Measurement aid: when enabled, every kernel launched by this library is
 * bracketed by HIP events recorded on the caller's stream.
 * mgr_profile_report synchronises the stream, writes one line per kernel
 * "name count total_ms\n" into buf (NUL terminated) and clears the records.
 * ------------------------------------------------------------------------ */
int mgr_profile_enable(int on);
/* Bracket only the kernel of this name (as it appears in the report); NULL or "" = every kernel.  Two events per
 * bracketed launch cost a few microseconds of GPU time each: a run that is itself being timed should name the one
 * kernel it needs. */
int mgr_profile_filter(const char* kernel_name);
/* Bracket only every n-th launch that passes the filter (n <= 1: every one): the two events around a launch keep the
 * kernels on either side from following it without a gap (~6 us each on this GPU), so a run that is being timed samples. */
int mgr_profile_sample_every(int n);
int mgr_profile_report(char* buf_host, size_t len, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MANUS_HIP_H */
