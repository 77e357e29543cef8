/* misplat.h -- C ABI of libmisplat.so: the MI355X (gfx950) RaDe-GS splat rasterizer.
 *
 * This is the drop-in boundary for the one hot path BASELINE.json's north_star names.
 * The reference (BasisResearch/collab-splats) has NO native code and no FFI of its own
 * (SURVEY.md section 2.1): the path leaves the repo through three Python entry points of the
 * third-party CUDA package gsplat-rade:
 *     gsplat.rendering.rasterization(...)             collab_splats/models/rade_gs_model.py:439-465
 *                                                     collab_splats/models/rade_features_model.py:450-476
 *     gsplat.cuda._wrapper.fully_fused_projection(...) collab_splats/models/rade_gs_model.py:373-394
 *     gsplat.cuda._wrapper.spherical_harmonics(...)    collab_splats/models/rade_features_model.py:430-434
 * plus the pure-PyTorch depth->normal stage    collab_splats/utils/camera_utils.py:176-279.
 * The functions below are what those Python entry points bind in this build (ctypes stub in
 * collab_splats_amd/_lib.py; the reference-side binding is shown in INTEGRATION.md).  Each entry
 * names the stage of the replaced call it implements.
 *
 * Rules (all entry points):
 *   - plain device pointers and sizes only; the caller (PyTorch) owns and allocates every
 *     buffer including scratch, so the caching allocator and stream order are respected;
 *   - asynchronous on `stream`; no hidden synchronisation, no allocation, no host read-back;
 *   - return 0 on success, a negative MISPLAT_E* code otherwise; never throws;
 *   - re-entrant: no mutable global state;
 *   - all floating point is fp32 (reference: mixed_precision=False,
 *     collab_splats/configs/rade_gs_method.py:31); indices int32; sort keys uint64.
 */
#ifndef MISPLAT_H
#define MISPLAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* misplat_stream_t; /* == hipStream_t */

#define MISPLAT_OK 0
#define MISPLAT_EINVAL (-1)      /* bad size / unsupported option (tile_size != 16, colour dim) */
#define MISPLAT_ELAUNCH (-2)     /* hipGetLastError() after a launch was not hipSuccess */
#define MISPLAT_EWORKSPACE (-3)  /* scratch buffer too small */

#define MISPLAT_TILE 16          /* pixels per tile side (gsplat default tile_size)          */
#define MISPLAT_REC 16           /* floats per packed Gaussian record / per gradient row      */
#define MISPLAT_BANDS 2          /* wavefronts (bands of 16 x 8 pixels) that composite one tile */

/* Scalar configuration of one call (host memory, passed by pointer, copied at launch). */
typedef struct misplat_params {
    int32_t n_gauss;   /* N */
    int32_t n_cams;    /* C (the reference always uses 1: rade_gs_model.py:94-95, 446-447) */
    int32_t width, height;
    int32_t tile_size; /* must be MISPLAT_TILE */
    int32_t tile_w, tile_h;
    int32_t antialiased;          /* rasterize_mode == "antialiased" (rade_gs_model.py:459) */
    int32_t opacity_aware_radius; /* tighten the extent to the alpha_min level set */
    float eps2d;          /* 0.3   rade_gs_model.py:382 */
    float near_plane;     /* 0.01  rade_gs_model.py:451 */
    float far_plane;      /* 1e10  rade_gs_model.py:452 */
    float radius_clip;    /* 0.0   rade_gs_model.py:386 */
    float radius_sigma;   /* 3.33 */
    float alpha_max;      /* 0.999 */
    float alpha_min;      /* 1/255 */
    float t_stop;         /* 1e-4 */
    float median_t;       /* 0.5 */
    float jacobian_margin;/* 0.3 */
    float plane_eps;      /* 1e-6 */
    int32_t ed_slot;      /* colour channel (0..3) the compositing kernels divide by max(alpha,1e-10)
                             (the "ED" of render_mode RGB+ED / ED, rade_gs_model.py:237), or -1     */
    int32_t reserved_q;
    /* Launch order of the compositing kernels (speed only; results never depend on it).  A tile is covered by
     * MISPLAT_BANDS independent wavefronts ("bands" of 16 x 8 pixels, two pixels per lane); a "unit" is one band of
     * one tile: unit = tile * MISPLAT_BANDS + band.  unit_work (or NULL): the forward writes the number of staged
     * Gaussians each unit composited -- its measured cost; unit_perm (or NULL): workgroup b of a compositing launch
     * processes unit unit_perm[b] instead of the default XCD-strip map (misplat_unit_order builds it, longest first). */
    const int32_t* unit_perm;
    int32_t* unit_work;
    /* View-keyed orders (unit_sel != NULL): unit_perm is then the base of a TABLE of records of unit_stride int32 each --
     * MISPLAT_ORDER_HEADER header words {tag lo, tag hi, valid, ...} followed by a permutation -- and unit_sel points to
     * four device words {slot, valid, tag lo, tag hi} that misplat_raster_fwd's projection kernel writes from a hash
     * of the call's cameras (viewmats, Ks): a compositing launch uses the permutation of record `slot` if `valid`, the
     * default map otherwise; the forward's order kernel stores the new permutation (and the tag) into that record.  A
     * training loop revisits its cameras every epoch: each view finds the order its own last visit measured. */
#define MISPLAT_ORDER_HEADER 16
    /* (or NULL) one byte per (camera, Gaussian) row, a speed hint that never changes a result: cleared by
     * misplat_project_pack_fwd, set by the ATOMIC compositing backward for every row it adds a gradient to, read by the
     * per-Gaussian backward kernels -- a row that was never set has an all-zero gradient row, which then is not fetched
     * (in a dense scene nine rows in ten; their 64-byte rows were the largest read of both kernels). */
    uint8_t* touched;
    /* Extension (not in gsplat's interface): bit 0 -- `scales` are log-scales, bit 1 -- `opacities` are logits; the fused
     * projection kernels (misplat_project_pack_fwd / _bwd, one camera; misplat_raster_fwd / _bwd) apply exp / sigmoid
     * themselves and return the gradients of the raw parameters -- the four activation launches of
     * rade_gs_model.py:443-444 and their backward disappear.  0 = activated values, as gsplat takes them. */
    int32_t activations;
    int32_t unit_stride;     /* see unit_sel */
    const int32_t* unit_sel; /* or NULL */
    int32_t unit_slots;      /* records in the table: a selector outside [0, unit_slots) counts as "no record" */
    int32_t front_pass;      /* see front_n */
    /* Front-only ordering (set by misplat_raster_fwd for its compositing forward; NULL / 0 everywhere else -- the
     * backward never reads behind the entries the forward used).  unit_reach (or NULL) [units]: the forward writes the
     * DEPTH of the deepest list entry each unit looked at (front_depths[row]; +inf: pixels were still alive at the end of
     * its list, 0: nothing looked at) -- the pivot of the view's next visit.  front_n (or NULL) [C*tiles]: >= 0 -- only
     * that many entries at the head of the tile's list exist (the sorted front part, misplat_raster_args.front_n); a unit
     * that reaches their end with pixels alive sets tile_flag[tile].  front_pass 1: the launch composites the flagged
     * tiles only, over their whole (by then fully sorted) lists. */
    const int32_t* front_n;
    int32_t* tile_flag;
    float* unit_reach;
    const float* front_depths;
} misplat_params;

/* ---- a2.1 projection: fully_fused_projection(means, None, quats, scales, viewmats, Ks, W, H, ...)
 * (rade_gs_model.py:373-394).  Inputs: means[N,3] quats[N,4] (wxyz, un-normalised) scales[N,3]
 * opacities[N] or NULL, viewmats[C,4,4] row-major world->camera, Ks[C,3,3].
 * Outputs, all [C,N,...]: radii int32[.,2], means2d[.,2], depths[.], conics[.,3],
 * compensations[.], ray_ts[.], ray_planes[.,2], normals[.,3]; rows with radii==0 are zero. */
int misplat_project_fwd(const misplat_params* p, const float* means, const float* quats,
                        const float* scales, const float* opacities, const float* viewmats,
                        const float* Ks, int32_t* radii, float* means2d, float* depths,
                        float* conics, float* compensations, float* ray_ts, float* ray_planes,
                        float* normals, misplat_stream_t stream);

/* Backward of the above.  v_* inputs are [C,N,...] gradients of the eight outputs (radii has
 * none); outputs v_means[N,3], v_quats[N,4], v_scales[N,3] are summed over cameras and fully
 * overwritten. */
int misplat_project_bwd(const misplat_params* p, const float* means, const float* quats,
                        const float* scales, const float* viewmats, const float* Ks,
                        const int32_t* radii, const float* v_means2d, const float* v_depths,
                        const float* v_conics, const float* v_compensations,
                        const float* v_ray_ts, const float* v_ray_planes, const float* v_normals,
                        float* v_means, float* v_quats, float* v_scales, misplat_stream_t stream);

/* The view-matrix gradient of the same projection: v_viewmats[C,4,4] (fp32, fully overwritten, bottom rows zero) from the
 * same inputs as misplat_project_bwd.  With Rw = V[c,:3,:3], t = V[c,:3,3]: v_V[c,:3,:3] = sum_g (v_mu (x) mean +
 * v_Rc Rg(q)^T), v_V[c,:3,3] = sum_g v_mu over the rows with radii > 0.  fp64 sums in a fixed order (two launches, no
 * atomics, no host read): two calls give the same bits.  Ks gets no gradient.  workspace: device memory of
 * misplat_project_bwd_pose_workspace(n_gauss, n_cams) bytes (depends on the sizes only; NULL is MISPLAT_EINVAL).
 * n_gauss == 0 writes zeros. */
int64_t misplat_project_bwd_pose_workspace(int32_t n_gauss, int32_t n_cams);
int misplat_project_bwd_pose(const misplat_params* p, const float* means, const float* quats,
                             const float* scales, const float* viewmats, const float* Ks,
                             const int32_t* radii, const float* v_means2d, const float* v_depths,
                             const float* v_conics, const float* v_compensations,
                             const float* v_ray_ts, const float* v_ray_planes, const float* v_normals,
                             void* workspace, float* v_viewmats, misplat_stream_t stream);

/* ---- a2.2 SH: spherical_harmonics(degrees_to_use, dirs, coeffs) (rade_features_model.py:430-434).
 * dirs[C*N,3] (normalised inside), coeffs[N,K,3] shared by the C cameras, radii[C*N,2] or NULL
 * (rows with radii==0 are skipped and get colour 0), colors[C*N,3] = raw SH (no +0.5). */
int misplat_sh_fwd(int32_t n_gauss, int32_t n_cams, int32_t K, int32_t degree, const float* dirs,
                   const float* coeffs, const int32_t* radii, float* colors,
                   misplat_stream_t stream);
int misplat_sh_bwd(int32_t n_gauss, int32_t n_cams, int32_t K, int32_t degree, const float* dirs,
                   const float* coeffs, const int32_t* radii, const float* v_colors,
                   float* v_coeffs /*[N,K,3]*/, float* v_dirs /*[C*N,3]*/,
                   misplat_stream_t stream);

/* ---- fused per-Gaussian stages (what rasterization() runs; same math as the entry points above,
 * without the SoA round trips).  project_pack_fwd writes the geometry part of the packed blend
 * record (layout: see misplat_pack) straight away; color_fwd fills the record's colour slots:
 *   sh_degree >= 0: colour = max(SH_deg(mean - camera_centre) . coeffs[N,K,3] + 0.5, 0), K <= 16
 *                   (rade_features_model.py:428-438; coefficients staged through LDS, coalesced);
 *   sh_degree <  0: the first n_color (<= 4) of the D colour channels are copied
 *                   (colors [N,D], or [C,N,D] when per_cam).
 * depth_channel != 0 puts the z-depth into colour slot n_color (RGB+ED / ED render modes).
 * The backward kernels consume the packed gradient rows v_grec[C*N,16] produced by
 * misplat_slab_reduce; v_means2d is passed separately (it is a retained autograd node). */
int misplat_project_pack_fwd(const misplat_params* p, const float* means, const float* quats,
                             const float* scales, const float* opacities, const float* viewmats,
                             const float* Ks, int32_t* radii, float* means2d, float* depths,
                             float* compensations, float* grec,
                             uint32_t* zero_words /* or NULL */, int32_t n_zero /* words the kernel clears for its
                             successors on the stream (the bucketing counters): saves a memset launch */,
                             float* lazy_rows /* or NULL.  Given (v_grec-shaped, [C*N,16]): on-demand colours -- the colour
                             slots of grec are left UNSET for misplat_blend_fwd_lazy, and these gradient rows are cleared */,
                             float* abs_rows /* or NULL: v_abs-shaped rows [C*N,2] cleared for the compositing backward
                             (misplat_blend_bwd_atomic, v_grec_is_zero bit 1): saves that memset launch */,
                             misplat_stream_t stream);
/* coeffs_rest (SH only, may be NULL): when given, coeffs_or_colors is features_dc[N,3] and
 * coeffs_rest is features_rest[N,K-1,3] -- the reference's two parameter tensors
 * (rade_gs_model.py:119-120) read in place instead of through its per-step torch.cat (:128-130);
 * v_coeffs_rest is the matching gradient output.
 * sh_aux[C*N,12] (SH only, may be NULL): written by color_fwd -- the 3x3 Jacobian d rgb / d dir of the clamped
 * colour (rows of clamped channels zeroed) and the three clamp flags -- and, when passed to color_bwd, used
 * instead of re-reading the 12 K bytes of coefficients per Gaussian (48 B instead of 192 B at degree 3). */
int misplat_color_fwd(const misplat_params* p, int32_t sh_degree, int32_t K_or_D, int32_t n_color,
                      int32_t per_cam, int32_t depth_channel, const float* means,
                      const float* viewmats, const float* coeffs_or_colors, const float* coeffs_rest,
                      const int32_t* radii, const float* depths, float* grec,
                      float* sh_aux /* or NULL */,
                      float* zero_rows /* or NULL: [C*N,16] cleared by the kernel -- the gradient rows the backward's
                      atomics add into (misplat_blend_bwd_atomic, v_grec_is_zero): saves the 64 B/row memset launch */,
                      misplat_stream_t stream);
int misplat_color_bwd(const misplat_params* p, int32_t sh_degree, int32_t K_or_D, int32_t n_color,
                      int32_t per_cam, const float* means, const float* viewmats,
                      const float* coeffs_or_colors, const float* coeffs_rest, const int32_t* radii,
                      const float* v_grec, float* v_coeffs_or_colors, float* v_coeffs_rest,
                      float* v_means_dir /*[N,3], SH only*/, const float* sh_aux /* or NULL */,
                      misplat_stream_t stream);
/* depth_slot: 12..15 = record slot carrying the depth channel, -1 = none.  v_means_dir may be
 * NULL.  v_depth_rows (or NULL; then depth_slot must be -1): the depth channel's gradient lives OUTSIDE the record -- row
 * g's value is v_depth_rows[g * v_depth_stride] (the N-D colour path keeps channels >= 4 in featx: pass a pointer into
 * v_featx).  Outputs v_means[N,3] v_quats[N,4] v_scales[N,3] v_opacities[N], summed over cameras. */
int misplat_project_pack_bwd(const misplat_params* p, int32_t depth_slot, const float* means,
                             const float* quats, const float* scales, const float* opacities,
                             const float* viewmats, const float* Ks, const int32_t* radii,
                             const float* compensations, const float* v_means2d, const float* v_grec,
                             const float* v_means_dir, float* v_means, float* v_quats,
                             float* v_scales, float* v_opacities, const float* v_depth_rows,
                             int32_t v_depth_stride, misplat_stream_t stream);

/* ---- a2.3 binning: for every tile the Gaussian rows whose rectangle mean2d +- radii touches it, in
 * (depth, row) order -- the order of gsplat's 64-bit (tile | depth) key sort, without the keys: the cell-ordered
 * bucketing (bucket_*, below) fills every tile's bucket in arbitrary order, then misplat_tile_sort orders every bucket by
 * (depth, row).  offsets arrays have C*tiles + 1 entries: the last one is the number of intersections. */
/* gsplat's meta["isect_ids"] on demand: (tile << 32) | bits(depth[flatten_ids[i]]). */
int misplat_isect_ids(const uint32_t* tiles_sorted, const int32_t* flatten_ids, const float* depths,
                      int64_t n_isects, uint64_t* isect_ids, misplat_stream_t stream);

/* Per-tile ordering: once the intersections have been bucketed by tile, one workgroup per tile sorts its bucket --
 * entries in registers, exchange through LDS: one counting pass on the bucket's own depth range + ranking inside the
 * bins, or stable LSD radix passes -- into the (depth, row) order, equal depths included: exactly the (tile, depth, id)
 * order of a global 64-bit key sort, without one.  Buckets arrive in arbitrary order (misplat_bucket_tiles).
 * offsets: n_tiles_total + 1 entries; n_isects: the number of intersections or an upper bound of it (only used to
 * size the grids of the size classes); payload (in/out): rows, or emission slots when isect_gid != NULL
 * (row = isect_gid[slot]); flatten_ids (out): rows in final order; scratch[2 * n_isects] backs the rare tiles
 * longer than 8192 entries. */
int misplat_tile_sort(const int32_t* offsets, int32_t n_tiles_total, int64_t n_isects,
                      const float* depths, const int32_t* isect_gid, int32_t* payload,
                      int32_t* flatten_ids, uint32_t* scratch, int32_t flags /* bit 1:
                      offsets[n_tiles_total + 1] holds the longest bucket (misplat_bucket_tiles writes it), so the
                      launches of unused size classes return at once; bit 2: the payload holds positions in the cell-ordered
                      row list (misplat_raster_args.depth_sorted): isect_gid = that list (row = isect_gid[entry], equal depths
                      come out in ROW order), depths is indexed by the entry */, misplat_stream_t stream);

/* ---- Cell-ordered bucketing (csrc/bucket.hip).  Replaces gsplat's isect_tiles +
 * radix sort + isect_offset_encode: every intersection is written once (its row) and no tile-id array exists.
 *   bucket_plan   (host only) number of screen cells and of counting workgroups for this configuration:
 *                 cellhist holds n_blocks * n_cells uint32, cell_count n_cells, cell_offs n_cells + 1;
 *   bucket_count  tiles_per_gauss[C*N], rect2[C*N] (x0 | y0 << 16, w | h << 16 of the tile rectangle), the
 *                 per-workgroup cell histograms, the global cell counts; counters[0] = number of intersections
 *                 (device int64; cell_count and counters[2] are zeroed here on `stream` unless already_zero);
 *   bucket_rows   cell_offs = scan of the cell counts, counters[1] = visible rows, order[0 .. n_vis) = the visible
 *                 rows in cell order and rect_sorted[0 .. n_vis) their rectangles (layout of rect2, capacity C*N);
 *                 cell_cursor[n_cells] (scratch) and tile_count[n_tiles + 1] must be zero on entry: cleared here unless
 *                 already_zero says an earlier kernel of the stream did (bit 0: cell_cursor, bit 1: tile_count);
 *                 n_isects_host (or NULL): 8 bytes of PINNED, device-mapped host memory that receives counters[0] as a
 *                 system-scope store from the kernel -- the caller polls it (misplat_wait_count), no copy is enqueued;
 *   bucket_tiles  (tile_count must be all zero on entry, as bucket_rows leaves it; it is NOT zero afterwards)
 *                 offsets[0 .. n_tiles + 1] (offsets[n_tiles] = number of intersections, offsets[n_tiles + 1] = the
 *                 longest bucket: n_tiles + 2 entries) and
 *                 payload[offsets[t] .. offsets[t + 1]) = the rows touching tile t, in arbitrary order
 *                 (misplat_tile_sort follows).  cum != NULL (deterministic backward): the payload
 *                 is the emission slot cum[row] + k and isect_gid[slot] = row.  Writes beyond cap_isects entries
 *                 are dropped: the caller compares counters[0] with cap_isects afterwards.
 * Nothing here needs a host read-back: all sizes live in `counters` on the device. */
#define MISPLAT_BUCKET_MAX_CELLS 2048
#define MISPLAT_BUCKET_MAX_BLOCKS 256
int misplat_bucket_plan(const misplat_params* p, int32_t* n_cells, int32_t* n_blocks);
int misplat_bucket_count(const misplat_params* p, const float* means2d, const int32_t* radii,
                         int32_t* tiles_per_gauss, uint32_t* rect2, uint32_t* cellhist, uint32_t* cell_count,
                         int64_t* counters, int32_t already_zero /* cell_count and counters were cleared by an
                         earlier kernel of the stream (misplat_project_pack_fwd's zero_words): no memset here */,
                         misplat_stream_t stream);
int misplat_bucket_rows(const misplat_params* p, const int32_t* tiles_per_gauss, const uint32_t* rect2,
                        const uint32_t* cellhist, const uint32_t* cell_count, uint32_t* cell_cursor, uint32_t* cell_offs,
                        int32_t* order, uint32_t* rect_sorted, int64_t* counters, int32_t* tile_count,
                        int64_t* n_isects_host /* or NULL */, int32_t already_zero, misplat_stream_t stream);
int misplat_bucket_tiles(const misplat_params* p, const int32_t* order, const uint32_t* rect_sorted,
                         const int64_t* counters, int32_t* tile_count, int32_t* offsets, const int64_t* cum,
                         int64_t cap_isects, int32_t* payload, int32_t* isect_gid, misplat_stream_t stream);

/* ---- a2.4 / a2.5 compositing.  Packed record per (camera, Gaussian), MISPLAT_REC floats:
 *   [0:2] mean2d  [2:5] conic  [5] opacity_eff  [6] ray_t  [7:9] ray_plane  [9:12] normal
 *   [12:16] colour channels 0..3 (unused channels zero).                         */
int misplat_pack(int64_t n_rows, int32_t color_dim, const float* means2d, const float* conics,
                 const float* opacities_eff, const float* ray_ts, const float* ray_planes,
                 const float* normals, const float* colors, float* grec, misplat_stream_t stream);

/* Forward: one wavefront per band of 16 x 8 pixels of a tile (two pixels per lane).
 * offsets: C*tiles + 1 entries (tile t owns flatten_ids[offsets[t] .. offsets[t+1])); n_isects: the number of
 * intersections or an upper bound (the backward's slab stride).
 * Outputs [C,H,W,...]: render[.,color_dim], alpha[.], exp_depth[.] (sum w*z, un-normalised),
 * med_depth[.], normal[.,3], last_ids[.], median_ids[.] (sorted positions; -1 = none).
 * color_dim in 1..4. */
int misplat_blend_fwd(const misplat_params* p, int32_t color_dim, const float* Ks,
                      const float* grec, const int32_t* flatten_ids, const int32_t* offsets,
                      int64_t n_isects, float* render, float* alpha, float* exp_depth,
                      float* med_depth, float* normal, int32_t* last_ids, int32_t* median_ids,
                      misplat_stream_t stream);
/* The same forward with ON-DEMAND SH colours: the colour slots of grec hold the "unset" pattern left by
 * misplat_project_pack_fwd(lazy_rows != NULL) and are filled here (grec is read AND written) for the records that are
 * staged past their cull -- in a dense scene most visible Gaussians never are.  16 coefficients per Gaussian: coeffs
 * [N,16,3], or features_dc [N,3] + coeffs_rest [N,15,3]. */
int misplat_blend_fwd_lazy(const misplat_params* p, int32_t color_dim, const float* Ks, float* grec,
                           const int32_t* flatten_ids, const int32_t* offsets, int64_t n_isects, float* render,
                           float* alpha, float* exp_depth, float* med_depth, float* normal, int32_t* last_ids,
                           int32_t* median_ids, const float* means, const float* viewmats, const float* coeffs,
                           const float* coeffs_rest, int32_t sh_degree, int32_t depth_channel, const float* depths,
                           float* sh_aux /* NULL */, misplat_stream_t stream);


/* Launch order for the compositing kernels (speed only): unit_perm[8 * ceil(units / 8)] from the per-unit cost
 * unit_work[units] the forward measured (misplat_params.unit_work), longest first inside every XCD strip;
 * units = C * tiles * MISPLAT_BANDS.  Padding entries hold `units` (no unit).  Pass the result as
 * misplat_params.unit_perm to any later compositing launch -- the backward of the same step, or the next forward of the
 * same view. */
int misplat_unit_order(const misplat_params* p, const int32_t* unit_work, int32_t* unit_perm,
                       misplat_stream_t stream);

/* Number of gradient planes (= bands per tile) the backward of this configuration writes. */
int misplat_blend_planes(const misplat_params* p);

/* Backward: every band re-traverses its tile list back to front and writes ONE gradient row
 * (record layout) per Gaussian that contributed to the band, to slab[band][slot] (slot = position in
 * emission order, so the rows of one Gaussian are contiguous), and sets slab_valid[band][slot] = 1.
 * slab: [planes, n_isects, 16] floats; slab_abs: [planes, n_isects, 2] or NULL (sum |dL/dmean2d|);
 * slab_valid: [planes, n_isects] bytes, zeroed here on `stream`.  No float atomics anywhere. */
int misplat_blend_bwd(const misplat_params* p, int32_t color_dim, const float* Ks,
                      const float* grec, const int32_t* flatten_ids, const int32_t* slots_sorted,
                      const int32_t* offsets, int64_t n_isects, const float* alpha,
                      const int32_t* last_ids, const int32_t* median_ids,
                      const float* render /* forward output, read only if ed_slot >= 0 */,
                      const float* v_render, const float* v_alpha, const float* v_exp_depth,
                      const float* v_med_depth, const float* v_normal, float* slab, float* slab_abs,
                      uint8_t* slab_valid,
                      misplat_stream_t stream);
/* Same backward with the rows added straight into v_grec[C*N,16] / v_abs[C*N,2] (or NULL) by
 * no-return fp32 atomics of 64 contiguous bytes: no slab and no reduce pass, but the sums depend on
 * arrival order.  v_grec / v_abs are zeroed here on `stream`. */
int misplat_blend_bwd_atomic(const misplat_params* p, int32_t color_dim, const float* Ks,
                             const float* grec, const int32_t* flatten_ids, const int32_t* offsets,
                             int64_t n_isects, const float* alpha, const int32_t* last_ids,
                             const int32_t* median_ids, const float* render, const float* v_render,
                             const float* v_alpha, const float* v_exp_depth, const float* v_med_depth,
                             const float* v_normal, float* v_grec, float* v_abs,
                             int32_t v_grec_is_zero /* bit 0: v_grec was cleared by misplat_color_fwd (zero_rows) and has
                             not been used since; bit 1: v_abs was cleared by the caller: skip that memset */,
                             misplat_stream_t stream);
/* ---- a8: N-D colours in one pass (rade_features_model.py:441-476: D = 16 fused channels, 17 with
 * RGB+ED).  n_channels = D' in 5..20; channels 0..3 live in the record's colour slots, channels 4..
 * in featx[C*N, 4*nxq] (nxq = ceil((D'-4)/4) float4s per row, zero padded); color_fwd_x writes both
 * from colors[(C,)N,D] (+ the depth channel); render is [C,H,W,n_channels].  Gradients: atomic mode
 * only (v_grec, v_featx, v_abs zeroed here on `stream`). */
int misplat_color_fwd_x(const misplat_params* p, int32_t D, int32_t per_cam, int32_t depth_channel,
                        int32_t nxq, const float* colors, const int32_t* radii, const float* depths,
                        float* grec, float* featx, misplat_stream_t stream);
int misplat_color_bwd_x(const misplat_params* p, int32_t D, int32_t per_cam, int32_t nxq,
                        const int32_t* radii, const float* v_grec, const float* v_featx,
                        float* v_colors, misplat_stream_t stream);
int misplat_blend_fwd_x(const misplat_params* p, int32_t n_channels, int32_t nxq, const float* Ks,
                        const float* grec, const float* featx, const int32_t* flatten_ids,
                        const int32_t* offsets, int64_t n_isects, float* render, float* alpha,
                        float* exp_depth, float* med_depth, float* normal, int32_t* last_ids,
                        int32_t* median_ids, misplat_stream_t stream);
int misplat_blend_bwd_x_atomic(const misplat_params* p, int32_t n_channels, int32_t nxq, const float* Ks,
                               const float* grec, const float* featx, const int32_t* flatten_ids,
                               const int32_t* offsets, int64_t n_isects, const float* alpha,
                               const int32_t* last_ids, const int32_t* median_ids, const float* render,
                               const float* v_render, const float* v_alpha, const float* v_exp_depth,
                               const float* v_med_depth, const float* v_normal, float* v_grec,
                               float* v_featx, float* v_abs, misplat_stream_t stream);

/* v_grec[r] = sum of the VALID slab rows of Gaussian row r (slots cum[r] .. cum[r]+tiles_per_gauss[r],
 * all planes) in a fixed order => bitwise reproducible.  v_abs[n_rows,2] likewise from slab_abs
 * (both may be NULL together). */
int misplat_slab_reduce(const misplat_params* p, int64_t n_rows, int64_t n_isects, const int64_t* cum,
                        const int32_t* tiles_per_gauss, const float* slab, const float* slab_abs,
                        const uint8_t* slab_valid, float* v_grec, float* v_abs,
                        misplat_stream_t stream);

/* ---- a4 depth->normal (camera_utils.py:176-279) fused with the error map of
 * rade_gs_model.py:212-214: n_d = normalize(cross(dP/drow, dP/dcol)) of the back-projected
 * expected / median z-depth maps (interior pixels; border 0), err[k] = 1 - <n_render, n_d[k]>.
 * depths: exp_depth[H,W], med_depth[H,W]; n_render[H,W,3]; outputs normals2[2,H,W,3], err[2,H,W]. 
 * accumulate != 0 (backward): the three gradients are ADDED to the output buffers (which then already hold the
 * gradients of the a3 epilogue, misplat_outputs_bwd) instead of stored. */
int misplat_depth_normal_fwd(int32_t width, int32_t height, float fx, float fy,
                             const float* exp_depth, const float* med_depth,
                             const float* n_render, float* normals2, float* err,
                             misplat_stream_t stream);
int misplat_depth_normal_bwd(int32_t width, int32_t height, float fx, float fy,
                             const float* exp_depth, const float* med_depth,
                             const float* n_render, const float* v_normals2 /*or NULL*/,
                             const float* v_err /*or NULL*/, float* v_exp_depth,
                             float* v_med_depth, float* v_n_render, int32_t accumulate, misplat_stream_t stream);

/* ---- a3 get_outputs post-processing (rade_gs_model.py:221-254), one pixel = one image element
 * (C = 1).  background3_host: 3 floats in HOST memory.  maxes4: 4-float device scratch receiving
 * the un-masked maxima of expected depth, median depth, (normal+1)/2 and render[...,3].
 *   rgb = clamp(render[:3] + (1-alpha)*bg, 0, 1); depth/median_depth/normals/depth_im =
 *   where(alpha > 0, x, max(x)) with normals = (expected_normals+1)/2; depth_im (or NULL) needs
 *   color_dim == 4.  The maxima carry no gradient (the reference detaches them). */
int misplat_outputs_fwd(int64_t n_pix, int32_t color_dim, const float* background3_host,
                        const float* render, const float* alpha, const float* exp_depth,
                        const float* med_depth, const float* exp_normal, float* maxes4, float* rgb,
                        float* depth, float* median_depth, float* normals, float* depth_im,
                        misplat_stream_t stream);
int misplat_outputs_bwd(int64_t n_pix, int32_t color_dim, const float* background3_host,
                        const float* render, const float* alpha, const float* v_rgb,
                        const float* v_depth, const float* v_median_depth, const float* v_normals,
                        const float* v_depth_im /* or NULL */, float* v_render, float* v_alpha,
                        float* v_exp_depth, float* v_med_depth, float* v_exp_normal,
                        misplat_stream_t stream);

/* ---- a5 get_loss_dict (rade_gs_model.py:289-307: depth_normal_lambda * ((1 - depth_ratio) * mean(depth_normal_error_map)
 * + depth_ratio * mean(middepth_normal_error_map)); the base model's L1 term mean |gt - rgb|) in two launches, and
 * its backward in one.  rgb / gt [n_pix,3] (16-byte aligned), err_exp / err_med [n_pix]; either pair may be NULL (that
 * loss is then not computed).  partials: 3 * 512 floats of device scratch.  rgb_loss / dn_loss: device scalars.
 * Reproducible bit for bit (fixed grid and summation tree, fp64 final sums). */
#define MISPLAT_LOSS_PARTIALS (3 * 512)
int misplat_loss_fwd(int64_t n_pix, const float* rgb, const float* gt, const float* err_exp, const float* err_med,
                     float depth_ratio, float depth_normal_lambda, float* partials, float* rgb_loss, float* dn_loss,
                     misplat_stream_t stream);
/* g_rgb_loss / g_dn_loss: the upstream gradients of the two loss values as DEVICE scalars (or NULL = 0);
 * v_rgb[n_pix,3] = -g / (3 n) sign(gt - rgb), v_err_exp / v_err_med[n_pix] = the constant images g lambda (1 - r) / n and
 * g lambda r / n.  v_rgb or the v_err pair may be NULL. */
int misplat_loss_bwd(int64_t n_pix, const float* rgb, const float* gt, const float* g_rgb_loss, const float* g_dn_loss,
                     float depth_ratio, float depth_normal_lambda, float* v_rgb, float* v_err_exp, float* v_err_med,
                     misplat_stream_t stream);

/* ---- the image term of the loss the model inherits (rade_gs_model.py:289 `super().get_loss_dict`: nerfstudio Splatfacto,
 * third-party and absent from the reference tree) [UNVERIFIED-UPSTREAM]:
 *   main_loss = (1 - ssim_lambda) * mean |gt - rgb| + ssim_lambda * (1 - SSIM(gt, rgb)),
 * SSIM as pytorch_msssim.SSIM(data_range=1.0, size_average=True, channel=3): 11-tap gaussian window (sigma 1.5), valid
 * region (H - 10) x (W - 10), K = (0.01, 0.03), mean over positions and channels.  rgb / gt: [H,W,3]; H, W >= 11.
 * scratch: misplat_ssim_scratch_floats(H, W) floats, written by the forward (three derivative maps + tile sums) and read
 * by the backward.  l1_loss: DEVICE scalar mean |gt - rgb| computed elsewhere (misplat_loss_fwd's rgb_loss), or NULL =
 * the forward sums it itself (its tiles hold both images anyway: fixed tile sums, fp64 final sum); ssim / main_loss:
 * device scalars (either may be NULL).  Two launches; reproducible bit for bit. */
int64_t misplat_ssim_scratch_floats(int32_t height, int32_t width);
int misplat_ssim_fwd(int32_t height, int32_t width, const float* rgb, const float* gt, float* scratch,
                     const float* l1_loss /* or NULL */, float ssim_lambda, float* ssim /* or NULL */,
                     float* main_loss /* or NULL */, misplat_stream_t stream);
/* v_rgb[H,W,3] = g_main * d main_loss / d rgb (both terms: the L1 sign gradient and the transposed window filter of the
 * forward's maps); g_main: DEVICE scalar (or NULL = 0).  One launch, no atomics. */
int misplat_ssim_bwd(int32_t height, int32_t width, const float* rgb, const float* gt, const float* scratch,
                     const float* g_main, float ssim_lambda, float* v_rgb, misplat_stream_t stream);

/* ---- the features model's decoder and cosine feature loss (rade_features_model.py:149-189, :545-584; utils/features.py:
 * 408-478): csrc/featloss.hip.
 *   x = bilinear(features [H,W,L] -> (main_h, main_w)) (align_corners=False, no antialiasing), h = relu(w_hidden x + b_hidden),
 *   p_b = w_out[b] h_b + b_out[b] with h_b = h resampled bilinearly to the branch's (H_b, W_b) (equal to resizing p_b),
 *   features_loss = loss_lambda * sum_b weights[b] * mean_q (1 - <p_b, gt_b> / (max(|p_b|, 1e-8) * max(|gt_b|, 1e-8))).
 * features: pixel (y, x) starts at features[(y * W + x) * pix_stride] (pix_stride >= latent: a channel slice of a wider
 * image is read in place); w_hidden [hidden, latent], b_hidden [hidden]; dims: HOST array [n_branches][3] = (C_b, H_b, W_b);
 * w_out / b_out / gt: HOST arrays of n_branches DEVICE pointers ([C_b, hidden], [C_b], [C_b, H_b, W_b]); weights: HOST
 * array [n_branches].  Limits: latent 1..32, hidden 1..256, 1..4 branches, C_b 1..2^20, every map at most 2^28 pixels.
 * scratch: misplat_featloss_scratch_floats(...) floats (decode_only != 0: what misplat_feature_decode needs), written by
 * the forward and read AND written by the backward; -1 for sizes outside the limits.  branch_sums (or NULL): device
 * [n_branches] sums of 1 - cos over a branch's pixels; features_loss (or NULL): device scalar.  Four or five launches;
 * no prediction is stored; every sum over pixels runs in a fixed order (final sums in fp64): reproducible bit for bit. */
int64_t misplat_featloss_scratch_floats(int32_t latent, int32_t hidden, int32_t main_h, int32_t main_w, int32_t n_branches,
                                        const int32_t* dims, int32_t decode_only);
int misplat_featloss_fwd(int32_t height, int32_t width, int32_t latent, int32_t pix_stride, const float* features,
                         int32_t hidden, const float* w_hidden, const float* b_hidden, int32_t main_h, int32_t main_w,
                         int32_t n_branches, const int32_t* dims, const float* const* w_out, const float* const* b_out,
                         const float* const* gt, const float* weights, float loss_lambda, float* scratch,
                         float* branch_sums /* or NULL */, float* features_loss /* or NULL */, misplat_stream_t stream);
/* g_loss: the upstream gradient of features_loss as a DEVICE scalar (or NULL = 0).  v_features [H,W,latent] (contiguous,
 * every element written: exact zeros where no tap of the resize lands; W * latent < 2^31), v_w_hidden [hidden, latent], v_b_hidden [hidden];
 * v_w_out / v_b_out: HOST arrays of n_branches DEVICE pointers.  Six launches, no atomics. */
int misplat_featloss_bwd(int32_t height, int32_t width, int32_t latent, int32_t hidden, const float* w_hidden, int32_t main_h,
                         int32_t main_w, int32_t n_branches, const int32_t* dims, const float* const* w_out,
                         const float* const* b_out, const float* const* gt, const float* weights, float loss_lambda,
                         float* scratch, const float* g_loss, float* v_features, float* v_w_hidden, float* v_b_hidden,
                         float* const* v_w_out, float* const* v_b_out, misplat_stream_t stream);
/* Inference: the predictions themselves.  out: HOST array of n_branches DEVICE pointers, each [C_b, H_b, W_b] or, with
 * channels_last != 0, [H_b * W_b, C_b].  Two or three launches. */
int misplat_feature_decode(int32_t height, int32_t width, int32_t latent, int32_t pix_stride, const float* features,
                           int32_t hidden, const float* w_hidden, const float* b_hidden, int32_t main_h, int32_t main_w,
                           int32_t n_branches, const int32_t* dims, const float* const* w_out, const float* const* b_out,
                           float* const* out, int32_t channels_last, float* scratch, misplat_stream_t stream);

/* ---- text-query similarity of rendered views and of Gaussians without the decoded features (rade_features_model.py:493-539,
 * :143-147; utils/features.py:237-325 compute_similarity): csrc/textquery.hip.  The text embeddings E [Q, C] (unit-norm rows,
 * the first n_positive positive, the others negative) meet a prediction p = w_out h + b_out only through E p = A h + c with
 * A = E w_out [Q, hidden] and c = E b_out [Q]; per pixel
 *   x = bilinear(features -> (work_h, work_w)) (the rule of the feature loss above; the image's own size: the latent as it is),
 *   hid = relu(w_hidden x + b_hidden), z_q = (A_q . hid + c_q) / softmax_temp,
 *   method 0 ("standard"): softmax(z)[:n_positive].sum(); method 1 ("pairwise"): exp(p) / (n_neg exp(p) + sum_j exp(n_j)) with
 *   p the mean of the positive z and n_j the negative ones; the maximum is subtracted before any exp; a NaN result is 0.
 * Limits: latent 1..32, hidden 1..256, n_queries 2..64, 1 <= n_positive <= n_queries - 1, channels 1..2^20, softmax_temp
 * finite and > 0, every map at most 2^28 pixels, at most 2^28 rows.  One launch each, no atomics, every sum in index order:
 * reproducible bit for bit.
 * fold: A and c from embeddings [Q, channels], w_out [channels, hidden], b_out [channels]; each output is one fp64 sum over the
 * channels in index order, rounded once.  Once per query set. */
int misplat_textquery_fold(int32_t n_queries, int32_t channels, int32_t hidden, const float* embeddings, const float* w_out,
                           const float* b_out, float* A, float* c, misplat_stream_t stream);
/* similarity [work_h, work_w] of an image features [H,W,latent] read through pix_stride as the feature loss reads it. */
int misplat_textquery_map(int32_t height, int32_t width, int32_t latent, int32_t pix_stride, const float* features, int32_t hidden,
                          const float* w_hidden, const float* b_hidden, int32_t n_queries, int32_t n_positive, const float* A,
                          const float* c, int32_t method, float softmax_temp, int32_t work_h, int32_t work_w, float* similarity,
                          misplat_stream_t stream);
/* similarity [n_rows] of latents [n_rows, latent] (row r starts at latents[r * row_stride]): the same body, no resize. */
int misplat_textquery_rows(int64_t n_rows, int32_t latent, int32_t row_stride, const float* latents, int32_t hidden,
                           const float* w_hidden, const float* b_hidden, int32_t n_queries, int32_t n_positive, const float* A,
                           const float* c, int32_t method, float softmax_temp, float* similarity, misplat_stream_t stream);
/* out [out_h, out_w] = bilinear(in [in_h, in_w]) by the same rule: the reference's F.interpolate of the heat map. */
int misplat_textquery_upsample(int32_t in_h, int32_t in_w, const float* in, int32_t out_h, int32_t out_w, float* out,
                               misplat_stream_t stream);

/* ---- the whole forward of rasterization() (rade_gs_model.py:439-465) as ONE host entry: csrc/raster.hip.
 * Every pointer is a caller-allocated device buffer of the size the per-stage entry points above document
 * (n_isects_host: 8 bytes of PINNED host memory).
 *   phases & 1 (A): project_pack_fwd, bucket_count, bucket_rows (which stores counters[0] into *n_isects_host), color_fwd
 *   phases & 2 (B): bucket_tiles, tile_sort; blend_fwd (+ unit_work), unit_order
 * B only reads device-side sizes, so it may be enqueued with a speculative cap_isects before the host knows the count:
 * the result is exact iff the count (misplat_wait_count) is <= cap_isects (else: clear tile_count and call B again
 * with the exact size).  Atomic gradient mode only (the deterministic slab needs the emission-slot scan between A and B). */
typedef struct misplat_raster_args {
    /* inputs (rasterization() arguments) */
    const float *means, *quats, *scales, *opacities, *colors, *colors_rest, *viewmats, *Ks;
    int32_t sh_degree;      /* -1: pass-through colours */
    int32_t K_or_D, n_color, per_cam, depth_channel;
    int32_t color_dim;      /* channels the compositing kernels carry (1..4) */
    int32_t reserved_c;
    int32_t lazy_colour;    /* != 0 (SH colours with K = 16, one pass): no colour kernel -- the compositing
                               forward evaluates the colour of a record when it first stages it (misplat_blend_fwd_lazy);
                               sh_aux is not written.  2: in addition v_grec_zero is NOT cleared as a whole -- only the
                               rows of the records whose colour gets set, which are the only rows the compositing backward
                               adds into: for a backward that reads flagged rows only (misplat_raster_bwd_plan bit 0);
                               any other backward must clear v_grec first (zero_flags bit 0 unset) */
    /* per (camera, Gaussian) outputs */
    int32_t* radii;
    float *means2d, *depths, *compensations, *grec, *sh_aux /* or NULL */;
    float* v_grec_zero; /* or NULL: gradient rows [C*N,16] cleared by the colour kernel (see misplat_color_fwd) */
    /* bucketing workspace + results */
    int32_t* tiles_per_gauss;
    uint32_t *rect2, *cellhist, *cell_count, *cell_offs;
    uint32_t* cell_cursor;  /* n_cells words of scratch; cell_count, cell_cursor, counters (4 words) and tile_count must be
                               slices of ONE allocation in this order: the projection kernel clears the whole range */
    int32_t* order;
    uint32_t* rect_sorted;
    int64_t* counters;
    int32_t *tile_count, *offsets, *payload, *flatten_ids;
    uint32_t* scratch;
    int64_t cap_isects;
    int64_t* n_isects_host; /* pinned host memory, or NULL */
    float* v_abs_zero; /* or NULL: |mean2d gradient| rows [C*N,2] cleared by the projection kernel */
    /* images */
    float *render, *alpha, *exp_depth, *med_depth, *normal;
    int32_t *last_ids, *median_ids;
    /* launch order (speed only): see misplat_params.unit_perm / unit_work */
    const int32_t* unit_perm_in;
    int32_t *unit_work, *unit_perm_out;
    /* measurement (or NULL): two hipEvent_t recorded on `stream` directly before and after the compositing forward; a
     * call that carries them is launched plainly (no graph) */
    void *ev_blend_begin, *ev_blend_end;
    /* view-keyed launch orders (misplat_params.unit_sel), or NULL: order_table[order_slots][order_stride] int32 --
     * zero-initialised by the caller once and kept between calls --, order_sel[4].  Phase A selects the record of the
     * call's cameras, phase B composites in that record's order (if it holds one) and stores the order it measured.
     * unit_perm_in / unit_perm_out are ignored then; unit_work is still needed. */
    int32_t *order_table, *order_sel;
    int32_t order_slots, order_stride;
    /* Front-only ordering for dense scenes (needs the view-keyed table; csrc/binning.hip).  unit_reach (or NULL) [units]:
     * the compositing forward's reach per unit; the order kernel turns it into per-tile depth pivots stored behind the
     * permutation of the view's record (order_stride >= MISPLAT_ORDER_HEADER + 8 * ceil(units / 8) + C * tiles).
     * front_n / tile_flag (both or neither) [C*tiles]: with them, phase B sorts only the part of every bucket at or in
     * front of front_margin x the pivot of the view's last visit (buckets of >= front_min_bucket entries; everything else,
     * and every tile of a view without a record, is sorted in full), composites, sorts the tiles whose pixels were still
     * alive at the end of their truncated list in full and composites those again: exact images either way.  flatten_ids
     * is then complete only for the tiles with front_n < 0 or tile_flag != 0; misplat_tile_sort over `payload` (which stays
     * a permutation of every bucket) completes it. */
    float* unit_reach;
    int32_t *front_n, *tile_flag;
    float front_margin;
    int32_t front_min_bucket;
    /* (or NULL) [C*N] floats: the bucket entries (payload) are then each row's POSITION in `order` (the cell-ordered row
     * list) instead of the row, and depth_sorted[position] = depths[row] -- the per-tile sort gathers its keys from a few
     * hundred KB around the tile instead of from all over depths[] (at 5 M Gaussians that gather was most of the sort's time).
     * flatten_ids holds rows either way.  Sorting such a payload by hand: misplat_tile_sort(flags | 4, depths = depth_sorted,
     * isect_gid = order).  Required by front_n. */
    float* depth_sorted;
    /* N-D colours in the one-entry path (a8: rade_features_model.py:427-476), nxq > 0: D' = color_dim composited channels
     * in 5..20, channels 0..3 in the record's colour slots, channels 4.. in featx[C*N, 4*nxq] (nxq = ceil((D' - 4) / 4)).
     *   sh_degree < 0:  colors [(C,)N,D] (D = K_or_D) are the channels (+ depth behind them if depth_channel);
     *   sh_degree >= 0: the model's call as ONE entry -- channels 0..2 = max(SH(colors | colors, colors_rest) + 0.5, 0),
     *                   channels 3.. = features[N, n_feat] (+ depth): no [N,16] concatenation exists anywhere.
     * v_featx_zero (or NULL): gradient rows [C*N, 4*nxq] cleared by the forward, like v_grec_zero.  lazy_colour must be 0. */
    const float* features;
    float *featx, *v_featx_zero;
    int32_t n_feat, nxq;
    int64_t est_isects; /* > 0: the caller's estimate of the intersection count (cap_isects may be a generous, long-lived
                           capacity): picks the per-tile sort's size classes; 0: 4/5 of cap_isects */
} misplat_raster_args;
/* Graph cache (optional, caller-owned, thread-safe; the library itself keeps no state): with a cache, the launch
 * sequence of a call is captured into a hipGraph the first time a given (params, args, phases, stream) block is seen
 * and replayed with one hipGraphLaunch afterwards -- small scenes are launch-bound (~16 launches per forward).  The
 * least recently used of max_entries graphs is evicted.  A cache must not outlive the device context. */
typedef struct misplat_graph_cache misplat_graph_cache;
misplat_graph_cache* misplat_graph_cache_create(int32_t max_entries);
void misplat_graph_cache_destroy(misplat_graph_cache* cache);
int misplat_graph_cache_stats(misplat_graph_cache* cache, int64_t* hits, int64_t* captures);
int misplat_raster_fwd(const misplat_params* p, const misplat_raster_args* a, int32_t phases, misplat_stream_t stream,
                       misplat_graph_cache* cache /* or NULL: plain launches */);
/* The whole backward of rasterization() as ONE host entry: misplat_blend_bwd_atomic, misplat_color_bwd,
 * misplat_project_pack_bwd back to back (arguments as documented there).  zero_flags: see misplat_blend_bwd_atomic;
 * with a cache the sequence is replayed as a graph when it contains no memset (zero_flags covers v_grec and v_abs).
 * With misplat_params.touched, one camera, 16 SH coefficients without sh_aux and >= 262 144 Gaussians the same results
 * come from two launches: the compositing backward, whose grid also clears the seven output tensors, and ONE kernel for
 * both per-Gaussian stages that visits only the flagged rows (v_means_dir is then not written). */
typedef struct misplat_raster_bwd_args {
    /* compositing backward: saved by the forward */
    const float *Ks, *grec;
    const int32_t *flatten_ids, *offsets;
    int64_t n_isects;   /* the number of list entries, or any upper bound inside flatten_ids' buffer (the forward's capacity):
                           every range comes from `offsets`, this only clamps them -- a caller that replays graphs passes the
                           capacity, because the exact count of a scene in training changes with every step */
    const float* alpha;
    const int32_t *last_ids, *median_ids;
    const float* render;
    /* upstream gradients of the five images (all given) */
    const float *v_render, *v_alpha, *v_exp_depth, *v_med_depth, *v_normal;
    float *v_grec, *v_abs /* or NULL */;   /* v_grec is WORKSPACE of this call: in the two-launch form without v_abs its rows hold sums
                                            * the per-Gaussian kernel finishes (slots 0 - 1, 5: csrc/blend.hip MSUM), not the layout of
                                            * misplat_blend_bwd_atomic -- take the mean2d gradient from v_means2d_out */
    const int32_t* unit_perm /* or NULL */;
    int32_t color_dim, zero_flags;
    /* per-Gaussian backward */
    int32_t sh_degree, K_or_D, n_color, per_cam, depth_slot, reserved;
    const float *means, *quats, *scales, *opacities, *colors, *colors_rest, *viewmats;
    const int32_t* radii;
    const float *compensations, *sh_aux /* or NULL */;
    const float* v_means2d /* or NULL: the mean2d gradient is columns 0:2 of v_grec */;
    float *v_colors, *v_colors_rest /* or NULL */, *v_means_dir /* or NULL */, *v_means, *v_quats, *v_scales, *v_opacities;
    /* measurement (or NULL): two hipEvent_t recorded on `stream` directly before and after the compositing backward; a
     * call that carries them is launched plainly (no graph) */
    void *ev_blend_begin, *ev_blend_end;
    /* or NULL: [N,2], the mean2d gradient as a tensor of its own (zeros where no gradient arrived) -- written by the
     * two-launch form only (misplat_raster_bwd_plan bit 0), where v_grec may hold defined values in flagged rows only
     * (misplat_raster_args.lazy_colour = 2) and cannot be sliced for it */
    float* v_means2d_out;
    /* view-keyed launch order: unit_perm is the table base, see misplat_params.unit_sel (or NULL / 0) */
    const int32_t* unit_sel;
    int32_t unit_stride, unit_slots;
    /* N-D colours (nxq > 0; see misplat_raster_args.featx): featx as the forward wrote it, v_featx [C*N, 4*nxq] (zero_flags
     * bit 2: cleared by the forward), depth_channel != 0 if a depth channel rides behind the user channels (its gradient is
     * read from where it sits: record slot or featx); sh_degree >= 0: features [N,n_feat] were the channels 3.. and
     * v_features [N,n_feat] receives their gradient, v_colors (/ v_colors_rest) the SH coefficients'; sh_degree < 0:
     * v_colors [(C,)N,D] receives all of them.  depth_slot is ignored. */
    const float *featx, *features;
    float *v_featx, *v_features;
    int32_t n_feat, nxq, depth_channel, reserved_x;
    /* featx == NULL (the forward ran with on-demand N-D records, misplat_raster_args.lazy_colour with nxq > 0: it wrote no
     * featx): channels 4.. are read from features [N,n_feat] and the depth channel from depths [C*N] */
    const float* depths;
} misplat_raster_bwd_args;
int misplat_raster_bwd(const misplat_params* p, const misplat_raster_bwd_args* b, misplat_stream_t stream,
                       misplat_graph_cache* cache /* or NULL */);
/* Host-only query: what misplat_raster_bwd does with these arguments.  Bit 0: the two-launch form (zeros written in the
 * background of the compositing backward, one kernel for the flagged rows); bit 1: replayable as a graph.  < 0: error. */
int misplat_raster_bwd_plan(const misplat_params* p, const misplat_raster_bwd_args* b);
/* Host-side wait for phase A's count: the caller stores -1 in *n_isects_host before the call; returns the count as
 * soon as the device-to-host copy has landed, or -1 after timeout_us. */
int64_t misplat_wait_count(const volatile int64_t* n_isects_host, int64_t timeout_us);
/* hipMemsetAsync(dst, 0, bytes) on `stream` (used to clear tile_count before phase B is enqueued a second time). */
int misplat_zero_bytes(void* dst, size_t bytes, misplat_stream_t stream);

/* ---- optimiser step --------------------------------------------
 * Fused multi-tensor Adam with torch.optim.Adam semantics (no weight decay, no amsgrad, maximize = False),
 * replacing the six per-group optimisers the reference configures at
 * collab_splats/configs/rade_gs_method.py:44-71 (lr per group, eps = 1e-15):
 *   m = m + (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g^2;
 *   p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * params / grads / exp_avg / exp_avg_sq: HOST arrays of n_tensors device pointers (16-byte aligned, fp32,
 * contiguous); numel, lr, step (t >= 1, already incremented): host arrays.  One launch, in place.
 * beta1 / beta2 / eps are doubles because torch forms 1 - beta and the bias corrections in double. */
#define MISPLAT_ADAM_MAX_TENSORS 8
int misplat_adam_step(int32_t n_tensors, float* const* params, const float* const* grads,
                      float* const* exp_avg, float* const* exp_avg_sq, const int64_t* numel,
                      const float* lr, const int64_t* step, double beta1, double beta2, double eps,
                      misplat_stream_t stream);

/* ---- row-selective Adam (optim.SelectiveAdam): the same step on the rows of an id list only (the Gaussians visible in the
 * step's views); every other row keeps its parameter and both moments bit for bit.  n_tensors (<= 8) row-major tensors of
 * n_rows rows and widths[i] floats per row; ids[ids_cap] (device, ids_cap <= n_rows): ascending row ids, of which the first
 * *count_dev (device, never read on the host) are valid -- union_ids / union_scan below write both.  lr, step (t >= 1, already
 * incremented -- for every tensor, whatever the list holds: torch SparseAdam's convention), beta1 / beta2 / eps as
 * misplat_adam_step; a listed row gets the bits misplat_adam_step gives it.  One launch, no host read, no allocation.
 * visible_rows: flags[r] = 1 where both radii of radii[n_cams][n_rows][2] (int32, 8-byte aligned) are positive for some
 * camera, else 0 -- the flags touched_bits takes. */
int misplat_adam_step_rows(int32_t n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                           float* const* exp_avg_sq, const int32_t* widths, int64_t n_rows, const float* lr,
                           const int64_t* step, double beta1, double beta2, double eps, const int32_t* ids, int64_t ids_cap,
                           const int64_t* count_dev, misplat_stream_t stream);
int misplat_visible_rows(const int32_t* radii, int32_t n_cams, int64_t n_rows, uint8_t* flags, misplat_stream_t stream);

/* ---- shared-Gaussian gradient reduce that moves only the rows that have a gradient (the gradient
 * set of collab_splats/configs/rade_gs_method.py:44-71; csrc/optim.hip, driven by collab_splats_amd/parallel.py).
 *   touched_bits  bits[ceil(n_rows / 8)]: bit (r & 7) of byte r >> 3 = flags[r] != 0 (flags: misplat_params.touched, 8-byte
 *                 aligned) -- the bitmap a rank contributes to the all-gather;
 *   union_count   gathered[world][nbytes] = the ranks' bitmaps; block_counts[ceil(nbytes / 256)] = rows set in the OR of
 *                 them, per block of 2 048 rows;
 *   union_scan    block_offsets[b] = sum of block_counts[0 .. b) (int64), *total = the union's size (one workgroup: the counts
 *                 are a few thousand; the caller reads the total when -- and if -- it needs it on the host);
 *   union_ids     ids[block_offsets[b] ...] = the set rows of block b, ascending: the same list on every rank;
 *   rows_pack     packed[u][W] = the rows ids[u] of n_tensors (<= 8) row-major tensors of `widths` floats per row, side by
 *                 side (W = sum of the widths); rows_unpack: the inverse (rows outside `ids` are not touched). */
#define MISPLAT_ROWS_MAX_TENSORS 8
int misplat_touched_bits(const uint8_t* flags, int64_t n_rows, uint8_t* bits, misplat_stream_t stream);
int misplat_union_count(const uint8_t* gathered, int32_t world, int64_t nbytes, int32_t* block_counts,
                        misplat_stream_t stream);
int misplat_union_scan(const int32_t* block_counts, int64_t n_blocks, int64_t* block_offsets, int64_t* total,
                       misplat_stream_t stream);
int misplat_union_ids(const uint8_t* gathered, int32_t world, int64_t nbytes, const int64_t* block_offsets, int32_t* ids,
                      int64_t ids_cap, misplat_stream_t stream);
/* count_dev (device, or NULL = n_ids): how many of the n_ids slots hold a row, for a caller that sized ids / packed from the
 * previous step's union and reads this step's size only after everything is enqueued: pack writes zeros into the slots behind
 * the count; unpack does NOTHING when the count exceeds n_ids (the caller then reduces the dense buffer instead). */
int misplat_rows_pack(int32_t n_tensors, const float* const* srcs, const int32_t* widths, const int32_t* ids, int64_t n_ids,
                      const int64_t* count_dev, float* packed, misplat_stream_t stream);
int misplat_rows_unpack(int32_t n_tensors, float* const* dsts, const int32_t* widths, const int32_t* ids, int64_t n_ids,
                        const int64_t* count_dev, const float* packed, misplat_stream_t stream);

/* Diagnosis (tests only; csrc/raster.hip): a 16-byte memset node + a kernel captured the way the graph cache captures, replayed
 * n_replays (<= 64) times with the 16 bytes overwritten with garbage in between; out_host[k] = the first counter after replay k
 * (= 1000 + k iff the memset node was applied).  counters16 / add8: device memory (16 / 8 bytes), out_host: host memory. */
int misplat_debug_memset_replay(void* counters16, void* add8, int32_t n_replays, int64_t* out_host, misplat_stream_t stream);

/* Measurement helper: dst[i] = src[i] over n_float4 16-byte elements (a plain streaming copy; bench.py times it to
 * report the HBM roof of the box it runs on).  variant: 0 plain, 1 non-temporal loads / stores, 2 four loads in flight
 * per lane + non-temporal stores, 3 the same with one contiguous piece per workgroup. */
int misplat_stream_copy(const void* src, void* dst, int64_t n_float4, int32_t variant, misplat_stream_t stream);

/* ---- TSDF fusion and marching cubes (csrc/tsdf.hip) ----------------------------------------------
 * Open3D's legacy ScalableTSDFVolume restated in fp32 (the oracle is tests/tsdf_restatement.py; Open3D itself is unpinned).
 * Units of 16^3 voxels; voxel g has its centre at (g + 0.5) voxel_size.  A DENSE unit map over the grid (lo, dims: units,
 * x fastest; at most MISPLAT_TSDF_MAX_UNITS) holds per unit: slot_map (int32 pool slot, -1 unallocated) and words (uint64:
 * bit j = view j of the batch touches the unit; zeroed by the caller before each batch).  pool: per slot 5 planes of 4096
 * fp32 (tsdf, w, r, g, b; colours 0..255), voxel i = lx + 16 ly + 256 lz.  depths [V,H,W] fp32 (<= 0 or > depth_trunc: no
 * data), masks [V,H,W] uint8 or NULL, rgbs [V,H,W,3] fp32 in [0,1] or NULL, viewmats [V,4,4] world->camera (OpenCV),
 * Ks [V,3,3]; V <= MISPLAT_TSDF_MAX_VIEWS. */
#define MISPLAT_TSDF_MAX_VIEWS 64
#define MISPLAT_TSDF_MAX_UNITS (1ll << 26)
typedef struct misplat_tsdf_grid {
    float voxel_size, sdf_trunc, depth_trunc;
    int32_t lo[3];     /* unit coordinate of map entry 0 */
    int32_t dims[3];   /* units per axis */
    int32_t reserved;
} misplat_tsdf_grid;
/* mark: words |= view bits of every unit a sampled pixel's box touches (sampling stride 4). */
int misplat_tsdf_mark(const misplat_tsdf_grid* grid, const float* depths, const uint8_t* masks, int32_t n_views,
                      int32_t height, int32_t width, const float* viewmats, const float* Ks, uint64_t* words,
                      misplat_stream_t stream);
/* alloc: a marked unit without a slot takes slot counters[0]++ (the caller grows the pool to counters[0] slots before
 * integrating); every marked unit is appended to touched ({map index, slot} pairs, capacity = map size) at counters[1]++
 * (counters[1] zeroed by the caller). */
int misplat_tsdf_alloc(const misplat_tsdf_grid* grid, const uint64_t* words, int32_t* slot_map, int32_t* counters,
                       int32_t* touched, misplat_stream_t stream);
/* unit lists (csrc/unitlists.h, exported by csrc/density.hip), for the users that list items per unit
 * (misplat_density_*, misplat_ptsdf_*): their n_pairs (unit map index, item) pairs, emitted while marking words, sorted by
 * unit after alloc, stable (keys and ids are used as scratch): a unit's items keep their order of emission.  ranges [n_units,
 * 2] = the part [begin, end) of ids_sorted that belongs to the unit in pool slot s, written for the units listed only.  Of the
 * grid voxel_size, lo and dims are read.  workspace: misplat_density_workspace(0, n_pairs) = misplat_ptsdf_workspace(0,
 * n_pairs) bytes. */
int misplat_unit_lists(const misplat_tsdf_grid* grid, const int32_t* slot_map, int32_t* keys, int32_t* ids, int64_t n_pairs,
                       int32_t n_units, void* workspace, int64_t workspace_bytes, int32_t* keys_sorted, int32_t* ids_sorted,
                       int32_t* ranges, misplat_stream_t stream);
/* integrate: the batch's views, in view order, into the voxels of the n_touched listed units. */
int misplat_tsdf_integrate(const misplat_tsdf_grid* grid, const int32_t* touched, int32_t n_touched, const uint64_t* words,
                           const float* depths, const uint8_t* masks, const float* rgbs, int32_t n_views, int32_t height,
                           int32_t width, const float* viewmats, const float* Ks, float* pool, misplat_stream_t stream);
/* order: the map indices of the allocated units in ascending map order.  scratch: 2 ceil(map / 4096) + 1 int32. */
int misplat_tsdf_order(const misplat_tsdf_grid* grid, const int32_t* slot_map, int32_t* scratch, int32_t* order,
                       misplat_stream_t stream);
/* mc_count: per voxel of the n_units ordered units, code (uint16: 256 | cube index if the cell is valid) and cnt (uint8: owned
 * vertex mask | triangles << 3), both indexed slot * 4096 + i; unit_counts / unit_offs [2][n_units] = vertices / triangles
 * per unit and their exclusive scans; totals[2] = vertex and triangle counts. */
int misplat_tsdf_mc_count(const misplat_tsdf_grid* grid, const int32_t* slot_map, const int32_t* order, int32_t n_units,
                          const float* pool, uint16_t* code, uint8_t* cnt, int32_t* unit_counts, int32_t* unit_offs,
                          int32_t* totals, misplat_stream_t stream);
/* mc_emit: vertices [M,3], colors [M,3] (0..1), triangles [T,3] int32 in the deterministic order (units in map order, voxels
 * x-fastest, a voxel's vertices +x, +y, +z, triangles in table order).  vert_base: int32 per voxel (scratch). */
int misplat_tsdf_mc_emit(const misplat_tsdf_grid* grid, const int32_t* slot_map, const int32_t* order, int32_t n_units,
                         const float* pool, const uint16_t* code, const uint8_t* cnt, const int32_t* unit_offs,
                         int32_t* vert_base, float* vertices, float* colors, int32_t* triangles, misplat_stream_t stream);

/* ---- kNN mapping of per-point values onto mesh vertices (csrc/meshmap.hip) ---------------------
 * The reference's features2vertex / normals2vertex restated in fp32 (the oracle is tests/meshmap_restatement.py).
 * vertices [M,3], points [N,3], values [N,D] fp32; 1 <= k <= 16, k <= M; every vertex finite with |x| / sdf_trunc
 * < 2^18 per axis (the caller checks it).  Neighbours are ordered by (d2, vertex index), d2 = ((dx dx + dy dy) + dz dz) in
 * fp32, d = sqrtf(d2); a point is valid iff d[0] <= sdf_trunc.  One workspace (bytes from misplat_meshmap_workspace for the
 * largest D the caller will aggregate) serves both calls; nothing in it must survive between them. */
/* workspace bytes for (M, N, k, D); -1 for sizes the library refuses. */
int64_t misplat_meshmap_workspace(int64_t n_vertices, int64_t n_points, int32_t k, int32_t n_channels);
/* knn: idx [N,k] int32 and dist [N,k] fp32 in ascending order, valid [N] uint8; an invalid row holds idx -1, dist +inf. */
int misplat_meshmap_knn(const float* vertices, int64_t n_vertices, const float* points, int64_t n_points, int32_t k,
                        float sdf_trunc, void* workspace, int64_t workspace_bytes, int32_t* idx, float* dist,
                        uint8_t* valid, misplat_stream_t stream);
/* aggregate: out [M,D] = sum w F / sum w over the valid (i, j) with idx = v, weights of DESIGN.md section 15, fp32 sums in
 * ascending (i, j) order (deterministic, no float atomics); 0 without a contribution.  n_unit 3: channels 0..2 are then
 * divided by (their norm + 1e-8); 0: none. */
int misplat_meshmap_aggregate(int64_t n_vertices, int64_t n_points, int32_t k, const int32_t* idx, const float* dist,
                              const uint8_t* valid, const float* values, int32_t n_channels, int32_t n_unit,
                              void* workspace, int64_t workspace_bytes, float* out, misplat_stream_t stream);

/* ---- radius-graph clustering of selected mesh vertices (csrc/cluster.hip) --------------------------
 * The reference's mesh_clustering restated in fp32 (the oracle is tests/meshquery_restatement.py).  vertices [M,3] fp32,
 * mask [M] uint8 (non-zero: selected); every vertex finite with |x| / radius < 2^18 per axis (the caller checks it).
 * Selected vertices i != j are joined iff d2 < r2, d2 = ((dx dx + dy dy) + dz dz) and r2 = radius radius in fp32; clusters are
 * the connected components with MORE than min_cluster_size members, numbered in ascending order of their smallest vertex.
 * Deterministic (integer atomics only); memory O(M). */
/* workspace bytes for M vertices; -1 for sizes the library refuses. */
int64_t misplat_cluster_workspace(int64_t n_vertices);
/* labels [M] int32: the cluster of each vertex, -1 if it is not selected or its component was dropped; sizes (capacity M
 * int32): sizes[c] = members of cluster c for c < n_clusters, the rest is not written; n_clusters: one int32 on the device. */
int misplat_cluster_radius(const float* vertices, int64_t n_vertices, const uint8_t* mask, float radius,
                           int32_t min_cluster_size, void* workspace, int64_t workspace_bytes, int32_t* labels,
                           int32_t* sizes, int32_t* n_clusters, misplat_stream_t stream);

/* ---- point-cloud cleaning (csrc/pointcloud.hip) ----------------------------------------------------
 * points [N,3] and queries [Nq,3] fp32, finite (the caller checks it); queries NULL: the points query themselves (n_queries
 * is then ignored) and a point counts among its own neighbours.  d2 = ((dx dx + dy dy) + dz dz) in fp32.  The oracle is
 * tests/pointcloud_restatement.py.  Deterministic (integer atomics only): two runs are bitwise equal. */
/* workspace bytes for n_points and the call `kind` (0 cells, 1 knn, 2 radius_count, 3 outlier_mask, 4 voxel_group); -1 for
 * sizes the library refuses. */
int64_t misplat_pointcloud_workspace(int64_t n_points, int32_t kind);
/* n_cells (one int32 on the device) = the number of occupied cells of edge `edge`: the occupancy measure the caller tunes
 * the kNN's cell edge with.  |x| / edge < 2^18 per axis. */
int misplat_pointcloud_cells(const float* points, int64_t n_points, float edge, void* workspace, int64_t workspace_bytes,
                             int32_t* n_cells, misplat_stream_t stream);
/* mean [Nq] = (the fp32 sum of sqrtf of the k smallest d2 in ascending order) / float(k), nearest [Nq] = sqrtf of the
 * smallest; 1 <= k <= min(32, N).  No distance cut-off.  edge: the cell edge of the finest of three hash levels (edge, 8 edge,
 * 64 edge), |x| / edge < 2^18 per axis for points and queries; lanes: 1 or 8 lanes per query.  Neither changes a result. */
int misplat_pointcloud_knn(const float* points, int64_t n_points, const float* queries, int64_t n_queries, int32_t k,
                           float edge, int32_t lanes, void* workspace, int64_t workspace_bytes, float* mean, float* nearest,
                           misplat_stream_t stream);
/* counts [Nq] int32 = the number of points with d2 < r2, r2 = radius radius in fp32 (strict).  |x| / radius < 2^18 per axis for
 * the points; a query beyond that range counts 0. */
int misplat_pointcloud_radius_count(const float* points, int64_t n_points, const float* queries, int64_t n_queries,
                                    float radius, void* workspace, int64_t workspace_bytes, int32_t* counts,
                                    misplat_stream_t stream);
/* keep [N] uint8 = avg > 0 and double(avg) < mu + std_ratio sigma, mu and sigma (n - 1 in the denominator) over the positive
 * avg in fp64 in a fixed reduction order; fewer than two positive values: keep = avg > 0. */
int misplat_pointcloud_outlier_mask(const float* avg, int64_t n_points, double std_ratio, void* workspace,
                                    int64_t workspace_bytes, uint8_t* keep, misplat_stream_t stream);
/* Voxel grouping: cell = floor((double(p) - origin) / voxel_size) per axis in fp64, |cell| < 2^20 (the caller checks it).
 * Voxels are numbered in ascending order of their smallest member.  order [N] int32: the points grouped by voxel, ascending
 * inside each; offsets [N + 1] int32: voxel v holds order[offsets[v] .. offsets[v + 1]) for v < n_voxels (one int32 on the
 * device), the entries from n_voxels on hold N. */
int misplat_pointcloud_voxel_group(const float* points, int64_t n_points, double origin_x, double origin_y, double origin_z,
                                   double voxel_size, void* workspace, int64_t workspace_bytes, int32_t* order,
                                   int32_t* offsets, int32_t* n_voxels, misplat_stream_t stream);
/* out [V,D] = per voxel and channel the fp64 sum of values [N,D] over the members in ascending point index, divided by the
 * member count in fp64 and rounded to fp32. */
int misplat_pointcloud_voxel_mean(const float* values, int64_t n_points, int32_t n_channels, const int32_t* order,
                                  const int32_t* offsets, int64_t n_voxels, float* out, misplat_stream_t stream);

/* ---- mesh finishing (csrc/meshclean.hip) -----------------------------------------------------------
 * vertices [M,3] fp32, triangles [T,3] int32 with every index in 0 .. M - 1 (the caller checks it), M < 2^31, T < 2^30; the
 * calls that number corners or edges in int32 (edge_stats, holes) also need 3 T < 2^31.  Every call builds the edge table in
 * its workspace: the undirected edges (lo, hi) of all triangles in a hash of capacity the power of two >= max(64, 6 T); an edge
 * (a, a) of a triangle with a repeated corner is ignored.  The oracle is tests/meshclean_restatement.py.  Deterministic
 * (integer atomics only, fp64 sums in a fixed order): two runs are bitwise equal. */
/* workspace bytes for the call `kind` (0 edge_stats, 1 components, 2 holes, 4 smooth: n_vertices, n_triangles; 3 plane_moments:
 * n_vertices = the number of points, n_triangles ignored); -1 for sizes the library refuses. */
int64_t misplat_meshclean_workspace(int64_t n_vertices, int64_t n_triangles, int32_t kind);
/* counts [3] int32 on the device: undirected edges, boundary edges (exactly one incident (face, corner)), non-manifold edges
 * (more than two); mean_length: one double on the device, the fp64 mean over the undirected edges of the fp32 length
 * sqrtf((dx dx + dy dy) + dz dz), 0 without an edge. */
int misplat_meshclean_edge_stats(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                 void* workspace, int64_t workspace_bytes, int32_t* counts, double* mean_length,
                                 misplat_stream_t stream);
/* Components of the faces under "share an undirected edge", numbered in ascending order of their smallest face: labels [T]
 * int32; sizes (capacity T int32): sizes[c] = faces of component c for c < n_components (one int32 on the device). */
int misplat_meshclean_components(const int32_t* triangles, int64_t n_vertices, int64_t n_triangles, void* workspace,
                                 int64_t workspace_bytes, int32_t* labels, int32_t* sizes, int32_t* n_components,
                                 misplat_stream_t stream);
/* The boundary edges in ascending (face, corner) order, each directed as its face runs: edges (capacity [3 T,2] int32),
 * length (capacity 3 T fp32), loop_of_edge (capacity 3 T int32): loops are the boundary edges connected through shared
 * vertices, numbered in ascending order of their smallest vertex; counts [2] int32 on the device: boundary edges, loops. */
int misplat_meshclean_holes(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                            void* workspace, int64_t workspace_bytes, int32_t* edges, int32_t* loop_of_edge, float* length,
                            int32_t* counts, misplat_stream_t stream);
/* out [L] double: out[l] = the fp64 sum of values[order[e]] over e = offsets[l] .. offsets[l + 1) - 1, in that order. */
int misplat_meshclean_segment_sum(const float* values, const int32_t* order, const int32_t* offsets, int64_t n_segments,
                                  double* out, misplat_stream_t stream);
/* Laplacian smoothing: `iterations` >= 1 rounds, each from the round before: with N(i) the distinct
 * vertices j != i that share a triangle edge with i, in ascending order, and w_ij = 1 / (|x_i - x_j| + 1e-12),
 * x_i' = x_i + lam (sum_j w_ij x_j / sum_j w_ij - x_i); every row of attributes [M, n_channels] (or NULL with 0 channels) takes
 * the same weights; a vertex without a neighbour keeps its row.  fp64 sums in that fixed order, fp32 stores.  The CSR of the
 * neighbours is built once: the 6 T directed edges sorted by (source, target); 6 T < 2^31 - 4096; workspace of kind 4
 * (misplat_meshclean_workspace).  The result lands in vertices_out / attributes_out; vertices_tmp / attributes_tmp (the same
 * shapes; may be NULL with one iteration) hold every other round. */
int misplat_meshclean_smooth(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                             const float* attributes, int32_t n_channels, int32_t iterations, double lam, void* workspace,
                             int64_t workspace_bytes, float* vertices_out, float* attributes_out, float* vertices_tmp,
                             float* attributes_tmp, misplat_stream_t stream);
/* RANSAC hypotheses over points [N,3] fp32, 3 <= N < 2^30, n_planes <= 2^24.  triples_in NULL: hypothesis i takes three
 * distinct indices from a counter-based hash of (seed, i, draw) and writes them to triples_out [H,3]; else it takes
 * triples_in [H,3] (in range: the caller checks it).  planes [H,4] fp32, 16-byte aligned: the unit normal and offset of the
 * plane through the three points, built in fp32 in a fixed order; four NaN for a triple that spans no plane. */
int misplat_meshclean_plane_build(const float* points, int64_t n_points, const int32_t* triples_in, uint32_t seed,
                                  int32_t n_planes, int32_t* triples_out, float* planes, misplat_stream_t stream);
/* counts [H] int32 = the number of points with |((a x + b y) + c z) + d| < threshold in fp32 (strict).  tile: 8, 16 or 32
 * hypotheses per workgroup; it changes no result. */
int misplat_meshclean_plane_count(const float* points, int64_t n_points, const float* planes, int32_t n_planes,
                                  float threshold, int32_t tile, int32_t* counts, misplat_stream_t stream);
/* The inliers of one plane ([4] fp32 on the device) by the same rule: mask [N] uint8, and moments [10] double on the device:
 * n, sum x, sum y, sum z, then the sums of (xx, xy, xz, yy, yz, zz) of the coordinates minus the inliers' mean; fp64, fixed
 * order. */
int misplat_meshclean_plane_moments(const float* points, int64_t n_points, const float* plane, float threshold,
                                    void* workspace, int64_t workspace_bytes, uint8_t* mask, double* moments,
                                    misplat_stream_t stream);

/* ---- quadric-error mesh simplification (csrc/decimate.hip) ---------------------------------------------
 * Edge collapses in rounds over state the caller owns: vertices [M,3] fp32, triangles [T,3] int32 (every index in 0 .. M - 1),
 * alive [T] int32 (1 for a live face; no live face has a repeated corner), quadrics [M,10] fp64, into [M] int32 (-1, or the
 * vertex a dead vertex collapsed into), attributes [M, n_channels] fp32 (or NULL with 0 channels).  1 <= M < 2^31,
 * 1 <= T, 6 T < 2^31 - 4096, n_alive = the number of live faces (>= 1).  The oracle is tests/decimate_restatement.py.
 * Deterministic (integer atomics only, fp64 in a written order): two runs are bitwise equal. */
/* workspace bytes for both calls; -1 for sizes the library refuses. */
int64_t misplat_decimate_workspace(int64_t n_vertices, int64_t n_triangles);
/* One round up to the selection: the CSRs of the live faces, (first != 0) the vertices' quadrics, every edge's target, cost and
 * validity, the two levels of minima, the selected edges (kept in the workspace for misplat_decimate_apply).  counts [3] int32
 * on the device: live faces found (equal to n_alive for a consistent caller), selected edges, the faces their collapses remove. */
int misplat_decimate_round(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                           const int32_t* alive, int64_t n_alive, double* quadrics, int32_t first, void* workspace,
                           int64_t workspace_bytes, int32_t* counts, misplat_stream_t stream);
/* Apply what the round call before it selected (same sizes, same workspace, n_selected = its counts[1]): need < 0 every selected
 * edge, else the shortest prefix in ascending (cost bits, edge key) whose removed faces reach `need`.  The lower end takes the
 * target, 0.5f (x_lo + x_hi) of every attribute and the sum of the quadrics; the higher end dies (into), its corners are rewired,
 * the faces of the edge die (alive). */
int misplat_decimate_apply(float* vertices, int64_t n_vertices, int32_t* triangles, int64_t n_triangles, int32_t* alive,
                           int64_t n_alive, float* attributes, int32_t n_channels, double* quadrics, int32_t* into,
                           int64_t n_selected, int64_t need, void* workspace, int64_t workspace_bytes, misplat_stream_t stream);
/* root [M] int32: the live vertex each vertex ended in (itself if it never collapsed). */
int misplat_decimate_resolve(const int32_t* into, int64_t n_vertices, int32_t* root, misplat_stream_t stream);

/* ---- oriented point clouds from depth and normal maps (csrc/depthcloud.hip) ----------------------------
 * depth [V,H,W] fp32, rgb and normals [V,H,W,3] fp32, masks / valid / edges / candidates [V,H,W] uint8 (non-zero: true),
 * c2w [V,3,4] fp32 (nerfstudio's OpenGL pose), intrinsics [V,4] fp32 (fx, fy, cx, cy); V <= 65535, H W < 2^31.  The oracle is
 * tests/depthcloud_restatement.py.  Every fp32 expression has one written order; integer atomics only: two runs are bitwise
 * equal. */
/* workspace bytes for the call `kind` (0 edges, 1 sample); -1 for sizes the library refuses. */
int64_t misplat_depthcloud_workspace(int64_t n_views, int64_t height, int64_t width, int32_t kind);
/* edges = the pixels with lap > threshold, lap = ((up + left) + (right + down)) - 4 inv of inv = 1 / (d + 1e-6) (0 outside the
 * image), dilated by a square of Chebyshev radius `dilation` (0..63) clipped at the border. */
int misplat_depthcloud_edges(const float* depth, int32_t n_views, int32_t height, int32_t width, float threshold,
                             int32_t dilation, void* workspace, int64_t workspace_bytes, uint8_t* edges,
                             misplat_stream_t stream);
/* candidates = depth > 0 and masks and valid and not edges, over n_pixels = V H W; each of the three may be NULL. */
int misplat_depthcloud_candidates(const float* depth, const uint8_t* masks, const uint8_t* valid, const uint8_t* edges,
                                  int64_t n_pixels, uint8_t* candidates, misplat_stream_t stream);
/* Per frame the min(S, n) candidates with the smallest (key, pixel), key = the 32-bit hash of (seed, frame_offset + v, pixel),
 * or keys [V,H,W] (uint32 bits) when not NULL.  frame_ids / pixel_ids (capacity V min(S, H W) int32): the taken pixels by
 * frame, then pixel; counts [V] int32; frame_base [V + 1] int32: the exclusive scan of counts, frame_base[V] the total.  All
 * on the device. */
int misplat_depthcloud_sample(const uint8_t* candidates, const int32_t* keys, int32_t n_views, int32_t height, int32_t width,
                              int32_t samples_per_frame, uint32_t seed, uint32_t frame_offset, void* workspace,
                              int64_t workspace_bytes, int32_t* frame_ids, int32_t* pixel_ids, int32_t* counts,
                              int32_t* frame_base, misplat_stream_t stream);
/* Per sample (frame v, pixel (u, w) = (pixel % W, pixel / W), depth d): R = c2w[:3,:3] diag(1,-1,-1), x = ((u + 0.5) - cx) d / fx,
 * y likewise, points = ((R0 x + R1 y) + R2 d) + t; out_normals = R n, n = 2 m - 1 with y and z flipped, divided by
 * max(sqrtf((nx nx + ny ny) + nz nz), 1e-12); colors = rgb there.  normals and out_normals: both or neither. */
int misplat_depthcloud_backproject(const float* depth, const float* rgb, const float* normals, const float* c2w,
                                   const float* intrinsics, int32_t n_views, int32_t height, int32_t width,
                                   const int32_t* frame_ids, const int32_t* pixel_ids, int64_t n_samples, float* points,
                                   float* out_normals, float* colors, misplat_stream_t stream);
/* keep [N] uint8 = no view drops the centre: per view c = (p - t) @ R, a centre with c.z <= 0 is not tested, iu = floorf((c.x fx /
 * c.z + cx) - 0.5) (iv likewise), dropped iff 0 < iu < W, 0 < iv < H and masks is 0 there. */
int misplat_depthcloud_gaussian_filter(const float* means, int64_t n_gauss, const float* c2w, const float* intrinsics,
                                       const uint8_t* masks, int32_t n_views, int32_t height, int32_t width, uint8_t* keep,
                                       misplat_stream_t stream);

/* ---- dense-grid screened Poisson surface reconstruction (csrc/poisson.hip) ---------------------------
 * A restated uniform-grid solve, neither Kazhdan's adaptive octree nor Open3D's code (the oracle is
 * tests/poisson_restatement.py; Open3D itself is unpinned).  G = 2^depth cells per axis, MISPLAT_POISSON_MIN_DEPTH <= depth <=
 * MISPLAT_POISSON_MAX_DEPTH; cell (i, j, k) has its centre at origin + (idx + 0.5) h and the linear index i + G (j + G k).  Every
 * grid is dense over G^3 cells; the fp32 grids are 16-byte aligned.  One workspace (bytes from misplat_poisson_workspace) serves
 * every call; its first 8 doubles are the solver's state {r.z, p.Ap, r.r, b.b, alpha, beta, done (0 running, 1 converged, 2
 * iteration cap, 3 p.Ap or r.z was 0), iterations} and must survive from cg_init to the last cg_iterate.  Every fp32 expression
 * of the splat, the system and the sampler has one written order; integer atomics only and fixed-shape reductions: two runs are
 * bitwise equal. */
#define MISPLAT_POISSON_MIN_DEPTH 4
#define MISPLAT_POISSON_MAX_DEPTH 9
/* workspace bytes for (depth, n_points: the most values misplat_poisson_mean will see); -1 for sizes the library refuses. */
int64_t misplat_poisson_workspace(int32_t depth, int64_t n_points);
/* splat: per point g = (p - origin) / h - 0.5, i0 = floor(g), f = g - i0; each of the 8 surrounding cells (indices clamped to the
 * grid) takes w = (wx wy) wz: w_grid += w, v_grid[a] += w n_a, c_grid[c] += w c_c, each as llrint(x 2^30) added with 64-bit integer
 * atomics.  w_grid [G^3], v_grid and c_grid [3][G^3] int64, zeroed here; colors and c_grid may be NULL together. */
int misplat_poisson_splat(const float* points, const float* normals, const float* colors, int64_t n_points, int32_t depth,
                          float origin_x, float origin_y, float origin_z, float h, int64_t* w_grid, int64_t* v_grid,
                          int64_t* c_grid, misplat_stream_t stream);
/* system: w = float(w_grid) 2^-30; d = float(in-grid neighbours) + (point_weight w) / wbar, wbar = float((double(sum w_grid) 2^-30)
 * / double(cells with w_grid > 0)); b = -0.5 ((dVx + dVy) + dVz), dV_a = V_a(i + e_a) - V_a(i - e_a), V = float(v_grid) 2^-30 and 0
 * outside the grid. */
int misplat_poisson_system(const int64_t* w_grid, const int64_t* v_grid, int32_t depth, float point_weight, void* workspace,
                           int64_t workspace_bytes, float* w, float* b, float* d, misplat_stream_t stream);
/* Jacobi-preconditioned conjugate gradients on (A x)(i) = d(i) x(i) - sum of the in-grid neighbours of x.  cg_init: x = 0, r = b,
 * z = r / d, p = z and the state.  cg_iterate: n_iters (<= 4096) iterations of {ap = A p, alpha; x += alpha p, r -= alpha ap, z = r /
 * d, beta; p = z + beta p}; alpha, beta and the done flag stay on the device, and once done is set (r.r <= tol^2 b.b, max_iters
 * reached, p.Ap or r.z zero) every kernel is a no-op, so overshooting is harmless.  The caller reads the state when it likes. */
int misplat_poisson_cg_init(const float* b, const float* d, int32_t depth, int32_t max_iters, void* workspace,
                            int64_t workspace_bytes, float* x, float* r, float* z, float* p, misplat_stream_t stream);
int misplat_poisson_cg_iterate(const float* d, int32_t depth, int32_t n_iters, double tol, int32_t max_iters, void* workspace,
                               int64_t workspace_bytes, float* x, float* r, float* z, float* p, float* ap,
                               misplat_stream_t stream);
/* sample: out [Nq, n_channels] = the trilinear value of field [n_channels][G^3] (cell-centred) at queries [Nq,3]: g as in splat, i0
 * clamped to 0 .. G - 2 and f to [0, 1]; v0 (1 - f) + v1 f along x, then y, then z.  1 <= n_channels <= 16. */
int misplat_poisson_sample(const float* field, int32_t n_channels, int32_t depth, float origin_x, float origin_y, float origin_z,
                           float h, const float* queries, int64_t n_queries, float* out, misplat_stream_t stream);
/* mean (one double on the device) = the fp64 sum of values [n] in a fixed two-level order, divided by n. */
int misplat_poisson_mean(const float* values, int64_t n, void* workspace, int64_t workspace_bytes, double* mean,
                         misplat_stream_t stream);
/* mc_pool: pool (5 G^3 fp32) = chi - iso as a fully allocated misplat_tsdf unit map: unit u = ux + U (uy + U uz), U = G / 16, in
 * slot u; plane 0 chi - iso, plane 1 (weight) 1, planes 2..4 (colour) 0.  misplat_tsdf_mc_count / _emit extract it with
 * voxel_size 1, lo 0, dims U, slot_map[u] = order[u] = u; a vertex v maps to origin + v h. */
int misplat_poisson_mc_pool(const float* chi, int32_t depth, float iso, float* pool, misplat_stream_t stream);

/* ---- Gaussian grouping: mask front sets and cross-view label banks (csrc/grouping.hip) ----------------
 * The oracle is tests/grouping_restatement.py; everything compared is an integer.  n_gauss < 2^31, width height < 2^31, mask
 * [H,W] int32 with ids 0..65535 (0: background; other values count as background), 1 <= num_patches <= 128, n_masks n_labels <=
 * 2^26.  Integer atomics only: two runs are bitwise equal.  No call reads anything back.
 * One workspace (bytes from misplat_grouping_workspace) serves every call; misplat_grouping_mask_ids leaves the id -> rank table
 * of its mask image at the front of it, which misplat_grouping_front and misplat_grouping_relabel read. */
/* workspace bytes for n_gauss Gaussians; -1 for sizes the library refuses. */
int64_t misplat_grouping_workspace(int64_t n_gauss);
/* radii [N,2] int32, means2d [N,2] fp32 of one camera: valid = any(radii > 1); flat = x + y W of the pixel rintf(mean) (half to
 * even) clamped to the image (a NaN lands on 0). */
int misplat_grouping_project(const int32_t* radii, const float* means2d, int64_t n_gauss, int32_t width, int32_t height,
                             int32_t* flat, uint8_t* valid, misplat_stream_t stream);
/* mask_ids (capacity 65535) = the positive ids present in mask, ascending; n_masks [1] = their number M.  On the device. */
int misplat_grouping_mask_ids(const int32_t* mask, int64_t n_pixels, void* workspace, int64_t workspace_bytes, int32_t* mask_ids,
                              int32_t* n_masks, misplat_stream_t stream);
/* mask_of [N] = the rank m of the mask a Gaussian is selected for, -1 for the others; counts [n_masks] = the set sizes.  A valid
 * Gaussian on a pixel of mask m is in the cell (m, min(y / ceil(H / P), P - 1), min(x / ceil(W / P), P - 1)); a cell of n keeps its
 * max((int64)(front_percentage n), 1) smallest by (depth, id), the product in double.  n_masks: what misplat_grouping_mask_ids
 * found for this mask with this workspace.  0 < front_percentage <= 1. */
int misplat_grouping_front(const int32_t* flat, const uint8_t* valid, const float* depths, int64_t n_gauss, const int32_t* mask,
                           int32_t width, int32_t height, int32_t num_patches, int32_t n_masks, double front_percentage,
                           void* workspace, int64_t workspace_bytes, int32_t* mask_of, int32_t* counts, misplat_stream_t stream);
/* out [n_pixels] = labels[rank of the pixel's id] + 1, 0 on background; labels [M] int64, the table as _front. */
int misplat_grouping_relabel(const int32_t* mask, int64_t n_pixels, const void* workspace, int64_t workspace_bytes,
                             const int64_t* labels, int32_t* out, misplat_stream_t stream);
/* The bank: per Gaussian the ascending list of its labels, bank_labels[bank_off[g] .. bank_off[g + 1]).
 * overlap: count [n_masks, n_labels] int32 (zeroed here) = the Gaussians with mask_of = m that carry label l. */
int misplat_grouping_overlap(const int32_t* mask_of, int64_t n_gauss, const int32_t* bank_off, const int32_t* bank_labels,
                             int32_t n_masks, int32_t n_labels, int32_t* count, misplat_stream_t stream);
/* labels [n_masks] int64: with n_labels = 0 the masks' own ranks; otherwise per mask the lowest label of maximal q =
 * float(count / (set_size + count + 1e-8)) (the quotient in double), or, when q < iou_threshold (fp32), the next new label,
 * numbered from n_labels in mask order.  n_new [1] = the number of new labels.  One workgroup. */
int misplat_grouping_assign(const int32_t* count, const int32_t* set_sizes, int32_t n_masks, int32_t n_labels, float iou_threshold,
                            int64_t* labels, int32_t* n_new, misplat_stream_t stream);
/* Every Gaussian with mask_of = m >= 0 gets labels[m] inserted into its list if absent.  merge_count: new_off [N + 1] = the
 * offsets of the merged lists (new_off[N]: the new number of pairs, which must stay < 2^31); merge_copy: the merged lists into
 * new_labels (capacity new_capacity >= new_off[N]) and sizes [n_labels_new] int32 += the Gaussians each label gained. */
int misplat_grouping_merge_count(const int32_t* mask_of, int64_t n_gauss, const int64_t* labels, int32_t n_masks,
                                 const int32_t* bank_off, const int32_t* bank_labels, void* workspace, int64_t workspace_bytes,
                                 int32_t* new_off, misplat_stream_t stream);
int misplat_grouping_merge_copy(const int32_t* mask_of, int64_t n_gauss, const int64_t* labels, int32_t n_masks,
                                const int32_t* bank_off, const int32_t* bank_labels, const int32_t* new_off, int64_t new_capacity,
                                int32_t* new_labels, int32_t* sizes, int32_t n_labels_new, misplat_stream_t stream);
/* flags [N] uint8 = the Gaussian carries `label`. */
int misplat_grouping_members(const int32_t* bank_off, const int32_t* bank_labels, int64_t n_gauss, int32_t label, uint8_t* flags,
                             misplat_stream_t stream);

/* ---- bilateral-grid colour correction of a training view and the grids' total-variation loss (the reference's call sites
 * rade_gs_model.py:231-234, :284-289; the operation is nerfstudio's, restated from the published method, DESIGN.md section
 * 24): csrc/bilagrid.hip.  grids [num, 12, L, GH, GW] fp32, channel 4 c + j = entry (c, j) of a 3 x 4 affine; per pixel
 *   x = px / (W - 1), y = py / (H - 1) (0 for a single column / row), z = 0.299 r + 0.587 g + 0.114 b (fp32, left to right),
 *   A = trilinear(grid at (z (L - 1), y (GH - 1), x (GW - 1))), border-clamped, in lerp form a + t (b - a) along x, y, z,
 *   out_c = A[c,0] r + A[c,1] g + A[c,2] b + A[c,3] (not clamped).
 * Limits: 1 <= GW, GH <= MISPLAT_BILAGRID_MAX_XY, 1 <= L <= MISPLAT_BILAGRID_MAX_L, 1 <= H, W <= 32768.  No atomics, every
 * sum in a fixed order: reproducible bit for bit.  No call synchronises. */
#define MISPLAT_BILAGRID_MAX_XY 256
#define MISPLAT_BILAGRID_MAX_L 16
#define MISPLAT_BILAGRID_TV_BLOCKS 1024  /* misplat_bilagrid_tv_fwd's partials: 3 * this many doubles */
/* floats of scratch misplat_bilagrid_slice_bwd needs; -1 for sizes outside the limits. */
int64_t misplat_bilagrid_scratch_floats(int32_t height, int32_t width, int32_t grid_w, int32_t grid_h, int32_t grid_l);
/* rgb, out [H, W, 3]; grid: ONE camera's [12, L, GH, GW].  One launch. */
int misplat_bilagrid_slice_fwd(int32_t height, int32_t width, const float* rgb, const float* grid, int32_t grid_w, int32_t grid_h,
                               int32_t grid_l, float* out, misplat_stream_t stream);
/* grids, v_grids: ALL cameras' [num, 12, L, GH, GW]; v_grids is written whole (camera `cam`: the gradient, the others: 0);
 * v_rgb [H, W, 3] includes the path through z: the slope of the interval floor(gz), 0 where gz <= 0 or gz >= L - 1.  A and the
 * slope are recomputed from rgb and the grid.  Three launches. */
int misplat_bilagrid_slice_bwd(int32_t height, int32_t width, const float* rgb, const float* grids, int32_t num, int32_t cam,
                               int32_t grid_w, int32_t grid_h, int32_t grid_l, const float* v_out, float* v_rgb, float* v_grids,
                               float* scratch, misplat_stream_t stream);
/* loss [1] = (1 / num) sum over the axes GW, GH, L of sum (G[i + 1] - G[i])^2 / (12 (n_axis - 1) (the other two sizes)); an
 * axis of size 1 adds 0.  Partial sums in fp64, met in index order.  Two launches. */
int misplat_bilagrid_tv_fwd(const float* grids, int32_t num, int32_t grid_w, int32_t grid_h, int32_t grid_l, double* partials,
                            float* loss, misplat_stream_t stream);
/* v_grids = v_loss[0] * d loss / d grids (v_loss: DEVICE scalar).  One launch. */
int misplat_bilagrid_tv_bwd(const float* grids, int32_t num, int32_t grid_w, int32_t grid_h, int32_t grid_l, const float* v_loss,
                            float* v_grids, misplat_stream_t stream);

/* ---- the Gaussian mixture's own density on the TSDF lattice, and its level sets (csrc/density.hip) ----
 * Restated from the published definition (SuGaR's density); the oracle is tests/density_restatement.py.  means [N,3], quats
 * [N,4] (wxyz, normalised inside), scales [N,3] > 0 and opacities [N] in [0,1], both ACTIVATED; 0 < cutoff r <= 6.  A Gaussian
 * with opacity < min_opacity, a non-finite parameter, a non-positive scale or a zero quaternion takes no part.  With R = R(q)
 * (columns e_a), A = diag(1 / s) R^T and m(x) = |A (x - mu)|^2:
 *   k_g(x) = o_g (exp(-m_g / 2) - exp(-r^2 / 2)) where m_g < r^2, else 0 (continuous at the cut-off);  d(x) = sum_g k_g(x).
 * Lattice, unit map and pool are misplat_tsdf's (voxel g centred at (g + 0.5) voxel_size, units of 16^3, 5 planes of 4096 fp32
 * per slot): of the grid only voxel_size, lo and dims are read.  A Gaussian is listed in a unit by a conservative fp32 test in
 * a fixed operation order (density.hip's head states it): the integer structures equal the restatement's bit for bit.
 * Order of calls: records; count (the host reads n_pairs); emit into zeroed words; misplat_tsdf_alloc (slot_map all -1,
 * counters zero: touched then lists the n_units allocated units); misplat_unit_lists (every unit's list is then ascending in
 * g); accumulate; then query and misplat_tsdf_mc_* at will. */
#define MISPLAT_DENSITY_REC 16          /* floats per record: mu[3], A[9] row-major, o, E[3] (E = -1: takes no part) */
#define MISPLAT_DENSITY_BATCH 64        /* records accumulate stages in LDS at a time */
#define MISPLAT_DENSITY_MAX_CHANNELS 16 /* channels of query's values */
/* workspace bytes that serve count (n_pairs = 0) or misplat_unit_lists (n_gauss = 0); -1 for sizes the library refuses
 * (n_gauss, n_pairs < 2^31). */
int64_t misplat_density_workspace(int64_t n_gauss, int64_t n_pairs);
/* records [N,16] (16-byte aligned); E_i = r sqrt(sum_a (R[i][a] s_a)^2), the half sides of the support's AABB. */
int misplat_density_records(const float* means, const float* quats, const float* scales, const float* opacities,
                            int64_t n_gauss, float cutoff, float min_opacity, float* records, misplat_stream_t stream);
/* count: pair_off [N + 1] = the exclusive scan of the (unit, Gaussian) pairs per Gaussian; n_pairs: DEVICE int64, their number
 * (exact also where the int32 scan has overflowed: the caller refuses >= 2^31 - 4096). */
int misplat_density_count(const misplat_tsdf_grid* grid, const float* means, const float* quats, const float* scales,
                          const float* opacities, int64_t n_gauss, float cutoff, float min_opacity, void* workspace,
                          int64_t workspace_bytes, int32_t* pair_off, int64_t* n_pairs, misplat_stream_t stream);
/* emit: keys / ids [n_pairs] = (unit map index, Gaussian) from pair_off[g] on, a Gaussian's units in ascending map order;
 * words[unit] = 1 for every unit listed (misplat_tsdf_alloc's input; zeroed by the caller). */
int misplat_density_emit(const misplat_tsdf_grid* grid, const float* means, const float* quats, const float* scales,
                         const float* opacities, int64_t n_gauss, float cutoff, float min_opacity, const int32_t* pair_off,
                         int64_t n_pairs, int32_t* keys, int32_t* ids, uint64_t* words, misplat_stream_t stream);
/* accumulate: plane 0 of every listed unit = d at its voxel centres, terms added in list order (two runs are bitwise equal);
 * plane 1 = 1, planes 2..4 = 0.  touched: misplat_tsdf_alloc's {map index, slot} pairs.  flags bit 0: no sub-brick skipping (by
 * default a wave passes over a record whose slabs miss its 8 x 8 x 16 brick). */
int misplat_density_accumulate(const misplat_tsdf_grid* grid, const int32_t* touched, int32_t n_units, const float* records,
                               const int32_t* ids_sorted, const int32_t* ranges, float cutoff, int32_t flags, float* pool,
                               misplat_stream_t stream);
/* query: at points [P,3], from the list of the unit that holds the point's voxel floor(p / voxel_size): density [P], grad
 * [P,3], dominant [P] (the g of the largest term, the lowest at a tie; -1 where d = 0), values_out [P,D] = sum k_g values[g] /
 * d (0 where d = 0) for values [N,D], 1 <= D <= 16; any output may be NULL (values and values_out go together).  A point
 * outside the map or in an unallocated unit gives 0 / 0 / -1 / 0. */
int misplat_density_query(const misplat_tsdf_grid* grid, const int32_t* slot_map, const float* records, const int32_t* ids_sorted,
                          const int32_t* ranges, float cutoff, const float* points, int64_t n_points, const float* values,
                          int32_t n_channels, float* density, float* grad, int32_t* dominant, float* values_out,
                          misplat_stream_t stream);
/* raycast: per ray (origins, dirs [M,3], used as given; t0, t1 [M]) and level (1 <= n_levels <= 4, each
 * finite and > 0, passed by value; the levels beyond n_levels are ignored) the first crossing of d from below the level to at
 * or above it, front to back: 64 samples over [t0, t1], per level 64 more over its bracket, then linear interpolation; d at a
 * sample is bit for bit what query gives there.  t_out [n_levels, M] fp32 and hit_out [n_levels, M] uint8 (0 / 0 for a miss,
 * and for a ray with a non-finite input or t1 <= t0).  One launch, one wave per ray. */
int misplat_density_raycast(const misplat_tsdf_grid* grid, const int32_t* slot_map, const float* records, const int32_t* ids_sorted,
                            const int32_t* ranges, float cutoff, const float* origins, const float* dirs, const float* t0,
                            const float* t1, int64_t n_rays, float level0, float level1, float level2, float level3,
                            int32_t n_levels, float* t_out, uint8_t* hit_out, misplat_stream_t stream);

/* ---- TSDF fusion of point clouds with origins, with space carving (csrc/pointtsdf.hip) ----
 * What the reference's TSDFFusion asks of vdbfusion's VDBVolume::Integrate, restated (the oracle is
 * tests/pointtsdf_restatement.py; vdbfusion itself is unpinned).  Lattice, unit map, words and slots are misplat_tsdf's; of the
 * grid voxel_size, sdf_trunc, lo and dims are read.  points [N,3] fp32; origins [3] (origin_stride 0) or [N,3] (origin_stride
 * 3).  Per ray o -> p, in fp32 in the order pointtsdf.hip's head states: a voxel walk from floor(o / h) (space_carving) or from
 * the voxel at L - sdf_trunc to L + sdf_trunc; per visited voxel with sdf > -sdf_trunc: sum_q += rint(min(sdf_trunc, sdf) /
 * sdf_trunc * 16384), count += 1; where |sdf| < sdf_trunc: rgb_sum += uint8(rgb 255), rgb_count += 1.  Planes per slot: sum_q
 * [4096] int64, count [4096] int32, rgb_sum [3][4096] int32, rgb_count [4096] int32 (112 KiB a unit), voxel i = lx + 16 ly +
 * 256 lz, zeroed by the caller when a slot is new.  Integer sums: the planes depend on no order of rays or calls.  A ray with a
 * non-finite coordinate, zero length or a coordinate at or beyond 2^22 voxels is skipped; a ray is walked only inside the map.
 * Order of calls per chunk of rays: count (the host reads n_pairs); emit into zeroed words; misplat_tsdf_alloc (the host reads
 * its counters and grows the planes); misplat_unit_lists; accumulate.  Then finalize and misplat_tsdf_mc_* at will. */
/* workspace bytes that serve count (n_pairs = 0), accumulate (n_rays = its n_touched, n_pairs = 0) or misplat_unit_lists
 * (n_rays = 0); -1 for sizes the library refuses (both < 2^31). */
int64_t misplat_ptsdf_workspace(int64_t n_rays, int64_t n_pairs);
/* count: pair_off [N + 1] = the exclusive scan of the units each ray passes inside the map; n_pairs: DEVICE int64, their
 * number. */
int misplat_ptsdf_count(const misplat_tsdf_grid* grid, const float* points, const float* origins, int32_t origin_stride,
                        int64_t n_rays, int32_t space_carving, void* workspace, int64_t workspace_bytes, int32_t* pair_off,
                        int64_t* n_pairs, misplat_stream_t stream);
/* emit: keys / ids [n_pairs] = (unit map index, ray) from pair_off[ray] on, in walk order; words[unit] = 1 for every unit
 * listed. */
int misplat_ptsdf_emit(const misplat_tsdf_grid* grid, const float* points, const float* origins, int32_t origin_stride,
                       int64_t n_rays, int32_t space_carving, const int32_t* pair_off, int64_t n_pairs, int32_t* keys, int32_t* ids,
                       uint64_t* words, misplat_stream_t stream);
/* accumulate: the n_pairs listed rays into the planes of the n_touched units of touched (misplat_tsdf_alloc's {map index,
 * slot} pairs), one workgroup per 8192 rays of a unit's list.  colors [N,3] fp32 in [0,1], or NULL (black).  workspace:
 * misplat_ptsdf_workspace(n_touched, 0) bytes. */
int misplat_ptsdf_accumulate(const misplat_tsdf_grid* grid, const int32_t* touched, int32_t n_touched, const float* points,
                             const float* origins, int32_t origin_stride, const float* colors, int32_t space_carving,
                             const int32_t* ids_sorted, const int32_t* ranges, int64_t n_pairs, void* workspace,
                             int64_t workspace_bytes, int64_t* sum_q, int32_t* count, int32_t* rgb_sum, int32_t* rgb_count,
                             misplat_stream_t stream);
/* finalize: pool [n_units, 5, 4096] fp32 of misplat_tsdf_mc_*: tsdf = (float)((double)sum_q / (double)count) / 16384 (in units
 * of sdf_trunc; 0 where count = 0), w = count >= min_weight ? count : 0, colours = rgb_sum / rgb_count in 0..255 (0 where
 * rgb_count = 0). */
int misplat_ptsdf_finalize(int32_t n_units, const int64_t* sum_q, const int32_t* count, const int32_t* rgb_sum,
                           const int32_t* rgb_count, int32_t min_weight, float* pool, misplat_stream_t stream);

/* ---- hole patches at the mesh's resolution: subdivision and fairing (csrc/meshfill.hip) ----
 * Restated from the published methods (longest-edge bisection, membrane fairing with the rim fixed); the oracle is
 * tests/meshfill_restatement.py.  vertices [M,3] fp32, triangles [T,3] int32 with every index in 0 .. M - 1.  Integer atomics
 * only, every fp64 sum in a fixed order: two runs are bitwise equal.  No call synchronises.
 *
 * Subdivision.  An undirected edge is splittable iff it has one incident face or two distinct ones, all with region != 0 and
 * three distinct corners, and its fp32 length sqrtf((dx dx + dy dy) + dz dz) > max_edge_len.  Priority: larger length bits, then
 * smaller mix32(lo, hi, 0), then smaller key lo << 32 | hi.  A round selects the splittable edges that are first among the
 * splittable edges of each of their faces.  1 <= T, 6 T < 2^31 - 4096. */
/* workspace bytes for round and apply at n_triangles faces (both carve it for the T they are given); -1 for sizes refused. */
int64_t misplat_meshfill_workspace(int64_t n_vertices, int64_t n_triangles);
/* One round up to the selection (kept in the workspace for misplat_meshfill_apply).  region [T] uint8.  counts [2] int32 on the
 * device: the selected edges, the faces they split. */
int misplat_meshfill_round(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                           const uint8_t* region, float max_edge_len, void* workspace, int64_t workspace_bytes, int32_t* counts,
                           misplat_stream_t stream);
/* Applies the round: limit < 0 every selected edge (n_selected of them), else the `limit` first in priority (counts is written
 * again for them).  Edge number s (a scan over the (face, corner) slots, each edge at the lowest corner of its smallest face)
 * creates vertex M + s = 0.5f (x_lo + x_hi), every attribute channel ([., n_channels]) the same; a split face (a, b, c), a -> b
 * the edge, becomes (a, m, c) in its slot and (m, b, c) in slot T + its rank among the split faces, which inherits region and
 * origin.  vertices / attributes need M + (the edges applied) rows, triangles / region / origin T + (the faces split). */
int misplat_meshfill_apply(float* vertices, int64_t n_vertices, int32_t* triangles, int64_t n_triangles, uint8_t* region,
                           int32_t* origin, float* attributes, int32_t n_channels, int64_t n_selected, int64_t limit,
                           void* workspace, int64_t workspace_bytes, int32_t* counts, misplat_stream_t stream);
/* Fairing.  free [M] uint8; a patch = free vertices connected by edges with both ends free, numbered by smallest vertex.  Per
 * iteration a free vertex moves to fp32(sum_j (double) x_j / |N(i)|) over its distinct neighbours in ascending index; a patch
 * stops after the first iteration whose largest |x' - x| (fp32, over its vertices and channels) is < tolerance.  Order of
 * calls: count (the host reads counts[0] = n_free and counts[1] = n_edges, the directed edges that leave a free vertex); build
 * (counts[2] = the patches; iterations [n_free] int32, one entry per patch, starts at 0); lds and / or step; finish.  counts [4]
 * int32 on the device.  A patch of more than MISPLAT_MESHFILL_LDS_VERTICES free vertices is left to step. */
#define MISPLAT_MESHFILL_LDS_VERTICES 4096
/* workspace bytes (count: n_free = n_edges = 0); -1 for sizes refused (6 T < 2^31 - 4096). */
int64_t misplat_meshfill_fair_workspace(int64_t n_vertices, int64_t n_triangles, int64_t n_free, int64_t n_edges);
int misplat_meshfill_fair_count(const int32_t* triangles, int64_t n_triangles, const uint8_t* free, int64_t n_vertices,
                                void* workspace, int64_t workspace_bytes, int32_t* counts, misplat_stream_t stream);
int misplat_meshfill_fair_build(const int32_t* triangles, int64_t n_triangles, const uint8_t* free, int64_t n_vertices,
                                int64_t n_free, int64_t n_edges, void* workspace, int64_t workspace_bytes, int32_t* iterations,
                                int32_t* counts, misplat_stream_t stream);
/* Iterations first .. first + count - 1 (1-based) of values [M, n_channels], one launch each: an odd iteration reads values_a
 * and writes values_b, an even one the other way (both hold the fixed rows; a stopped patch is copied).  fixed = 0: measured
 * (iterations[p] is set when patch p is seen to have stopped; counts[3] = the patches still running after the last one);
 * fixed != 0: patch p runs iff the iteration is <= iterations[p] (attributes). */
int misplat_meshfill_fair_step(float* values_a, float* values_b, int64_t n_vertices, int64_t n_triangles, int32_t n_channels,
                               int64_t n_free, int64_t n_edges, int32_t first, int32_t count, float tolerance, int32_t fixed,
                               void* workspace, int64_t workspace_bytes, int32_t* iterations, int32_t* counts,
                               misplat_stream_t stream);
/* Every patch that fits, to its end in ONE workgroup (both iterates of its xyz in LDS), in place in vertices; iterations[p] is
 * set for them; counts[3] = the patches that do not fit.  Same bits and counts as step. */
int misplat_meshfill_fair_lds(float* vertices, int64_t n_vertices, int64_t n_triangles, int64_t n_free, int64_t n_edges,
                              int32_t n_patches, float tolerance, int32_t max_iterations, void* workspace, int64_t workspace_bytes,
                              int32_t* iterations, int32_t* counts, misplat_stream_t stream);
/* iterations[p] = n_done for every patch that was never seen stopped. */
int misplat_meshfill_fair_finish(int64_t n_free, int32_t n_done, int32_t* iterations, const int32_t* counts,
                                 misplat_stream_t stream);

/* Curvature (thin-plate) fairing (the oracle is tests/meshsmooth_restatement.py, bit for bit).  N(i) the
 * distinct edge-neighbours of vertex i in ascending order, n_i their number; F the free vertices, R the fixed vertices with a
 * free neighbour, S = F + R.  U_i(x) = (sum_{j in N(i)} x_j) / (double) n_i - x_i in fp64; the energy sum_{i in S} |U_i|^2 is
 * minimised over the free coordinates by plain conjugate gradients on A = L^T L, one independent CG per coordinate, all fp64,
 * from the fp32 positions, rounded to fp32 once.  A patch is a connected set of free vertices, two being connected when they
 * are adjacent or share a neighbour in R. */
#define MISPLAT_MESHFILL_CG_VERTICES 65536
/* The components that make the patches: (src [E], tgt [E]) the directed edges that leave a vertex of S; every edge whose target
 * is free unites its ends in parent [M] int32 (parent[v] = v on entry); root [M] int32 = every vertex's smallest member. */
int misplat_meshfill_curv_patches(const int32_t* src, const int32_t* tgt, int64_t n_edges, const uint8_t* free, int64_t n_vertices,
                                  int32_t* parent, int32_t* root, misplat_stream_t stream);
/* workspace bytes of curv_solve: x, r, p, q over the n_free free places, t and t / n over the n_rows places of S; -1 refused. */
int64_t misplat_meshfill_curv_workspace(int64_t n_free, int64_t n_rows);
/* One persistent workgroup of 1024 threads per patch, for the whole solve.  The S-list: places 0 .. n_free - 1 the free
 * vertices by patch and then by vertex (patch p: free_offset[p] .. free_offset[p + 1]), places n_free .. n_rows - 1 the rows of
 * R the same way (patch p: n_free + rim_offset[p] ..).  vertex [n_rows]: the place's vertex; row / degree [n_rows]: where its
 * distinct neighbours start in neighbour / place [n_entries] (as vertices, and as places with -1 for a vertex outside S), and
 * how many they are.  code [P]: 0 solve, else leave unchanged (1 no neighbour, 2 no fixed neighbour, 3 more than
 * MISPLAT_MESHFILL_CG_VERTICES free vertices).  Every dot product: thread t adds the patch's elements t, t + 1024, ... in
 * ascending order, then wgprims.h's block_sum.  A column whose p.q is 0 takes alpha = beta = 0.  After iteration k the patch
 * stops iff sum_c r_c.r_c <= rtol^2 sum_c r0_c.r0_c (0 iterations if the right-hand side is 0), or at max_iterations (< 0: the
 * patch's free count).  out [M,3] holds the input's positions on entry; the free vertices of a patch that iterated are
 * written.  iterations [P] int32, converged [P] uint8, residual [P] fp64 = sqrt of the final ratio. */
int misplat_meshfill_curv_solve(const float* vertices, float* out, int64_t n_vertices, const int32_t* free_offset,
                                const int32_t* rim_offset, const int32_t* vertex, const int32_t* row, const int32_t* degree,
                                const int32_t* neighbour, const int32_t* place, int64_t n_free, int64_t n_rows, int64_t n_entries,
                                const int32_t* code, int32_t n_patches, double rtol, int32_t max_iterations, void* workspace,
                                int64_t workspace_bytes, int32_t* iterations, uint8_t* converged, double* residual,
                                misplat_stream_t stream);

/* ---- minimum-area hole triangulation and Delaunay-like edge flips (csrc/meshtri.hip) ----
 * The oracle is tests/meshtri_restatement.py, bit for bit.  Integer atomics only: two runs are bitwise equal.  No call
 * synchronises.
 *
 * Triangulation.  The boundary edges of misplat_meshclean_holes, listed by loop: edges [B,2] int32, order [B] int32 (the edges by
 * loop, in list order inside a loop), offsets [L + 1] int32, fill [L] uint8 (the loops to close).  A loop of n edges is
 * triangulated iff it is filled, 3 <= n <= MISPLAT_MESHTRI_MAX_LOOP and it is a simple cycle (its n tails are distinct, its n
 * heads are distinct and they are the same vertices).  Its polygon: p_0 the smallest vertex, p_{i+1} the head of the edge whose
 * tail is p_i, q_0 = p_0, q_i = p_{n-i}.  W[i][i+1] = 0, W[i][j] = min over i < k < j of ((W[i][k] + W[k][j]) + (double) A(i,k,j))
 * in fp64, strict < in ascending k, A = 0.5f sqrtf((cx cx + cy cy) + cz cz) of the fp32 cross product of q_k - q_i and q_j - q_i.
 * A loop of at most MISPLAT_MESHTRI_LDS_LOOP edges keeps its table (n (n - 1) / 2 entries of 8 + 2 bytes: 154000 bytes at 176,
 * with the polygon 156816 of the 163840 a workgroup may declare) in LDS; a longer one, up to MISPLAT_MESHTRI_MAX_LOOP (a stated
 * limit: 523776 entries, 5.2 MB), in the workspace.  Both run the same code and give the same bits. */
#define MISPLAT_MESHTRI_LDS_LOOP 176
#define MISPLAT_MESHTRI_MAX_LOOP 1024
/* Loops of at most this many edges run in a workgroup of 256 with 21 KB of LDS (misplat_meshtri_dp's path 1); no result depends on it. */
#define MISPLAT_MESHTRI_SMALL_LOOP 64
/* code [L] int32: 0 triangulated, 1 not a simple cycle, 2 fewer than 3 edges, 3 more than MAX_LOOP, -1 not filled; polygon [B]
 * int32: q_0 .. q_{n-1} of every triangulated loop at offsets[l]. */
int misplat_meshtri_order(const int32_t* edges, const int32_t* order, const int32_t* offsets, const uint8_t* fill, int64_t n_edges,
                          int64_t n_loops, int32_t* code, int32_t* polygon, misplat_stream_t stream);
/* workspace bytes for tables of n_entries entries in all (the loops above MISPLAT_MESHTRI_LDS_LOOP); -1 for sizes refused. */
int64_t misplat_meshtri_workspace(int64_t n_entries);
/* The tables and the faces of the loops with code 0.  paths: 1 the loops up to SMALL_LOOP edges, 2 those up to LDS_LOOP, 4 the longer
 * ones (slab_offset [L] int64: where a loop's table starts, in entries; the others take neither it nor the workspace).  Loop l
 * writes its n - 2 faces (q_i, q_k, q_j), by ascending apex k = 1 .. n - 2, from row face_base[l] of faces [n_faces,3] int32,
 * and W[0][n-1] into area[area_slot[l]] ([n_area] fp64); a loop whose rows or slot lie outside is skipped. */
int misplat_meshtri_dp(const float* vertices, int64_t n_vertices, const int32_t* polygon, const int32_t* offsets, const int32_t* code,
                       int64_t n_loops, int32_t paths, const int64_t* slab_offset, int64_t n_entries, void* workspace,
                       int64_t workspace_bytes, const int32_t* face_base, int64_t n_faces, const int32_t* area_slot, int64_t n_area,
                       int32_t* faces, double* area, misplat_stream_t stream);
/* The angle-and-area weight (the oracle is tests/meshsmooth_restatement.py, bit for bit): an entry is the
 * pair (b, a), a the area sum above, b = max(W[i][k].b, W[k][j].b, bad(T, left), bad(T, right)) for the candidate T = (q_i, q_k,
 * q_j), left = the rim face (q_{i+1}, q_i, o_i) if k - i = 1, else (q_i, q_{S[i][k]}, q_k) with S the stored split; right likewise
 * across (k, j); the top entry (0, n - 1) also takes bad(T, (q_0, q_{n-1}, o_{n-1})).  bad of two oriented faces: n1, n2 their fp64
 * cross products (edge vectors in fp64 from the fp32 coordinates, dot = (x x' + y y') + z z'), c = dot(n1, n2) / sqrt(dot(n1, n1)
 * dot(n2, n2)), bad = clamp((int) floor((1 - c) 0.5 STEPS), 0, STEPS), 0 if either squared length is 0 or the value is not a
 * number.  Entries compare lexicographically on (b, a), strict < in ascending k.  An entry is 8 + 2 + 2 bytes and a polygon vertex
 * 28 (its coordinates, its index, its rim corner's coordinates): 12 n (n - 1) / 2 + 28 n <= 163840 holds up to n = 163. */
#define MISPLAT_MESHTRI_ANGLE_STEPS 1024
#define MISPLAT_MESHTRI_ANGLE_LDS_LOOP 163
/* order, and rim [B] int32: rim[offsets[l] + i] = o_i, the third corner of the one face of triangles [T,3] that holds the polygon's
 * edge (q_i, q_{i+1}) (i = n - 1: the closing edge (q_{n-1}, q_0)), -1 where there is none.  The workspace holds the mesh's edge
 * table (rim_workspace(T) bytes; -1 for sizes refused: 1 <= T, 6 T < 2^31 - 4096). */
int64_t misplat_meshtri_rim_workspace(int64_t n_triangles);
int misplat_meshtri_order_rim(const int32_t* edges, const int32_t* order, const int32_t* offsets, const uint8_t* fill, int64_t n_edges,
                              int64_t n_loops, const int32_t* triangles, int64_t n_triangles, void* workspace, int64_t workspace_bytes,
                              int32_t* code, int32_t* polygon, int32_t* rim, misplat_stream_t stream);
/* misplat_meshtri_workspace and misplat_meshtri_dp under the angle-and-area weight: the paths split at SMALL_LOOP and
 * ANGLE_LDS_LOOP; badness [n_area] int32 takes the top entry's b beside area. */
int64_t misplat_meshtri_angle_workspace(int64_t n_entries);
int misplat_meshtri_angle_dp(const float* vertices, int64_t n_vertices, const int32_t* polygon, const int32_t* rim,
                             const int32_t* offsets, const int32_t* code, int64_t n_loops, int32_t paths, const int64_t* slab_offset,
                             int64_t n_entries, void* workspace, int64_t workspace_bytes, const int32_t* face_base, int64_t n_faces,
                             const int32_t* area_slot, int64_t n_area, int32_t* faces, double* area, int32_t* badness,
                             misplat_stream_t stream);
/* Flips.  An undirected edge is flippable iff it has exactly two distinct incident faces, both with region != 0 and three
 * distinct corners, f_max runs it against f_min (f_min = (a, b, c) rotated, f_max holds b -> a and d), c != d, the edge (c, d) is
 * not in the mesh, the fp64 sum cot(c) + cot(d) (each dot / |cross| of the two edge vectors at the corner, from the fp32
 * coordinates) is < -min_violation, and each new face's normal has a positive dot product with the sum of the old faces'
 * unnormalised normals.  Priority: the larger fp64 bits of -(cot c + cot d), then the smaller mix32(lo, hi, 0), then the smaller
 * key.  One round: the flippable edges that are first among the flippable edges of each of their faces are selected; of those
 * that want the same new edge the smallest key flips; f_min <- (a, d, c), f_max <- (d, b, c) in place.  counts [1] int32 on the
 * device: the flips applied.  1 <= T, 6 T < 2^31 - 4096. */
int64_t misplat_meshtri_flip_workspace(int64_t n_vertices, int64_t n_triangles);
int misplat_meshtri_flip_round(const float* vertices, int64_t n_vertices, int32_t* triangles, int64_t n_triangles,
                               const uint8_t* region, double min_violation, void* workspace, int64_t workspace_bytes, int32_t* counts,
                               misplat_stream_t stream);

/* ---- identity training for Gaussian grouping (Gaussian Grouping / Gaga; the reference's unfinished setup_train,
 * utils/grouping.py:110-136, restated from the published method): csrc/identity.hip.  A linear classifier weight [classes, dim],
 * bias [classes] (dim 1..32, classes 1..4096) over rendered identity images or the Gaussians' identity vectors.
 *   2-D: z = W x + b per pixel, ce = logsumexp(z) - z[target - 1], loss = sum_labelled ce / max(n_labelled, 1); target [H, W]
 *   int32, 0 = unlabelled, t in 1..classes = class t - 1, anything else counts as unlabelled and is reported in counts[1].
 *   3-D: loss = sum_pairs KL(softmax(W e_s + b) || softmax(W e_t + b)) / max(n_pairs, 1) over the pairs (sample[j], table[j][i])
 *   whose entry is neither -1 nor its own sample.
 * features [H, W, dim] float32 with its pixels pix_stride >= dim floats apart.  scratch: misplat_identity_scratch_floats(rows,
 * dim, classes, mode) floats (mode 0: rows = H * W pixels; mode 1: rows = n_samples * k pairs; -1 outside the limits, rows at
 * most 2^28): per-row scalars and the weight gradient's partial sums per row split (at most 64 splits), written by the forward,
 * read and written by the backward.  counts: device int32 [2] = (labelled pixels or valid pairs, targets out of range).  No
 * [classes, rows] buffer exists; every sum runs in a fixed order, the last stage in fp64; no atomics. */
int64_t misplat_identity_scratch_floats(int64_t rows, int32_t dim, int32_t classes, int32_t mode);
int misplat_identity_loss_fwd(int32_t height, int32_t width, int32_t dim, int32_t pix_stride, const float* features,
                              int32_t classes, const float* weight, const float* bias, const int32_t* target, float* scratch,
                              int32_t* counts, float* loss, misplat_stream_t stream);
/* g_loss: the upstream gradient as a DEVICE scalar (or NULL = 0).  v_features [H, W, dim] contiguous, every element written
 * (exact zeros at unlabelled pixels), v_weight [classes, dim], v_bias [classes]. */
int misplat_identity_loss_bwd(int32_t height, int32_t width, int32_t dim, int32_t pix_stride, const float* features,
                              int32_t classes, const float* weight, const float* bias, const int32_t* target, float* scratch,
                              const int32_t* counts, const float* g_loss, float* v_features, float* v_weight, float* v_bias,
                              misplat_stream_t stream);
/* Inference, one launch: labels [rows] = argmax class + 1 (ties: the smallest class), confidence (or NULL) [rows] = the
 * largest softmax probability. */
int misplat_identity_labels(int64_t rows, int32_t dim, int32_t pix_stride, const float* features, int32_t classes,
                            const float* weight, const float* bias, int32_t* labels, float* confidence, misplat_stream_t stream);
/* identities [n_rows, dim]; sample [n_samples] int64; table [n_samples, k] int32, k 1..16. */
int misplat_identity_3d_fwd(int64_t n_rows, int32_t dim, const float* identities, int32_t classes, const float* weight,
                            const float* bias, int32_t n_samples, int32_t k, const int64_t* sample, const int32_t* table,
                            float* scratch, int32_t* counts, float* loss, misplat_stream_t stream);
/* rev_offsets [n_rows + 1] int64 / rev_slots int32: a CSR over rows of the slots (2 * pair + side; side 0 the sample, 1 the
 * table entry) that name the row, ascending within a row; v_identities [n_rows, dim], every element written. */
int misplat_identity_3d_bwd(int64_t n_rows, int32_t dim, const float* identities, int32_t classes, const float* weight,
                            const float* bias, int32_t n_samples, int32_t k, const int64_t* sample, const int32_t* table,
                            const int64_t* rev_offsets, const int32_t* rev_slots, float* scratch, const int32_t* counts,
                            const float* g_loss, float* v_identities, float* v_weight, float* v_bias, misplat_stream_t stream);

/* ---- Evaluation metrics (csrc/evalmetrics.hip): per-view scores of B stacked views, two launches
 * each (per-workgroup partial sums, then one workgroup per view adds them in fp64 in an order that depends on H and W
 * only), no atomics, no host read.  All: 1 <= n_views <= 65535, height * width < 2^31, NULL where not allowed or a
 * size outside that is MISPLAT_EINVAL.  Images are [B, H, W, C] fp32, channel-interleaved.
 *
 * Image scores: out [B, 4] = {mse, l1, ssim, psnr}: means over the 3 H W values of (pred - gt)^2 and |pred - gt|; the
 * valid-region SSIM of the training loss (11-tap gaussian window, sigma 1.5, (H - 10) x (W - 10) positions, C1 = 0.01^2,
 * C2 = 0.03^2), NaN when want_ssim == 0; psnr = -10 log10(mse) (+inf for mse == 0).  want_ssim needs H, W >= 11.
 * scratch: the floats the _scratch_floats call returns (-1 for sizes out of range). */
int64_t misplat_eval_image_scratch_floats(int32_t n_views, int32_t height, int32_t width);
int misplat_eval_image(int32_t n_views, int32_t height, int32_t width, const float* pred, const float* gt, int32_t want_ssim,
                       float* scratch, float* out, misplat_stream_t stream);
/* Normals: pred, gt [B, H, W, 3]; valid (or NULL) [B, H, W] bytes, 0 = excluded; encoded: v <- 2 v - 1 first; normalize:
 * both vectors scaled to unit length, a pixel with a squared length <= 1e-12 excluded.  theta = acos(clamp(dot, -1, 1)).
 * out [B, 5] = {mean theta (radians), fraction theta < 11.25 deg, < 22.5 deg, < 30 deg, count}; NaN means and fractions for
 * count == 0.  map (or NULL) [B, H, W]: every pixel's theta, NaN where excluded.  Depth: pred, gt [B, H, W]; a pixel counts
 * where valid (or NULL) is non-zero, both depths are finite and > 0 and gt <= max_depth (max_depth <= 0: no limit).
 * out [B, 8] = {abs_rel, sq_rel, rmse, rmse_log, delta < 1.25, < 1.25^2, < 1.25^3, count} (Eigen et al. 2014).
 * scratch: the floats the one _scratch_floats call returns, 8-byte aligned. */
int64_t misplat_eval_pixels_scratch_floats(int32_t n_views, int32_t height, int32_t width);
int misplat_eval_normals(int32_t n_views, int32_t height, int32_t width, const float* pred, const float* gt,
                         const uint8_t* valid, int32_t encoded, int32_t normalize, float* map, float* scratch, float* out,
                         misplat_stream_t stream);
int misplat_eval_depth(int32_t n_views, int32_t height, int32_t width, const float* pred, const float* gt,
                       const uint8_t* valid, float max_depth, float* scratch, float* out, misplat_stream_t stream);

/* ---- Colour-corrected evaluation (csrc/colorcorrect.hip): pred [B, H, W, 3] fp32 is warped onto gt's
 * colours by num_iters rounds of a masked least-squares fit of the 10 quadratic monomials (r^2, rg, rb, g^2, gb, b^2, r, g,
 * b, 1) per output channel: fp64 normal equations, symmetric eigensolve, eigenvalues <= 2^-46 lambda_max dropped; a pixel
 * counts for channel c where pred_c, the current image's c and gt_c all lie in [eps, 1 - eps] (fp32 comparisons); the
 * warp is applied to every pixel and clipped to 0..1.  Three launches per round, no atomics, no host read; a view's
 * result does not depend on n_views.  corrected [B, H, W, 3] fp32 (not pred or gt; pred's bits for num_iters == 0);
 * warps [B, num_iters, 10, 3] fp64 and counts [B, num_iters, 3] int64: each round's fit and mask counts (may be NULL for
 * num_iters == 0).  1 <= n_views <= 65535, height * width < 2^31, 0 <= num_iters <= 64, 0 <= eps < 0.5: anything else is
 * MISPLAT_EINVAL before any launch.  scratch: the floats the _scratch_floats call returns (-1 for sizes out of range), 8-byte
 * aligned. */
int64_t misplat_colorcorrect_scratch_floats(int32_t n_views, int32_t height, int32_t width);
int misplat_colorcorrect(int32_t n_views, int32_t height, int32_t width, const float* pred, const float* gt, int32_t num_iters,
                         float eps, float* scratch, float* corrected, double* warps, int64_t* counts, misplat_stream_t stream);

/* ---- MCMC densification (csrc/mcmc.hip): Kheradmand et al. 2024, restated from the published method.
 * seed and step are the two words of the counter-based generator (csrc/hashmix.h): the same pair gives the same bits in
 * every run, on every rank and under any launch shape.  All: 1 <= n, m < 2^31, a NULL where none is allowed is
 * MISPLAT_EINVAL before any launch.
 *
 * Noise, every training step, in place on means [n, 3]: with o = sigmoid(opacities[i]) (logits), s = exp(scales[i]) (logs),
 * R the rotation of the normalised wxyz quats[i] (16-byte aligned), g = 1 / (1 + exp(-100 ((1 - o) - 0.995))) and z three
 * standard normals (Box-Muller over the words mix32(mix32(seed, step, 1), i, 0..3)):
 * means[i] += fl32(R diag(s^2) R^T (z g scaler)).  One launch. */
#define MISPLAT_MCMC_N_MAX 51    /* the largest ratio of the relocation; binoms is at most [51, 51] */
#define MISPLAT_MCMC_NOTHING 1   /* *status of misplat_mcmc_sample: every weight is 0 */
int misplat_mcmc_noise(int64_t n, float* means, const float* opacities, const float* scales, const float* quats, float scaler,
                       uint32_t seed, uint32_t step, misplat_stream_t stream);
/* Sampling: m draws with replacement from the n ACTIVATED opacities [n] fp32, in exact integer arithmetic.  Row i weighs
 * q_i = (uint32)(min(o_i, 1) 2^24), 0 for o_i <= 0 or NaN and, when has_min_opacity, for o_i <= min_opacity; draw j is the
 * first i with incl[i] > (u_j total) >> 64, incl the int64 inclusive sum of q, total = incl[n - 1], u_j the 64 bits
 * mix32(k, j, 0) << 32 | mix32(k, j, 1), k = mix32(seed, step, 2).  A row of weight 0 is never drawn.  idx [m] int64;
 * counts (or NULL) [n] int32 = how often each row was drawn (zeroed here, then integer atomics: order-independent);
 * status [1] int32 on the device = 0, or MISPLAT_MCMC_NOTHING when total == 0 (idx is then -1 throughout and counts 0;
 * nothing is divided).  workspace: misplat_mcmc_sample_workspace_bytes(n) bytes (-1 for n out of range), 8-byte aligned. */
int64_t misplat_mcmc_sample_workspace_bytes(int64_t n);
int misplat_mcmc_sample(int64_t n, const float* opacities, int32_t has_min_opacity, float min_opacity, int64_t m, uint32_t seed,
                        uint32_t step, void* workspace, int64_t workspace_bytes, int64_t* idx, int32_t* counts, int32_t* status,
                        misplat_stream_t stream);
/* Relocation (the paper's Eq. 9) of m entries: opacities [m] (activated), scales [m, 3] (activated), ratios [m] int32, clamped
 * to 1 .. n_max here; binoms [n_max, n_max] fp64, binoms[i][k] = C(i, k) (0 for k > i), 1 <= n_max <= MISPLAT_MCMC_N_MAX.
 *   o' = 1 - (1 - o)^(1 / n)   (as -expm1(log1p(-o) / n));
 *   D = sum_{i = 1..n} sum_{k = 0..i-1} C(i - 1, k) (-1)^k / sqrt(k + 1) o'^(k + 1), in fp64 in this order;
 *   s' = (o / D) s   (s for o <= 0).
 * new_opacities [m] = o', new_scales [m, 3] = s', each rounded to fp32 once. */
int misplat_mcmc_relocation(int64_t m, const float* opacities, const float* scales, const int32_t* ratios, const double* binoms,
                            int32_t n_max, float* new_opacities, float* new_scales, misplat_stream_t stream);

/* Library identification ("misplat <version> gfx950"). */
const char* misplat_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MISPLAT_H */
