/*
 * gradslam_hip.h — C-ABI of the MI355X (gfx950) dense-SLAM hot path.
 *
 * One shared library (gradslam_amd/csrc/libgradslam_hip.so) exports exactly these entry
 * points.  They replace the *bodies* of the reference's Python functions listed beside
 * each declaration (file:line are relative to the gradslam reference checkout).  The
 * reference has no FFI layer (it is pure Python on PyTorch); INTEGRATION.md shows the
 * ctypes stub a gradslam maintainer would add at each call site.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - plain pointers + explicit sizes, no torch types, no C++ types, no exceptions;
 *   - return value: GS_OK (0) or a GS_ERR_* code; gs_last_error() gives a message;
 *   - nothing here allocates: the caller (torch) owns every buffer, scratch included;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*), no host sync
 *     unless the function name ends in _sync;
 *   - one call handles ONE sequence of the batch (the reference's batch index b is a host-side loop) except
 *     the *_batch_* entry points at the end, which run the frame loop of B sequences per launch;
 *   - images are channels-last row-major (H, W, C) float32; map attributes are (N, 3)
 *     or (N, 1) float32 row-major; index tables are int64 (rows, 4) = [b, n, h, w];
 *   - 4x4 matrices are 16 contiguous float32, row-major, on the device.
 *
 * Arithmetic is specified operation-by-operation in DESIGN.md §arithmetic; the CPU oracle
 * (oracle/gs_oracle.c, same signatures with prefix gs_or_) restates it in plain C.
 */
#ifndef GRADSLAM_HIP_H
#define GRADSLAM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* exported from libgradslam_hip.so (the library is built with -fvisibility=hidden) */
#define GS_API __attribute__((visibility("default")))

#define GS_OK 0
#define GS_ERR_INVALID 1 /* bad argument (null pointer, non-positive size, ...) */
#define GS_ERR_HIP 2     /* a HIP runtime call failed; see gs_last_error() */
#define GS_ERR_CAPACITY 3 /* an output would exceed the caller-provided capacity */

/* ABI version; bumped on any signature change. */
GS_API int gs_abi_version(void);
/* Message of the last non-OK return on this thread (never NULL). */
GS_API const char* gs_last_error(void);
/* Bytes of device scratch the functions below need for a map of `n_map` points and an
 * image of `n_pix` pixels (caller allocates once, reuses every frame). */
GS_API int64_t gs_scratch_bytes(int64_t n_map, int64_t n_pix);

/* Optional in-library kernel timing with HIP events recorded on the launch stream (used by
 * bench.py for the roofline line; off by default).  gs_profile_begin arms up to max_records
 * timed launches, gs_profile_end synchronises the device and aggregates,
 * gs_profile_read returns per kernel group: total milliseconds, launches, and work units
 * (kind 0 brute-force KNN: pair distances; other kinds: algorithmic bytes).
 * kinds: 0 brute-force KNN, 1 ICP linearise, 2 frame maps, 3 map projection, 4 association,
 * 5 fuse/append, 6 compaction / grid build, 7 ICP solve/update, 8 fused ICP search+linearise. */
GS_API int gs_profile_begin(int max_records);
GS_API int gs_profile_end(void);
GS_API int gs_profile_read(int kind, double* ms_total, int64_t* launches, double* work_total);

/* ---------------------------------------------------------------- K1: frame maps ------
 * depth -> local vertex map, local normal map, confidence alpha, validity mask.
 * Replaces RGBDImages._compute_vertex_map (structures/rgbdimages.py:643-679) incl.
 * inverse_intrinsics (geometry/projutils.py:405-450) and the pixel meshgrid,
 * RGBDImages._compute_normal_map (structures/rgbdimages.py:710-743),
 * RGBDImages.valid_depth_mask (:320-332) and get_alpha as called by fuse_with_map
 * (slam/fusionutils.py:69-72, :657).  Any of vertex/normal/alpha/valid may be NULL.
 * two_sigma_sq = (float)(2*sigma*sigma) evaluated in double by the caller. */
GS_API int gs_frame_maps_f32(const float* depth, const float* K16, int H, int W, float two_sigma_sq,
                      float* vertex, float* normal, float* alpha, uint8_t* valid, void* stream);

/* local maps + pose -> global vertex / normal maps.
 * Replaces RGBDImages._compute_global_vertex_map (structures/rgbdimages.py:681-708) and
 * _compute_global_normal_map (:745-762).  gnormal may be NULL.  pose16 == NULL means the
 * reference's "no poses" branch (plain copy). */
GS_API int gs_global_maps_f32(const float* vertex, const float* normal, const float* depth,
                       const float* pose16, int H, int W, float* gvertex, float* gnormal,
                       void* stream);

/* get_alpha on an arbitrary (n,3) point array (slam/fusionutils.py:16-73). */
GS_API int gs_alpha_f32(const float* points, int64_t n, float two_sigma_sq, float eps, float* alpha,
                 void* stream);

/* Reverse mode of gs_alpha_f32 = what PyTorch autograd computes through get_alpha (slam/fusionutils.py:69-72; the
 * reference's own gradient check: tests/slam/test_fusionutils.py:56-75): points_bar[i] = alpha_bar[i] * d alpha_i / d p_i
 * (zero where the clamp is active), sigma_terms[i] (may be NULL) = alpha_bar[i] * alpha_i * |p_i|^2, so that
 * d loss / d sigma = sum_i sigma_terms[i] / sigma^3. */
GS_API int gs_alpha_backward_f32(const float* points, int64_t n, float two_sigma_sq, float eps,
                          const float* alpha_bar, float* points_bar, float* sigma_terms, void* stream);

/* ------------------------------------------------------- K2: ICP source / target sets --
 * Valid pixels of the [::ds, ::ds] lattice, raster order -> compact point list.
 * Replaces downsample_rgbdimages (odometry/icputils.py:623-669).  out_* have room for
 * ceil(H/ds)*ceil(W/ds) rows; out_nrm/out_rgb (and gnormal/rgb) may be NULL.
 * count_out: device int64[1]. */
GS_API int gs_downsample_frame_f32(const float* gvertex, const float* gnormal, const float* rgb,
                            const float* depth, int H, int W, int ds, float* out_pts,
                            float* out_nrm, float* out_rgb, int64_t* count_out, void* scratch,
                            void* stream);

/* Project every map point into a frame: pix[n] = h*W + w of the pixel it lands on, or -1
 * when it is not "active".  Replaces the arithmetic of find_active_map_points
 * (slam/fusionutils.py:249-274): inverse_transformation, Pointclouds.transform
 * (structures/pointclouds.py:466-573), pinhole_projection_ (:575-614, geometry/projutils.py
 * :225-238), the in-frame test and round/clamp.  pose16 is camera-to-world. */
GS_API int gs_project_map_f32(const float* points, int64_t n_map, const float* pose16,
                       const float* K16, int H, int W, int32_t* pix, void* stream);

/* pix[] -> ordered table rows [b, n, h, w] (find_active_map_points' return value,
 * slam/fusionutils.py:276-282).  rows_out has room for n_map rows; count_out device int64. */
GS_API int gs_active_table_i64(const int32_t* pix, int64_t n_map, int W, int64_t b, int64_t* rows_out,
                        int64_t* count_out, void* scratch, void* stream);

/* Active map points whose pixel lies on the [::ds, ::ds] lattice, in map order, gathered.
 * Replaces downsample_pointclouds (odometry/icputils.py:596-620) fed by
 * find_active_map_points.  out_* have room for `cap` rows: the kernels never write past cap, count_out[0]
 * always receives the TRUE number of selected points (the caller compares it with cap).
 * normals/colors optional. */
GS_API int gs_select_targets_f32(const int32_t* pix, int64_t n_map, int W, int ds, const float* points,
                          const float* normals, const float* colors, float* out_pts,
                          float* out_nrm, float* out_rgb, int64_t cap, int64_t* count_out,
                          void* scratch, void* stream);

/* downsample_pointclouds on an explicit table (rows of one sequence): keeps rows with
 * h % ds == 0 and w % ds == 0, gathers map attributes by n.  (odometry/icputils.py:596-620) */
GS_API int gs_downsample_table_f32(const int64_t* rows, int64_t n_rows, int ds, const float* points,
                            const float* normals, const float* colors, float* out_pts,
                            float* out_nrm, float* out_rgb, int64_t* count_out, void* scratch,
                            void* stream);

/* ------------------------------------------------------------------ K3: exact 1-NN -----
 * For every src point the index of the nearest tgt point (squared L2, lowest index on
 * ties) and that squared distance.  Replaces chamferdist.chamfer.knn_points as called at
 * odometry/icputils.py:200 (third-party, chamferdist==1.0.0, requirements.txt:2).
 * best_scratch: device uint64[n_src].  out_idx int64[n_src], out_d2 float[n_src] (may be NULL). */
GS_API int gs_knn1_f32(const float* src, int64_t n_src, const float* tgt, int64_t n_tgt,
                int64_t* out_idx, float* out_d2, uint64_t* best_scratch, void* stream);

/* Same result through the uniform-grid engine the ICP loop uses (targets counting-sorted into
 * cells once, Chebyshev-shell search with an exactness bound, brute-force pass for queries it
 * cannot resolve): bit-identical to gs_knn1_f32.  scratch: gs_knn1_grid_scratch_bytes().
 * unresolved_out (HOST pointer, may be NULL; forces a stream sync): queries finished by brute force. */
GS_API int64_t gs_knn1_grid_scratch_bytes(int64_t n_src, int64_t n_tgt);
GS_API int gs_knn1_grid_f32(const float* src, int64_t n_src, const float* tgt, int64_t n_tgt,
                            int64_t* out_idx, float* out_d2, void* scratch, int64_t* unresolved_out_host,
                            void* stream);

/* --------------------------------------------------------- K4: Gauss-Newton system -----
 * gauss_newton_solve (odometry/icputils.py:93-232): KNN + rows A_i = [n, s x n],
 * b_i = n.(d - s).  A (n_src,6) and b (n_src) are written densely for ALL src rows plus a
 * keep mask (dist filter, :203-208); idx int64[n_src].  dist_thresh < 0 means None. */
GS_API int gs_gauss_newton_rows_f32(const float* src, int64_t n_src, const float* tgt,
                             const float* tgt_normals, int64_t n_tgt, float dist_thresh,
                             float* A, float* b, int64_t* idx, uint8_t* keep,
                             uint64_t* best_scratch, void* stream);

/* solve_linear_system (odometry/icputils.py:22-90): x = (A^T A + damp I)^-1 A^T b for
 * A (n_rows, ncols), 1 <= ncols <= 8 (the SLAM path uses 6).  keep may be NULL.
 * x: device float[ncols]. */
GS_API int gs_solve_normal_eq_f32(const float* A, const float* b, const uint8_t* keep, int64_t n_rows,
                           int ncols, float damp, float* x, void* stream);

/* se3_exp (geometry/se3utils.py:77-115): xi(6) -> T(4x4). */
GS_API int gs_se3_exp_f32(const float* xi6, float* T16, void* stream);

/* Reverse mode of gs_se3_exp_f32 (PyTorch autograd through geometry/se3utils.py:77-115): xi_bar(6) from T_bar(4x4). */
GS_API int gs_se3_exp_backward_f32(const float* xi6, const float* Tbar16, float* xi_bar6, void* stream);

/* relative_transformation(T01, T02, orthogonal_rotations=False) (geometry/geometryutils.py:413-478; the
 * arithmetic of GroundTruthOdometryProvider.provide, odometry/groundtruth.py:74-78, and of the dataset
 * loaders' pose preprocessing, datasets/tum.py:497-499): out[m] = compose(inv(T01[m]), T02[m]) for n
 * pairs of 4x4 float32 matrices. */
GS_API int gs_relative_pose_f32(const float* T01, const float* T02, int64_t n, float* out, void* stream);

/* transform_pointcloud (geometry/geometryutils.py:737-794): out = R p + t. */
GS_API int gs_transform_points_f32(const float* pts, int64_t n, const float* T16, float* out,
                            void* stream);

/* Whole LM loop on the device, no host sync.
 * mode 0: point_to_plane_ICP      (odometry/icputils.py:235-367)
 * mode 1: point_to_plane_gradICP  (odometry/icputils.py:370-545)
 * src is NOT modified (a working copy lives in scratch).  init16: initial transform.
 * compose16 (may be NULL): if given, T_out = T_icp * compose16, i.e. the caller's
 * compose_transformations(transform, prev_pose) (slam/icpslam.py:245-247) fused in.
 * out_T16: device float[16]; out_idx (may be NULL): int64[n_src] neighbour indices of the
 * last iteration's first linearisation (:328,:367).  icp_scratch: gs_icp_scratch_bytes(). */
typedef struct gs_icp_params {
  int mode;          /* 0 = ICP, 1 = gradICP */
  int numiters;      /* default 20 */
  float damp;        /* initial damping, default 1e-8 */
  float dist_thresh; /* < 0: None */
  float lambda_max;  /* gradICP, default 2.0 */
  float B;           /* gradICP, default 1.0 */
  float B2;          /* gradICP, default 1.0 */
  float nu;          /* gradICP, default 200.0 */
} gs_icp_params;

GS_API int64_t gs_icp_scratch_bytes(int64_t n_src, int64_t n_tgt);
GS_API int gs_icp_f32(const float* src, int64_t n_src, const float* tgt, const float* tgt_normals,
               int64_t n_tgt, const float* init16, const float* compose16,
               const gs_icp_params* params_host, float* out_T16, int64_t* out_idx,
               void* icp_scratch, void* stream);

/* ------------------------------------------------- K7: backward of the frame maps ------
 * Reverse mode of gs_frame_maps_f32 w.r.t. depth: depth_bar (H,W) from the adjoints of the local
 * vertex map, normal map and alpha (any may be NULL), as PyTorch autograd does through
 * structures/rgbdimages.py:643-743 and slam/fusionutils.py:69-72.  scratch_6hw: 6*H*W floats,
 * needed when normal_bar is given.  K_bar16 (may be NULL): the gradient w.r.t. the 4x4 intrinsics as autograd
 * produces it through inverse_intrinsics (geometry/projutils.py:437-449): entries [0,0] (fx), [0,2] (cx), [1,1] (fy),
 * [1,2] (cy), zero elsewhere; needs kbar_scratch of gs_frame_maps_backward_kbar_scratch_bytes(H, W) bytes (fixed-order
 * float64 block sums).  depth_bar may be NULL when only K_bar16 is wanted. */
GS_API int64_t gs_frame_maps_backward_kbar_scratch_bytes(int H, int W);
GS_API int gs_frame_maps_backward_f32(const float* depth, const float* K16, int H, int W, float two_sigma_sq,
                                      const float* vertex_bar, const float* normal_bar, const float* alpha_bar,
                                      float* depth_bar, float* scratch_6hw, float* K_bar16, void* kbar_scratch,
                                      void* stream);
/* Reverse mode of gs_global_maps_f32 w.r.t. the local maps (rgbdimages.py:681-762):
 * vertex_bar = R^T (gvertex_bar * valid), normal_bar = R^T gnormal_bar.  (No pose gradient.) */
GS_API int gs_global_maps_backward_f32(const float* gvertex_bar, const float* gnormal_bar, const float* depth,
                                       const float* pose16, int H, int W, float* vertex_bar, float* normal_bar,
                                       void* stream);
/* ... and w.r.t. the pose: pose_bar (4x4, last row zero) with R_bar = sum_p valid_p gvertex_bar_p (x) v_p +
 * sum_p gnormal_bar_p (x) n_p and t_bar = sum_p valid_p gvertex_bar_p (the recovered pose of a frame feeds the
 * global maps that are fused into the map: this is the link map -> pose -> ICP of the reference's graph). */
GS_API int64_t gs_global_maps_pose_backward_scratch_bytes(int H, int W);
GS_API int gs_global_maps_pose_backward_f32(const float* vertex, const float* normal, const float* depth,
                                            const float* gvertex_bar, const float* gnormal_bar, int H, int W,
                                            float* pose_bar16, void* scratch, void* stream);
/* Reverse mode of gs_downsample_frame_f32 (points): gvertex_bar (H,W,3) = zeros with the compact
 * adjoints pts_bar scattered back to the valid lattice pixels (odometry/icputils.py:654-660). */
GS_API int gs_downsample_frame_backward_f32(const float* pts_bar, const float* depth, int H, int W, int ds,
                                            float* gvertex_bar, void* scratch, void* stream);

/* ------------------------------------------------------------- K7: (grad)ICP backward ----
 * Both solvers are differentiable: mode 1 (gradICP, odometry/icputils.py:479-545) through the soft accept and
 * damping functions, mode 0 (hard LM, :310-367) through the accepted steps only (the accept test and the
 * damping schedule are constants, as in the reference's autograd graph).
 * Differentiable gradICP (config C3): gs_icp_tape_f32 is gs_icp_f32 that additionally records the
 * forward tape (caller-owned, gs_icp_tape_bytes(n_src, numiters) bytes: per-iteration source cloud,
 * neighbour indices of both searches, float32 normal equations, trace).  gs_icp_backward_f32 then
 * turns dL/dT (T_bar16, the gradient w.r.t. the UN-composed transform returned with compose16 ==
 * NULL) into dL/d(src), dL/d(tgt), dL/d(tgt_normals), dL/d(init) exactly as PyTorch autograd does
 * through odometry/icputils.py:479-545 (indices and the dist_thresh filter are constants).  Any of
 * the four outputs may be NULL.  mode must be 1 (gradICP).  scratch: gs_icp_backward_scratch_bytes. */
GS_API int64_t gs_icp_tape_bytes(int64_t n_src, int numiters);
GS_API int gs_icp_tape_f32(const float* src, int64_t n_src, const float* tgt, const float* tgt_normals,
                           int64_t n_tgt, const float* init16, const float* compose16,
                           const gs_icp_params* params_host, float* out_T16, int64_t* out_idx,
                           void* icp_scratch, void* tape, void* stream);
GS_API int64_t gs_icp_backward_scratch_bytes(int64_t n_src, int64_t n_tgt);
GS_API int gs_icp_backward_f32(const void* tape, const float* src, int64_t n_src, const float* tgt,
                               const float* tgt_normals, int64_t n_tgt, const float* init16,
                               const gs_icp_params* params_host, const float* T_bar16, float* src_bar,
                               float* tgt_bar, float* normals_bar, float* init_bar16, void* scratch,
                               void* stream);

/* gs_icp_f32 with DEVICE-SIDE point counts: n_src_bound / n_tgt_bound are upper bounds used for
 * launch geometry and scratch sizing (src / tgt buffers must hold that many rows); the actual
 * counts are read on the device from n_src_dev / n_tgt_dev (e.g. the count_out of
 * gs_downsample_frame_f32 / gs_select_targets_f32), so the host never reads them back: no sync
 * between selecting the ICP point sets and solving.  Either pointer may be NULL (= the bound is exact). */
GS_API int gs_icp_dc_f32(const float* src, int64_t n_src_bound, const int64_t* n_src_dev, const float* tgt,
                         const float* tgt_normals, int64_t n_tgt_bound, const int64_t* n_tgt_dev,
                         const float* init16, const float* compose16, const gs_icp_params* params_host,
                         float* out_T16, int64_t* out_idx, void* icp_scratch, void* stream);

/* The SLAM loop's solve without gathering the target set: the targets are the rows of the surfel map
 * (map_points / map_normals, n_map_bound rows, actual count in n_map_dev or NULL) whose projection `pix`
 * (gs_project_map_*_f32 with the previous pose) lies on the [::ds, ::ds] pixel lattice -- the set
 * find_active_map_points + downsample_pointclouds select (slam/icpslam.py:241-242, odometry/icputils.py:
 * 596-597) -- binned straight from the map.  Same transform, bit for bit, as gs_icp_dc_f32 on the output of
 * gs_select_targets_f32 (candidate order and ties follow the map row order, which is the order of the
 * compacted set).  icp_scratch: gs_icp_scratch_bytes(n_src_bound, n_map_bound). */
GS_API int gs_icp_map_dc_f32(const float* src, int64_t n_src_bound, const int64_t* n_src_dev,
                             const float* map_points, const float* map_normals, const int32_t* pix,
                             int64_t n_map_bound, const int64_t* n_map_dev, int W, int ds, const float* init16,
                             const float* compose16, const gs_icp_params* params_host, float* out_T16,
                             void* icp_scratch, void* stream);

/* Per-iteration record kept in icp_scratch for the backward pass / diagnostics:
 * gs_icp_trace_f32 copies (numiters, 12) floats = [err, new_err, damp_after, sigmoid, xi(6), pad(2)]. */
GS_API int gs_icp_trace_f32(const void* icp_scratch, int numiters, float* trace_out, void* stream);

/* ------------------------------------------------- K5: surfel association (PointFusion) -
 * find_similar_map_points on an explicit table (slam/fusionutils.py:381-401):
 * mask[r] = |f - p| < dist_th  &&  f_n . p_n > dot_th  for row r = [b, n, h, w]. */
GS_API int gs_similar_rows_f32(const int64_t* rows, int64_t n_rows, const float* points,
                        const float* normals, const float* gvertex, const float* gnormal, int W,
                        float dist_th, float dot_th, uint8_t* mask, void* stream);

/* find_best_unique_correspondences on an explicit table (slam/fusionutils.py:489-544):
 * per pixel the row minimising (1/(ccount+1e-20), |p-f|^2, n); output rows sorted by (h, w)
 * as [b, n, h, w].  best_pix: device int32[H*W] work array (also returned: winner n or -1). */
GS_API int gs_best_unique_rows_f32(const int64_t* rows, int64_t n_rows, const float* points,
                            const float* ccounts, const float* gvertex, int H, int W, int64_t b,
                            int32_t* best_pix, int64_t* rows_out, int64_t* count_out,
                            void* scratch, void* stream);

/* Fused find_correspondences (slam/fusionutils.py:549-577) without tables:
 * pix[] (from gs_project_map_f32) + map + frame -> best_pix[H*W] = winning map index or -1.
 * similar (may be NULL): uint8[n_map] = is_similar_mask scattered by map index. */
GS_API int gs_associate_f32(const int32_t* pix, int64_t n_map, const float* points,
                     const float* normals, const float* ccounts, const float* gvertex,
                     const float* gnormal, int H, int W, float dist_th, float dot_th,
                     int32_t* best_pix, uint8_t* similar, void* scratch, void* stream);

/* best_pix[] -> ordered table rows [b, n, h, w] sorted by (h, w). */
GS_API int gs_best_table_i64(const int32_t* best_pix, int H, int W, int64_t b, int64_t* rows_out,
                      int64_t* count_out, void* scratch, void* stream);
/* table rows -> best_pix[] (for fuse_with_map called with an explicit table). */
GS_API int gs_rows_to_best_pix(const int64_t* rows, int64_t n_rows, int H, int W, int32_t* best_pix,
                        void* stream);

/* ------------------------------------------------------ K6: merge + append (PointFusion) -
 * fuse_with_map (slam/fusionutils.py:653-720) + Pointclouds.append_points
 * (structures/pointclouds.py:1117-1237) on a capacity-backed surfel store:
 *   matched rows n = best_pix[p]:  cc' = cc + a;  x' = (cc*x + a*f) * (1/cc')  for points,
 *   normals, colours;  every other row is rewritten as (cc*x)*(1/cc) exactly as the
 *   reference does (renorm_all != 0; 0 skips that and leaves unmatched rows untouched).  The reference skips
 *   the merge when the correspondence table OF THE WHOLE BATCH is empty (:659); this call sees one sequence, so
 *   renorm_all = 1 skips it when this sequence's table is empty and renorm_all = 2 never skips it (the caller knows
 *   that another sequence of the batch has matches);
 *   unmatched valid pixels are appended in raster order at rows n_map .. n_map+n_new-1.
 * The arrays must have room for n_map + H*W rows.  n_map_host is the current size;
 * new_count_out: device int64[1] receives n_map + n_new. */
GS_API int gs_fuse_append_f32(float* points, float* normals, float* colors, float* ccounts,
                       int64_t n_map_host, int64_t capacity, const int32_t* best_pix,
                       const float* gvertex, const float* gnormal, const float* rgb,
                       const float* alpha, const float* depth, int H, int W, int renorm_all,
                       int64_t* new_count_out, void* scratch, void* stream);

/* update_map_aggregate (slam/fusionutils.py:725-758) / pointclouds_from_rgbdimages
 * (structures/utils.py:7-57): append every valid pixel, raster order.  normals / colors /
 * ccounts (with gnormal / rgb / alpha) may be NULL. */
GS_API int gs_append_valid_f32(float* points, float* normals, float* colors, float* ccounts,
                        int64_t n_map_host, int64_t capacity, const float* gvertex,
                        const float* gnormal, const float* rgb, const float* alpha,
                        const float* depth, int H, int W, int64_t* new_count_out, void* scratch,
                        void* stream);

/* ICP source set of a frame without compaction (the points of downsample_rgbdimages,
 * odometry/icputils.py:654-668, computed from the LOCAL vertex map and the pose as in
 * structures/rgbdimages.py:681-708): out_pts (ceil(H/ds) * ceil(W/ds), 3), raster order, NaN where the
 * lattice pixel has no depth.  The grid path of gs_icp_f32 / gs_icp_dc_f32 ignores NaN source points
 * (no search, no row, out_idx = -1), so the lattice is a valid `src` as is. */
GS_API int gs_lattice_source_f32(const float* vertex, const float* depth, const float* pose16, int H, int W, int ds,
                                 float* out_pts, void* stream);

/* ---- dataset -> device ingest (datasets/tum.py:448-477 _preprocess_color / _preprocess_depth; the same
 * two steps in datasets/icl.py and datasets/scannet.py).  raw: the decoded PNG on the device (depth
 * uint16 (H0, W0); colour uint8 (H0, W0, 3)); out: float32 (H, W) / (H, W, 3).  Depth: cv2.INTER_NEAREST
 * to (H, W), then / scale_div (TUM 5000, ICL 5000, ScanNet 1000) in float64, cast last.  Colour:
 * cv2.INTER_LINEAR in float64 with float32 weights, optional / 255.  Same size: exact copy. */
GS_API int gs_ingest_depth_u16_f32(const uint16_t* raw, int H0, int W0, float* out, int H, int W,
                                   double scale_div, void* stream);
GS_API int gs_ingest_color_u8_f32(const uint8_t* raw, int H0, int W0, float* out, int H, int W, int normalize,
                                  void* stream);
/* Streaming ingest (round 4; datasets/tum.py:352-434 per frame, datasets/datautils.py:73-118): n_frames native-size frames
 * in one launch -- depth uint16 (n, H, W) -> float32 metres (raw / scale_div in float64, then float32), colour uint8
 * (n, H, W, 3) -> float32 (optionally / 255): the arithmetic of the two entry points above without a resize.  Either pair
 * may be NULL.  n_frames * H * W must be a multiple of 4. */
GS_API int gs_ingest_frames_native_f32(const uint16_t* depth_raw, const uint8_t* color_raw, int64_t n_frames, int H, int W,
                                       double scale_div, int normalize, float* depth_out, float* color_out, void* stream);
/* Device-side address of a pinned host allocation (hipHostGetDevicePointer), for kernels that read raw frames straight
 * from host memory; GS_ERR_INVALID when the range is not device-mapped. */
GS_API int gs_host_device_pointer(const void* host_ptr, void** dev_ptr_out);

/* ---- the per-frame map pipeline with the surfel count kept ON THE DEVICE -------------------
 * Same kernels and results as the functions they are named after; `n_map_bound` (host) is an
 * upper bound of the surfel count used for launch geometry / scratch sizing, the actual count is
 * read by the kernels from `n_map_dev` (int64[1], typically the new_count_out of the previous
 * frame's gs_fuse_append_dc_f32).  With these, one PointFusion frame (slam/icpslam.py:137-161 +
 * slam/fusionutils.py:761-789) never returns to the host: no read-back, no stream sync.
 * new_count_out must not alias n_map_dev.  Capacity must cover n_map_bound + H*W rows. */
GS_API int gs_project_map_dc_f32(const float* points, int64_t n_map_bound, const int64_t* n_map_dev,
                                 const float* pose16, const float* K16, int H, int W, int32_t* pix,
                                 void* stream);
GS_API int gs_select_targets_dc_f32(const int32_t* pix, int64_t n_map_bound, const int64_t* n_map_dev, int W,
                                    int ds, const float* points, const float* normals, const float* colors,
                                    float* out_pts, float* out_nrm, float* out_rgb, int64_t cap,
                                    int64_t* count_out, void* scratch, void* stream);
GS_API int gs_associate_dc_f32(const int32_t* pix, int64_t n_map_bound, const int64_t* n_map_dev,
                               const float* points, const float* normals, const float* ccounts,
                               const float* gvertex, const float* gnormal, int H, int W, float dist_th,
                               float dot_th, int32_t* best_pix, uint8_t* similar, void* scratch, void* stream);
GS_API int gs_fuse_append_dc_f32(float* points, float* normals, float* colors, float* ccounts,
                                 int64_t n_map_bound, const int64_t* n_map_dev, int64_t capacity,
                                 const int32_t* best_pix, const float* gvertex, const float* gnormal,
                                 const float* rgb, const float* alpha, const float* depth, int H, int W,
                                 int renorm_all, int64_t* new_count_out, void* scratch, void* stream);
GS_API int gs_append_valid_dc_f32(float* points, float* normals, float* colors, float* ccounts,
                                  int64_t n_map_bound, const int64_t* n_map_dev, int64_t capacity,
                                  const float* gvertex, const float* gnormal, const float* rgb,
                                  const float* alpha, const float* depth, int H, int W,
                                  int64_t* new_count_out, void* scratch, void* stream);

/* Backward of gs_fuse_append_f32 = reverse mode of fuse_with_map (slam/fusionutils.py:653-720): adjoints of
 * the fused map (n_new rows; the first n_old are the merged old rows, the rest the appended pixels in raster
 * order) -> adjoints of the old map rows (values BEFORE the merge are passed in) and of the frame's global
 * vertex / normal maps, colours (H, W, 3) and alpha (H, W).  best_pix: the correspondence table used in the
 * forward.  scratch: gs_scratch_bytes(n_old, H * W). */
GS_API int gs_fuse_append_backward_f32(const float* points, const float* normals, const float* colors,
                                       const float* ccounts, int64_t n_old, const int32_t* best_pix,
                                       const float* gvertex, const float* gnormal, const float* rgb,
                                       const float* alpha, const float* depth, int H, int W, int renorm_all,
                                       const float* P_bar, const float* N_bar, const float* C_bar,
                                       const float* F_bar, int64_t n_new, float* old_points_bar,
                                       float* old_normals_bar, float* old_colors_bar, float* old_ccounts_bar,
                                       float* gvertex_bar, float* gnormal_bar, float* rgb_bar, float* alpha_bar,
                                       void* scratch, void* stream);

/* update_map_fusion (slam/fusionutils.py:761-789) of one sequence as ONE call: global maps of the frame under
 * `pose16` (structures/rgbdimages.py:681-762), projection + association of the map (fusionutils.py:198-577) and
 * the confidence-weighted merge + ordered append (fusionutils.py:580-722), regrouped into 4 launches (round 5: no pick pass over the map).  Same
 * results, bit for bit, as gs_global_maps_f32 + gs_project_map_dc_f32 + gs_associate_dc_f32 +
 * gs_fuse_append_dc_f32.  vertex / normal: LOCAL maps (H, W, 3); alpha (H, W); outputs gvertex / gnormal
 * (H, W, 3), best_pix (H*W) (the correspondence table, -1 = none), new_count_out (must not alias n_map_dev;
 * n_map_dev may be NULL = the bound is exact).  capacity >= n_map_bound + H*W. */
GS_API int64_t gs_update_map_scratch_bytes(int64_t n_map_bound, int H, int W);
GS_API int gs_update_map_fusion_dc_f32(float* points, float* normals, float* colors, float* ccounts,
                                       int64_t n_map_bound, const int64_t* n_map_dev, int64_t capacity,
                                       const float* vertex, const float* normal, const float* depth,
                                       const float* rgb, const float* alpha, const float* pose16, const float* K16,
                                       int H, int W, float dist_th, float dot_th, int renorm_all, float* gvertex,
                                       float* gnormal, int32_t* best_pix, int64_t* new_count_out, void* scratch,
                                       void* stream);

/* ---- the frame loop for B INDEPENDENT sequences per call -----------------------------------------------
 * The reference loops `for b in range(B)` over the sequences of a batch (odometry/gradicp.py:105,
 * odometry/icp.py:84, slam/fusionutils.py:710-713); one 640x480 sequence cannot fill an MI355X (its frame is a
 * chain of ~50 dependent launches).  These entry points run EVERY kernel of a frame for all B
 * sequences at once (workgroup b serves sequence b mod B, so with B = 8 every sequence lives on one XCD), which
 * pays the dependent-launch floor once per B frames.  Per sequence the results are bit-identical to the
 * one-sequence entry points they are named after (same device functions).  The descriptor arrays are HOST arrays
 * of device pointers; nothing is read back. */
typedef struct gs_map_view {
  float* points;        /* (capacity, 3) */
  float* normals;       /* (capacity, 3) */
  float* colors;        /* (capacity, 3); may be NULL where only points / normals are read */
  float* ccounts;       /* (capacity, 1); idem */
  int64_t capacity;     /* rows the buffers hold */
  int64_t n_bound;      /* host-side upper bound of the surfel count (launch geometry, scratch sizing) */
  const int64_t* n_dev; /* device int64[1]: the actual count, or NULL when n_bound is exact */
} gs_map_view;

/* K1 for n_frames = B x frames_per_K frames in one launch (an RGBDImages of B sequences x L frames: frames_per_K =
 * L): frame f = b * L + l reads the (H, W) depth image at depth + b * depth_stride_seq + l * depth_stride_frame
 * (strides in floats: a contiguous stack has L*H*W and H*W; a one-frame slice frames[:, s] of a longer stack keeps
 * the stack's strides, so no copy is needed) and the intrinsics K16 + 16 * b; outputs are dense: vertex / normal
 * (n_frames, H, W, 3), alpha (n_frames, H, W); normal / alpha may be NULL.  Same arithmetic as gs_frame_maps_f32. */
GS_API int gs_frame_maps_batch_f32(const float* depth, int64_t depth_stride_seq, int64_t depth_stride_frame,
                                   const float* K16, int n_frames, int frames_per_K, int H, int W, float two_sigma_sq,
                                   float* vertex, float* normal, float* alpha, void* stream);

/* ICPSLAM._localize (slam/icpslam.py:238-247) for B sequences: ICP source = the live frame's [::ds, ::ds] lattice
 * under the previous pose (gs_lattice_source_f32), targets = the map rows that project onto that lattice in the
 * previous frame (gs_project_map_dc_f32 + the selection of gs_select_targets_f32, binned straight from the map),
 * numiters (grad)LM iterations, result composed with the previous pose: out_pose16 = T_icp * prev_pose16
 * (the transform gs_icp_map_dc_f32 returns).  scratch: gs_localize_scratch_bytes(H, W, ds, rows) bytes per sequence
 * with rows = max(map.capacity, map.n_bound): the layout follows the CAPACITY of the map buffers, so that it does not
 * move from frame to frame while the map grows inside them (after the call the scratch holds the solver state / trace
 * at the offset gs_icp_trace_f32 expects, the binned targets and the candidate lists of the solve). */
typedef struct gs_localize_seq {
  const float* vertex;      /* live frame, LOCAL vertex map (H, W, 3); gs_localize_batch_f32 needs it (inside the one-call
                             * step it may be NULL: the local vertex of a lattice pixel is then computed from depth and K16) */
  const float* depth;       /* live frame depth (H, W) */
  const float* K16;         /* intrinsics of the previous frame */
  const float* prev_pose16; /* pose of the previous frame (initial guess and composition) */
  gs_map_view map;          /* points + normals are read; n_bound > 0 */
  float* out_pose16;        /* recovered pose of the live frame */
  void* scratch;
} gs_localize_seq;
GS_API int64_t gs_localize_scratch_bytes(int H, int W, int ds, int64_t n_map_bound);
GS_API int gs_localize_batch_f32(const gs_localize_seq* seqs_host, int B, int H, int W, int ds,
                                 const gs_icp_params* params_host, void* stream);
/* Diagnostics of the candidate lists of ordinary source points (round 4; tests, tools; synchronises the stream) for the
 * last solve a scratch was used for; H, W, ds and map_rows (= max(map.capacity, map.n_bound) of that call) locate the
 * counters in the scratch: out[h] = source points whose list gave no proof in launch h of the solve (h = 2 x
 * iteration + half; they were re-searched by the 2x2x2 scan and got a new list), out[64 + h] = source points whose list
 * was empty (no radius fitted the slots: re-searched as well), out[128 + h] = source points that had no list in launch h
 * because neither the 2x2x2 stage nor the cubes could prove them (as without lists).  All zero when the solve kept no
 * lists (GRADSLAM_HIP_ICP_LISTS=0, blocks walking several groups of row units) and for the launches before the lists
 * start (GRADSLAM_HIP_ICP_LISTS_FROM).  out_host holds 192 values.  With GRADSLAM_HIP_DEBUG_GRID set the call also
 * prints the header of the solve's target grid to stderr. */
GS_API int gs_localize_list_stats_i64(const void* scratch, int H, int W, int ds, int64_t map_rows, int64_t* out192_host,
                                      void* stream);
/* Diagnostics of the last solve a scratch was used for (ABI v3; tests, tools; synchronises the stream; arguments as
 * gs_localize_list_stats_i64): out8[3] = source points whose list the list-building launch flagged as weak (counted only
 * with GRADSLAM_HIP_ICP_WEAK_ROOM > 0); every other word of out8 is 0 (they reported an engine that has been retired;
 * the signature stays). */
GS_API int gs_localize_solve_stats_i64(const void* scratch, int H, int W, int ds, int64_t map_rows, int64_t* out8_host,
                                       void* stream);

/* update_map_fusion (slam/fusionutils.py:761-789) for B sequences: gs_update_map_fusion_dc_f32 per sequence, 4
 * launches for the whole batch.  scratch: gs_update_map_scratch_bytes(map.n_bound, H, W) per sequence. */
typedef struct gs_update_seq {
  gs_map_view map;          /* all four attributes, capacity >= n_bound + H*W */
  const float* vertex;      /* LOCAL vertex / normal maps (H, W, 3) */
  const float* normal;
  const float* depth;       /* (H, W) */
  const float* rgb;         /* (H, W, 3) */
  const float* alpha;       /* (H, W) */
  const float* pose16;      /* the frame's (recovered) pose */
  const float* K16;
  float* gvertex;           /* out: global maps (H, W, 3) */
  float* gnormal;
  int32_t* best_pix;        /* out, optional: correspondence table (H*W), -1 = none.  NULL (for every sequence of the call): */
                            /* not written -- maps and counts are the same, the winners' scattered stores are saved        */
  int64_t* new_count_out;   /* out: device int64[1]; must not alias map.n_dev */
  void* scratch;
} gs_update_seq;
GS_API int gs_update_map_fusion_batch_f32(const gs_update_seq* seqs_host, int B, int H, int W, float dist_th,
                                          float dot_th, int renorm_all, void* stream);

/* One frame of PointFusion.step (slam/icpslam.py:140-178 with the _map override of slam/pointfusion.py:107-112) for B
 * sequences in ONE call: the live frames' local maps (gs_frame_maps_batch_f32), the poses (gs_localize_batch_f32) and the
 * map update under those poses (gs_update_map_fusion_batch_f32) -- the same kernels in the same order, enqueued from
 * C so that the host cost of a frame is one foreign call (49 launches; the host runs frames ahead of the device, so the
 * launches wait in the queue: a graph replay of the ICP launches, which round 3 had, bought nothing and went with that engine).
 * vertex / normal / alpha of all sequences must be dense ((B, H, W, 3) / (B, H, W): seqs[b].vertex = seqs[0].vertex +
 * b * 3 * H * W, ...) and the depth images equally strided (seqs[b].depth = seqs[0].depth + b * stride). */
typedef struct gs_step_seq {
  const float* depth;        /* live frame (H, W) */
  const float* rgb;          /* (H, W, 3) */
  const float* K16;          /* intrinsics (of the previous = live frame) */
  const float* prev_pose16;  /* pose of the previous frame */
  float* out_pose16;         /* out: recovered pose of the live frame (must not alias prev_pose16) */
  float* vertex;             /* out, optional (with alpha): LOCAL vertex map (H, W, 3) */
  float* normal;             /* out: LOCAL normal map (H, W, 3) */
  float* alpha;              /* out, optional (with vertex): sample confidences (H, W).  vertex and alpha both NULL (for every  */
                             /* sequence of the call; needs gvertex == NULL): not written -- the step computes the local vertex */
                             /* of a pixel from depth and K16 where it uses it (same bits); gs_frame_maps_batch_f32 on demand  */
  float* gvertex;            /* out, optional: global maps under the recovered pose.  Both NULL (for every sequence of the */
  float* gnormal;            /* call): not written -- the update computes the global vertex / normal of a pixel where it   */
                             /* uses them (same bits) and skips its per-pixel pass; gs_global_maps_f32 gives them on demand */
  int32_t* best_pix;         /* out, optional: correspondence table (H*W).  NULL (for every sequence of the call): not written */
  int64_t* new_count_out;    /* out: device int64[1], must not alias map.n_dev */
  gs_map_view map;           /* all four attributes; n_bound > 0; capacity >= n_bound + H*W */
  void* loc_scratch;         /* gs_localize_scratch_bytes(H, W, ds, map.capacity) */
  void* upd_scratch;         /* gs_update_map_scratch_bytes(map.capacity, H, W) */
} gs_step_seq;
GS_API int gs_pointfusion_step_batch_f32(const gs_step_seq* seqs_host, int B, int H, int W, int ds,
                                         const gs_icp_params* params_host, float two_sigma_sq, float dist_th,
                                         float dot_th, int renorm_all, void* stream);

/* API-level projective / Lie helpers (the SLAM kernels fuse their own copies; these are the drop-in names).
 * gs_project_points_f32: project_points (geometry/projutils.py:92-238) on n points of cdim (3 | 4) coordinates; point i
 *   uses the 4x4 matrix proj16 + 16 * (i / pts_per_mat); out_uv (n, 2) = (x'/z', y'/z'), z' = 1 where it is 0.
 * gs_unproject_points_f32: unproject_points (geometry/projutils.py:241-402): (K^-1 [u v w]) * depth, pdim (2 | 3).
 * gs_lie_small_f32: op 0 so3_hat (3 -> 3x3), 1 se3_hat (6 -> 4x4), 2 so3_exp (3 -> 3x3) (geometry/se3utils.py:11-74). */
GS_API int gs_project_points_f32(const float* cam_coords, int cdim, int64_t n, const float* proj16, int64_t pts_per_mat,
                                 float* out_uv, void* stream);
GS_API int gs_unproject_points_f32(const float* pixel_coords, int pdim, int64_t n, const float* kinv9,
                                   int64_t pts_per_mat, const float* depths, float* out_xyz, void* stream);
GS_API int gs_lie_small_f32(int op, const float* in, float* out, void* stream);

/* ------------------------------------------------------------------ the model view ------
 * A surfel map seen from a pose: a z-buffered point render of B maps under L views each (the reference
 * has no such call; its Pointclouds.open3d / .plotly viewers are the nearest thing, structures/pointclouds.py:1239, :1296).
 * Row i of a map lands on the pixel (h, w) that gs_project_map_f32 gives it for the view's pose and the image size
 * H x W (which need not be the capture size); its depth z is the third camera-frame coordinate of that projection.  The
 * winner of a pixel is the row of smallest z, the lowest row index among equal z: one 64-bit key (bits(z) << 32 | i)
 * under atomicMin, so every output is a pure function of the inputs (no dependence on thread order).
 * Filters (all off at 0): rows with ccount < min_confidence are skipped (min_confidence > 0); with cull_backfaces rows
 * whose camera-frame normal nc has (nc0 q0 + nc1 q1) + nc2 q2 >= 0 at their camera-frame point q are skipped; a row
 * competes for every pixel of the (2 radius + 1)^2 square around (h, w) clipped to the image, radius in 0..3.
 * Outputs per sequence, (L, H, W, C) row-major, any may be NULL: depth (C = 1) = z of the winner, else 0; color (3) =
 * its colour, else 0; normal (3) = its normal rotated into the camera frame, else 0; confidence (1) = its ccount, else
 * 0; index (int64, no C) = its row, else -1.  map.normals / colors / ccounts may be NULL where no requested output or
 * filter reads them; map.capacity is not used; maps of 2^32 rows or more are rejected.  poses16: L camera-to-world
 * matrices; K16: one intrinsics matrix.  scratch: gs_render_scratch_bytes(L, H, W) bytes per sequence (its contents
 * before and after the call mean nothing).  Views are served 4 per launch; the map is read once per launch. */
typedef struct gs_render_seq {
  gs_map_view map;
  const float* poses16;  /* (L, 16) */
  const float* K16;
  float* depth;          /* out (L, H, W) */
  float* color;          /* out (L, H, W, 3) */
  float* normal;         /* out (L, H, W, 3) */
  float* confidence;     /* out (L, H, W) */
  int64_t* index;        /* out (L, H, W) */
  void* scratch;
} gs_render_seq;
GS_API int64_t gs_render_scratch_bytes(int views, int H, int W);
GS_API int gs_render_map_dc_f32(const gs_render_seq* seqs_host, int B, int L, int H, int W, int radius,
                                float min_confidence, int cull_backfaces, void* stream);

/* Reverse mode of gs_render_map_dc_f32.  The render is a hard z-buffer: which row wins which pixel (the `index` image of
 * the forward, passed back in) and the two filters are constants; gradients flow through the values written for the
 * winner.  With T = [R t; 0 1] the view's pose, row n the winner of pixel i and zb / cb / ob / fb the adjoints of the
 * depth / colour / normal / confidence images at i:
 *   points_bar[n][k] += R[k][2] zb;  normals_bar[n][k] += sum_j R[k][j] ob_j;  colors_bar[n] += cb;  ccounts_bar[n] += fb;
 *   poses_bar[v][k][j] += n_k ob_j (j < 3);  poses_bar[v][k][2] += (p_k - t_k) zb;  poses_bar[v][k][3] -= R[k][2] zb
 * summed over all pixels and views a row wins (row outputs) / all pixels of the view (poses_bar[v], bottom row zero).
 * K16 gets no gradient.  map, poses16, K16, H, W and radius must be those of the forward call (the map rows are
 * re-projected to find the pixels they could have won); map.colors / ccounts / capacity are not used.  Any upstream image
 * may be NULL: its terms are skipped; they are read only at pixels with a winner (their contents at empty pixels mean
 * nothing).  Any output may be NULL.  The row outputs hold map.n_bound rows ((n_bound, 3), ccounts_bar (n_bound)), every
 * row is written: rows that win nothing and rows at or beyond the count (map.n_dev included) receive exact zeros, so the
 * buffers need no clearing.  scratch: gs_render_backward_scratch_bytes(L, H, W, map.n_bound) bytes per sequence, needed
 * with poses_bar.  No float atomics: sums are taken in float64 in a fixed order, every output is bitwise reproducible and
 * poses_bar[v] does not depend on the other views of the call.  Views are served 4 per launch: with L > 4 the row outputs
 * are rounded to float32 after each group of 4 views and the next group adds its float64 sums to those float32 values
 * (one more rounding per group, in view order); B sequences are served 8 per launch, each exactly as in a call of its own. */
typedef struct gs_render_backward_seq {
  gs_map_view map;
  const float* poses16;        /* (L, 16) */
  const float* K16;
  const int64_t* index;        /* (L, H, W): the index image the forward wrote */
  const float* depth_bar;      /* upstream adjoints: (L, H, W) */
  const float* color_bar;      /* (L, H, W, 3) */
  const float* normal_bar;     /* (L, H, W, 3) */
  const float* confidence_bar; /* (L, H, W) */
  float* points_bar;           /* out (n_bound, 3) */
  float* normals_bar;          /* out (n_bound, 3) */
  float* colors_bar;           /* out (n_bound, 3) */
  float* ccounts_bar;          /* out (n_bound) */
  float* poses_bar;            /* out (L, 16) */
  void* scratch;
} gs_render_backward_seq;
GS_API int64_t gs_render_backward_scratch_bytes(int views, int H, int W, int64_t n_bound);
GS_API int gs_render_map_backward_dc_f32(const gs_render_backward_seq* seqs_host, int B, int L, int H, int W,
                                         int radius, void* stream);

/* ------------------------------------------------------------------ surfel radii ------
 * Keller et al. give every surfel a radius; the map fuses it like any per-surfel attribute (a one-channel float32
 * feature layer, gs_fuse_features_batch with the colour fusion's weights) and the model view turns it into a splat size.
 *
 * gs_surfel_radius_f32: the radius of every depth sample of n images.  depth: image i starts at depth + i *
 * depth_stride (H * W contiguous floats); normal: the frames' LOCAL normal maps, image i at normal + i * normal_stride
 * (H * W * 3 contiguous floats); K16: n intrinsics matrices (n, 16).  float32, one rounding per operation, no FMA:
 *   fbar = 0.5f * (K[0][0] + K[1][1]);  r0 = (0.70710678f * z) / fbar;  c = fabsf(n_z)
 *   rho  = fminf(r0 / c, 2.0f * r0)   (c == 0: 2.0f * r0)      -- Keller's radius, ElasticFusion's cap on oblique surfaces
 *   valid = z > 0 and n finite and not all zero;  rho = +0.0f where not valid
 * radius (n, H, W) float32 and valid (n, H, W) uint8 (may be NULL) are contiguous outputs.
 *
 * gs_render_map_radii_dc_f32: gs_render_map_dc_f32 with a square per row.  radii_host: a host array of B device
 * pointers, radii_host[b] = map.n_bound floats (metres) for sequence b.  Row n of radius rho whose camera-frame depth in a
 * view is q2 > 0 competes for the (2 r + 1)^2 square around its pixel, clipped to the image, with
 *   x = (rho * fbar) / q2   (float32, two operations, fbar of the view's K16 as above)
 *   r = (rho > 0 and 0 < x < inf) ? min(max_radius, (int)floorf(x)) : 0          max_radius in 0..8
 * (a radius that is 0, negative, NaN or +inf gives r = 0).  Keys, atomicMin, the resolve pass, the filters, the outputs
 * and the scratch (gs_render_scratch_bytes) are those of gs_render_map_dc_f32: the images are a pure function of the
 * inputs, and where every row of a view has r = k <= 3 they are bit for bit those of radius = k.
 *
 * gs_render_map_radii_backward_dc_f32: gs_render_map_backward_dc_f32 for that forward (radii_host and max_radius must be
 * the forward's; scratch: gs_render_backward_scratch_bytes).  Each row is re-projected with its own r to find the pixels
 * it could have won; the radii are a constant of the gradient, like the winners.  The same sums in the same order: no
 * float atomics, bitwise reproducible. */
GS_API int gs_surfel_radius_f32(const float* depth, int64_t depth_stride, const float* normal, int64_t normal_stride,
                                const float* K16, int64_t n, int H, int W, float* radius, uint8_t* valid, void* stream);
GS_API int gs_render_map_radii_dc_f32(const gs_render_seq* seqs_host, const float* const* radii_host, int B, int L, int H,
                                      int W, int max_radius, float min_confidence, int cull_backfaces, void* stream);
GS_API int gs_render_map_radii_backward_dc_f32(const gs_render_backward_seq* seqs_host, const float* const* radii_host,
                                               int B, int L, int H, int W, int max_radius, void* stream);

/* ------------------------------------------------------------------ pruning the map ------
 * A stable, out-of-place compaction of B maps (the reference never removes a surfel; Keller et al.'s point-based fusion
 * drops those that stay unstable).  With n = min(*n_dev, n_bound) (n_bound when n_dev is NULL), row r < n survives iff
 *   (keep == NULL || keep[r] != 0)  &&  (!use_confidence || r >= young_from || features[r] >= min_confidence)
 * in float32: a NaN confidence fails the test, a confidence bit-equal to min_confidence passes.  Survivor k of the input
 * is row k of every destination, moved bit for bit; *n_out = number of survivors, *removed_out = n - *n_out; destination
 * rows at or beyond *n_out are not written.  Rows are appended in birth order and the compaction keeps order, so "young"
 * is a row index: young_from = marks[young_mark] as it stands before the call (young_mark = -1: every row is old enough).
 * marks: up to 64 ascending row indices on the device ("epoch marks": the counts at earlier steps); the call rewrites
 * each mark m as the number of survivors among the rows < min(m, n).
 * normals / colors / features may be NULL (their destinations are then not used); use_confidence needs features with
 * F == 1 (the confidence count).  A destination must not be its source (GS_ERR_INVALID): the scatter of one tile lands
 * on the input of lower tiles that other blocks may still have to read.  scratch: gs_prune_scratch_bytes(n_bound) bytes
 * per sequence.  Sequences are served 8 per group of launches (count, tile scan, scatter, marks), whatever their sizes;
 * nothing is read back.  Every argument is checked before the first HIP call. */
typedef struct gs_prune_seq {
  const float* points;      /* (n_bound, 3) */
  const float* normals;     /* (n_bound, 3) or NULL */
  const float* colors;      /* (n_bound, 3) or NULL */
  const float* features;    /* (n_bound, F) or NULL; channel 0 is the confidence count when F == 1 */
  int32_t F;
  int64_t n_bound;          /* host-side upper bound of the row count (launch geometry, scratch sizing) */
  const int64_t* n_dev;     /* device int64[1]: the actual count, or NULL when n_bound is exact */
  float* points_out;        /* destinations: (capacity_out, 3) / (capacity_out, F) */
  float* normals_out;
  float* colors_out;
  float* features_out;
  int64_t capacity_out;     /* rows the destinations hold, >= n_bound */
  const uint8_t* keep;      /* (n_bound) or NULL */
  int64_t* marks;           /* device int64[n_marks], rewritten in place; may be NULL with n_marks == 0 */
  int32_t n_marks;          /* 0..64 */
  int32_t young_mark;       /* index into marks, or -1 */
  int64_t* n_out;           /* device int64[1] */
  int64_t* removed_out;     /* device int64[1] or NULL */
  void* scratch;
} gs_prune_seq;
GS_API int64_t gs_prune_scratch_bytes(int64_t n_bound);
GS_API int gs_prune_map_dc_f32(const gs_prune_seq* seqs_host, int B, float min_confidence, int use_confidence,
                               void* stream);

/* ------------------------------------------------------------------ free-space carving ------
 * Which rows of B maps do L depth frames each see through (Keller et al.'s "free-space violations"; the reference never
 * removes a surfel)?  The pass only marks; the removal is gs_prune_map_dc_f32 with the keep mask written here.
 * With n = min(*map.n_dev, map.n_bound) (n_bound when n_dev is NULL), row r < n with point p, and view l with the
 * camera-to-world pose T_l = poses16 + 16 l, the intrinsics K16 and the H x W depth image D_l = depth + l *
 * depth_stride_view: the row projects as in gs_project_map_f32 / gs_render_map_dc_f32 (the same device function: the
 * pixel (h, w) the map update and the model view give it, u_hi = (float)((double)W - 0.999), v_hi likewise), z is the
 * third camera-frame coordinate of that projection.  Row r VIOLATES view l iff all of
 *   - it projects into the frame, in front of the camera (rows behind the camera or outside the frame never violate);
 *   - D_l[h, w] > 0 (false for 0, negative values and NaN: no measurement, no evidence);
 *   - for every pixel (hh, ww) of the (2 window + 1)^2 square around (h, w), clipped to the image, with D_l[hh, ww] > 0:
 *     (D_l[hh, ww] - z) > margin, in float32, one subtraction and one compare.  Equality does not violate, a NaN z does
 *     not violate, pixels without depth abstain: the row lies in front of the nearest measured depth of its window.
 * violations[r] = number of views of the call that r violates; keep[r] = (violations[r] < min_views) ? 1 : 0.  Rows in
 * [n, n_bound) get violations = 0 and keep = 0 and are never read.  Both outputs hold n_bound elements, every one is
 * written (no clearing needed); either may be NULL, not both.  Only map.points, map.n_bound and map.n_dev are read.  Rows
 * of a depth image are contiguous; depth_stride_view is in floats (a (B, L, H, W, 1) stack is read in place).
 * margin finite and >= 0, window in 0..3, min_views >= 1, H * W < 2^31; every argument is checked before the first HIP
 * call.  One launch per 8 sequences whatever L is; no atomics, nothing is read back; the outputs are integers and a pure
 * function of the inputs. */
typedef struct gs_carve_seq {
  gs_map_view map;
  const float* depth;          /* view 0: (H, W), rows contiguous */
  int64_t depth_stride_view;   /* floats from one view's image to the next */
  const float* poses16;        /* (L, 16) */
  const float* K16;
  int32_t* violations;         /* out (n_bound) or NULL */
  uint8_t* keep;               /* out (n_bound) or NULL */
} gs_carve_seq;
GS_API int gs_free_space_dc_f32(const gs_carve_seq* seqs_host, int B, int L, int H, int W, float margin, int window,
                                int min_views, void* stream);

/* ------------------------------------------------------------------ voxel thinning ------
 * Which rows of B maps are the one surfel their voxel keeps (the voxel_down_sample of point-cloud libraries, without
 * averaging; the reference never removes a surfel)?  The pass only marks; the removal is gs_prune_map_dc_f32 with the
 * keep mask written here.  Additions only: the ABI version stays.
 * Per sequence, with n = min(*n_dev, n_bound) (n_bound when n_dev is NULL) and voxel_size a finite float32 > 0:
 *   - voxel of a row: q_c = floorf(p_c / voxel_size) per component, the correctly rounded float32 division, then floorf;
 *   - a row is GRIDDABLE iff all three p_c are finite and -2^20 <= q_c < 2^20 (tested on the float);
 *   - key = ((q_x + 2^20) << 42) | ((q_y + 2^20) << 21) | (q_z + 2^20): 63 bits;
 *   - score = the uint32 bit pattern of the confidence when confidence >= +0.0f holds in float32, else 0 (NaN and
 *     negative values score 0, -0.0 scores as +0.0, +inf is the largest); without a confidence pointer every score is 0;
 *   - among the griddable rows r < n of one voxel the WINNER has the largest score, ties go to the lowest row;
 *   - keep[r] = 1 iff r < n and the row is not griddable or is its voxel's winner; rows in [n, n_bound) get 0 and never
 *     compete; a non-griddable row is always kept and never competes;
 *   - winner[r] (int64) = the winner of r's voxel, r itself for a non-griddable row, -1 for r >= n.
 * Both outputs hold n_bound elements, every one is written (no clearing needed); either may be NULL, both only with
 * n_bound == 0.  confidence: (n_bound) floats (feature channel 0 of a surfel map with F == 1) or NULL.  unplaced: device
 * int32[1] or NULL; the call clears it and counts the rows for which the table ran out (they are kept, winner = r): it
 * stays 0 at the table's load of at most one half.  scratch: gs_voxel_keep_scratch_bytes(n_bound) bytes per sequence,
 * 16-byte aligned: an open-addressing table of the power of two >= max(2 n_bound, 1024) slots of 16 bytes (32 - 64
 * bytes per row of the bound), cleared by the call.  n_bound < 2^31.  Every argument is checked before the first HIP
 * call.  Two launches per 8 sequences (elect, resolve) after the clears; integer atomics only, no data-dependent loop
 * without a bound, nothing is read back; the outputs are integers, a pure function of the inputs and bitwise
 * reproducible; a second pass over the compacted map removes nothing. */
typedef struct gs_voxel_keep_seq {
  const float* points;       /* (n_bound, 3) */
  const float* confidence;   /* (n_bound) or NULL */
  int64_t n_bound;           /* host-side upper bound of the row count (launch geometry, table sizing) */
  const int64_t* n_dev;      /* device int64[1]: the actual count, or NULL when n_bound is exact */
  uint8_t* keep;             /* out (n_bound) or NULL */
  int64_t* winner;           /* out (n_bound) or NULL */
  int32_t* unplaced;         /* out: device int32[1] or NULL */
  void* scratch;
  int64_t scratch_bytes;
} gs_voxel_keep_seq;
GS_API int64_t gs_voxel_keep_scratch_bytes(int64_t n_bound);
GS_API int gs_voxel_keep_dc_f32(const gs_voxel_keep_seq* seqs_host, int B, float voxel_size, void* stream);

/* ------------------------------------------------------------------ bilateral depth filter ------
 * The edge-preserving pre-pass on the raw depth of Keller et al. and KinectFusion (no counterpart in the reference),
 * batched over n frames of H x W.  Frame f starts at depth + f * stride_frame and its row h at + h * stride_row (in
 * elements; stride_row >= W, rows contiguous): a frame slice of a longer stack and a channels-first stack are read in
 * place.  out (n, H, W) and the optional wsum (n, H, W) are contiguous.
 * A pixel is valid when d > 0 (false for 0, negatives and NaN).  An invalid centre is copied through, wsum = 0.  For a
 * valid centre q the window is visited in row-major order (dy = -radius..radius outer, dx inner, the centre in its
 * place); a neighbour p outside the image or invalid is skipped, otherwise, in float32 with one rounding per operation,
 *   g = alpha_of(dx, dy, 0, two_sigma_space_sq, eps 0)    e = alpha_of(d_p - d_q, 0, 0, two_sigma_range_sq, eps 0)
 *   w = g * e    S = S + w * d_p    W = W + w,            out_q = S / W,  wsum_q = W
 * with the specified exp of the alpha map.  two_sigma_*_sq = (float)(2 * sigma * sigma) evaluated in
 * double by the caller; both must be finite and > 0.  radius 0 ... 8; radius 0 returns the input bits.  out / wsum must
 * not overlap depth (GS_ERR_INVALID): blocks read each other's halo.  One launch per 65535 frames; every argument is
 * checked before the first HIP call. */
GS_API int gs_bilateral_depth_f32(const float* depth, int64_t stride_frame, int64_t stride_row, int n, int H, int W,
                                  int radius, float two_sigma_space_sq, float two_sigma_range_sq, float* out,
                                  float* wsum, void* stream);
/* Reverse mode of the above: depth_bar (n, H, W) from out_bar (n, H, W), the forward's out and wsum and the depth it
 * read.  A gather per input pixel in the window order of the forward, without atomics: bitwise reproducible.  Which
 * neighbours are valid is a constant of the gradient; at an invalid pixel depth_bar = out_bar.  The weights w are the
 * forward's float32 values, every other factor and both sums are float64, rounded once at the store.  depth_bar must
 * not overlap an input. */
GS_API int gs_bilateral_depth_backward_f32(const float* depth, int64_t stride_frame, int64_t stride_row,
                                           const float* out, const float* wsum, const float* out_bar, int n, int H,
                                           int W, int radius, float two_sigma_space_sq, float two_sigma_range_sq,
                                           float* depth_bar, void* stream);

/* ------------------------------------------------------------------ projective ICP against the model view ------
 * Frame-to-model tracking by projective data association (Keller et al., KinectFusion; no counterpart in the reference,
 * whose trackers search a 1-NN): every pixel of the live frame's [::stride, ::stride] lattice is carried by the current
 * pose estimate T into the model view -- the `index` image gs_render_map_dc_f32 wrote for the pose model_pose16 -- and is
 * paired with the map row that won the pixel it lands on; a point-to-plane Gauss-Newton step with constant damping
 * follows.  Slot k = i * Wl + j (Wl = ceil(W / stride)) stands for pixel (h, w) = (i stride, j stride); in float32, one
 * rounding per operation, with the device functions of the association and of the ICP solve:
 *   code 1  unless depth[h, w] > 0 (false for NaN)
 *   s = T v (the chain of gs_transform_points_f32), g = R_T n (the same chain without the translation)
 *   code 2  unless s projects into the model view (gs_project_map_f32's pixel for model_pose16, K16, H, W) at (h', w')
 *   code 3  unless 0 <= row = index[h', w'] < min(*map.n_dev, map.n_bound): a stale index is never dereferenced
 *   code 4  unless |s - points[row]| < dist_th;  code 5 unless g . normals[row] > dot_th   (gs_similar_rows_f32's tests)
 *   code 0: the row (a[6], b) of gs_gauss_newton_rows_f32 for source s and target points[row], normals[row]
 * The 28 sums (21 upper-triangular a_i a_j, 6 a_i b, b b) are float64 sums of exact products, in a FIXED order: chunks of
 * 256 consecutive slots (the last one padded with +0.0; a rejected slot is +0.0), inside a chunk a pairwise adjacent tree
 * (8 levels), the chunk partials added in ascending chunk order starting from the first.  No float atomics: every output
 * is bitwise reproducible.  An iteration then solves (AtA + damp I) xi = Atb as gs_solve_normal_eq_f32 does, and sets
 * T <- se3_exp(xi) T (the 4x4 product of the ICP loop); with no inlier xi = 0 and T keeps its bits.
 * gs_projective_icp_batch_f32 runs numiters iterations from init_pose16 for B sequences (8 per launch, two launches per
 * iteration, nothing read back) and writes out_pose16 and, when trace is not NULL, one row [inliers, (float)sum b b,
 * xi(6)] per iteration.  out_pose16 may be init_pose16.  scratch: gs_projective_icp_scratch_bytes(H, W, stride) bytes per
 * sequence.  dot_th = cos(angle threshold), dist_th in metres; damp > 0.  Every argument is checked before the first HIP
 * call. */
typedef struct gs_picp_seq {
  const float* vertex;        /* live frame, LOCAL vertex map (H, W, 3) */
  const float* normal;        /* live frame, LOCAL normal map (H, W, 3) */
  const float* depth;         /* live frame depth (H, W) */
  const float* K16;
  const int64_t* index;       /* (H, W): winning map row of the model view, or -1 */
  const float* model_pose16;  /* camera-to-world pose of the model view */
  gs_map_view map;            /* points + normals are read; colors / ccounts / capacity are not used */
  const float* init_pose16;   /* initial estimate (the batch entry) / the pose to linearise at (the rows entry) */
  float* out_pose16;          /* out: the estimate after numiters iterations (not used by the rows entry) */
  float* trace;               /* out, optional: (numiters, 8) */
  void* scratch;
} gs_picp_seq;
typedef struct gs_picp_params {
  int stride;
  int numiters;
  float damp;
  float dist_th;
  float dot_th;
} gs_picp_params;
GS_API int64_t gs_projective_icp_scratch_bytes(int H, int W, int stride);
GS_API int gs_projective_icp_batch_f32(const gs_picp_seq* seqs_host, int B, int H, int W,
                                       const gs_picp_params* params_host, void* stream);
/* ONE linearisation of one sequence at T = init_pose16: per slot (nslots = ceil(H / stride) * ceil(W / stride)) the code
 * (0 = used), the row (the index image's entry where one was read, i.e. codes 0, 3, 4, 5; else -1), a6 (nslots, 6) and b
 * (zeros unless the slot is used), plus the 28 sums (float64) and the inlier count.  Any output may be NULL. */
GS_API int gs_projective_icp_rows_f32(const gs_picp_seq* seq_host, int H, int W, int stride, float dist_th,
                                      float dot_th, int32_t* code, int64_t* row, float* a6, float* b, double* sums28,
                                      int64_t* count, void* stream);

/* ------------------------------------------------------------------ projective ICP: taped forward and backward ------
 * gs_projective_icp_tape_batch_f32 is gs_projective_icp_batch_f32 (same kernels, the same pose and trace bits) whose
 * finish kernel also writes, per iteration, the pose it linearised at (16 floats), the 28 float64 sums, the step xi (6
 * floats, 0 without inliers) and the inlier count to tapes_host[b], a device buffer of
 * gs_projective_icp_tape_bytes(numiters) bytes (328 per iteration: double S[28], float T[16], float xi[6], float pad[2],
 * int64 count), 8-byte aligned.
 *
 * gs_projective_icp_backward_batch_f32 is the reverse-mode pass through the numiters iterations: from pose_bar16 =
 * dL/d(out_pose) (its top three rows are read) to vertex_bar (H, W, 3; zero off the lattice), points_bar / normals_bar
 * (the first map.n_bound rows are written) and init_pose_bar16 (top three rows, a zero bottom row).  Differentiated per
 * used slot: s = R v + t, a = [m ; s x m], b = m . (p - s), A = sum a a^T, g = sum a b, xi = (A + damp I)^-1 g,
 * T <- exp(xi) T.  Constants: which slots are used and their rows (codes 1-5, both gates, the projection, the index
 * image), the device count, K, model_pose, depth and the live normal; the float32 roundings of the forward are treated as
 * the identity; an iteration without inliers passes the adjoint through.  The association is recomputed with the
 * forward's device functions at the taped float32 pose, so the inputs (the map rows included) must hold what they held
 * at the forward; a stale index entry is never dereferenced.  float64 inside, rounded once.  vertex_bar and
 * init_pose_bar16 are bitwise reproducible (the forward's fixed reduction shape, no atomics); points_bar / normals_bar
 * are float64 atomic adds, reproducible up to the order of the float64 additions (bitwise reproducible through
 * gs_projective_icp_ordered_backward_batch_f32, below).  Any output may be NULL: its work and
 * its buffer are skipped (with both map outputs NULL nothing of map size is touched).  scratch:
 * gs_projective_icp_backward_scratch_bytes(H, W, stride, n_map) bytes per sequence, n_map = map.n_bound when a map output
 * is asked for, else 0; scratch_bytes is what the caller provides and is checked.  8 sequences per launch, 2 numiters + 1
 * launches (plus one per map output), nothing read back.  Every argument is checked before the first HIP call. */
typedef struct gs_picp_backward_seq {
  const float* vertex;        /* the forward's inputs, as in gs_picp_seq */
  const float* normal;
  const float* depth;
  const float* K16;
  const int64_t* index;
  const float* model_pose16;
  gs_map_view map;
  const void* tape;           /* what the taped forward wrote */
  const float* pose_bar16;    /* upstream adjoint of the pose */
  float* vertex_bar;          /* out (H, W, 3), or NULL */
  float* points_bar;          /* out (n_bound, 3), or NULL */
  float* normals_bar;         /* out (n_bound, 3), or NULL */
  float* init_pose_bar16;     /* out (16), or NULL */
  void* scratch;
  int64_t scratch_bytes;
} gs_picp_backward_seq;
GS_API int64_t gs_projective_icp_tape_bytes(int numiters);
GS_API int gs_projective_icp_tape_batch_f32(const gs_picp_seq* seqs_host, void* const* tapes_host, int B, int H, int W,
                                            const gs_picp_params* params_host, void* stream);
GS_API int64_t gs_projective_icp_backward_scratch_bytes(int H, int W, int stride, int64_t n_map);
GS_API int gs_projective_icp_backward_batch_f32(const gs_picp_backward_seq* seqs_host, int B, int H, int W,
                                                const gs_picp_params* params_host, void* stream);

/* ------------------------------------------------------------------ projective ICP backward: the ordered mode ------
 * gs_projective_icp_ordered_backward_batch_f32 is the backward pass above -- of the plain tape (huber_delta = 0,
 * taped_scale = 0), of the robust tape (huber_delta > 0: gs_projective_icp_robust_backward_batch_f32, further down) and
 * of the scaled tape (taped_scale != 0: gs_projective_icp_scaled_backward_batch_f32; huber_delta is then not read) --
 * with BITWISE REPRODUCIBLE points_bar / normals_bar.  The point stage of an iteration does not add a slot's two
 * 3-vectors atomically; it records them, per slot k of the lattice:
 *   contrib[k][0:3] the contribution to points_bar[row], contrib[k][3:6] the one to normals_bar[row] (float64; zeros for
 *   a map output that is not asked for), key[k] = the slot's row, or 0x7fffffff for a slot that contributes nothing.
 * A settle step follows: one stable radix sort of the pairs (sequence << 32 | key, slot) of all sequences of a launch
 * group (up to 8), then one thread per run of equal keys.  The order contract: acc[row] starts at +0.0; the iterations
 * are processed numiters - 1 down to 0; in an iteration a row's run sum starts at 0.0 and adds the contributions of its
 * slots in ascending slot id, then acc[row] = acc[row] + run_sum; a row that nobody touches ends as +0.0; an iteration
 * without inliers records nothing (every key reads "none"); acc is rounded to float32 once at the end.  vertex_bar and
 * init_pose_bar16 have the bits of the other entries.  A launch group in which no map output is asked for runs the
 * launches of the other entries: nothing is recorded or sorted.
 * key_out (numiters, nslots) int32 / contrib_out (numiters, nslots, 6) float64, nslots = ceil(H / stride) ceil(W /
 * stride), device, either may be NULL: the record as it stood after the point stage of iteration `it`, in slice `it`
 * (a test's view of the pass).  They are written only for a sequence in a group that records (contrib_out only for a
 * sequence with a map output; where a key is "none" the contribution is not defined): fill them beforehand.
 * scratch per sequence: gs_projective_icp_ordered_backward_scratch_bytes(H, W, stride, n_map) bytes (n_map as above: the
 * other entries' scratch plus the record, 48 + 4 bytes per slot); sort_scratch: one buffer for the call,
 * gs_projective_icp_ordered_backward_sort_scratch_bytes(B, H, W, stride) bytes, 8-byte aligned (keys and values of
 * min(B, 8) nslots pairs, in and out, and the sort's temporary storage; not read when no map output is asked for).
 * Neither grows with numiters.  Both return 0 on bad arguments (the second also when min(B, 8) nslots >= 2^31).
 * Refused, before the first HIP call like every other bad argument: map.n_bound >= 0x7fffffff, min(B, 8) nslots >= 2^31. */
typedef struct gs_picp_ordered_backward_seq {
  gs_picp_backward_seq base;
  int32_t* key_out;           /* out (numiters, nslots), or NULL */
  double* contrib_out;        /* out (numiters, nslots, 6), or NULL */
} gs_picp_ordered_backward_seq;
GS_API int64_t gs_projective_icp_ordered_backward_scratch_bytes(int H, int W, int stride, int64_t n_map);
GS_API int64_t gs_projective_icp_ordered_backward_sort_scratch_bytes(int B, int H, int W, int stride);
GS_API int gs_projective_icp_ordered_backward_batch_f32(const gs_picp_ordered_backward_seq* seqs_host, int B, int H,
                                                        int W, const gs_picp_params* params_host, float huber_delta,
                                                        int taped_scale, void* sort_scratch,
                                                        int64_t sort_scratch_bytes, void* stream);

/* ------------------------------------------------------------------ projective ICP with a colour term ------
 * The projective ICP above plus a photometric row per slot (Steinbruecker / Kerl; Kintinuous, ElasticFusion, Open3D's
 * hybrid odometry): geometry alone does not constrain a pose on a wall or a floor, the texture does.  In float32, one
 * rounding per operation, no FMA in what is added here (gs_picp_color.hip spells out every operation):
 *
 * gs_model_intensity_f32: color (B, H, W, 3) and index (B, H, W) of gs_render_map_dc_f32 -> out (B, H, W, 4) =
 * (I, gx, gy, ok) per pixel, 16-byte aligned: I = (0.299 R + 0.587 G) + 0.114 B, gx = 0.5 (I[h, w+1] - I[h, w-1]),
 * gy = 0.5 (I[h+1, w] - I[h-1, w]); ok = 1 iff the pixel and its four neighbours are inside the image and have index >= 0,
 * else ok = 0 and gx = gy = 0 (a hole of the view never leaks a gradient).  Built once per localisation.
 *
 * A slot gets a colour row iff its code is 0 and ok = 1 at the pixel (h', w') the association read.  With q = R_m^T (s -
 * t_m) the camera-frame point and (u, v) the continuous pixel of the projector, Il the luma of color at the slot's pixel:
 *   r   = Il - ((I + gx (u - w')) + gy (v - h'))                     first-order model intensity at (u, v)
 *   Jq  = (gx fx / q2, gy fy / q2, -(gx fx q0 + gy fy q1) / q2^2),   Js = R_m Jq
 *   a_c = color_weight [Js, s x Js],  b_c = color_weight r           (the layout and signs of the geometric row)
 * color_weight is in metres per intensity unit, finite and >= 0.  The 28 terms of a slot are the exact float64 product of
 * the geometric factors plus that of the colour factors, the sum rounded once; then the fixed reduction order, the solve
 * and the update of the plain call: no float atomics, bitwise reproducible.  `count` stays the number of geometric
 * inliers (an iteration without one keeps the pose bits); the colour rows are counted alongside.
 * gs_projective_icp_color_batch_f32: as gs_projective_icp_batch_f32; base.trace rows are 9 floats: [inliers, (float) joint
 * sum of squares, xi(6), colour rows]; base.scratch: gs_projective_icp_color_scratch_bytes(H, W, stride) bytes.  Two
 * launches per iteration for 8 sequences, nothing read back.  Every argument is checked before the first HIP call. */
typedef struct gs_picp_color_seq {
  gs_picp_seq base;              /* as in the plain call (trace: (numiters, 9)) */
  const float* color;            /* live frame colour (H, W, 3) */
  const float* model_intensity;  /* (H, W, 4) of gs_model_intensity_f32 for the model view */
} gs_picp_color_seq;
GS_API int gs_model_intensity_f32(const float* color, const int64_t* index, int B, int H, int W, float* out,
                                  void* stream);
GS_API int64_t gs_projective_icp_color_scratch_bytes(int H, int W, int stride);
GS_API int gs_projective_icp_color_batch_f32(const gs_picp_color_seq* seqs_host, int B, int H, int W,
                                             const gs_picp_params* params_host, float color_weight, void* stream);
/* ONE joint linearisation at T = base.init_pose16: the outputs of gs_projective_icp_rows_f32 (sums28 now the joint sums),
 * plus per slot ac6 (nslots, 6), bc and colored (int32: 1 where the slot has a colour row; ac6 / bc are zero elsewhere),
 * and the number of colour rows.  Any output may be NULL. */
GS_API int gs_projective_icp_color_rows_f32(const gs_picp_color_seq* seq_host, int H, int W, int stride, float dist_th,
                                            float dot_th, float color_weight, int32_t* code, int64_t* row, float* a6,
                                            float* b, float* ac6, float* bc, int32_t* colored, double* sums28,
                                            int64_t* count, int64_t* color_count, void* stream);

/* ------------------------------------------------------------------ projective ICP: robust (Huber) weights ------
 * Opt-in Huber weights for every solve above (additions only: no struct or signature above changes, the tape row and
 * every *_scratch_bytes function are reused).  huber_delta (metres) applies to the point-to-plane residual b of a used
 * slot, color_huber_delta (intensity units of the map's colours) to the colour residual r before color_weight is applied;
 * both finite and >= 0, 0 = off.  In float32, one rounding per operation, no FMA:
 *   w  = |b| > huber_delta       ? huber_delta / |b|       : 1        (a NaN residual is not clipped)
 *   wc = |r| > color_huber_delta ? color_huber_delta / |r| : 1        (1 when color_huber_delta is 0)
 * The 28 terms of a used slot are (double)w * ((double)x * (double)y) -- the exact product, then one rounding -- and in
 * the joint solve (double)w * ((double)x_g * (double)y_g) + (double)wc * ((double)x_c * (double)y_c).  Everything else is
 * the plain solve's: the reduction order, the finish, the update, the counts (the inlier count does not depend on the
 * weights), "no geometric inlier keeps the pose bits".  The sum of squares (sums28[27], the second float of a trace row,
 * S[27] of a tape row) is the WEIGHTED sum of squares.  With every delta 0 an entry below launches the kernels of its
 * plain counterpart: the same bits.
 *
 * gs_projective_icp_robust_batch_f32: gs_projective_icp_batch_f32 (tapes_host NULL) or gs_projective_icp_tape_batch_f32
 * (per sequence a tape buffer) with Huber weights.
 * gs_projective_icp_robust_rows_f32: gs_projective_icp_rows_f32 plus weight (nslots): w of a used slot, 0 elsewhere; a6 / b
 * stay the unweighted rows, sums28 are the weighted sums.
 * gs_projective_icp_robust_backward_batch_f32: gs_projective_icp_backward_batch_f32 for a tape of the robust forward
 * with the same huber_delta.  The weight is differentiated; the clip flag of a used slot is a constant like the
 * association and is recomputed as the forward computed it (the float32 b at the taped pose against huber_delta).  With
 * c = xi . a, e = u . a, w' = -w / b for a clipped slot and 0 otherwise: ab = w ((b - c) u - e xi), and
 * bb = e (w + w' (b - c)) takes the place of e in sb, points_bar and normals_bar; the scalar stage is unchanged (the
 * taped S is the weighted system).  Reproducibility, NULL outputs, scratch and launch count as in the plain pass.
 * gs_projective_icp_color_robust_batch_f32 / _rows_f32: the colour entries with both thresholds; the rows entry also
 * returns weight (nslots) and color_weight_out (nslots): wc of a slot with a colour row, 0 elsewhere; ac6 / bc stay
 * unweighted.  Every argument is checked before the first HIP call. */
GS_API int gs_projective_icp_robust_batch_f32(const gs_picp_seq* seqs_host, void* const* tapes_host, int B, int H, int W,
                                              const gs_picp_params* params_host, float huber_delta, void* stream);
GS_API int gs_projective_icp_robust_rows_f32(const gs_picp_seq* seq_host, int H, int W, int stride, float dist_th,
                                             float dot_th, float huber_delta, int32_t* code, int64_t* row, float* a6,
                                             float* b, float* weight, double* sums28, int64_t* count, void* stream);
GS_API int gs_projective_icp_robust_backward_batch_f32(const gs_picp_backward_seq* seqs_host, int B, int H, int W,
                                                       const gs_picp_params* params_host, float huber_delta,
                                                       void* stream);
GS_API int gs_projective_icp_color_robust_batch_f32(const gs_picp_color_seq* seqs_host, int B, int H, int W,
                                                    const gs_picp_params* params_host, float color_weight,
                                                    float huber_delta, float color_huber_delta, void* stream);
GS_API int gs_projective_icp_color_robust_rows_f32(const gs_picp_color_seq* seq_host, int H, int W, int stride,
                                                   float dist_th, float dot_th, float color_weight, float huber_delta,
                                                   float color_huber_delta, int32_t* code, int64_t* row, float* a6,
                                                   float* b, float* ac6, float* bc, int32_t* colored, float* weight,
                                                   float* color_weight_out, double* sums28, int64_t* count,
                                                   int64_t* color_count, void* stream);

/* ------------------------------------------------------------------ projective ICP: Huber threshold from the median ------
 * Opt-in (additions only; the ABI version, every struct and every signature above stay): the threshold of the robust
 * weights is estimated from the residuals, per sequence and per iteration, at the pose T_k that iteration k linearises
 * at.  With n the number of used slots and b_i their float32 residuals (the values the robust kernel weights):
 *   med     = the LOWER MEDIAN of |b_i|: the element of 0-based rank (n - 1) / 2 in ascending order (an element of the
 *             set, never an average: exact; selected on the bit patterns, which order like the non-negative floats)
 *   c       = (float)huber_k * 1.4826f              one float32 product (huber_k = 1.345: the usual Huber constant)
 *   delta_k = c * med (one float32 product), then huber_floor where the product is not above it (a NaN included)
 *   n == 0:   delta_k = +0.0f, and the pose keeps its bits as in every other entry
 * Weights and terms are those of the robust entries with delta_k for huber_delta; delta_k == 0 (a zero median) switches
 * the weights off for that iteration, which then has the plain solve's bits.  huber_k must be finite and > 0,
 * huber_floor finite and >= 0.  Two more launches per iteration for 8 sequences (a residual pass over the lattice and one
 * select block per sequence: an 11 + 11 + 10 bit radix selection on integer counters) and one small clearing launch per
 * call; nothing read back, no float atomics: bitwise reproducible.
 * scratch: gs_projective_icp_scaled_scratch_bytes / gs_projective_icp_color_scaled_scratch_bytes (the plain / colour
 * scratch, then the key table (nslots uint32), 2048 counters and the threshold), 16-byte aligned.
 * gs_projective_icp_scaled_batch_f32: gs_projective_icp_robust_batch_f32 with the rule; tapes_host as there (NULL:
 * untaped; a taped row holds delta_k in pad[0]); deltas_host: NULL, or per sequence a device buffer of numiters floats
 * that receives delta_k.
 * gs_projective_icp_scaled_rows_f32: gs_projective_icp_robust_rows_f32 with the threshold derived at init_pose16, which
 * also goes to delta_out (1 float, or NULL).
 * gs_projective_icp_color_scaled_batch_f32: gs_projective_icp_color_robust_batch_f32 with the rule for the geometric
 * threshold; color_huber_delta stays a constant.
 * gs_projective_icp_scaled_backward_batch_f32: gs_projective_icp_robust_backward_batch_f32 for a tape of the scaled
 * forward: every iteration's threshold is read from its tape row and is a constant of the pass, like the clip flags (no
 * gradient flows through the median).  Every argument is checked before the first HIP call. */
GS_API int64_t gs_projective_icp_scaled_scratch_bytes(int H, int W, int stride);
GS_API int64_t gs_projective_icp_color_scaled_scratch_bytes(int H, int W, int stride);
GS_API int gs_projective_icp_scaled_batch_f32(const gs_picp_seq* seqs_host, void* const* tapes_host,
                                              float* const* deltas_host, int B, int H, int W,
                                              const gs_picp_params* params_host, float huber_k, float huber_floor,
                                              void* stream);
GS_API int gs_projective_icp_scaled_rows_f32(const gs_picp_seq* seq_host, int H, int W, int stride, float dist_th,
                                             float dot_th, float huber_k, float huber_floor, int32_t* code, int64_t* row,
                                             float* a6, float* b, float* weight, double* sums28, int64_t* count,
                                             float* delta_out, void* stream);
GS_API int gs_projective_icp_color_scaled_batch_f32(const gs_picp_color_seq* seqs_host, float* const* deltas_host, int B,
                                                    int H, int W, const gs_picp_params* params_host, float color_weight,
                                                    float huber_k, float huber_floor, float color_huber_delta,
                                                    void* stream);
GS_API int gs_projective_icp_scaled_backward_batch_f32(const gs_picp_backward_seq* seqs_host, int B, int H, int W,
                                                       const gs_picp_params* params_host, void* stream);

/* The rule for the COLOUR residual of the joint solve, next to (or without) the one for the geometric residual:
 *   cdelta = max(c_c * med_c, color_huber_floor),  c_c = (float)color_huber_k * 1.4826f,
 *   med_c  = the LOWER median (rank (n - 1) / 2) of |r| over the slots that have a colour row, r the colour residual
 *            BEFORE color_weight is applied, with the bits the joint linearise kernel forms;
 *   n == 0, a median of 0 or a product that is not above the floor (a NaN included): cdelta = color_huber_floor.
 * A threshold in the units of the residuals themselves: the same scene in colours of 0 ... 1 and of 0 ... 255 gets
 * thresholds a factor of 255 apart without a constant being retuned.  huber_k / color_huber_k: finite and >= 0, each
 * switches its rule on when > 0; with 0 the floor of that residual is its constant threshold (0: off), as huber_delta /
 * color_huber_delta are in gs_projective_icp_color_robust_batch_f32.  With both 0 the entries run the robust entries'
 * launches.  The launches are those of the geometric rule, whichever thresholds are asked for: ONE residual pass (one
 * association per slot, a key table and a first-digit histogram per residual asked for) and ONE select launch of
 * B x (thresholds asked for) blocks; one clearing launch per call.  Nothing read back, integer atomics only.
 * scratch: gs_projective_icp_color_joint_scaled_scratch_bytes (gs_projective_icp_color_scaled_scratch_bytes, then the
 * colour residual's key table, 2048 counters and threshold), 16-byte aligned; 0 for bad sizes.
 * gs_projective_icp_color_joint_scaled_batch_f32: deltas_host / cdeltas_host: NULL, or per sequence a device buffer of
 * numiters floats that receives the geometric / the colour threshold of every iteration; a table is written only when
 * its rule is on.
 * gs_projective_icp_color_joint_scaled_rows_f32: gs_projective_icp_color_robust_rows_f32 with the thresholds derived at
 * init_pose16; delta_out / cdelta_out (1 float each, or NULL) receive them, each only when its rule is on. */
GS_API int64_t gs_projective_icp_color_joint_scaled_scratch_bytes(int H, int W, int stride);
GS_API int gs_projective_icp_color_joint_scaled_batch_f32(const gs_picp_color_seq* seqs_host, float* const* deltas_host,
                                                          float* const* cdeltas_host, int B, int H, int W,
                                                          const gs_picp_params* params_host, float color_weight,
                                                          float huber_k, float huber_floor, float color_huber_k,
                                                          float color_huber_floor, void* stream);
GS_API int gs_projective_icp_color_joint_scaled_rows_f32(const gs_picp_color_seq* seq_host, int H, int W, int stride,
                                                         float dist_th, float dot_th, float color_weight, float huber_k,
                                                         float huber_floor, float color_huber_k,
                                                         float color_huber_floor, int32_t* code, int64_t* row, float* a6,
                                                         float* b, float* ac6, float* bc, int32_t* colored,
                                                         float* weight, float* color_weight_out, double* sums28,
                                                         int64_t* count, int64_t* color_count, float* delta_out,
                                                         float* cdelta_out, void* stream);

/* ------------------------------------------------------------------ projective ICP: per-pixel weights ------
 * Opt-in (additions only; the ABI version, every struct, every signature and every *_scratch_bytes function above stay):
 * one float32 image of pixel weights (H, W) per sequence, read at the pixel p of each lattice slot: a mask, a sensor
 * model (1 / sigma^2(z)), a learned confidence.  The weights travel as a host array of B device pointers next to the
 * sequences; a NULL entry: that sequence has no weights (every wp = 1).  The rule, per slot with wp = weights[p]:
 *   code 1  unless depth[p] > 0, as ever
 *   code 6  ("masked") unless wp > 0 && wp < +inf in float32: zero, negative, NaN and +inf all mask.  Nothing is validated
 *           on the host and nothing is read back.  A masked slot is not associated, not counted as an inlier and not part
 *           of any median; it contributes +0.0 to every term and has no colour row
 *   codes 2 .. 5 as ever
 *   a used slot's total weight is wt = wp * h, ONE float32 product, h the Huber weight of its raw residual b (1.0f
 *   without a threshold; the clip flag is taken from the unweighted float32 b); every one of its 28 terms is
 *   (double)wt * ((double)x * (double)y); in the joint solve the colour products carry wp * wc in the same way.
 * The inlier count stays the integer number of used slots; the sum of squares is the weighted one; with huber_k /
 * color_huber_k the median is that of the unweighted |b| / |r| over the used / coloured slots, masked slots excluded.
 * The reduction order, the finish, the solve, the update and "no inlier keeps the pose bits" are untouched.  Hence, bit
 * for bit: weights of all 1.0f give the pose, trace, thresholds and tape of the unweighted entries, and weight 0 on a
 * set of pixels gives what depth 0 on those pixels gives (the code tables differ in 6 against 1).
 * Thresholds: huber_k > 0 switches the median rule on with huber_delta as its floor, else huber_delta is the constant
 * threshold (0: none); color_huber_k / color_huber_delta alike.  scratch: that of the unweighted entry with the same
 * thresholds (gs_projective_icp_scaled_scratch_bytes with huber_k > 0, else gs_projective_icp_scratch_bytes; the colour
 * entries: gs_projective_icp_color_joint_scaled_scratch_bytes with either rule on, else
 * gs_projective_icp_color_scratch_bytes).  One 4-byte load per slot on top of the robust kernels' work.
 * gs_projective_icp_weighted_batch_f32: tapes_host / deltas_host as in gs_projective_icp_scaled_batch_f32 (either NULL).
 * gs_projective_icp_weighted_rows_f32: `weight` (nslots) receives wt of a used slot, 0 elsewhere; delta_out is written
 * with huber_k > 0 only.  gs_projective_icp_color_weighted_batch_f32 / _rows_f32: the joint solve; color_weight_out
 * receives wp * wc.
 * gs_projective_icp_weighted_backward_batch_f32: the reverse-mode pass for a tape of the weighted forward, atomic
 * (ordered = 0: key_out / contrib_out and the sort scratch are not read) or ordered, for the three tapes as in
 * gs_projective_icp_ordered_backward_batch_f32 (huber_delta, taped_scale).  With W = wp h: A = sum W a a^T, g = sum W a b;
 * per used slot and iteration, e = u . a, c = xi . a:  weights_bar[p] += h e (b - c);  ab is multiplied by wp h;  the
 * residual's adjoint is e wp (h + h' (b - c)).  Which slots are masked is a constant of the pass.  weights_bar_host: NULL,
 * or per sequence a device image (H, W) or NULL; it is accumulated in float64 per slot by the slot's own thread and rounded
 * once: bitwise reproducible, the same bits in both modes; +0.0 off the lattice, for masked slots and slots never used.
 * scratch per sequence: gs_projective_icp_weighted_backward_scratch_bytes(H, W, stride, n_map, ordered) (the mode's
 * scratch plus 8 bytes per slot) for a sequence whose weights_bar is asked for, else the mode's own scratch: an output
 * that is not asked for costs nothing.  Every argument is checked before the first HIP call; a NULL weights array is refused. */
GS_API int gs_projective_icp_weighted_batch_f32(const gs_picp_seq* seqs_host, const float* const* weights_host,
                                                void* const* tapes_host, float* const* deltas_host, int B, int H, int W,
                                                const gs_picp_params* params_host, float huber_delta, float huber_k,
                                                void* stream);
GS_API int gs_projective_icp_weighted_rows_f32(const gs_picp_seq* seq_host, const float* weights, int H, int W, int stride,
                                               float dist_th, float dot_th, float huber_delta, float huber_k,
                                               int32_t* code, int64_t* row, float* a6, float* b, float* weight,
                                               double* sums28, int64_t* count, float* delta_out, void* stream);
GS_API int gs_projective_icp_color_weighted_batch_f32(const gs_picp_color_seq* seqs_host,
                                                      const float* const* weights_host, float* const* deltas_host,
                                                      float* const* cdeltas_host, int B, int H, int W,
                                                      const gs_picp_params* params_host, float color_weight,
                                                      float huber_delta, float huber_k, float color_huber_delta,
                                                      float color_huber_k, void* stream);
GS_API int gs_projective_icp_color_weighted_rows_f32(const gs_picp_color_seq* seq_host, const float* weights, int H, int W,
                                                     int stride, float dist_th, float dot_th, float color_weight,
                                                     float huber_delta, float huber_k, float color_huber_delta,
                                                     float color_huber_k, int32_t* code, int64_t* row, float* a6,
                                                     float* b, float* ac6, float* bc, int32_t* colored, float* weight,
                                                     float* color_weight_out, double* sums28, int64_t* count,
                                                     int64_t* color_count, float* delta_out, float* cdelta_out,
                                                     void* stream);
GS_API int64_t gs_projective_icp_weighted_backward_scratch_bytes(int H, int W, int stride, int64_t n_map, int ordered);
GS_API int gs_projective_icp_weighted_backward_batch_f32(const gs_picp_ordered_backward_seq* seqs_host,
                                                         const float* const* weights_host,
                                                         float* const* weights_bar_host, int B, int H, int W,
                                                         const gs_picp_params* params_host, float huber_delta,
                                                         int taped_scale, int ordered, void* sort_scratch,
                                                         int64_t sort_scratch_bytes, void* stream);

/* ------------------------------------------------------------------ projective ICP: the outlier mask ------
 * Opt-in (additions only; the ABI version, every struct and every signature above stay): from the residuals of a solve
 * to the image of the pixels that moved.  Per sequence, at the float32 pose init_pose16, over EVERY pixel of the live
 * frame (stride 1 whatever the solve's stride):
 *   association  code, b of each pixel as gs_projective_icp_rows_f32 gives them at stride 1 (with weights: a masked
 *                pixel has code 6, as in the weighted entries)
 *   scale        med = the lower median of |b| over the code-0 pixels (the radix selection of the scaled entries);
 *                hi_t = max(((float)hi * 1.4826f) * med, floor), lo_t alike: float32, one rounding per product; +0.0
 *                without a code-0 pixel; a threshold of 0 makes no pixel strong or eligible by its residual
 *   classes      strong = (code == 0 && |b| > hi_t && hi_t > 0) || code == 4 || code == 5;
 *                eligible = strong || (code == 0 && |b| > lo_t && lo_t > 0); codes 1, 2, 3 and 6 have class 0
 * gs_picp_outlier_classes_batch_f32 writes, per sequence, the class byte of every pixel (bit 0 strong, bit 1 eligible)
 * to classes_host[b] (H, W) and, when thresholds_host is not NULL, (hi_t, lo_t) to thresholds_host[b].  weights_host:
 * NULL (no weights) or per sequence a device image (H, W) or NULL.  seqs_host: out_pose16 and trace are not used;
 * scratch: gs_picp_outlier_classes_scratch_bytes(H, W) bytes per sequence, 16-byte aligned.  hi >= lo > 0, floor >= 0,
 * all finite.  8 sequences per launch; nothing is read back; no float atomics; bitwise reproducible.
 * gs_region_mask_u8 maps B class images (B, H, W) and their depth to the mask (B, H, W) of 0 / 1:
 *   seed(p) = strong(p) and at least min_support (1 .. 9) of the 3 x 3 window around p are strong (p counts, pixels
 *   outside the image do not);  M_0 = seed;  M_{i+1}(p) = M_i(p) || (eligible(p) && some 4-neighbour q inside the image
 *   has M_i(q) && fabsf(depth(p) - depth(q)) <= grow_depth), for exactly grow (0 .. 16) steps.
 * One launch, tiles with a halo in LDS, integer outputs, bitwise reproducible.  Every argument of both entries is checked
 * before the first HIP call. */
GS_API int64_t gs_picp_outlier_classes_scratch_bytes(int H, int W);
GS_API int gs_picp_outlier_classes_batch_f32(const gs_picp_seq* seqs_host, const float* const* weights_host,
                                             uint8_t* const* classes_host, float* const* thresholds_host, int B, int H,
                                             int W, float dist_th, float dot_th, float hi, float lo, float floor,
                                             void* stream);
GS_API int gs_region_mask_u8(const uint8_t* classes, const float* depth, uint8_t* mask, int64_t B, int H, int W,
                             int min_support, int grow, float grow_depth, void* stream);

/* ------------------------------------------------------------------ feature layers ------
 * A C-channel feature per surfel (an embedding, class logits, any network output), fused from per-pixel feature images
 * with the weights and the correspondences of the colour fusion.  A layer of one sequence is emb (capacity, C), float32
 * (GS_FEATURE_F32) or float16 (GS_FEATURE_F16), and weight (capacity) float32; row r belongs to map row r.
 *
 * gs_fuse_features_batch runs AFTER the map update of the frame, on the update's correspondence table best_pix (H * W
 * int32, as gs_update_map_fusion_batch_f32 / gs_pointfusion_step_batch_f32 write it; NULL: every pixel with depth is
 * appended), the frame's depth and alpha, and the map count BEFORE the update, n_old = min(*n_old_dev, n_old_bound)
 * (n_old_bound when n_old_dev is NULL).  In raster order,
 *   row(p) = best_pix[p]         if 0 <= best_pix[p] < n_old                  (matched)
 *            n_old + rank(p)     if best_pix[p] < 0 and depth[p] > 0          (appended: rank = such pixels before p)
 *            none                otherwise (a stale entry >= n_old counts as none)
 * and with valid(p) = feat != NULL && (valid == NULL || valid[p] != 0), a = alpha[p], w = weight[row]:
 *   matched, valid      w2 = w + a; inv = 1.0f / (w2 == 0.0f ? 1.0f : w2);
 *                       emb[row, c] = ((w * emb[row, c]) + (a * feat[p, c])) * inv; weight[row] = w2
 *                       (float32, one rounding per operation, no FMA: the colour merge of the map update)
 *   matched, not valid  untouched
 *   appended, valid     emb[row] = feat[p] (the bits), weight[row] = a
 *   appended, not valid emb[row] = +0, weight[row] = +0.0f
 * A float16 layer is converted to float32, merged as above and stored round-to-nearest-even.  A map row is matched by
 * at most one pixel, so every row has one writer: no atomics, bitwise reproducible.  row_of_pix (H * W int32) receives
 * row(p), -1 for none; *n_out = n_old + appended pixels (the map's own new count).  feat (H, W, C) is of the layer's
 * dtype.  Rows at or beyond *n_out are not written.
 *
 * gs_compact_features_batch: stable, out-of-place compaction by keep (uint8) over the first n = min(*n_dev, n_bound)
 * rows: survivor k becomes row k of emb_out / weight_out, moved bit for bit; *n_out = survivors; destination rows at or
 * beyond it are not written.  With the same keep it selects the rows gs_prune_map_dc_f32 selects.
 *
 * scratch: gs_scratch_bytes(rows, pixels) bytes per sequence (rows = n_old_bound and pixels = H * W for the fusion;
 * rows = n_bound and pixels = 0 for the compaction).  Sequences are served 8 per group of launches; nothing is read
 * back.  GS_ERR_INVALID, before the first HIP call: NULL pointers, C outside 1 .. 4096, an unknown dtype,
 * capacity < n_old_bound + H * W, n_old_bound + H * W >= 2^31 (so H * W >= 2^31), capacity_out < n_bound, emb / emb_out
 * not 16-byte aligned (feat too when C * sizeof(elem) is a multiple of 16), a destination equal to its source. */
#define GS_FEATURE_F32 0
#define GS_FEATURE_F16 1
typedef struct gs_feature_fuse_seq {
  void* emb;                 /* (capacity, C), 16-byte aligned */
  float* weight;             /* (capacity) */
  int64_t capacity;          /* >= n_old_bound + H * W */
  int64_t n_old_bound;       /* host-side upper bound of the map count before the update */
  const int64_t* n_old_dev;  /* device int64[1]: that count, or NULL when n_old_bound is exact */
  const int32_t* best_pix;   /* (H * W) or NULL */
  const float* depth;        /* (H, W) */
  const float* alpha;        /* (H, W) */
  const void* feat;          /* (H, W, C) or NULL: no pixel is valid */
  const uint8_t* valid;      /* (H * W) or NULL: every pixel */
  int32_t* row_of_pix;       /* (H * W) */
  int64_t* n_out;            /* device int64[1] */
  void* scratch;
} gs_feature_fuse_seq;
GS_API int gs_fuse_features_batch(const gs_feature_fuse_seq* seqs_host, int B, int H, int W, int C, int dtype,
                                  void* stream);
typedef struct gs_feature_compact_seq {
  const void* emb;           /* (n_bound, C), 16-byte aligned */
  const float* weight;       /* (n_bound) */
  int64_t n_bound;
  const int64_t* n_dev;      /* device int64[1], or NULL when n_bound is exact */
  const uint8_t* keep;       /* (n_bound) */
  void* emb_out;             /* (capacity_out, C), 16-byte aligned */
  float* weight_out;         /* (capacity_out) */
  int64_t capacity_out;      /* >= n_bound */
  int64_t* n_out;            /* device int64[1] */
  void* scratch;
} gs_feature_compact_seq;
GS_API int gs_compact_features_batch(const gs_feature_compact_seq* seqs_host, int B, int C, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GRADSLAM_HIP_H */
