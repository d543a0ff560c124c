/* libuuo_hip.so -- C ABI of the MI355X (gfx950) SMPL-to-marker fitting hot path.
 *
 * The reference (NicholasMilef/UUO-Mocap) is pure Python and has no FFI layer; its boundary for this
 * path is a set of Python callables.  This header is the C-ABI a binding for those
 * callables sits on: plain pointers and sizes, no torch types.  Each entry point cites the reference
 * interface it replaces (paths relative to the reference checkout).  The Python mirror of the
 * reference's operator surface (the uuo_mocap_amd package) binds these symbols with ctypes; INTEGRATION.md
 * shows the stub a reference maintainer would add.
 *
 * Conventions
 *  - every function returns 0 on success, a negative errno-style code otherwise; the message for the
 *    calling thread is available from uuo_last_error().
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Nothing synchronises the
 *    device unless the comment says so; no hidden allocation happens inside the *_eval / kernel-only
 *    calls (they use the workspace created by uuo_fit_create).
 *  - pointers named `d_*` are device pointers (HBM), `h_*` host pointers.  All floats are fp32,
 *    row-major, contiguous.  Rotations are 3x3 row-major (9 floats).
 *  - the library owns no threads and keeps no global state besides the last-error string.
 */
#ifndef UUO_HIP_H
#define UUO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UUO_NUM_JOINTS 24
#define UUO_NUM_BETAS 10
#define UUO_NUM_POSE_FEATS 207
#define UUO_NUM_EXTRA_JOINTS 21

typedef struct uuo_model uuo_model_t; /* device copies of the SMPL tables */
typedef struct uuo_fit uuo_fit_t;     /* per-sequence workspace (F frames, M markers) */

const char* uuo_last_error(void);
/* 3 since uuo_problem_t grew `w_soft` / `soft_tau` (2) and `n_corners` / `d_bary` (3), round 4; a binding checks it before it
 * hands structures over.  (`robust_sigma`, appended last, left it at 3: a binding must zero the structure it fills.) */
int uuo_abi_version(void);

/* ---- model ------------------------------------------------------------------------------------
 * Replaces smplx.create("./body_models/", model_type="smpl", gender="neutral", batch_size=1) as used
 * by SmplInference.__init__ (src/video_mocap/utils/smpl.py:22-27).  Host arrays in smplx's layouts:
 * v_template [V,3], shapedirs [V,3,10], posedirs [207,V*3], J_regressor [24,V], lbs_weights [V,24],
 * parents [24] (parents[0] ignored), extra_joint_vids [21] (VertexJointSelector ids). */
int uuo_model_create(const float* h_v_template, const float* h_shapedirs, const float* h_posedirs,
                     const float* h_J_regressor, const float* h_lbs_weights, const int64_t* h_parents,
                     const int64_t* h_extra_joint_vids, int num_verts, uuo_model_t** out);
int uuo_model_destroy(uuo_model_t* model);
int uuo_model_num_verts(const uuo_model_t* model);
/* EXTENSION (not reference behaviour; the point-to-surface chamfer term, uuo_fit_set_surface, and uuo_ring_closest_points):
 * the model's triangles, h_faces [NF,3] int32 vertex ids (SmplInference.faces).  Builds every vertex's one-ring -- its incident
 * faces in ascending face id, a CSR table -- on the host and uploads it with the faces.  A vertex may have no face.  A vertex
 * with more than UUO_RING_MAX_VALENCE incident faces, or a face naming a vertex outside the model, is refused.  May be called
 * again (the tables are replaced; synchronises the device).  uuo_ring_table is the host half on its own: h_off [V+1],
 * h_ring [3 NF] (the first h_off[V] entries are written); no device is touched. */
#define UUO_RING_MAX_VALENCE 32
int uuo_model_set_faces(uuo_model_t* model, const int32_t* h_faces, int NF);
int uuo_ring_table(const int32_t* h_faces, int NF, int V, int32_t* h_off, int32_t* h_ring);

/* ---- SMPL forward (materialising) ---------------------------------------------------------------
 * Replaces SmplInference.forward (src/video_mocap/utils/smpl.py:29-50) = smplx SMPL.forward with
 * pose2rot=False: d_poses [F,23,9], d_betas [betas_rows,10] with betas_rows in {1,F}, d_root [F,9],
 * d_trans [F,3] or NULL.  Outputs d_verts [F,V,3] and d_joints [F,45,3] (either may be NULL). */
int uuo_smpl_forward(uuo_model_t* model, void* stream, int F, const float* d_poses, const float* d_betas,
                     int betas_rows, const float* d_root, const float* d_trans, float* d_verts,
                     float* d_joints);

/* Backward of uuo_smpl_forward for given upstream gradients (what torch autograd computes through smplx.lbs when a
 * caller differentiates SmplInference.forward itself, e.g. a user-written closure; reference utils/smpl.py:29-50).
 *   d_up_verts  [F,6890,3] dL/dvertices or NULL,  d_up_joints [F,45,3] dL/djoints or NULL (at least one)
 *   d_g_poses [F,23,3,3], d_g_betas [F,10] (per frame: sum the rows if betas had one row), d_g_root [F,1,3,3],
 *   d_g_trans [F,3];  d_scratch: F*24 floats of device scratch.  Asynchronous on `stream`.
 * With d_up_verts the backward is dense (every vertex carries a gradient): v_posed and the transposed 207 x 20670 blend
 * contraction run on the matrix pipe (csrc/dense_bwd.hip); the library keeps ~80 MB of scratch per stream and frame count
 * for it (allocated on first use, freed with the model). */
int uuo_smpl_backward(uuo_model_t* model, void* stream, int F, const float* d_poses, const float* d_betas,
                      int betas_rows, const float* d_root, const float* d_trans, const float* d_up_verts,
                      const float* d_up_joints, float* d_g_poses, float* d_g_betas, float* d_g_root, float* d_g_trans,
                      float* d_scratch);

/* ---- K=1 nearest neighbour ------------------------------------------------------------------------
 * Replaces pytorch3d.ops.knn_points(K=1) as reached through pytorch3d.loss.chamfer_distance from
 * weighted_chamfer_distance (src/video_mocap/losses/chamfer_distance.py:5-21) and
 * markers_utils.py:471-475,575-579: for every query x[n,i] the first index of the minimum of
 * ((dx*dx)+(dy*dy))+(dz*dz) over y[n,:] (separately rounded, no FMA).  d_x [N,P1,3], d_y [N,P2,3];
 * d_y_subset (optional, [P2s] int32) restricts/reorders the candidates: candidate c is
 * y[n, d_y_subset[c]] and the reported index is c.  Outputs d_dist [N,P1], d_idx [N,P1] (int32). */
int uuo_nn_argmin(void* stream, int N, int P1, int P2, const float* d_x, const float* d_y,
                  const int32_t* d_y_subset, int P2s, float* d_dist, int32_t* d_idx, void* d_workspace_u64);

/* ---- marker placement -----------------------------------------------------------------------------
 * Replaces compute_nearest_points (src/video_mocap/optimization.py:402-642; use_mean, granularity
 * "full"): idx[m] = argmin_v mean_{f valid} ||verts[f,v]-markers[f,m]||, numpy fp32 semantics
 * (sequential-in-f accumulation, first index).  d_valid [F] uint8.  Output d_idx [M] int32. */
int uuo_assign_mean_argmin(void* stream, int F, int M, int V, const float* d_verts, const float* d_markers,
                           const uint8_t* d_valid, int32_t* d_idx, void* d_workspace_u64);

/* EXTENSION (not reference behaviour; the reference assumes that a marker column holds one physical marker for the whole
 * capture): the placement per TRACKLET.  d_seg [F,M] int32 names the tracklet of every entry, -1 = none; ids are 0..S-1, each
 * id lives in one column and its frames form one run that only -1 entries may interrupt.
 *   idx[s] = argmin_v (1/n_s) sum_{f : seg[f,col(s)] == s, valid[f]} ||verts[f,v] - markers[f,col(s)]||
 * with uuo_assign_mean_argmin's arithmetic: fp32, norm sqrt((dx dx + dy dy) + dz dz), the sum sequential in f, one correctly
 * rounded divide by the count n_s of the frames actually summed, lowest vertex id on ties.  A tracklet with no summed frame
 * gets -1; entries with ids outside 0..S-1 are ignored.  d_valid [F] uint8, d_idx [S] int32, d_workspace_u64 [S].
 * Asynchronous: no host read-back (the counts are formed in the kernel). */
int uuo_assign_segments_argmin(void* stream, int F, int M, int V, int S, const float* d_verts, const float* d_markers,
                               const int32_t* d_seg, const uint8_t* d_valid, int32_t* d_idx, void* d_workspace_u64);

/* ---- rigidity matrix of the marker segmentation ---------------------------------------------------
 * Replaces the double loop of segment_rigid (src/video_mocap/markers/markers_utils.py:254-259):
 *   d_std[i*M+j] = np.std(np.linalg.norm(points[:, i] - points[:, j], axis=-1))     d_points [F,M,3] float32
 * in numpy's float32 arithmetic and numpy's summation order (pairwise summation, 8 accumulators per 128-element block,
 * 8192-element reduction chunks), so the values -- which the average-linkage clustering cuts at 5 mm -- are bit-equal
 * to the reference's.  d_std [M,M] float32 (the reference stores them in a float64 matrix: exact).  Asynchronous. */
int uuo_rigid_distance_std(void* stream, int F, int M, const float* d_points, float* d_std);

/* ---- EXTENSION: soft-assignment (soft-min) nearest neighbour ----------------------------------------
 * Not reference behaviour (the reference's chamfer term is the hard K=1 minimum above; BASELINE's north star names a
 * soft assignment).  softmin[n,i] = -tau log sum_j exp(-|x[n,i]-y[n,j]|^2 / tau); d_dmin / d_sumexp ([N,P1]) are the
 * exact minimum and the normaliser sum_j exp((dmin - d2)/tau), kept for the backward.  Backward: gradients of
 * sum_i grad_softmin[n,i] softmin[n,i] with respect to x (d_gx [N,P1,3]) and y (d_gy [N,P2,3]); either may be NULL.
 * d_ws: N*P1 uint64. */
int uuo_soft_nn_forward(void* stream, int N, int P1, int P2, const float* d_x, const float* d_y, float tau,
                        float* d_softmin, float* d_dmin, float* d_sumexp, void* d_ws);
int uuo_soft_nn_backward(void* stream, int N, int P1, int P2, const float* d_x, const float* d_y, float tau,
                         const float* d_dmin, const float* d_sumexp, const float* d_grad_softmin, float* d_gx,
                         float* d_gy);

/* ---- barycentric marker placement ------------------------------------------------------------------
 * Replaces igl.signed_distance + trimesh.triangles.points_to_barycentric in compute_nearest_points with
 * compute_locations.use_barycentric (src/video_mocap/optimization.py:494-500,519-523): for every query
 * d_points[f,m] the closest point on the triangle mesh (d_verts[f] [V,3], d_faces [NF,3] int32).
 * Outputs, all [F,M,...]: d_dist (unsigned Euclidean distance), d_face (winning face, lowest index on
 * exact ties, -1 if no face is usable), d_closest [.,3] and d_bary [.,3] (trimesh "cramer" coordinates of
 * the closest point with respect to the face's corners in d_faces order).  fp32 throughout. */
int uuo_mesh_closest_points(void* stream, int F, int M, int V, int NF, const float* d_verts,
                            const int32_t* d_faces, const float* d_points, float* d_dist, int32_t* d_face,
                            float* d_closest, float* d_bary);

/* EXTENSION (not reference behaviour): the closest point on the ONE-RING of a given vertex -- the pick of the point-to-surface
 * chamfer term (uuo_fit_set_surface) on caller-given vertices.  For every query d_points[f,m] and its vertex d_nn_idx[f,m]
 * (int32; normally uuo_nn_argmin's result): the closest point on the faces incident to that vertex, with the arithmetic and
 * the conventions of uuo_mesh_closest_points (lowest face id on exact ties, "cramer" coordinates).  A vertex without a face
 * stands for itself: d_face -1, the closest point is the vertex, d_bary (1, 0, 0) on the corners (v, v, v).  d_verts [F,V,3]
 * with V the model's vertex count; outputs [F,M,...] as there.  Needs uuo_model_set_faces.  Asynchronous. */
int uuo_ring_closest_points(void* stream, uuo_model_t* model, int F, int M, const float* d_verts, const float* d_points,
                            const int32_t* d_nn_idx, float* d_dist, int32_t* d_face, float* d_closest, float* d_bary);

/* ---- stage problems -------------------------------------------------------------------------------
 * One closure evaluation (forward + backward) of the three L-BFGS stages, on flat parameter vectors
 * packed exactly as the reference hands them to torch.optim.LBFGS:
 *   UUO_STAGE_CHAMFER  closure_stage_chamfer   (optimization.py:187-275)  x = [trans 3F | z F | betas 10 | pose 207F]
 *   UUO_STAGE_MARKER   closure_stage_marker_pose (optimization.py:329-394) x = [pose 207F | betas 10 | root 9F | trans 3F]
 *   UUO_STAGE_PART     closure_fit_subtree     (markers/markers_utils.py:454-562) x = [z 1 | trans 3F | betas 10]
 * and of the root stage (optim_root, optimization.py:21-144: translation, yaw and shape with the body pose held; the reference
 * cannot run its own -- it reads a config key no config has and an undefined o_betas -- so this is a corrected restatement):
 *   UUO_STAGE_ROOT         yaw_lock, a yaw per frame          x = [trans 3F | z F | betas 10]
 *   UUO_STAGE_ROOT_SHARED  constrained_rotation, one yaw      x = [trans 3F | z 1 | betas 10]
 *     R_f  = Rz(z_f) root_f  (z_0 for every frame in the shared packing; the product as it is, no Gram-Schmidt)
 *     loss = w_data sum_fm mask_fm min_v |x_fm - v_fv|^2 / sum mask  (all vertices; 0 when sum mask = 0)
 *          + w_betas mean_l (betas_l - o_betas_l)^2
 *          + w_tv mean over (F-1) 3 entries of ((trans_{t+1} - trans_t) - (mm_{t+1} - mm_t))^2,  mm_t = mean_m x_tm over ALL
 *            columns, missing ones (exact zeros) included; F < 2: 0.  w_tv: uuo_fit_set_root_trans_vel
 *   d_o_pose is the fixed body pose, d_root the input root orientation; w_pose, d_assign and d_subset are not read (the
 *   whole-body vertex table is the library's own); pose_cache_id must be non-zero (the pose blend is computed once per id);
 *   w_soft, robust_sigma, w_offsets and every side term of the workspace are refused, and so are lock-step batches
 *   (uuo_batch_create) and uuo_lbfgs_solve_shared.  d_nn_idx of uuo_closure_eval reports vertex ids.
 * (3 is not a public value: the library uses it internally.)
 */
enum { UUO_STAGE_CHAMFER = 0, UUO_STAGE_MARKER = 1, UUO_STAGE_PART = 2, UUO_STAGE_ROOT = 4, UUO_STAGE_ROOT_SHARED = 5 };

typedef struct {
  int32_t stage;             /* UUO_STAGE_* */
  int32_t F, M;              /* frames, markers */
  const float* d_markers;    /* [F,M,3]; exact zeros = missing (optimization.py:703-715) */
  const float* d_o_pose;     /* [F,23,9]: prior target (chamfer, marker) / the fixed body pose (part) */
  const float* d_o_betas;    /* [10] prior target */
  const float* d_root;       /* [F,9] fixed root orientation (chamfer, part); unused for marker */
  const int32_t* d_assign;   /* marker stage: [M] vertex id per marker column */
  const int32_t* d_subset;   /* part stage: [n_subset] vertex ids (candidate order = tie order) */
  int32_t n_subset;
  float w_data;              /* full_chamfer / marker / chamfer weight */
  float w_pose;              /* reg_pose_body weight (0 = term absent) */
  float w_betas;             /* reg_betas weight (0 = term absent) */
  float marker_distance;     /* MARKER_DISTANCE, utils/settings.py:1 */
  uint64_t pose_cache_id;    /* part stage: non-zero = the body pose d_o_pose is constant for every evaluation that
                                carries this id, so the pose-corrective blend (207 x 20670 contraction, 70 % of the
                                forward's arithmetic) is computed once and re-used; 0 = recompute every evaluation */
  /* EXTENSION (not reference behaviour; BASELINE's north star names a soft-assignment Chamfer distance, configs[2] a
   * "soft-assignment path" of hmr_part.yaml): the data term's hard minimum over the vertices joined or replaced by the soft
   * minimum  -tau log sum_v exp(-|x - v|^2 / tau).  w_soft = 0: the reference's term alone.
   *   UUO_STAGE_PART    loss_data = (1 / (F M)) sum_{f,m} (w_data min_v d2 + w_soft softmin) over the candidate's vertices
   *                     (markers/markers_utils.py:471-475); fused closure k_part_soft: needs pose_cache_id != 0 and M <= 16
   *   UUO_STAGE_CHAMFER loss_data = (1 / sum mask) sum_{f,m} mask_fm (w_data min_v d2 + w_soft softmin) over all vertices
   *                     (losses/chamfer_distance.py:5-21); soft-min kernels + the dense backward on the matrix pipe; not
   *                     available inside lock-step batches (uuo_batch_*) */
  float w_soft;              /* stages.<stage>.losses.soft_chamfer (0 = absent) */
  float soft_tau;            /* temperature in m^2 (> 0 when w_soft != 0) */
  /* Marker stage on a three-corner (barycentric) placement -- compute_locations.use_barycentric of the reference
   * (optimization.py:494-523; the closure's virtual markers are `placement @ vertices`, :345-351, every row of the placement
   * holding the barycentric coordinates of a surface point at its face's three corners).  n_corners = 3: d_assign is
   * [M][3] vertex ids, d_bary [M][3] their weights, virtual marker m = sum_k d_bary[m][k] v[d_assign[m][k]].
   * n_corners = 0 or 1: the one-hot placement of the shipped configs, d_assign [M], d_bary unused. */
  int32_t n_corners;
  const float* d_bary;
  /* EXTENSION (not reference behaviour; unlabeled captures carry ghost points that the plain square lets pull on the body
   * without bound): each data item's square s replaced by the Geman-McClure term of SMPLify's GMoF,
   *   rho(s) = s sigma^2 / (sigma^2 + s)   (-> s as sigma -> inf, -> sigma^2 as s -> inf),   rho'(s) = (sigma^2 / (sigma^2 + s))^2
   *   UUO_STAGE_CHAMFER s = min_v |x - v|^2 (the assignment is unchanged: rho is monotone), same mask and 1 / sum mask
   *   UUO_STAGE_PART    the same over the candidate's vertices, same 1 / (F M)
   *   UUO_STAGE_MARKER  s = (|x - vm| - d0)^2, one-hot and three-corner placements, same mask and 1 / (F M)
   * Separate kernel instantiations (the plain ones are unchanged); available inside lock-step batches.  Needs w_soft = 0.
   * robust_sigma = 0: the reference's square. */
  float robust_sigma;        /* sigma in metres (>= 0, finite) */
  /* EXTENSION (not reference behaviour; MoSh's latent markers -- the reference's stages.marker.use_sdf appends virtual markers
   * to its parameters, a path it cannot run): marker stage only.  w_offsets > 0 appends one rest-space offset o_m per marker
   * column, shared by all frames and skinned with the body, to the parameters:
   *   x = [pose 207F | betas 10 | root 9F | trans 3F | offsets 3M]
   *   virtual marker  vm[f,m] = sum_k b[m,k] (T_R[f,a[m,k]] (vp[f,a[m,k]] + o_m) + T_t[f,a[m,k]]) + trans_f
   *   loss = w_data (1/(F M)) sum mask rho(|x - vm|^2)  (marker_distance leaves the data term: the offset carries the stand-off)
   *        + w_offsets (1/M) sum_m (|o_m| - marker_distance)^2  + the pose and shape priors as before
   * One-hot and three-corner placements, with robust_sigma and the joint-acceleration term.  Refused for the chamfer and part
   * stages, inside lock-step batches (uuo_batch_*) and by uuo_lbfgs_solve_shared.  0: off (and uuo_problem_num_params, the
   * packing and every result are those without the field).  >= 0, finite. */
  float w_offsets;
} uuo_problem_t;

int uuo_fit_create(uuo_model_t* model, int F, int M, uuo_fit_t** out);
int uuo_fit_destroy(uuo_fit_t* fit);
/* EXTENSION (not reference behaviour; the reference fits every frame on its own, and its temporal terms stop in a debugger):
 * a joint-acceleration smoothness term on the 24 kinematic joints J_t = G_j^t + trans_t of the chamfer and marker stages,
 *   a_t = J_t - 2 J_{t+1} + J_{t+2} (t = 0 .. F-3),   loss += w sum_t |a_t|^2 / ((F - 2) 72)
 * in units of m^2 per frame^2: the weight belongs to the frame rate of the sequence handed over.  F < 3: no terms.
 * A setting of the WORKSPACE (0 at creation) that applies to every uuo_closure_eval, uuo_lbfgs_solve, uuo_lbfgs_solve_shared
 * and uuo_time_closure on `fit` until it is set again; workspaces shared by several problems need it set before each call.
 * Refused (at evaluation) for the part stage and with w_soft != 0, and inside lock-step batches (uuo_batch_*).
 * w >= 0, finite. */
int uuo_fit_set_joint_accel(uuo_fit_t* fit, float w);
/* EXTENSION (not reference behaviour; the reference's foot_contact / foot_velocity terms sit on its part stage, assume a floor
 * at z = 0 and are enabled in no shipped config): a contact-gated foot-lock term on the feet (SMPL joints 10 and 11,
 * J_t = G_j^t + trans_t) of the chamfer and marker stages, with contact labels c[F][2] in [0, 1] (left, right) and the gate
 * g[t][s] = c[t][s] c[t-1][s]:
 *   v[t][s] = J[t][foot_s] - J[t-1][foot_s] (t = 1 .. F-1, all three components),   loss += w sum_t sum_s g[t][s] |v[t][s]|^2 / ((F - 1) 6)
 * in units of m^2 per frame^2, like the joint-acceleration term: the weight belongs to the frame rate of the sequence handed
 * over.  No floor height is assumed.  F < 2: no terms.
 * A setting of the WORKSPACE (0 / null at creation) with the lifetime rules of uuo_fit_set_joint_accel.  `d_contacts` is a
 * device pointer to [F][2] floats that the caller keeps alive and may rewrite; it is read at every evaluation, not copied.  It
 * may be null only with w == 0.  Refused (at evaluation) for the part stage and with w_soft != 0, and inside lock-step batches
 * (uuo_batch_*).  w >= 0, finite. */
int uuo_fit_set_foot_lock(uuo_fit_t* fit, float w, const float* d_contacts);
/* EXTENSION (not reference behaviour; the reference's floor terms -- the chamfer stage's `ground` = mean(relu(-joints_z)) and
 * the part stage's foot_contact -- act on JOINTS, which sit 5-10 cm above the sole, and run on its operator-composed route): a
 * floor-contact term on K = k_left + k_right SOLE VERTICES of the chamfer and marker stages.  z is up; the plane lies at
 * `height`.  d_vids[K] are model vertex ids, the left foot's k_left points first; s(p) is the foot of point p; z[t][p] the world
 * z of the skinned vertex, translation included; c[F][2] in [0, 1] the contact labels (left, right) of uuo_fit_set_foot_lock:
 *   pen[t][p] = max(height - z[t][p], 0)                            (always on: nothing goes through the floor)
 *   flo[t][s] = max(min_{p: s(p) = s} z[t][p] - height, 0)          (the foot's lowest point; the first in list order on ties)
 *   loss += w_pen sum_t sum_p pen^2 / (F K)  +  w_con sum_t sum_s c[t][s] flo[t][s]^2 / (2 F)
 *   dL/dz[t][p] = -2 w_pen pen[t][p] / (F K)  +  [p = argmin of its foot] w_con c[t][s] flo[t][s] / F       (x, y: 0)
 * in m^2.  Both pieces are C^1 at their hinge; the min is piecewise smooth, as the nearest-vertex chamfer is.  Frames are not
 * coupled: F = 1 is a valid problem.
 * A setting of the WORKSPACE (off at creation) with the lifetime rules of uuo_fit_set_joint_accel.  `d_vids` and `d_contacts`
 * are device pointers that the caller keeps alive; they are read at every evaluation, not copied (the ids are read back once,
 * here, to be checked).  Both weights 0 switches the term off, and the pointers may then be null.  Errors: a negative or
 * non-finite weight, a non-finite height, K outside 2 .. 16, a foot without points, a vertex id outside [0, V), w_con > 0 with
 * null contacts.  Works with robust_sigma, the joint-acceleration and foot-lock terms, the latent marker offsets, three-corner
 * placements and the point-to-surface term.  Refused (at evaluation) for the part stage and with w_soft != 0, and inside
 * lock-step batches (uuo_batch_*). */
int uuo_fit_set_floor(uuo_fit_t* fit, float w_pen, float w_con, float height, const int32_t* d_vids, int32_t k_left,
                      int32_t k_right, const float* d_contacts);
/* EXTENSION (not reference behaviour; SMPLify's interpenetration term is the classic of this kind, the reference has none): a
 * bone-capsule self-penetration term on the 24 kinematic world joints J = G_j^t of the chamfer and marker stages (the
 * translation is not read: the term is translation invariant).  Capsule c = (u, v, alpha, beta, r): two joints, two parameters
 * on the line through them, a radius in metres; a_c = J_u + alpha (J_v - J_u), b_c = J_u + beta (J_v - J_u); alpha == beta is a
 * sphere, values outside [0, 1] reach past the joints.  Pair k = (i, j): two capsule indices.  For every frame and pair
 *   (s, t) = closest-point parameters of the segments [a_i, b_i], [a_j, b_j] (Ericson, Real-Time Collision Detection 5.1.9: a
 *            segment with |b - a|^2 <= 1e-12 is a point, den = A E - b^2 <= 1e-6 A E is parallel and takes s = 0)
 *   c_i = a_i + s (b_i - a_i),  c_j = a_j + t (b_j - a_j),  delta = c_i - c_j,  d = |delta|,  pen = max(r_i + r_j - d, 0)
 *   loss += w sum_t sum_k pen^2 / F            (1 / F only: a weight does not depend on the pair list)
 *   dL/dc_i = -(2 w / F) pen delta / d = -dL/dc_j   (s, t held fixed; d == 0: no gradient, pen^2 still counts)
 *   gamma_i = alpha_i + s (beta_i - alpha_i):  dL/dJ_{u_i} += (1 - gamma_i) dL/dc_i,  dL/dJ_{v_i} += gamma_i dL/dc_i  (same for j)
 * in m^2.  Frames are not coupled: F = 1 is a valid problem.  The radii do not follow the shape parameters.
 * A setting of the WORKSPACE (off at creation) with the lifetime rules of uuo_fit_set_joint_accel.  The three lists are HOST
 * arrays -- h_cap_joints [C][2], h_cap_geom [C][3] (alpha, beta, radius), h_pairs [P][2] -- checked and COPIED at the call: the
 * library owns the device copies and a joint -> (pair, end) table it builds from them, in pair order, from which the kernel
 * sums the joints' gradients without atomics (results are bit-reproducible).  A call with the lists of the previous call
 * uploads nothing.  w == 0 switches the term off; the pointers may then be null, and every result is that of a workspace that
 * never had the setting.  Errors (-22): a negative or non-finite w, C outside 1 .. 32, P outside 1 .. 256, a joint id outside
 * [0, 24) or u == v, a non-finite alpha or beta, a radius <= 0 or non-finite, a pair index outside [0, C) or i == j, null arrays
 * with w > 0.  Works with robust_sigma, the joint-acceleration, foot-lock and floor-contact terms, the latent marker offsets,
 * three-corner placements, the point-to-surface term and the per-frame vertex table.  Refused (at evaluation) for the part stage
 * and with w_soft != 0, and inside lock-step batches (uuo_batch_*). */
int uuo_fit_set_capsules(uuo_fit_t* fit, float w, int32_t n_caps, const int32_t* h_cap_joints, const float* h_cap_geom,
                         int32_t n_pairs, const int32_t* h_pairs);
/* EXTENSION (not reference behaviour; SMPLify's angle prior on knees and elbows is the classic of this kind, the reference has
 * none): a joint-angle limit term on the body pose of the chamfer and marker stages, the only term that looks at a joint's own
 * rotation.  Body joint j = 1 .. 23, R its local rotation as the closure's forward uses it (after the stage's Gram-Schmidt
 * normalisation), row-major:
 *   s = 1/2 (R21 - R12, R02 - R20, R10 - R01),  c = 1/2 (R00 + R11 + R22 - 1),  n = |s|,  theta = atan2(n, c),
 *   omega = kappa s,  kappa = theta / n                       (the axis-angle vector of R)
 *   n < 1e-4 and c >= 0: kappa = 1, d kappa = 0 (identity);  n < 1e-4 and c < 0: the joint contributes nothing (half turn)
 *   pen[j][k] = max(omega_k - hi[j][k], 0) + max(lo[j][k] - omega_k, 0)      k = x, y, z;  lo <= hi, -inf / +inf = no bound
 *   loss += w sum_t sum_j sum_k pen^2 / F                     (1 / F only, as for the capsules)
 *   dL/d omega_k = (2 w / F) (max(omega_k - hi, 0) - max(lo - omega_k, 0))
 * in rad^2.  Frames are not coupled: F = 1 is a valid problem.  The root orientation, z, the translation and the shape are not
 * read.  The gradient reaches the raw 3x3 pose entries through the stage's own Gram-Schmidt backward: third raw rows receive
 * exact zeros from the term, as from the data term.
 * A setting of the WORKSPACE (off at creation) with the lifetime rules of uuo_fit_set_joint_accel.  h_lo, h_hi are HOST arrays
 * [23][3] (row j - 1 is SMPL joint j), checked and COPIED at the call: the library owns the device copy.  A call with the tables
 * of the previous call uploads nothing; new tables wait for the last evaluation that read the old ones, on its stream alone.
 * w == 0 switches the term off; the pointers may then be null, and every result is that of a workspace that never had the
 * setting.  Errors (-22): a negative or non-finite w, a NaN bound, lo > hi, lo = +inf or hi = -inf, null arrays with w > 0; a
 * refused call changes nothing: the weight and the tables of the last accepted call stay in force.
 * Sums in a fixed order, no atomics: results are bit-reproducible.  Works with robust_sigma, the joint-acceleration, foot-lock,
 * floor-contact and self-penetration terms, the latent marker offsets, three-corner placements, the point-to-surface term and
 * the per-frame vertex table.  Refused (at evaluation) for the part stage and with w_soft != 0, and inside lock-step batches
 * (uuo_batch_*). */
int uuo_fit_set_joint_limits(uuo_fit_t* fit, float w, const float* h_lo, const float* h_hi);
/* EXTENSION (not reference behaviour; SMPLify's learned pose prior, the max-mixture of Gaussians over the 69 axis-angle
 * components of the body pose): a mixture pose prior on the chamfer and marker stages.  theta [69] is the concatenation of the
 * body joints' axis-angle vectors omega_j, j = 1 .. 23, each formed as for uuo_fit_set_joint_limits (same R, same branches: a joint
 * within 1e-4 of a half turn has omega_j = 0 and receives no gradient).  Component k = 0 .. K-1, 1 <= K <= 16: mean mu_k [69],
 * A_k [69][69] lower triangular with A_k A_k^T the inverse covariance, offset b_k = -log pi_k + 1/2 log det Sigma_k shifted so
 * that the least is 0:
 *   e_k = 1/2 |A_k^T (theta - mu_k)|^2 + b_k,   E = min_k e_k (ties: the lowest k),   loss += w sum_t E(theta_t) / F
 *   dE/d theta = A_k* (A_k*^T (theta - mu_k*))   for the winner k*; no gradient through the choice.
 * Frames are not coupled: F = 1 is a valid problem.  The root orientation, z, the translation and the shape are not read.  The
 * gradient reaches the raw 3x3 pose entries through the stage's own Gram-Schmidt backward: third raw rows receive exact zeros.
 * A setting of the WORKSPACE (off at creation) with the lifetime and ordering rules of uuo_fit_set_joint_limits.  h_means
 * [K][69], h_chol [K][69][69] (A_k row-major; what is above the diagonal is not read) and h_offsets [K] are HOST float32 arrays,
 * checked and COPIED at the call.  A call with the arrays of the previous call uploads nothing; new ones wait for the last
 * evaluation that read the old table, on its stream alone.  w == 0 switches the term off; K is then not looked at and the
 * pointers may be null, and every result is that of a workspace that never had the setting.  Errors (-22), each with its own
 * text: a negative or non-finite w, K outside 1 .. 16, null arrays with w > 0, a non-finite entry, a non-positive diagonal entry
 * of an A_k, a negative offset; a refused call changes nothing.
 * Sums in an order fixed by the indices alone, no atomics: results are bit-reproducible, and a frame's result does not depend on
 * the frames around it.  Works with what uuo_fit_set_joint_limits works with, with that term, the pose-acceleration term, the
 * pose prior's weights and the key-point reprojection term.  Refused (at evaluation, -22) for the part stage and with
 * w_soft != 0, and inside lock-step batches (uuo_batch_*).  uuo_problem_t and uuo_abi_version() are unchanged. */
int uuo_fit_set_pose_gmm(uuo_fit_t* fit, float w, int K, const float* h_means, const float* h_chol, const float* h_offsets);
/* EXTENSION (not reference behaviour): a pose-acceleration term on the LOCAL rotations of the 23 body joints of the chamfer and
 * marker stages.  R_t[j] is joint j's local rotation in frame t as the forward forms it (the stage's Gram-Schmidt of the raw
 * entries, or the raw entries themselves where the stage does not normalise), u[23] >= 0 joint weights:
 *   a_t[j] = R_t[j] - 2 R_{t+1}[j] + R_{t+2}[j]                          t = 0 .. F-3
 *   loss += w / ((F - 2) 207) sum_t sum_j u[j] |a_t[j]|_F^2
 *   dL/dR_s[j] = 2 w / ((F - 2) 207) u[j] (a_s - 2 a_{s-1} + a_{s-2})    a_t outside 0 .. F-3 counts as 0
 * in rad^2 per frame^4: the weight belongs to the frame rate.  The term couples neighbouring frames.  With F < 3 it has no terms:
 * no kernel runs and every result is that of a workspace without the setting.  The root orientation, z, the translation and the
 * shape are not read.  The gradient reaches the raw 3x3 pose entries through the stage's own Gram-Schmidt backward: third raw
 * rows receive exact zeros from the term; a joint of weight 0 receives nothing.
 * A setting of the WORKSPACE (off at creation) with the lifetime rules of uuo_fit_set_joint_limits.  h_joint_weights is a HOST
 * array [23] (entry j - 1 is SMPL joint j) or null (ones), checked and COPIED at the call.  A call with the table of the
 * previous call uploads nothing; a new table waits for the last evaluation that read the old one, on its stream alone.
 * w == 0 switches the term off and looks at nothing else.  Errors (-22): a negative or non-finite w, a NaN, negative or
 * non-finite joint weight; a refused call changes nothing.
 * Sums in a fixed order, no atomics: results are bit-reproducible.  Works with what uuo_fit_set_joint_limits works with, with
 * that term, the pose prior's weights and the key-point reprojection term.  Refused (at evaluation, -22) for the part stage
 * and with w_soft != 0, and inside lock-step batches (uuo_batch_*).  uuo_problem_t and uuo_abi_version() are unchanged. */
int uuo_fit_set_pose_accel(uuo_fit_t* fit, float w, const float* h_joint_weights);
/* EXTENSION (not reference behaviour; the reference's author left `weighted_mse_loss(pose_body, o_pose_body, img_mask[...])`
 * commented out in its chamfer closure): a weight per (frame, body joint) on the pose prior of the chamfer and marker stages,
 * w[F][23] >= 0 (row j - 1 of a frame is SMPL joint j).  With raw the optimised raw body rotations and o = d_o_pose:
 *   prior = w_pose / (F 207) sum_t sum_j w[t][j] sum_e (raw[t][j][e] - o[t][j][e])^2
 *   d prior / d raw[t][j][e] = 2 w_pose / (F 207) w[t][j] (raw - o)
 * in place of the uniform w_pose / (F 207) sum (raw - o)^2.  The normaliser stays F 207, not sum w: w == 1 everywhere is the
 * uniform term (to rounding: other kernels form it), and a weight means the same whatever the number of frames it is lowered
 * on.  Frames are not coupled: F = 1 is a valid problem.  Every entry of a (frame, joint) with w == 0 receives an exact +0 from
 * the prior; a third raw row that sits on its target receives exact zeros whatever its weight, and uuo_lbfgs_solve decides the
 * compact packing from the problem's own w_pose and rows, as without the setting.
 * A setting of the WORKSPACE (null at creation) with the lifetime rules of uuo_fit_set_foot_lock: `d_weights` is a device
 * pointer to [F][23] floats that the caller keeps alive and may rewrite; it is read at every evaluation, not copied, and not
 * checked (finite values >= 0 are the caller's duty).  Null switches the setting off, and every result is that of a workspace
 * that never had it.  With w_pose == 0 there is no prior to weigh and the setting changes nothing.
 * Sums in a fixed order, no atomics: results are bit-reproducible.  Works with robust_sigma, the joint-acceleration, foot-lock,
 * floor-contact, self-penetration and joint-angle limit terms, the latent marker offsets, three-corner placements, the
 * point-to-surface term and the per-frame vertex table.  Refused (at evaluation, -22) for the part stage and with w_soft != 0,
 * and inside lock-step batches (uuo_batch_*).  uuo_problem_t and uuo_abi_version() are unchanged. */
int uuo_fit_set_prior_weights(uuo_fit_t* fit, const float* d_weights);
/* EXTENSION (not reference behaviour; SMPLify's data term is the classic of this kind; the reference projects key points in its
 * 2D-prior stage only): a 2D key-point reprojection term on the 24 kinematic joints J[t][j] = G_j^t + trans_t of the chamfer
 * and marker stages.  Frame t carries a pinhole camera in WORLD axes, d_cam[t] = 16 floats: A (3x3, row-major), b (3), fx, fy,
 * cx, cy; d_targets[t][j] are two image coordinates, d_conf[t][j] >= 0 a confidence:
 *   p = A J + b,  u = (fx p_x / p_z + cx, fy p_y / p_z + cy),  r = u - y,  s = |r|^2
 *   valid[t][j] = c > 0 and p finite and p_z >= min_depth
 *   loss += w / (48 F) sum_valid c rho(s)        rho(s) = s sigma^2 / (sigma^2 + s) (Geman-McClure);  sigma == 0: rho(s) = s
 *   k = 2 w c rho'(s) / (48 F),   rho' = (sigma^2 / (sigma^2 + s))^2;  sigma == 0: 1
 *   dL/dp = k (r_x fx / p_z, r_y fy / p_z, -(r_x fx p_x + r_y fy p_y) / p_z^2),   dL/dJ = A^T dL/dp
 * in the camera's own units (pixels, or units of the image size): the weight belongs to them.  48 F is the size of the target
 * array.  An invalid pair contributes exact zeros to the loss and to the gradient.  Frames are not coupled: F = 1 is a valid
 * problem.  The gradient reaches the translation, the shape, the root orientation (z in the chamfer stage) and the body pose.
 * A setting of the WORKSPACE (off at creation) with the lifetime rules of uuo_fit_set_floor: the three arrays are device
 * pointers that the caller keeps alive and may rewrite; they are read at every evaluation, not copied and not checked (finite
 * values and confidences >= 0 are the caller's duty).  w == 0 switches the term off, nothing else is then looked at and the
 * pointers may be null; every result is that of a workspace that never had the setting.  Errors (-22): a negative or non-finite
 * w, sigma < 0, non-finite or with a square that is no normal float (outside [1e-18, 1e18]), min_depth <= 0 or non-finite, a
 * null array with w > 0.  Sums in a fixed order, no atomics: results are bit-reproducible.  Works with robust_sigma, the
 * joint-acceleration, foot-lock, floor-contact, self-penetration and joint-angle limit terms, the pose prior's weights, the
 * latent marker offsets, three-corner placements, the point-to-surface term and the per-frame vertex table.  Refused (at
 * evaluation, -22) for the part stage and with w_soft != 0, and inside lock-step batches (uuo_batch_*).  uuo_problem_t and
 * uuo_abi_version() are unchanged. */
int uuo_fit_set_keypoints2d(uuo_fit_t* fit, float w, float sigma, float min_depth, const float* d_cam, const float* d_targets,
                            const float* d_conf);
/* EXTENSION (not reference behaviour; MoSh-style fitters score a marker by its distance to the SKIN less its stand-off, the
 * reference's chamfer term by its distance to the nearest VERTEX): on = 1 replaces the chamfer stage's data term
 * min_v |x - v|^2 by the point-to-surface term on the one-ring of the nearest vertex v^ the closure's search finds anyway:
 *   p, b = closest point of x on the faces incident to v^ (ascending face id, lowest id on exact ties; no incident face: v^
 *          itself), b its barycentric weights at the winning face's corners i_0..2
 *   s    = (|x - p| - surface_distance)^2,   loss_data = w_data (1 / sum mask) sum mask rho(s)   (rho: robust_sigma)
 * The face is picked in the search's vertex buffer; p, b and s are then formed on the three corners re-skinned in fp32.
 * b is held fixed in the gradient (the envelope theorem: exact wherever the term is differentiable):
 *   d s / d v[i_k] = -2 (|x - p| - surface_distance) / |x - p| b_k (x - p);   |x - p| = 0: no gradient.
 * Mask and normaliser are the vertex term's; d_nn_idx of uuo_closure_eval still reports v^; works with robust_sigma and the
 * joint-acceleration and foot-lock terms.  Needs uuo_model_set_faces on the workspace's model.
 * A setting of the WORKSPACE (off at creation) with the lifetime rules of uuo_fit_set_joint_accel -- uuo_problem_t stays as it
 * is.  Refused (at evaluation) for the marker and part stages and with w_soft != 0, by uuo_lbfgs_solve_shared, and inside
 * lock-step batches (uuo_batch_*, whose workspaces cannot carry it).  surface_distance: metres, >= 0, finite.  on = 0: every
 * result is that of a workspace that never had the term. */
int uuo_fit_set_surface(uuo_fit_t* fit, int32_t on, float surface_distance);
/* EXTENSION: the corners and weights the last surface-term evaluation (uuo_fit_set_surface) on `fit` used: d_corners
 * [F,M,3] int32 vertex ids, d_bary [F,M,3] their weights (either may be NULL); hidden markers carry (v^, v^, v^).  Device to
 * device on `stream`, ordered behind that evaluation.  Fails if no such evaluation has run on the workspace. */
int uuo_fit_surface_corners(uuo_fit_t* fit, void* stream, int32_t* d_corners, float* d_bary);
/* EXTENSION (not reference behaviour; see uuo_assign_segments_argmin): the marker stage's one-hot closure on a PER-FRAME vertex
 * table.  With d_assign_fm set, item (f, m) of the marker closure takes its vertex from d_assign_fm[f M + m] instead of
 * uuo_problem_t.d_assign[m]; an entry < 0 is an item of weight 0.  Everything else is unchanged: the data term's definition, its
 * 1 / (F M) normaliser, marker_distance, the priors, the solver's fused statistics; works with robust_sigma and the
 * joint-acceleration and foot-lock terms (separate kernel instantiations, the plain ones are unchanged).
 * A setting of the WORKSPACE (null at creation) with the lifetime rules of uuo_fit_set_joint_accel -- uuo_problem_t stays as it
 * is (d_assign must still be a valid [M] table; it is not read).  `d_assign_fm` is a device pointer to [F][M] int32 that the
 * caller keeps alive and may rewrite; it is read at every evaluation, not copied.  NULL = off: every result is that of a
 * workspace that never had the table.  Refused (at evaluation) for the chamfer and part stages, with n_corners == 3, with
 * w_offsets != 0 (an offset per column has no meaning once the column changes identity) and with w_soft != 0, by
 * uuo_lbfgs_solve_shared, and inside lock-step batches (uuo_batch_*). */
int uuo_fit_set_frame_assign(uuo_fit_t* fit, const int32_t* d_assign_fm);
/* The root stages' translation-velocity weight w_tv (stages.root.losses.trans_vel of the reference, optimization.py:106-110).
 * A setting of the WORKSPACE (0 at creation) that only evaluations of UUO_STAGE_ROOT and UUO_STAGE_ROOT_SHARED read: every
 * other stage ignores it, so no other problem has to reset it.  w >= 0, finite. */
int uuo_fit_set_root_trans_vel(uuo_fit_t* fit, float w);
/* number of parameters of a stage at (F): 211F+10 / 219F+10 / 3F+11; the marker stage with w_offsets != 0: 219F+10+3M; the root
 * stages: 4F+10 (UUO_STAGE_ROOT) / 3F+11 (UUO_STAGE_ROOT_SHARED) */
int uuo_problem_num_params(const uuo_problem_t* p);

/* One closure evaluation at d_x: writes loss to d_loss[0] and the flat gradient to d_grad.
 * d_nn_idx (optional, [F,M] int32) receives the nearest-vertex assignment of the chamfer/part data term
 * (vertex ids for chamfer, candidate positions for part).  Asynchronous on `stream`. */
int uuo_closure_eval(uuo_fit_t* fit, void* stream, const uuo_problem_t* p, const float* d_x, float* d_loss,
                     float* d_grad, int32_t* d_nn_idx);

/* ---- L-BFGS ----------------------------------------------------------------------------------------
 * Replaces torch.optim.LBFGS(params, max_iter, tolerance_grad, tolerance_change, lr,
 * line_search_fn="strong_wolfe").step(closure) as constructed at optimization.py:176-183,319-326 and
 * markers/markers_utils.py:428-435 (history 100, max_eval = max_iter*5/4, c1 1e-4, c2 0.9; torch 2.10
 * semantics incl. max_ls = max_eval - evals).  d_x is updated in place.  Synchronises `stream`
 * (one small read-back per closure evaluation). */
typedef struct {
  int32_t max_iter;
  int32_t history_size;     /* 100 */
  float lr;
  float tolerance_grad;
  float tolerance_change;
  int32_t max_eval;         /* <=0: max_iter*5/4 */
  int32_t verbose;          /* print "<name> <iteration> <loss>" per closure like the reference's verbose flag */
} uuo_lbfgs_options_t;

typedef struct {
  int32_t n_iter;
  int32_t n_eval;
  float first_loss;
  float final_loss;
  int32_t stop_reason;      /* 0 max_iter, 1 max_eval, 2 grad tol, 3 step tol, 4 loss tol, 5 gtd, 6 initial grad tol */
  float device_ms;          /* HIP-event time of the whole solve */
} uuo_lbfgs_stats_t;

/* optional per-closure callback (mirrors iter_fn / verbose prints, optimization.py:259-272,378-391): called on
 * the host, from the thread that called uuo_lbfgs_solve, after each closure evaluation with (user, evaluation
 * index, loss, device pointer of the parameter vector that was evaluated -- valid, and ordered after the
 * evaluation on the solve's stream, until the callback returns). */
typedef void (*uuo_eval_callback_t)(void* user, int eval_index, float loss, const float* d_x_eval);

int uuo_lbfgs_solve(uuo_fit_t* fit, void* stream, const uuo_problem_t* p, float* d_x,
                    const uuo_lbfgs_options_t* opt, uuo_lbfgs_stats_t* stats, uuo_eval_callback_t cb,
                    void* cb_user);

/* EXTENSION (BASELINE configs[3] "shared beta over xGMI"; NOT reference behaviour -- the reference fits every sequence with
 * its own betas, test/test.py:57-112): uuo_lbfgs_solve called together by the `world` ranks of a group, one stage problem
 * (same stage) per rank, as ONE joint L-BFGS problem whose 10 betas are shared by all ranks' sequences.  Each rank keeps its
 * own parameters and a replica of the betas on its own device; the driver is uuo_lbfgs_solve's, and all that crosses the
 * ranks goes through `gather` -- called on the host, from the calling thread, at the same points on every rank:
 *   once at the start (the betas themselves: rank 0's values win), once per closure evaluation (16 doubles + a status word: loss, g.d,
 *   gradient norms of the rank's own parameters, max|d|, its 10 betas-gradient entries) and once per iteration (the new
 *   Gram rows of the history, 627 doubles).  `gather(user, mine, n, all)` must fill all[r*n .. r*n+n) with rank r's `mine`
 *   for r = 0..world-1 (an all_gather: RCCL / gloo through torch.distributed in the Python mirror) and return 0.  Every rank
 *   reduces the gathered tables in rank order, so all ranks take bit-identical decisions and end with bit-identical betas.
 * With world = 1 the result is bit-identical to uuo_lbfgs_solve (chamfer and marker stages). */
typedef int (*uuo_gather_fn)(void* user, const double* mine, int n, double* all);
typedef struct {
  uuo_gather_fn gather;
  void* user;
  int32_t rank, world;
} uuo_shared_t;
int uuo_lbfgs_solve_shared(uuo_fit_t* fit, void* stream, const uuo_problem_t* p, float* d_x,
                           const uuo_lbfgs_options_t* opt, uuo_lbfgs_stats_t* stats, const uuo_shared_t* shared,
                           uuo_eval_callback_t cb, void* cb_user);

/* Node-local transport for uuo_shared_t.gather: a mailbox in POSIX shared memory (csrc/mailbox.hip).  One table per
 * concurrent lane of solves (name: "/something", the same on every rank; rank 0 creates it, the others wait for it);
 * uuo_mailbox_gather is a uuo_gather_fn whose `user` is the mailbox: rank r copies its message into its row and reads the
 * other rows as their sequence words arrive -- no system call, collective library or interpreter on the path of the
 * 17 doubles a closure evaluation exchanges.  Messages are <= 640 doubles.  `timeout_s` (<= 0: 120 s) bounds every wait. */
typedef struct uuo_mailbox uuo_mailbox_t;
int uuo_mailbox_open(const char* name, int32_t rank, int32_t world, double timeout_s, uuo_mailbox_t** out);
int uuo_mailbox_close(uuo_mailbox_t* mb);
int uuo_mailbox_gather(void* mailbox, const double* mine, int n, double* all);
int uuo_mailbox_stats(uuo_mailbox_t* mb, unsigned long long* gathers, unsigned long long* nanoseconds);

/* The same driver for a closure composed on the host (the reference's optional objectives: the 2D reprojection fit,
 * utils/hmr_utils.py:170-425 (step at :367) -- which also has a fused closure of its own, uuo_reprojection_* above; the chamfer / marker / part stages with velocity, ground, foot-contact,
 * per-part or reprojection terms, optimization.py:187-275,329-394, markers/markers_utils.py:454-562): replaces
 * torch.optim.LBFGS(params, ..., line_search_fn="strong_wolfe").step(closure) over the flat parameter vector d_x
 * (n floats, torch's order = the order of the params list).  `closure(user, stream, d_x_eval, d_loss, d_grad)` must
 * enqueue on `stream` the work that writes the loss (1 float) and the gradient (n floats) at d_x_eval and return 0;
 * a non-zero return aborts the solve with that code.  The history, the two-loop products, the line search and every
 * termination test run on the device / in the library as in uuo_lbfgs_solve. */
typedef int (*uuo_closure_fn)(void* user, void* stream, const float* d_x_eval, float* d_loss, float* d_grad);
int uuo_lbfgs_minimize(void* stream, int n, float* d_x, const uuo_lbfgs_options_t* opt, uuo_lbfgs_stats_t* stats,
                       uuo_closure_fn closure, void* user, uuo_eval_callback_t cb, void* cb_user);
/* ---- the 2D-prior fit as one fused closure ----------------------------------------------------------------
 * Replaces the closure of optim_reprojection (utils/hmr_utils.py:281-365: two SMPL forwards, perspective_projection
 * :14-52, masked key-point L2 :321 and a one-directional chamfer_distance :333 per evaluation) and, with
 * uuo_reprojection_solve, the torch.optim.LBFGS(...).step(closure) at :367 for ONE yaw hypothesis.  Parameter vector, in the
 * order of the reference's params list (:276-279):  x = [yaw 1 | body translation 3F (HMR axes) | camera translation 3 |
 * betas 10 (in the list but detached, :218,292: zero gradient, never moves)]  = 3F + 14 floats.
 * The body pose, the shape and the HMR root orientation are constants of this solve, so the caller runs ONE forward
 * (uuo_smpl_forward: HMR pose, the solve's betas, the HMR root orientation, zero translation) and hands its joints and
 * vertices over; the closure needs no skinning (uuo_mocap_amd/csrc/reprojection.hip). */
typedef struct {
  int32_t F, M, V, J;        /* frames, markers, vertices, joints per frame (SMPL + vertex joints: 45; at most 64) */
  const float* d_markers;    /* [F,M,3] */
  const float* d_joints0;    /* [F,J,3] joints of that forward (joint 0 = the pelvis the root rotation turns about) */
  const float* d_verts0;     /* [F,V,3] vertices of that forward */
  const float* d_kp_target;  /* [F,J,2] HMR key points (NaN already replaced by 0, :236) */
  const float* d_mask;       /* [F] 1 = frame has a valid HMR camera (:240) */
  float focal[2];            /* mean focal length / 256 (:258) */
  float center[2];           /* camera centre (zeros in HMR 2.0, hmr_utils.py:96) */
  float w_reprojection, w_chamfer; /* stages.reprojection_part.losses */
} uuo_reprojection_problem_t;
typedef struct uuo_reprojection uuo_reprojection_t;
int uuo_reprojection_create(const uuo_reprojection_problem_t* p, uuo_reprojection_t** out);
int uuo_reprojection_destroy(uuo_reprojection_t* h);
int uuo_reprojection_num_params(const uuo_reprojection_problem_t* p); /* 3F + 14 */
/* One closure evaluation at d_x: loss to d_loss[0], gradient to d_grad[3F+14]; optional outputs: d_kp [F,J,2] the projected
 * key points (+0.5, as the reference's joints_2d), d_nn_idx [F,M] the nearest vertex of every marker, -1 for a marker that
 * has none (NaN coordinates: it adds nothing to the loss or the gradient, the divisor stays F M).  Asynchronous. */
int uuo_reprojection_eval(uuo_reprojection_t* h, void* stream, const float* d_x, float* d_loss, float* d_grad,
                          float* d_kp, int32_t* d_nn_idx);
/* uuo_lbfgs_solve for this closure.  The reference returns quantities of the LAST closure evaluation (its `nonlocal`
 * temporaries, :296-299,383-425), which is not necessarily the accepted point: d_x_last (optional, 3F+14) and d_kp_last
 * (optional, [F,J,2]) receive that evaluation's parameter vector and key points. */
int uuo_reprojection_solve(uuo_reprojection_t* h, void* stream, float* d_x, const uuo_lbfgs_options_t* opt,
                           uuo_lbfgs_stats_t* stats, float* d_x_last, float* d_kp_last, uuo_eval_callback_t cb,
                           void* cb_user);

/* How the solver's host threads wait for the device's reports (one 192-byte block in pinned memory per closure evaluation).
 * Default: they spin -- lowest latency, one CPU per solve in flight.  spin_polls >= 0: after that many polls a wait sleeps
 * sleep_ns nanoseconds at a time (for hosts whose CPU quota is smaller than the number of solves in flight: a throttled
 * cgroup stalls every thread of the process); spin_polls < 0 restores pure spinning.  Process-wide. */
int uuo_set_wait_policy(int spin_polls, int sleep_ns);

/* device -> device copy of `bytes` bytes ordered on `stream` (closures written in Python move the evaluated point and
 * the gradient between their own tensors and the driver's vectors with it) */
int uuo_copy_device(void* stream, void* d_dst, const void* d_src, size_t bytes);

/* ---- lock-step batches of independent solves ---------------------------------------------------------
 * The reference solves the candidate body parts of find_best_part_fits one after the other
 * (markers/markers_utils.py:416-610: one torch.optim.LBFGS(...).step(closure) per sub-tree, 202 of them for a 10-marker
 * limb) and likewise the yaw hypotheses (multimodal.py:462-574).  They are independent problems of one stage and one
 * (F, M): a batch steps up to B of them together -- one round = one closure evaluation of every live problem, every
 * kernel of the round launched ONCE for all of them -- with the decisions and the arithmetic of uuo_lbfgs_solve
 * (results are bit-identical to solving each problem alone).  Part-stage problems of one batch share the body pose
 * (d_o_pose) and hence one pose-blend cache.  uuo_batch_solve synchronises `stream`; stats[i].device_ms is 0. */
typedef struct uuo_batch uuo_batch_t;
int uuo_batch_create(uuo_model_t* model, int stage, int F, int M, int B, uuo_batch_t** out);
int uuo_batch_destroy(uuo_batch_t* batch);
int uuo_batch_solve(uuo_batch_t* batch, void* stream, const uuo_problem_t* problems /* [nb] */,
                    float* const* d_xs /* [nb] device vectors, updated in place */, int nb,
                    const uuo_lbfgs_options_t* opt, uuo_lbfgs_stats_t* stats /* [nb] */);
/* Ranking scores of part-stage candidates at d_xs (normally the vectors uuo_batch_solve has just solved; same problems, same
 * batch): h_scores[i] = pytorch3d chamfer_distance(markers_subset, vertices[:, subset_i]) in BOTH directions (mean / mean,
 * squared L2) -- what find_best_part_fits ranks its candidates by (markers/markers_utils.py:566-579, one SMPL forward and two
 * K=1 searches per candidate there).  One batched forward + one score kernel for all candidates; synchronises `stream`. */
int uuo_batch_part_scores(uuo_batch_t* batch, void* stream, const uuo_problem_t* problems, float* const* d_xs, int nb,
                          float* h_scores /* [nb] host */);

/* device -> host copy of n floats, ordered on `stream`, complete on return (for uuo_eval_callback_t users that only
 * hold the raw pointer, e.g. the iter_fn adapter). */
int uuo_copy_to_host(void* stream, const float* d_src, float* h_dst, int n);

/* ---- benchmarking helpers (used by bench.py for the roofline object) -------------------------------
 * average device milliseconds per closure evaluation over `iters` back-to-back evaluations, measured with
 * HIP events on `stream`; dominant_kernel_only 1: the fp32 skinning kernel alone (k_skin2), 2: the skinning kernel of the chamfer
 * closure's search alone (k_skin3, fp16 matrix pipe on split operands), one event pair per launch. */
int uuo_time_closure(uuo_fit_t* fit, void* stream, const uuo_problem_t* p, const float* d_x, int iters,
                     int dominant_kernel_only, float* ms_per_eval);

#ifdef __cplusplus
}
#endif
#endif /* UUO_HIP_H */
