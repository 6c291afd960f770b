/*
 * mpsfm_hip.h — C ABI of libmpsfm_hip.so, the MI355X (gfx950) replacement for the
 * pyceres / pycolmap native boundary that MP-SfM's bundle adjustment and triangulation
 * numerics cross (reference call sites cited per entry point below; paths are relative
 * to the reference checkout).
 *
 * Conventions
 *   - Plain C, no exceptions, no torch types.  Every entry point returns 0 on success or a
 *     negative MPSFM_E* code; mpsfm_last_error() gives a thread-local message.
 *   - The caller owns every buffer.  The library never retains a host pointer after a call
 *     returns (handles own device copies only).
 *   - All floating point is IEEE double.  Indices are int32 (counts int64).
 *   - Quaternions are stored (x, y, z, w) — Eigen order — as in
 *     mpsfm/sfm/mapper/bundle_adjustment.py:113-122 (pose.rotation.quat).
 *   - The library fails loudly (MPSFM_ENODEVICE) when no gfx950 device is present; there is
 *     no CPU fallback inside it.
 */
#ifndef MPSFM_HIP_H
#define MPSFM_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPSFM_ABI_VERSION 2

/* ---- error codes -------------------------------------------------------------------- */
#define MPSFM_OK 0
#define MPSFM_EINVAL (-1)     /* malformed problem (index out of range, NULL pointer, ...) */
#define MPSFM_ENODEVICE (-2)  /* no HIP device / not gfx950 */
#define MPSFM_ENOMEM (-3)     /* host or device allocation failed */
#define MPSFM_EHIP (-4)       /* a HIP runtime call failed */
#define MPSFM_ENUMERIC (-5)   /* the initial point could not be evaluated (NaN / z<=0 in a log) */
#define MPSFM_EUNSUPPORTED (-6)
#define MPSFM_ECOMM (-7)      /* the all-reduce hook reported a failure */

/* ---- loss functions ------------------------------------------------------------------
 * pycolmap.LossFunctionType as mapped in mpsfm/sfm/mapper/bundle_adjustment.py:44-48.
 * rho(s), s = squared residual norm (Ceres semantics):
 *   TRIVIAL  rho = s
 *   SOFT_L1  rho = 2 a^2 (sqrt(1 + s/a^2) - 1)
 *   CAUCHY   rho = a^2 log(1 + s/a^2)
 * Every loss is wrapped as Scaled(rho, magnitude): cost = 1/2 * magnitude * rho(s).      */
enum mpsfm_loss_type { MPSFM_LOSS_TRIVIAL = 0, MPSFM_LOSS_SOFT_L1 = 1, MPSFM_LOSS_CAUCHY = 2 };

/* ---- the flat BA problem -------------------------------------------------------------
 * Exactly what Optimizer.__build_problem (bundle_adjustment.py:67-185) gathers before it
 * calls pyceres.solve: the images of the bundle (with gauge flags), the 3-D points their
 * observations reference, one 2-residual PINHOLE reprojection block per observation
 * (pycolmap.create_default_bundle_adjuster, :85-104) and one 1-residual log-depth block per
 * valid depth prior (pycolmap.create_depth_bundle_adjuster, :163-176).                   */
typedef struct mpsfm_ba_problem {
  int32_t n_cams;  /* images (poses) referenced by the observation lists            */
  int32_t n_pts;   /* 3-D points                                                      */
  int32_t n_intr;  /* distinct PINHOLE intrinsics                                     */

  const double* cam_intr;        /* [n_intr][4]  fx fy cx cy; constant (:92-94)      */
  const int32_t* cam_intr_idx;   /* [n_cams]                                          */
  const uint8_t* pose_const;     /* [n_cams] 1: quat and translation constant
                                    (first bundle image :114-116, fix_pose, or an image
                                    outside the bundle that sees a variable point)     */
  int32_t gauge_axis_cam;        /* camera whose translation x is held fixed
                                    (SubsetManifold(3,[0]), :117-121), or -1           */
  const uint8_t* pt_const;       /* [n_pts] 1: point constant                          */

  int64_t n_obs;                 /* reprojection residual blocks                        */
  const int32_t* obs_cam;        /* [n_obs]                                             */
  const int32_t* obs_pt;         /* [n_obs]                                             */
  const double* obs_xy;          /* [n_obs][2] pixel measurement (Point2D.xy)           */
  int32_t reproj_loss_type;      /* mpsfm_loss_type (reference default SOFT_L1, :24)    */
  double reproj_loss_scale;      /* a  = reproj_loss_scale * kp_std (:101)              */
  double reproj_loss_magnitude;  /* k  = 1 / kp_std^2 (:99)                             */

  int64_t n_dobs;                /* log-depth residual blocks (0: reprojection only)    */
  const int32_t* dobs_cam;       /* [n_dobs]                                            */
  const int32_t* dobs_pt;        /* [n_dobs]                                            */
  const double* dobs_depth;      /* [n_dobs] prior depth d sampled at the keypoint      */
  const double* dobs_magnitude;  /* [n_dobs] m = d^2 / clip(var,1e-6) (:161)            */
  const double* dobs_param;      /* [n_dobs] a = mult * rob_std * sqrt(var) / d (:160)  */
  int32_t depth_loss_type;       /* CAUCHY in ba(), TRIVIAL in refine_3d_points()       */
  const double* shift_logscale;  /* [n_cams][2] constant per-image (shift b, log-scale s)
                                    of the prior, NULL = zeros (:83, :178-182)          */
} mpsfm_ba_problem;

/* Parameters the solver updates in place, like Ceres does through the pybind11 views. */
typedef struct mpsfm_ba_state {
  double* cam_quat_xyzw; /* [n_cams][4] */
  double* cam_t;         /* [n_cams][3] */
  double* pts;           /* [n_pts][3]  */
} mpsfm_ba_state;

/* Sum-all-reduce hook for landmark-sharded BA: called with a buffer of `count` doubles that
 * must be replaced by its element-wise sum over all ranks before the hook returns (or, for a
 * device buffer, before later work on `stream`).  `on_device` is 1 when `buf` is device
 * memory of the handle's device.  Return 0 on success. */
typedef int (*mpsfm_allreduce_fn)(void* user, double* buf, int64_t count, int on_device,
                                  void* stream);

/* Solver options.  mpsfm_ba_default_options() fills the pyceres.SolverOptions() defaults
 * that Optimizer.solve leaves untouched (bundle_adjustment.py:285-293). */
typedef struct mpsfm_ba_options {
  int32_t max_num_iterations;               /* 50    */
  double function_tolerance;                /* 1e-6  */
  double gradient_tolerance;                /* 1e-10 */
  double parameter_tolerance;               /* 1e-8  */
  double initial_trust_region_radius;       /* 1e4   */
  double max_trust_region_radius;           /* 1e16  */
  double min_trust_region_radius;           /* 1e-32 */
  double min_relative_decrease;             /* 1e-3  */
  double min_lm_diagonal;                   /* 1e-6  */
  double max_lm_diagonal;                   /* 1e32  */
  int32_t max_num_consecutive_invalid_steps;/* 5     */
  int32_t jacobi_scaling;                   /* 1     */
  int32_t device;                           /* HIP device ordinal                      */
  void* stream;                             /* hipStream_t to run on, NULL = own stream */
  int32_t verbose;                          /* >0: per-iteration line on stderr         */
  mpsfm_allreduce_fn allreduce;             /* NULL: single shard (or the native RCCL communicator below) */
  void* allreduce_user;
  /* landmark sharding over the GPUs of a node: this rank's position ... */
  int32_t world_size;                       /* 0 / 1: single shard; > 1 with the hook: lets the per-rank maxima (gradient
                                               tolerance test) travel in per-rank slots of the summed buffer           */
  int32_t rank;
  /* ... and, with use_rccl = 1, the library's OWN communicator: ncclCommInitRank(world_size, comm_id, rank) at
     mpsfm_ba_create, ncclAllReduce(sum, fp64) on the handle's stream for every exchange (no host callback per LM
     iteration).  comm_id comes from mpsfm_comm_unique_id() on one rank; the caller hands it to the others. */
  int32_t use_rccl;
  uint8_t comm_id[128];
} mpsfm_ba_options;

#define MPSFM_MAX_TRACE 64

enum mpsfm_termination {
  MPSFM_TERM_FUNCTION_TOLERANCE = 0,
  MPSFM_TERM_GRADIENT_TOLERANCE = 1,
  MPSFM_TERM_PARAMETER_TOLERANCE = 2,
  MPSFM_TERM_MAX_ITERATIONS = 3,
  MPSFM_TERM_MIN_RADIUS = 4,
  MPSFM_TERM_INVALID_STEPS = 5, /* Ceres FAILURE: too many consecutive invalid steps */
  MPSFM_TERM_NO_VARIABLES = 6
};

typedef struct mpsfm_ba_summary {
  double initial_cost;       /* includes fixed_cost */
  double final_cost;         /* includes fixed_cost */
  double fixed_cost;         /* blocks whose camera and point are both constant */
  int32_t num_iterations;    /* LM iterations performed (iteration 0 not counted) */
  int32_t num_successful_steps;
  int32_t num_unsuccessful_steps;
  int32_t termination;       /* mpsfm_termination */
  int64_t num_residual_blocks;   /* reprojection + depth blocks in the problem   */
  int64_t num_residual_evals;    /* residual blocks x (cost or Jacobian) evaluations */
  int64_t num_jacobian_evals;    /* Jacobian sweeps */
  int32_t reduced_dim;       /* order of the reduced camera system */
  double final_radius;
  double time_total_s;       /* wall time of the solve, device-synchronised */
  double time_linearize_s;   /* device time: track sweep (residual/Jacobian/Schur reduce) */
  double time_dense_s;       /* device time: reduced camera system factor + solve          */
  double time_update_s;      /* device time: back-substitution + candidate cost sweep      */
  int32_t trace_len;
  double trace_cost[MPSFM_MAX_TRACE];     /* cost after each iteration (index 0 = initial)  */
  double trace_radius[MPSFM_MAX_TRACE];
  uint8_t trace_accepted[MPSFM_MAX_TRACE];
} mpsfm_ba_summary;

typedef struct mpsfm_ba_handle mpsfm_ba_handle;

/* -- library ------------------------------------------------------------------------- */
int mpsfm_abi_version(void);
const char* mpsfm_last_error(void);
/* number of visible gfx950 devices (0 on a CPU-only host; does not initialise a context) */
int mpsfm_device_count(void);
void mpsfm_ba_default_options(mpsfm_ba_options* opt);
/* ncclGetUniqueId of the RCCL library found in the process (dlopen): 128 bytes for mpsfm_ba_options.comm_id */
int mpsfm_comm_unique_id(uint8_t id[128]);

/* -- bundle adjustment: replaces pyceres.solve(options, bundler.problem, summary)
 *    (bundle_adjustment.py:184, 285-293) ---------------------------------------------- */

/* One-shot: upload, solve, write the refined poses/points back into `state`. */
int mpsfm_ba_solve(const mpsfm_ba_problem* problem, mpsfm_ba_state* state,
                   const mpsfm_ba_options* options, mpsfm_ba_summary* summary);

/* Resident form: the problem lives in HBM between calls (what bench.py times). */
int mpsfm_ba_create(const mpsfm_ba_problem* problem, const mpsfm_ba_state* initial,
                    const mpsfm_ba_options* options, mpsfm_ba_handle** out);
int mpsfm_ba_set_state(mpsfm_ba_handle* h, const mpsfm_ba_state* state); /* H2D            */
int mpsfm_ba_reset_state(mpsfm_ba_handle* h);  /* D2D: back to the state given at create   */
int mpsfm_ba_solve_resident(mpsfm_ba_handle* h, mpsfm_ba_summary* summary);
int mpsfm_ba_get_state(mpsfm_ba_handle* h, mpsfm_ba_state* state);       /* D2H            */
void mpsfm_ba_destroy(mpsfm_ba_handle* h);

/* Cost of the current resident state: 1/2 sum rho, split by block kind. */
int mpsfm_ba_eval_cost(mpsfm_ba_handle* h, double* cost_reproj, double* cost_depth);

/* One Jacobian/Schur track sweep at the current state with trust-region radius `radius`
 * (no parameter update): the launches bench.py prices against the HBM roofline.
 * `elapsed_ms` receives the HIP-event time of the whole sweep (dense chunks, reduction of their slabs,
 * general chunks and long tracks). */
int mpsfm_ba_sweep_once(mpsfm_ba_handle* h, double radius, float* elapsed_ms);
/* The parts of the last mpsfm_ba_sweep_once: ms = {k_track_sweep_dense, k_reduce_slabs, general + long-track kernels},
 * info = {dense chunks, general chunks, long tracks, destination parts of the reduction}.  Either pointer may be NULL. */
int mpsfm_ba_sweep_parts(mpsfm_ba_handle* h, float ms[3], int64_t info[4]);
/* Download the reduced camera system built by the last sweep: S (n x n, row-major, symmetric)
 * and rhs (n); n = summary.reduced_dim = 6 x variable cameras, rows in the CALLER's camera order
 * (the handle keeps its own slot order, see mpsfm_ba_dense_plan).  Test/diagnostic entry point. */
int mpsfm_ba_get_reduced_system(mpsfm_ba_handle* h, double* S, double* rhs, int32_t n);
int mpsfm_ba_reduced_dim(mpsfm_ba_handle* h);
/* Solution y (scaled coordinates, length n) of the last dense solve.  Test/diagnostic. */
int mpsfm_ba_get_dense_solution(mpsfm_ba_handle* h, double* y, int32_t n);
/* Factor + solve only, on the last assembled system (prices the MFMA dense solve). */
int mpsfm_ba_dense_solve_once(mpsfm_ba_handle* h, float* elapsed_ms);
/* How the handle factors the reduced camera system (what Ceres' fill-reducing ordering and sparse
 * Cholesky do behind bundle_adjustment.py:288).  info[0..9] = camera slots (= variable cameras),
 * 32-column tile columns of the system incl. the alignment padding, levels of the tile elimination tree (= factorisation launches),
 * nested-dissection depth (-1: caller's camera order), 1 if the back substitution uses the
 * inverse accumulators, work items, tile products, inverse roles, 6x6 blocks of S stored,
 * back-substitution launches. */
int mpsfm_ba_dense_plan(mpsfm_ba_handle* h, int64_t info[10]);

/* -- point covariances: replaces pycolmap.estimate_ba_covariance(POINTS)
 *    (bundle_adjustment.py:244-261).  cov[j] = (sum_i magnitude * Jp_i^T Jp_i)^-1 over the
 *    reprojection blocks of point j with every other variable held constant.
 *    A point with fewer than two observations gets NaN in all nine entries: one observation
 *    leaves the sum with rank 2, and the count decides, not a pivot, so the answer is the same
 *    on every run.  A point with two or more observations whose sum is not numerically positive
 *    definite gets NaN as well.  The summation order over the observations of a point is free
 *    (atomics): results of two calls agree to rounding, not bit for bit. ------------------- */
int mpsfm_point_covs(const mpsfm_ba_problem* problem, const mpsfm_ba_state* state,
                     int32_t device, double* covs /* [n_pts][3][3] */);

/* -- per-track triangulation numerics: the arithmetic inside
 *    pycolmap.IncrementalTriangulator / ObservationManager used at
 *    mpsfm/sfm/mapper/triangulator.py:48,53-55,123-128 and mapper/base.py:686-797 -------- */
typedef struct mpsfm_tracks {
  int32_t n_cams, n_tracks, n_intr;
  const double* cam_quat_xyzw; /* [n_cams][4] */
  const double* cam_t;         /* [n_cams][3] */
  const double* cam_intr;      /* [n_intr][4] */
  const int32_t* cam_intr_idx; /* [n_cams]    */
  const int64_t* track_start;  /* [n_tracks+1] CSR offsets into the element arrays */
  const int32_t* el_cam;       /* [n_el] */
  const double* el_xy;         /* [n_el][2] */
} mpsfm_tracks;

/* Linear multi-view triangulation of every track (COLMAP TriangulateMultiViewPoint):
 * xyz[t] = smallest eigenvector of sum_i (P_i - x_i x_i^T P_i)^T (...), dehomogenised.
 * A track of fewer than two elements has no two rays to intersect: xyz[t] is NaN in all three
 * coordinates.  A rank-deficient track of two or more elements (the same camera and pixel twice,
 * cameras with one centre and one ray) gets the plain arithmetic: some vector of the null space,
 * dehomogenised, which may be non-finite. */
int mpsfm_triangulate_tracks(const mpsfm_tracks* tracks, int32_t device,
                             double* xyz /* [n_tracks][3] out */);

/* Per-track quality numbers at given points: max pairwise triangulation angle (radians),
 * per-element squared reprojection error and cheirality flags.  Any output pointer may be NULL.
 *   max_tri_angle  largest angle between the rays of two elements, by the law of cosines on squared
 *                  lengths, folded to [0, pi/2]; exactly 0 for a track of fewer than two elements and
 *                  for a pair with a ray of zero length (the point at a projection centre).
 *   el_front       1 where the depth zc of the point in the element's camera is >= 2^-52 (DBL_EPSILON).
 *   el_sq_err      the plain formula |K (xc, yc) / zc + c - xy|^2 whatever the sign of zc: finite, and
 *                  possibly small, for a point mirrored behind the camera; inf or NaN for zc == 0.
 *                  (COLMAP's CalculateSquaredReprojectionError returns DBL_MAX for zc < eps instead.)
 *                  A caller must therefore treat el_front == 0 as "bad" by itself, as
 *                  reprojection_decisions in mpsfm_amd/sfm/scene/observations.py does. */
int mpsfm_filter_tracks(const mpsfm_tracks* tracks, const double* xyz /* [n_tracks][3] */,
                        int32_t device, double* max_tri_angle /* [n_tracks] */,
                        double* el_sq_err /* [n_el] */, uint8_t* el_front /* [n_el] */);

/* -- depth lifting of low-parallax points (mpsfm/sfm/mapper/triangulator.py:49-83, 125-161) for a batch of tracks in
 *    one call.  Per track t, with the elements in the order given:
 *      risky[t]      = max_tri_angle[t] < min_angle_rad, the angle bit for bit that of mpsfm_filter_tracks for the same
 *                      inputs (tracks of 0 or 1 elements have angle 0: risky whenever min_angle_rad > 0).
 *      lift_el[t]    of a risky track: the position in the track of the first element e whose camera is activated and
 *                      whose bilinear sample of valid_map at the keypoint is exactly 1 (PriorUtils.valid_at_kps);
 *                      -1 where no element lifts (the caller deletes such a point without a replacement).
 *      lift_depth[t] = d, the bilinear sample of depth_map at the same coordinate.
 *      lift_xyz[t]   = R^T (((x - cx) / fx, (y - cy) / fy, 1) d - t) with the pose and intrinsics of that element's
 *                      camera, every operation rounded on its own.
 *      el_keep[e']   = (row 2 of R' times lift_xyz + t'_2 >= 2^-52) for EVERY element e' of a lifted track, the lifting
 *                      element included (a sampled depth <= 0 drops it).
 *    A track that is not risky, and a risky one that does not lift, get lift_el = -1 and zeros in lift_depth, lift_xyz
 *    and el_keep.  Two phases with one host wait each: the angles (the kernel of mpsfm_filter_tracks), then, for the
 *    risky tracks only, the maps of the activated cameras that occur in them in one staged upload and the lift launch
 *    (one wavefront per risky track).  Without a risky track the call ends after the first phase.
 *    MPSFM_EINVAL: what mpsfm_filter_tracks refuses; NULL maps, NULL arrays of maps, NULL outputs; an activated
 *    camera of a risky track with a NULL map, map_h < 2, map_w < 2 or more than 2^30 pixels; min_angle_rad NaN or
 *    negative.  n_tracks == 0 returns 0 before any device work. -------------------------------------------------- */
typedef struct mpsfm_lift_maps {   /* per camera of mpsfm_tracks, in the same order */
  const uint8_t* activated;        /* [n_cams] image.depth.activated */
  const int32_t* map_h;            /* [n_cams], read where activated */
  const int32_t* map_w;            /* [n_cams], read where activated */
  const double* const* depth_map;  /* [n_cams] -> H*W depth.data; an entry may be NULL where not activated */
  const uint8_t* const* valid_map; /* [n_cams] -> H*W depth.valid; likewise */
  const double* sx;                /* [n_cams] camera.sx */
  const double* sy;                /* [n_cams] camera.sy */
} mpsfm_lift_maps;

typedef struct mpsfm_lift_info {
  int64_t n_risky, n_lifted, n_no_lift; /* risky tracks; those with and without a lifting element */
  int32_t n_maps_uploaded;              /* cameras whose two maps went to the device */
  int64_t bytes_uploaded;               /* bytes of those maps */
  double ms;                            /* device time of the angle launch plus the lift launch (HIP events) */
} mpsfm_lift_info;

int mpsfm_lift_tracks(const mpsfm_tracks* tracks, const double* xyz /* [n_tracks][3] current points */,
                      const mpsfm_lift_maps* maps, double min_angle_rad, int32_t device,
                      uint8_t* risky /* [n_tracks] */, int32_t* lift_el /* [n_tracks] position in the track, -1: none */,
                      double* lift_depth /* [n_tracks] */, double* lift_xyz /* [n_tracks][3] */,
                      uint8_t* el_keep /* [n_el] */, mpsfm_lift_info* info /* may be NULL */);

/* -- row f2: track-graph logic of pycolmap.IncrementalTriangulator as MpsfmTriangulator drives it
 *    (mpsfm/sfm/mapper/triangulator.py:32-48, 88-100, 123, 165-175): Find / Create / Continue, Complete, Merge,
 *    Retriangulate with the fork's ignore_image_ids.  COLMAP 3.11 semantics (the fork's source is not in the reference
 *    tree: parity unpinned).  The scene stays with the caller: it hands over the keypoints + correspondence graph once
 *    and the mutable state before a call; every call leaves an operation log the caller replays on its
 *    ObservationManager (add_point3D / add_observation / delete_point3D).  Keypoints are addressed by their global
 *    index kp_start[image] + point2D_idx; points by their index in the state's arrays (new points continue that range). */
typedef struct mpsfm_tri_options {       /* pycolmap.IncrementalTriangulatorOptions fields used by the calls below */
  int32_t max_transitivity;              /* 1   (only the direct correspondences are implemented)                 */
  double create_max_angle_error;         /* 2.0 degrees                                                            */
  double continue_max_angle_error;       /* 2.0                                                                    */
  double merge_max_reproj_error;         /* 4.0 px                                                                 */
  double complete_max_reproj_error;      /* 4.0 px                                                                 */
  int32_t complete_max_transitivity;     /* 5                                                                      */
  double re_max_angle_error;             /* 5.0                                                                    */
  double re_min_ratio;                   /* 0.2                                                                    */
  int32_t re_max_trials;                 /* 1                                                                      */
  double min_angle;                      /* 1.5 (the mapper overrides it to 0.001, mapper/base.py:35-40)          */
  int32_t ignore_two_view_tracks;        /* 1   (the mapper overrides it to 0)                                     */
} mpsfm_tri_options;
typedef struct mpsfm_tri_graph {
  int32_t n_images;
  const int64_t* kp_start;   /* [n_images+1] */
  const double* kp_xy;       /* [n_kp][2] Point2D.xy */
  const double* cam_intr;    /* [n_images][4] PINHOLE fx fy cx cy */
  const int64_t* corr_start; /* [n_kp+1] CSR of the correspondence graph */
  const int64_t* corr_kp;    /* [n_corr] matched keypoint (global index) */
} mpsfm_tri_graph;
typedef struct mpsfm_tri_state {
  const uint8_t* registered;      /* [n_images] image.has_pose */
  const double* cam_quat_xyzw;    /* [n_images][4] */
  const double* cam_t;            /* [n_images][3] */
  const int64_t* kp_point;        /* [n_kp] index of the keypoint's 3-D point in xyz, or -1 */
  int64_t n_points;
  const double* xyz;              /* [n_points][3] */
} mpsfm_tri_state;
typedef struct mpsfm_triangulator mpsfm_triangulator;
enum mpsfm_tri_op { MPSFM_TRI_ADD_POINT = 0 /* a = point, b = track length, xyz */, MPSFM_TRI_ADD_OBS = 1 /* a = point, b = keypoint */,
                    MPSFM_TRI_DELETE_POINT = 2 /* a = point */ };

void mpsfm_tri_default_options(mpsfm_tri_options* o);
int mpsfm_triangulator_create(const mpsfm_tri_graph* graph, int32_t device, mpsfm_triangulator** out);
void mpsfm_triangulator_destroy(mpsfm_triangulator* h);
int mpsfm_triangulator_set_state(mpsfm_triangulator* h, const mpsfm_tri_state* state);
int mpsfm_triangulator_triangulate_image(mpsfm_triangulator* h, const mpsfm_tri_options* o, int32_t image, int64_t* count);
int mpsfm_triangulator_complete_image(mpsfm_triangulator* h, const mpsfm_tri_options* o, int32_t image, int64_t* count);
/* n < 0: every track (complete_all_tracks / merge_all_tracks) */
int mpsfm_triangulator_complete_tracks(mpsfm_triangulator* h, const mpsfm_tri_options* o, const int64_t* points, int64_t n, int64_t* count);
int mpsfm_triangulator_merge_tracks(mpsfm_triangulator* h, const mpsfm_tri_options* o, const int64_t* points, int64_t n, int64_t* count);
int mpsfm_triangulator_retriangulate(mpsfm_triangulator* h, const mpsfm_tri_options* o, const int32_t* ignore_images, int32_t n_ignore,
                                     int64_t* count);
/* operation log of the last call, in the order the operations happened */
int64_t mpsfm_triangulator_num_ops(mpsfm_triangulator* h);
int64_t mpsfm_triangulator_num_points(mpsfm_triangulator* h);
int mpsfm_triangulator_get_ops(mpsfm_triangulator* h, int32_t* type, int64_t* a, int64_t* b, double* xyz /* [n_ops][3] */);
/* track elements (global keypoint indices) of the log's ADD_POINT operations, concatenated in log order */
int64_t mpsfm_triangulator_num_op_elements(mpsfm_triangulator* h);
int mpsfm_triangulator_get_op_elements(mpsfm_triangulator* h, int64_t* els);
int mpsfm_triangulator_stats(mpsfm_triangulator* h, int64_t* batch, int64_t* batch_hits, int64_t* host_estimates);

/* COLMAP's EstimateTriangulation (LORANSAC<TriangulationEstimator, ..., InlierSupportMeasurer, CombinationSampler>, what
 * IncrementalTriangulator::Create / CompleteImage run per candidate track; reference call sites
 * mpsfm/sfm/mapper/triangulator.py:88-100, 123) for many independent candidate tracks in ONE launch: one thread per
 * candidate, at most 64 views each (MPSFM_EUNSUPPORTED beyond).  The engine above uses the same kernel for its batches.
 * A candidate without a model, and any candidate of 0 or 1 views, gives ok = 0, xyz = (0, 0, 0) and inlier = 0 for each of
 * its views; its neighbours in the batch are not affected.  min_num_trials[i] is taken as given (0: the stop rule alone
 * ends the loop; C(n, 2) or more: every pair is drawn). */
typedef struct mpsfm_tri_candidates {
  int64_t n_candidates;
  const int64_t* cand_start;          /* [n_candidates+1] CSR into the view arrays                                  */
  const double* view_cam_from_world;  /* [n_views][3][4] row-major                                                  */
  const double* view_intr;            /* [n_views][4] PINHOLE fx fy cx cy                                           */
  const double* view_xy;              /* [n_views][2] pixel measurement                                             */
  double min_tri_angle;               /* radians (options.min_angle)                                                */
  double max_error;                   /* radians when residual_type = 0, pixels when 1                              */
  int32_t residual_type;              /* 0 = ANGULAR_ERROR (Create), 1 = REPROJECTION_ERROR (CompleteImage)         */
  const int64_t* min_num_trials;      /* [n_candidates] or NULL = C(n,2) up to 15 views, else 0 (Create's rule)     */
} mpsfm_tri_candidates;
int mpsfm_tri_estimate_batch(const mpsfm_tri_candidates* c, int32_t device, double* xyz /* [n][3] */, uint8_t* ok /* [n] */,
                             uint8_t* inlier /* [n_views] */);

/* -- row f3: depth-block selection of Optimizer.__build_problem for a whole bundle in one launch
 *    (mpsfm/sfm/mapper/bundle_adjustment.py:124-161) and the whitened log-depth errors of
 *    update_truncation_multiplier (:295-333).  Per keypoint that has a 3-D point: bilinear samples of the validity
 *    mask and the depth map (PriorUtils._data_at_kps, image/mixins/priorutils.py:49-62: grid_sample, zero padding,
 *    align_corners=True, keypoints scaled by camera.sx / sy), the camera-frame depth of the point
 *    (points3D_utils.py:9-25), the masks and the loss weights.
 *    flags bit 0: valid_at_kps (sample == 1), bit 1: depth > 0, bit 2: 1/f < depth/depth3d < f,
 *          bit 3: |log d.clip - log z.clip| / sqrt(var) < 3 (gross_outliers test, :145-147)
 *    magnitude = d^2 / clip(var, 1e-6) (:161), param = multiplier * sqrt(var) / d (:160),
 *    whitened  = (log d - log z) / clip(sqrt(var) / d, 1e-6) (:323-329). ------------------------------------- */
typedef struct mpsfm_depth_gather {
  int32_t n_images;
  const int32_t* map_h; const int32_t* map_w;    /* [n_images] */
  const double* const* depth_map;                 /* [n_images] -> H*W, depth.data ("update") or depth.data_prior */
  const uint8_t* const* valid_map;                /* [n_images] -> H*W, depth.valid */
  const double* sx; const double* sy;             /* [n_images] camera.sx, camera.sy */
  const double* cam_quat_xyzw; const double* cam_t; /* [n_images][4], [n_images][3] */
  int64_t n_obs;                                  /* keypoints with a 3-D point, all images */
  const int32_t* obs_img;                         /* [n_obs] image index */
  const double* obs_xy;                           /* [n_obs][2] keypoint, original image scale */
  const double* obs_var;                          /* [n_obs] depth.uncertainty_update[point2D_idx] */
  const int32_t* obs_pt;                          /* [n_obs] index into pts */
  int32_t n_pts;
  const double* pts;                              /* [n_pts][3] */
  int32_t scale_filter; double scale_filter_factor; int32_t gross_outliers;
  double multiplier;                              /* param_multiplier * truncation_multiplier * rob_std (:109,159) */
} mpsfm_depth_gather;

int mpsfm_depth_blocks(const mpsfm_depth_gather* g, int32_t device, uint8_t* flags /* [n_obs] */, double* depth,
                       double* depth3d, double* magnitude, double* param, double* whitened /* each [n_obs] */);

/* -- row f3, the other half: the per-image prior scale fit of Optimizer.__build_shiftscale_problem
 *    (mpsfm/sfm/mapper/bundle_adjustment.py:187-242) and the robust sigma of update_truncation_multiplier (:295-333,
 *    fit_robust_gaussian_mad :10-15) over the same descriptor, with exact medians selected on the device: one host wait
 *    and O(n_images) results per call.  obs_img must not decrease (MPSFM_EINVAL otherwise): an image's observations
 *    are a range.  d, v = bilinear samples of the depth and the validity map, z = camera-frame depth, all formed as
 *    mpsfm_depth_blocks forms them.  PINHOLE only; one map set per call; the maps are uploaded by every call.
 *    what & FIT, per image i with img_mode[i] = 1 (0: the image is skipped, the reference's `continue`):
 *      base selection v == 1 (n_valid counts it); img_filter[i] = 1 keeps 1/f < d / z < f (f = g->scale_filter_factor),
 *      2 keeps 1/1.5 < map_scale[i] / (z / max(d, 1e-6) * im_scale[i]) < 1.5; r = max(z / d, 1e-6), a NaN stays a NaN.
 *      fit_counts[i] = n_valid, n_sel, n_nan (NaNs among the selected r); fit_ratio[i] = the order statistics of rank
 *      (m - 1) / 2 and m / 2 among the m = n_sel - n_nan ranked r (NaN when m = 0): np.median(np.log(r)) is
 *      0.5 (log lo + log hi), NaN when n_nan > 0; fit_flags[i]: EMPTY = n_sel is 0, EMPTY_METRIC = also filter 2.
 *    what & SIGMA, over all observations of the call: selection v == 1 and d > 0,
 *      w = (log d - log z) / max(sqrt(var) / d, 1e-6); sigma_counts = n_sel, n_nan; sigma_stats = mu (mean of the two
 *      middle order statistics of the ranked w), mad (the same of |w - mu|; NaN when one of them is a NaN); both NaN
 *      when nothing is ranked.  sigma = 1.4826 mad, NaN when n_nan > 0.
 *    ratio, whitened [n_obs] and selected [n_obs] (bit 0: v == 1 of a fitted image, bit 1: selected for FIT, bit 2:
 *    selected for SIGMA) are optional (NULL: not written).  n_obs = 0: 0, with empty results.  Integer atomics only:
 *    every output is the same bit pattern whatever the scheduling. ------------------------------------------------- */
#define MPSFM_DEPTH_STATS_FIT 1
#define MPSFM_DEPTH_STATS_SIGMA 2
#define MPSFM_DEPTH_STATS_EMPTY 1u
#define MPSFM_DEPTH_STATS_EMPTY_METRIC 2u
int mpsfm_depth_stats(const mpsfm_depth_gather* g, int32_t what, const uint8_t* img_mode /* [n_images] */,
                      const uint8_t* img_filter /* [n_images] */, const double* im_scale /* [n_images] */,
                      const double* map_scale /* [n_images] */, int32_t device, int64_t* fit_counts /* [n_images][3] */,
                      double* fit_ratio /* [n_images][2] */, uint32_t* fit_flags /* [n_images] */, int64_t* sigma_counts /* [2] */,
                      double* sigma_stats /* [2] */, double* ratio, double* whitened, uint8_t* selected);

/* -- depth-from-normals integration: replaces the per-image solve of Image.integrate()
 *    (mpsfm/sfm/scene/image/integration.py:133-137 -> _integrate :383-520): IRLS over a 5-point SPD
 *    system on the H*W log-depths with Jacobi-preconditioned CG (scipy/cupy `cg` semantics), bilateral
 *    weights sigmoid(k ((A2 z)^2 - (A1 z)^2)), depth-prior and sparse-depth terms.  Maps are row-major
 *    [H][W]; `normals` is [H][W][3] in the reference's channel order (nx = ch 1, ny = ch 0, nz = -ch 2,
 *    :273-275); `normals_var` holds the diagonal (00, 11, 22) of the per-pixel normal covariance. ---- */
#define MPSFM_INT_MAX_IRLS 16
typedef struct mpsfm_int_problem {
  int32_t H, W;
  const double* depth_prior;        /* depth.data_prior                                   */
  const double* depth_uncertainty;  /* depth.uncertainty (variance)                       */
  const uint8_t* valid;             /* depth.valid                                        */
  const double* normals;            /* normals.data                                       */
  const double* normals_var;        /* diag of normals.uncertainty                        */
  const double* depth_init;         /* depth.data: the map being refined (checkpoint)     */
  double K[4];                      /* (K[1,1] sy, K[0,0] sx, K[1,2] sy, K[0,2] sx), :118-124 */
  int32_t n_sparse;                 /* sparse 3-D points projected into the map (:99-116) */
  const int32_t* sparse_x; const int32_t* sparse_y;
  const double* sparse_depth3d; const double* sparse_zvar;
  /* Image.default_conf (mpsfm/sfm/scene/image/base.py:30-55) */
  double large_number, tol, step_size, cg_tol, lambda1, lambda2, k;
  double depth_magnitude_multiplier, normals_magnitude_multiplier, scale_filter_factor;
  int32_t max_iter, cg_max_iter, scale_filter;
  /* state the reference caches on the image between calls (IntVars, :18-29) */
  int32_t init;                     /* _integrate(init=...)                                */
  int32_t integrated;               /* in                                                  */
  double energy_old;                /* in                                                  */
  double* wu; double* wv;           /* [H*W] in (when init && integrated) / out, may be NULL */
} mpsfm_int_problem;

typedef struct mpsfm_int_summary {
  int32_t changed;                  /* 1: depth_out holds the new map; 0: frame skipped     */
  int32_t irls_iterations, cg_iterations_total, integrated_out;
  double energy_initial, energy_final, energy_old_out;
  int32_t cg_iters[MPSFM_INT_MAX_IRLS];
  double energies[MPSFM_INT_MAX_IRLS + 1];
  float ms;                         /* device time of the solve (HIP events)                */
} mpsfm_int_summary;

int mpsfm_integrate_depth(const mpsfm_int_problem* problem, int32_t device, double* depth_out /* [H*W] */,
                          mpsfm_int_summary* summary);

/* The same solve for a batch of images in ONE sequence of launches (what MpsfmMapper.integrate_bundle loops
 * over, reference mapper/base.py:619-631): kernels run on a (pixels, image) grid, every image keeps its own
 * IRLS / CG state and stops on its own tests, so the results equal those of n single calls (bit for bit while
 * the batch has fewer than 400 000 pixels in total; larger batches use two pixels per thread in the CG
 * kernels, which regroups the partial sums: last-bit differences) while the launch and synchronisation latency
 * is paid once.  All images must share H, W and the configuration
 * scalars (MPSFM_EINVAL otherwise); summaries[i].ms is the device time of the whole batch. */
int mpsfm_integrate_depth_batch(int32_t n_images, const mpsfm_int_problem* problems /* [n] */, int32_t device,
                                double* const* depth_out /* [n] pointers to H*W */, mpsfm_int_summary* summaries /* [n] */);

/* ---- row f4: uncertainty propagation through the integration (reference
 *    mpsfm/sfm/scene/image/integration.py:51-79 `IntegrationUncertainty`, :522-574 `calculate_hessian`,
 *    :576-616 `calculate_int_covs_at_points / _at_kps`).  The "Hessian" is the matrix of calc_Amat built at
 *    the depth checkpoint `depth_init` with weights recomputed from it (init=False) and, when use_sparse==0
 *    (conf.ignore_depths, the default), without the sparse-point term; no scale filter.  The reference solves
 *    H x = e_k per query pixel with cholespy (float32) and returns x.sum(0): the column sum of H^-1, which by
 *    symmetry is (H^-1 1)[k] — computed here by ONE preconditioned-CG solve in float64 to `rtol`.
 *    var_out[i] = value at pixel (qx[i], qy[i]); field_out (may be NULL) receives the whole H*W field.
 *    summary: cg_iters[0] iterations, changed = 1 when the tolerance was met, ms = device time. ---- */
int mpsfm_integration_variances(const mpsfm_int_problem* problem, int32_t device, int32_t use_sparse, int32_t n_query,
                                const int32_t* qx, const int32_t* qy, double rtol, int32_t max_iter,
                                double* var_out /* [n_query] */, double* field_out /* [H*W] or NULL */,
                                mpsfm_int_summary* summary);

/* ---- depth-consistency check of a registered image against its local bundle (reference
 *    mpsfm/sfm/mapper/depthconsistency.py:62-159 check_depth_consistency, :224-246 check_bundle_depth_concistency;
 *    reconstruction/mixins/depth_utils.py:9-48 reproject_depth).  For every pair (a, b) both legs a -> b and b -> a:
 *    every pixel of the source map is unprojected with the map intrinsics and projected into the target map; it is in
 *    canvas when p.x >= 0, p.x + 0.5 < W, p.y >= 0, p.y + 0.5 < H and its depth there is > 0.  The z-buffer keeps the
 *    LAST writer in raster order per target pixel (int(p.y), int(p.x)) (the reference's find_min_buffer compares against
 *    an all-inf buffer).  Test value t = (buffer - depth_target) / sqrt((std_bar c)^2 + (std_target c)^2) with std_bar^2
 *    the (2,2) entry of the source pixel's lifted covariance (unscaled intrinsics, map coordinates, var / psm^2) rotated
 *    by R_t^T R_s ... R_s^T R_t, std_target = sqrt(var_target / psm_target^2).  surface |t| < s, occluded t > s,
 *    invalid t < -s.  counts[p][leg] = {in canvas, surface, occluded, invalid} (leg 0: a -> b, 1: b -> a);
 *    codes[2 p + leg] (may be NULL, as may the array itself) receives one byte per SOURCE pixel, bit 0 in canvas,
 *    bit 1 surface, bit 2 occluded, bit 3 invalid.  Values <= 0 of the depth maps of every image in a pair are set to
 *    0.1 in the caller's arrays, as the reference does in place.  An empty pair list is a no-op. ---- */
typedef struct mpsfm_dc_image {
  int32_t H, W;
  double* depth;                /* [H][W] depth.data (in/out: the <= 0 -> 0.1 clamp is written back) */
  const double* variance;       /* [H][W] depth.uncertainty                                          */
  double prior_std_multiplier;  /* depth.conf.prior_std_multiplier                                   */
  double intr_scaled[4];        /* fx sx, fy sy, cx sx, cy sy: PINHOLE of the map                    */
  double intr[4];               /* fx fy cx cy of the camera (lifted covariance)                     */
  double cam_from_world[12];    /* [3][4] row-major                                                  */
} mpsfm_dc_image;

typedef struct mpsfm_dc_summary {
  float ms;          /* device time of the launches (HIP events), transfers excluded */
  int32_t n_legs;
  int64_t n_pixels;  /* source pixels over all legs */
} mpsfm_dc_summary;

int mpsfm_depth_consistency(int32_t n_images, mpsfm_dc_image* images /* [n_images] */, int32_t n_pairs,
                            const int32_t* pair_a, const int32_t* pair_b /* [n_pairs] */, double c, double score_thresh,
                            int32_t device, int64_t* counts /* [n_pairs][2][4] */,
                            uint8_t* const* codes /* [2 n_pairs] pointers to Hs*Ws, or NULL */,
                            mpsfm_dc_summary* summary /* may be NULL */);

/* ---- options of the LO-RANSAC estimators below (their defaults differ: see each typedef) ---- */
typedef struct mpsfm_ransac_options {
  double max_error;                  /* pixels (mpsfm_align3d_estimate: the units of tgt) */
  double min_inlier_ratio;
  double confidence;
  double dyn_num_trials_multiplier;
  int64_t min_num_trials;
  int64_t max_num_trials;
  uint64_t seed;                     /* sampler seed (see mpsfm_abs_pose_estimate) */
  int32_t batch_trials;              /* trials per generated / scored batch; 0: default */
  int32_t reserved;
} mpsfm_ransac_options;
#ifdef __cplusplus
static_assert(sizeof(mpsfm_ransac_options) == 64 && offsetof(mpsfm_ransac_options, seed) == 48 &&
                  offsetof(mpsfm_ransac_options, batch_trials) == 56,
              "ABI of mpsfm_abs_pose_options / mpsfm_rel_pose_options");
#endif

/* ---- absolute pose: LO-RANSAC with P3P samples and EPnP local optimisation on one 2D-3D problem (reference
 *    mpsfm/sfm/estimators/absolute_pose.py:6-25 -> pycolmap.estimate_and_refine_absolute_pose, estimation half;
 *    call sites mpsfm/sfm/mapper/registration.py:169, :232, :263, base.py:329-336).  COLMAP 3.11
 *    EstimateAbsolutePose (LORANSAC<P3PEstimator, EPNPEstimator, InlierSupportMeasurer>) restated from the upstream
 *    sources as recalled; the reference's COLMAP fork is not in its tree: parity unpinned.
 *    Points go through CamFromImg ((x - cx) / fx, (y - cy) / fy); the threshold is max_error / ((fx + fy) / 2).  Residual:
 *    squared reprojection error in the normalised plane, DBL_MAX at camera depth <= DBL_EPSILON; inlier: residual <=
 *    threshold^2.  Support: more inliers, then the smaller inlier residual sum.  max_num_trials is first capped by
 *    ComputeNumTrials(floor(min_inlier_ratio 1e5), 1e5, confidence, multiplier); after each new best model the dynamic
 *    bound is ComputeNumTrials(best inliers, N, ...) = ceil(log(1 - confidence) / log(1 - (k / N)^3) multiplier).  A sample
 *    model that becomes the best with >= 4 inliers starts up to 10 EPnP rounds on the current inlier set, continued while the
 *    inlier count grows.  P3P: Grunert's quartic, roots with |imag| <= 1e-10, negative lengths rejected, pose by Horn's
 *    closed-form absolute orientation; a sample whose three world points are collinear (sin^2 of the angle at the first
 *    point <= 1e-20) gives no model (upstream would return an arbitrary rotation about the line).
 *    SAMPLER (deliberate deviation from COLMAP's RandomSampler): counter-based, trial t draws from (seed, t) alone.  With
 *    mix(z) = z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB, z ^= z >> 31 (splitmix64's
 *    finaliser), PHI = 0x9E3779B97F4A7C15 and all arithmetic mod 2^64:
 *        base = mix(seed + (t + 1) PHI);  draw j = 1, 2, ...: r_j = mix(base + j PHI), index = floor(r_j N / 2^64)
 *    the first three distinct indices, in draw order, are the sample (a repeated index is drawn again).
 *    Sample models do not depend on the loop state, so trials are generated and scored in batches of batch_trials
 *    (0: default) and the host replays the sequential loop over the scored table; trials past the stop inside the last
 *    batch are wasted work, not a different result.  Scoring sums are fixed-order: results are identical run to run.
 *    inlier_mask[i] = 1 for the inliers of the final model.  N < 3, N > INT32_MAX, NULL pointers, non-finite inputs and
 *    invalid options are MPSFM_EINVAL before any HIP call.  No model: result->success = 0 and return value 0. ---- */
/* defaults of the reference's call: max_error 12.0, min_inlier_ratio 0.25 (pycolmap default 0.1), confidence 0.99999,
 * dyn_num_trials_multiplier 3.0, min_num_trials 100, max_num_trials 10000 */
typedef mpsfm_ransac_options mpsfm_abs_pose_options;

typedef struct mpsfm_abs_pose_result {
  double cam_from_world[12];  /* [3][4] row-major, the RANSAC model (sample or local) */
  int64_t num_inliers;
  int64_t num_trials;         /* LORANSAC's report.num_trials */
  int64_t max_num_trials;     /* after the min_inlier_ratio cap */
  int64_t num_models;         /* P3P models scored (all batches, wasted ones included) */
  int32_t success;
  int32_t lo_rounds;          /* EPnP local estimates run */
  int32_t num_batches;
  float ms;                   /* device time of the launches (HIP events), transfers and host work excluded */
} mpsfm_abs_pose_result;

int mpsfm_abs_pose_estimate(int64_t n, const double* points2D /* [n][2] pixels */, const double* points3D /* [n][3] */,
                            const double* intr /* PINHOLE fx fy cx cy */, const mpsfm_abs_pose_options* options,
                            int32_t device, uint8_t* inlier_mask /* [n] */, mpsfm_abs_pose_result* result);

/* ---- relative pose: LO-RANSAC with five-point samples and five-point local optimisation on one two-view problem, then the
 *    pose of the best essential matrix (reference mpsfm/sfm/estimators/relative_pose.py:7-17 ->
 *    pycolmap.essential_matrix_estimation; call sites mpsfm/sfm/mapper/registration.py:247-248, base.py:259-260).  COLMAP 3.11
 *    EstimateEssentialMatrix (LORANSAC<EssentialMatrixFivePointEstimator x2, InlierSupportMeasurer>) and
 *    PoseFromEssentialMatrix restated as recalled; parity with the reference's COLMAP fork unpinned.
 *    Points go through CamFromImg of their camera; the threshold is 0.5 (max_error / f1 + max_error / f2) with f = (fx + fy) / 2.
 *    Residual: squared Sampson error of x2^T E x1 in normalised coordinates; inlier: residual <= threshold^2.  Support,
 *    min_inlier_ratio cap, dynamic bound and stop test as in mpsfm_abs_pose_estimate with sample size 5 (exponent 5).  A
 *    sample model that becomes the best with more than 5 inliers starts up to 10 rounds of the non-minimal five-point
 *    estimator on the current inlier set, continued while the inlier count grows.
 *    Five-point solver: the 4-D nullspace of Q (minimal: Householder QR of the 5 x 9 Q; non-minimal: the eigenvectors of the
 *    4 smallest eigenvalues of Q^T Q, reduced on the device in a fixed order, where upstream takes an SVD of Q), the 10 x 20
 *    cubic constraints, Gauss-Jordan, the degree-10 determinant of B(z), real roots (|imag| <= 1e-10 (1 + |z|)), three
 *    Gauss-Newton steps of each root on the ten constraints.  A sample whose Q has rank < 5 gives no model.  Each E is
 *    scaled to unit Frobenius norm with its largest-magnitude entry positive (the first in row-major order on ties), and the
 *    models of a trial are ordered lexicographically by their row-major entries: choices of ours that make the result
 *    independent of the nullspace basis and the root-finding route.
 *    Sampler: the counter recipe of mpsfm_abs_pose_estimate, the first FIVE distinct indices.
 *    Pose: E = U diag(s) V^T with det U = det V = +1 (third columns flipped), t = U[:, 2] with its largest-magnitude
 *    component positive (ours: fixes the candidate order), R1 = U W V^T, R2 = U W^T V^T, W = [[0,1,0],[-1,0,0],[0,0,1]];
 *    candidates (R1, t), (R2, t), (R1, -t), (R2, -t); every inlier triangulated by two-view DLT, counted when both depths
 *    (third coordinate in each camera) lie in (DBL_EPSILON, 1000 |t|); the most points win, the later candidate on a tie.
 *    inlier_mask = RANSAC's mask of the best E.  Argument checks as mpsfm_abs_pose_estimate (N < 5 ...), before any HIP call.
 *    No model: result->success = 0 and return value 0. ---- */
/* defaults (pycolmap RANSACOptions): max_error 4.0, min_inlier_ratio 0.01, confidence 0.9999,
 * dyn_num_trials_multiplier 3.0, min_num_trials 1000, max_num_trials 100000 */
typedef mpsfm_ransac_options mpsfm_rel_pose_options;

typedef struct mpsfm_rel_pose_result {
  double E[9];                   /* row-major, canonical form */
  double cam2_from_cam1[12];     /* [3][4] row-major, |t| = 1 */
  int64_t num_inliers;
  int64_t num_trials;            /* LORANSAC's report.num_trials */
  int64_t max_num_trials;        /* after the min_inlier_ratio cap */
  int64_t num_models;            /* model slots scored (all batches, 10 per trial) */
  int64_t lo_rounds;             /* local estimates run */
  int64_t num_batches;
  int64_t num_cheirality_points; /* inliers in front of both cameras for the chosen pose */
  int32_t success;
  float ms;                      /* device time of the launches (HIP events), transfers and host work excluded */
} mpsfm_rel_pose_result;

int mpsfm_rel_pose_estimate(int64_t n, const double* points1 /* [n][2] pixels */, const double* points2 /* [n][2] pixels */,
                            const double* intr1, const double* intr2 /* PINHOLE fx fy cx cy */, const mpsfm_rel_pose_options* options,
                            int32_t device, uint8_t* inlier_mask /* [n] */, mpsfm_rel_pose_result* result);

/* ---- two-view geometry: geometric verification of ONE image pair (reference
 *    mpsfm/sfm/scene/correspondences/utils.py:13-32 -> pycolmap.estimate_calibrated_two_view_geometry).  COLMAP 3.11
 *    EstimateCalibratedTwoViewGeometry, DetectWatermark and EstimateTwoViewGeometryPose restated as recalled; the
 *    reference's COLMAP fork is not in its tree: parity unpinned.  Stateless, one call per pair (many pairs per call:
 *    mpsfm_two_view_geometry_batch below); EstimateMultiple / multiple_models / force_H_use and cameras other than PINHOLE are not provided.
 *    Three LO-RANSACs run over the same n matches with the same options and the same seed (the counter sampler of
 *    mpsfm_abs_pose_estimate, the first 5 / 7 / 4 distinct indices); support measure, min_inlier_ratio cap, dynamic bound
 *    and stop test as there, with the sample size as exponent:
 *      E  exactly mpsfm_rel_pose_estimate's estimator: normalised points, threshold 0.5 (max_error / f1 + max_error / f2).
 *      F  LORANSAC<FundamentalMatrixSevenPointEstimator, FundamentalMatrixEightPointEstimator> on pixels, threshold
 *         max_error, residual = squared Sampson error.  Seven-point: no normalisation, the 2-D nullspace F1, F2 of the 7 x 9
 *         epipolar matrix (Householder QR), the cubic det(l F1 + (1 - l) F2) = 0, real roots under the |imag| rule of the
 *         five-point solver, up to three models; a sample of rank < 7 gives no model.  Local optimisation from 8 inliers:
 *         eight-point with Hartley normalisation (centroid, RMS distance sqrt(2)), rank 2 enforced, T2^T F T1.
 *      H  LORANSAC<HomographyMatrixEstimator x2> on pixels, threshold max_error, residual = squared forward transfer
 *         error |x2 - pi(H x1)|^2 (DBL_MAX when the third coordinate is 0).  Normalised DLT (two rows per match), sample
 *         size 4, local optimisation from 5 inliers; a sample with three collinear points (sin of the angle <= 1e-10) in
 *         either image or of rank < 8 gives no model.
 *    Choices of ours, as for E: every F and H has unit Frobenius norm with its largest-magnitude entry positive (first in
 *    row-major order on ties), a trial's models are ordered lexicographically.  Deviation: the non-minimal estimators take
 *    the eigenvector of the smallest eigenvalue of the 9 x 9 Gram matrix of the normalised design matrix, reduced on the
 *    device in a fixed order, where upstream takes an SVD of the design matrix.
 *    Decision, with nE, nF, nH the inlier counts of the three reports:
 *      1. no leg has a model, or nE, nF, nH are all < min_num_inliers                        DEGENERATE
 *      2. else E has a model, nE / nF > min_E_F_inlier_ratio and nE >= min_num_inliers:      mask of the larger of E and F
 *         (E on equality); nH / nE > max_H_inlier_ratio: PLANAR_OR_PANORAMIC and H's mask if nH is strictly larger;
 *         otherwise CALIBRATED
 *      3. else F has a model and nF >= min_num_inliers: F's mask; nH / nF > max_H_inlier_ratio: PLANAR_OR_PANORAMIC with
 *         the same replacement rule; otherwise UNCALIBRATED
 *      4. else H has a model and nH >= min_num_inliers: H's mask, PLANAR_OR_PANORAMIC
 *      5. else DEGENERATE.  Ratios follow IEEE double division.
 *    n < min_num_inliers: DEGENERATE, an empty mask, return value 0.  MULTIPLE is never produced.
 *    Watermark (detect_watermark, before the pose): with b = watermark_border_size x the image diagonal, the chosen inliers
 *    whose points lie outside [b, w - b] x [b, h - b] in BOTH images; if their share of the chosen inliers is >=
 *    watermark_min_inlier_ratio, a LO-RANSAC for a 2-D translation runs over them (sample size 1, model mean(x2 - x1),
 *    residual |x2 - x1 - t|^2, threshold max_error, min_inlier_ratio = watermark_min_inlier_ratio); its inliers / the chosen
 *    inliers >= watermark_min_inlier_ratio: WATERMARK.
 *    Pose (compute_relative_pose): CALIBRATED: PoseFromEssentialMatrix of the E leg's model on the CHOSEN inliers;
 *    UNCALIBRATED: the same with E = K2^T F K1 (canonical form); decomposition, candidate order and cheirality rule of
 *    mpsfm_rel_pose_estimate.  PLANAR_OR_PANORAMIC: Hn = K2^-1 H K1 divided by its middle singular value, sign such that
 *    det > 0; max |Hn^T Hn - I| < 1e-3: the single candidate (R = Hn, t = 0); otherwise the four (R, t) of Hn = R + t n^T.
 *    OUR candidate order: the two rotations Ra, Rb with Ra's row-major entries lexicographically smaller, ta and tb signed so
 *    that their largest-magnitude component is positive: (Ra, ta), (Rb, tb), (Ra, -ta), (Rb, -tb).  Most cheirality points
 *    (depths in (DBL_EPSILON, 1000 |t|)) win, the later candidate on a tie; then PANORAMIC if t == 0 else PLANAR.
 *    tri_angle: the median (mean of the two middle values for an even count, 0 without points) of
 *    CalculateTriangulationAngle (the geometric angle, not the reference's Python helper) over the winner's cheirality
 *    points, projection centres 0 and -R^T t.  Other configs: identity pose, tri_angle 0.
 *    E, F, H: the best model of each leg that has one (zeros otherwise), whatever the config.
 *    Argument checks (NULL, n < 0 or > INT32_MAX, non-finite points, intrinsics as above, sizes <= 0, invalid options)
 *    are MPSFM_EINVAL before any HIP call.  Results are bitwise identical run to run and for every batch_trials. ---- */
enum {
  MPSFM_TVG_UNDEFINED = 0, MPSFM_TVG_DEGENERATE = 1, MPSFM_TVG_CALIBRATED = 2, MPSFM_TVG_UNCALIBRATED = 3, MPSFM_TVG_PLANAR = 4,
  MPSFM_TVG_PANORAMIC = 5, MPSFM_TVG_PLANAR_OR_PANORAMIC = 6, MPSFM_TVG_WATERMARK = 7, MPSFM_TVG_MULTIPLE = 8
};
enum { MPSFM_TVG_LEG_E = 0, MPSFM_TVG_LEG_F = 1, MPSFM_TVG_LEG_H = 2, MPSFM_TVG_LEG_T = 3 /* watermark translation */ };

typedef struct mpsfm_two_view_options {
  mpsfm_ransac_options ransac;        /* of all legs */
  int64_t min_num_inliers;
  double min_E_F_inlier_ratio;
  double max_H_inlier_ratio;
  double watermark_min_inlier_ratio;
  double watermark_border_size;       /* fraction of the image diagonal */
  int32_t detect_watermark;           /* 0 / 1 */
  int32_t compute_relative_pose;      /* 0 / 1 */
} mpsfm_two_view_options;

typedef struct mpsfm_two_view_leg {
  int64_t num_inliers;     /* of the leg's best model */
  int64_t num_trials;      /* LORANSAC's report.num_trials */
  int64_t max_num_trials;  /* after the min_inlier_ratio cap */
  int64_t lo_rounds;
  int64_t num_batches;
  int32_t success;         /* the leg has a model */
  int32_t reserved;
} mpsfm_two_view_leg;

typedef struct mpsfm_two_view_result {
  double E[9], F[9], H[9];        /* row-major, canonical form */
  double cam2_from_cam1[12];      /* [3][4] row-major */
  double tri_angle;               /* radians */
  mpsfm_two_view_leg leg[4];      /* MPSFM_TVG_LEG_* */
  int64_t num_inliers;            /* of inlier_mask */
  int64_t num_cheirality_points;  /* of the chosen pose */
  int64_t num_border_inliers;     /* watermark test */
  int32_t config;                 /* MPSFM_TVG_* */
  int32_t success;                /* config is neither UNDEFINED nor DEGENERATE */
  int32_t watermark;              /* the watermark test fired */
  float ms;                       /* device time of the launches (HIP events), transfers and host work excluded */
} mpsfm_two_view_result;
#ifdef __cplusplus
static_assert(sizeof(mpsfm_two_view_options) == 112 && offsetof(mpsfm_two_view_options, min_num_inliers) == 64 &&
                  offsetof(mpsfm_two_view_options, detect_watermark) == 104,
              "ABI of mpsfm_two_view_options");
static_assert(sizeof(mpsfm_two_view_leg) == 48, "ABI of mpsfm_two_view_leg");
static_assert(sizeof(mpsfm_two_view_result) == 552 && offsetof(mpsfm_two_view_result, tri_angle) == 312 &&
                  offsetof(mpsfm_two_view_result, leg) == 320 && offsetof(mpsfm_two_view_result, config) == 536,
              "ABI of mpsfm_two_view_result");
#endif

/* COLMAP 3.11 TwoViewGeometryOptions as recalled: ransac max_error 4, min_inlier_ratio 0.25, confidence 0.999, multiplier 3,
 * min_num_trials 100, max_num_trials 10000; min_num_inliers 15, min_E_F_inlier_ratio 0.95, max_H_inlier_ratio 0.8,
 * watermark_min_inlier_ratio 0.7, watermark_border_size 0.1, detect_watermark 1, compute_relative_pose 0 */
void mpsfm_two_view_default_options(mpsfm_two_view_options* options);

int mpsfm_two_view_geometry(int64_t n, const double* points1 /* [n][2] pixels */, const double* points2 /* [n][2] pixels */,
                            const double* intr1, const double* intr2 /* PINHOLE fx fy cx cy */,
                            const int32_t* size1, const int32_t* size2 /* width, height */,
                            const mpsfm_two_view_options* options, int32_t device, uint8_t* inlier_mask /* [n] */,
                            mpsfm_two_view_result* result);

/* ---- two-view geometry of MANY image pairs in one call (reference mpsfm/sfm/scene/correspondences/utils.py:51-77, the pool
 *    over all matched pairs).  Pair k owns the matches [pair_start[k], pair_start[k + 1]) of points1 / points2 and of
 *    inlier_mask, row k of intr1 / intr2 / size1 / size2 and results[k]; one set of options serves all pairs, as the reference
 *    passes it.  results[k] and pair k's slice of inlier_mask are IDENTICAL (every field but ms, bitwise) to what
 *    mpsfm_two_view_geometry returns for that pair alone with the same options, whatever the other pairs, their order and
 *    pairs_per_group: every problem sees the operations of its single call in the same order.
 *    Pairs are processed in groups of consecutive pairs; within a group every leg type (E, F, H, then the watermark
 *    translation) runs as one lockstep LO-RANSAC over the group's pairs: one launch generates, one scores the next batch of
 *    every pair, one synchronisation serves them all.  pairs_per_group 0: consecutive pairs while the group's device tables
 *    stay under 256 MiB, at most 256 pairs; an explicit value is used as given up to 4096.
 *    results[k].ms is the device time of the whole group pair k ran in (all pairs of a group share it); a pair with
 *    n < min_num_inliers or n < 4 is DEGENERATE as in the single call, takes part in no launch and reports ms 0.
 *    Checks, all MPSFM_EINVAL before any HIP call, the message naming the pair: NULL pointers (report may be NULL),
 *    num_pairs < 0, pair_start[0] != 0, a decreasing offset, a pair of more than INT32_MAX matches, non-finite points,
 *    intrinsics / sizes the single call refuses, invalid options, pairs_per_group < 0.  num_pairs == 0: returns 0 and touches
 *    nothing. ---- */
typedef struct mpsfm_two_view_batch_report {
  int64_t num_groups;
  int64_t num_syncs;     /* stream synchronisations of the call */
  int64_t num_launches;  /* kernel launches of the call */
  float ms;              /* device time of all launches (sum over the groups) */
  int32_t reserved;
} mpsfm_two_view_batch_report;
#ifdef __cplusplus
static_assert(sizeof(mpsfm_two_view_batch_report) == 32 && offsetof(mpsfm_two_view_batch_report, num_syncs) == 8 &&
                  offsetof(mpsfm_two_view_batch_report, num_launches) == 16 && offsetof(mpsfm_two_view_batch_report, ms) == 24,
              "ABI of mpsfm_two_view_batch_report");
#endif

int mpsfm_two_view_geometry_batch(int64_t num_pairs, const int64_t* pair_start /* [num_pairs + 1], pair_start[0] == 0 */,
                                  const double* points1 /* [N][2] */, const double* points2 /* [N][2], N = pair_start[num_pairs] */,
                                  const double* intr1, const double* intr2 /* [num_pairs][4] */,
                                  const int32_t* size1, const int32_t* size2 /* [num_pairs][2] */,
                                  const mpsfm_two_view_options* options, int32_t pairs_per_group /* 0: default */, int32_t device,
                                  uint8_t* inlier_mask /* [N] */, mpsfm_two_view_result* results /* [num_pairs] */,
                                  mpsfm_two_view_batch_report* report /* may be NULL */);

/* ---- registration: the per-match arithmetic of MpsfmRegistration (reference mpsfm/sfm/mapper/registration.py).
 *
 *    mpsfm_registration_pairs: the 2D-3D pairs of one register_next_image for ALL reference images in one launch
 *    (:68-94 _find_2D3D_pairs, :341-373 _collect_pairs, :375-382 _lift_points_to_3d).  Per match i with reference image
 *    r = match_ref[i], reference keypoint ref_xy[i] and point index p = match_pt[i] (-1: the keypoint has no 3-D point):
 *      p >= 0 and not pt_risky[p]      xyz = pts[p]                                              kind TRIANGULATED
 *      else, lifted_registration != 0  d = bilinear sample of refs[r].depth_map at ref_xy[i] (PriorUtils._data_at_kps:
 *                                      grid_sample, bilinear, zero padding, align_corners=True, keypoint scaled by sx, sy;
 *                                      no validity and no d > 0 test, as the reference),
 *                                      xyz = R_r^T ([(x - cx) / fx, (y - cy) / fy, 1] d - t_r)   kind LIFTED
 *      else                            xyz = 0                                                   kind DROPPED
 *    Every product and sum of the sample and of the lift is rounded on its own (no fused multiply-add): the sample equals
 *    the NumPy restatement bit for bit.
 *
 *    mpsfm_init_pair_candidates: the candidate points of an init pair, image 1 at the identity and image 2 at
 *    cam2_from_cam1 (:38-66 _candidate_points3D_for_init, :384-391 _lift_points_for_init, :419-441
 *    _candidate_lift_for_init).  Per match i that `select` keeps (NULL: all), as `what` asks:
 *      MPSFM_INIT_TRIANGULATE  the two-view EstimateTriangulation (COLMAP 3.11 as recalled: LORANSAC over
 *                              TriangulationEstimator with the angular residual) with the device functions of
 *                              mpsfm_tri_estimate_batch: ok and xyz equal that entry point's on the same candidate bit for
 *                              bit (xyz = 0 where not ok);
 *      MPSFM_INIT_LIFT         d = bilinear sample of prior_map (depth.data_prior) at xy1, valid <=> the bilinear sample of
 *                              valid_map there == 1 exactly, xyz = [(x - cx) / fx, (y - cy) / fy, 1] (d rescale);
 *      for each candidate      the reference's calculate_triangulation_angle in degrees and has_point_positive_depth
 *                              (depth >= 2^-52) in both cameras.
 *    THE ANGLE IS THE REFERENCE'S, NOT THE GEOMETRIC ONE (mpsfm/utils/geometry.py:54-65 takes norms where its variable
 *    names say squared norms): with b = |C1 - C2|, r1 = |X - C1|, r2 = |X - C2| (plain lengths) it is
 *    a = acos((r1 + r2 - b) / (2 sqrt(r1 r2))), folded as min(a, pi - a), 0 when the denominator is 0, NaN where acos
 *    gives NaN (Python's min(nan, x) is nan).  The reference's thresholds act on this value.
 *    Matches that `select` drops, and the kinds `what` does not ask for, get zeros.
 *
 *    Both: caller owns all buffers, nothing is retained; MPSFM_EINVAL for NULL pointers, negative counts, match_ref or
 *    match_pt out of range and maps smaller than 2 x 2, checked on the host before anything is launched;
 *    MPSFM_ENODEVICE without a device.  *ms (may be NULL): device time of the launch (HIP events), transfers excluded. ---- */
enum { MPSFM_REG_DROPPED = 0, MPSFM_REG_TRIANGULATED = 1, MPSFM_REG_LIFTED = 2 };

typedef struct mpsfm_reg_image {
  int32_t map_h, map_w;
  const double* depth_map;  /* depth.data, [map_h][map_w] */
  double sx, sy;            /* camera.sx, camera.sy: keypoint -> map coordinates */
  double intr[4];           /* PINHOLE fx fy cx cy */
  double quat_xyzw[4];      /* cam_from_world rotation */
  double t[3];              /* cam_from_world translation */
} mpsfm_reg_image;

int mpsfm_registration_pairs(int32_t n_refs, const mpsfm_reg_image* refs /* [n_refs] */, int64_t n_matches,
                             const int32_t* match_ref /* [n] index into refs */, const double* ref_xy /* [n][2] */,
                             const int32_t* match_pt /* [n] index into pts or -1 */,
                             const uint8_t* pt_risky /* [n_pts] or NULL: none */, int32_t n_pts, const double* pts /* [n_pts][3] */,
                             int32_t lifted_registration, int32_t device, double* xyz /* [n][3] */,
                             uint8_t* kind /* [n] MPSFM_REG_* */, float* ms /* may be NULL */);

enum { MPSFM_INIT_TRIANGULATE = 1, MPSFM_INIT_LIFT = 2 };
/* bits of mpsfm_init_candidates.flags */
enum {
  MPSFM_INIT_TRI_OK = 1, MPSFM_INIT_TRI_POSDEPTH1 = 2, MPSFM_INIT_TRI_POSDEPTH2 = 4,
  MPSFM_INIT_VALID = 8, MPSFM_INIT_LIFT_POSDEPTH1 = 16, MPSFM_INIT_LIFT_POSDEPTH2 = 32
};

typedef struct mpsfm_init_pair {
  int64_t n_matches;
  const double* xy1;          /* [n][2] keypoints of image 1 */
  const double* xy2;          /* [n][2] keypoints of image 2 */
  const uint8_t* select;      /* [n] or NULL: 0 = skip this match */
  double intr1[4], intr2[4];  /* PINHOLE fx fy cx cy */
  double cam2_from_cam1[12];  /* [3][4] row-major */
  int32_t map_h, map_w;
  const double* prior_map;    /* depth.data_prior of image 1, [map_h][map_w] (MPSFM_INIT_LIFT) */
  const uint8_t* valid_map;   /* depth.valid of image 1 as 0 / 1 bytes (MPSFM_INIT_LIFT) */
  double sx, sy;              /* camera1.sx, camera1.sy */
  double rescale;             /* factor on the sampled prior depth (1: none) */
  double tri_min_angle;       /* radians; EstimateTriangulationOptions default 0 */
  double tri_max_error;       /* radians; default 2 degrees */
  int32_t what;               /* MPSFM_INIT_TRIANGULATE | MPSFM_INIT_LIFT */
  int32_t reserved;
} mpsfm_init_pair;

typedef struct mpsfm_init_candidates {
  uint8_t* flags;          /* [n] MPSFM_INIT_* bits */
  double* tri_xyz;         /* [n][3] */
  double* tri_angle_deg;   /* [n]    */
  double* lift_xyz;        /* [n][3] */
  double* lift_angle_deg;  /* [n]    */
  double* d_prior;         /* [n] the sampled prior depth, before rescale */
  float ms;                /* out: device time of the launch */
} mpsfm_init_candidates;

int mpsfm_init_pair_candidates(const mpsfm_init_pair* pair, int32_t device, mpsfm_init_candidates* out);

/* ---- thinning a dense matcher's output: the fixed-radius neighbour geometry of the reference's
 *    mpsfm/extraction/pairwise (models/utils/generic.py sparse_nms, models/utils/warp.py assign_keypoints,
 *    match_dense_2view.py:127-161), which the reference does with a SciPy KD-tree on the host.  All distance arithmetic is
 *    fp64 dx*dx + dy*dy with every operation rounded on its own; the comparisons below are exact.
 *
 *    mpsfm_radius_nms: greedy radius suppression.  The points are visited in priority order; a visited point that is still
 *    alive is kept and suppresses every point at squared distance <= radius*radius.  Priority is `order` when given (a
 *    permutation of 0 .. n-1, highest priority first), else score descending with ties going to the LOWER INDEX (-0.0
 *    counts as +0.0).  The reference's own order among equal scores is whatever its unstable torch.argsort gives; `order`
 *    lets a caller impose one.  keep[i] = 1 for kept points; the result does not depend on how the device schedules the
 *    work.
 *
 *    mpsfm_thin_dense_matches: both passes of the `dense` leg for one pair in one call, the survivors never leaving the
 *    device.  Pass 1 is the suppression over [sparse0; dense0] with scores [100 ...; dscores], pass 2 the suppression over
 *    [sparse1; the dense1 of pass 1's survivors] with the same scores; n_sparse == 0 is the dense-only branch.  keep[j] = 1
 *    for the dense matches that survive both.  REFERENCE_SLICE: the reference takes the survivors of a pass as
 *    sparse_nms(comb, ...)[n_sparse:] - n_sparse, which assumes that all n_sparse sparse points survive.  When only
 *    k < n_sparse of them do (matched sparse keypoints closer than the radius), that expression ALSO DROPS THE FIRST
 *    n_sparse - k SURVIVING DENSE MATCHES (in index order).  reference_slice != 0 reproduces this in both passes,
 *    reference_slice == 0 keeps every surviving dense match.  Scores above 100 are not special: such a dense match outranks
 *    the sparse points, as it does in the reference.
 *
 *    mpsfm_assign_keypoints: ids[i] = the keypoint nearest to query[i] among those with squared distance strictly
 *    < max_error*max_error (a query at exactly max_error gets -1, as SciPy's query with distance_upper_bound does), the
 *    lowest index among equidistant nearest ones, -1 when there is none.  Either side empty: all -1, nothing is launched.
 *
 *    All three: caller owns all buffers, nothing is retained; MPSFM_EINVAL for NULL pointers, negative counts or radius,
 *    more than 2^27 points, non-finite coordinates, scores or radius, a bounding box wider than DBL_MAX and an `order` that
 *    is no permutation, checked on the host before any device is touched; an empty call returns 0 without a device;
 *    MPSFM_ENODEVICE without a device. ---- */
typedef struct mpsfm_nms_info {
  int32_t rounds;           /* round launches up to and including the first that left no point undecided */
  int32_t launches;         /* round launches enqueued (rounds go out in groups, the count is read once per group) */
  int32_t cells;            /* occupied grid cells */
  int32_t max_cell_points;  /* the largest cell population */
  float ms;                 /* device time from the first kernel to the last (HIP events), transfers excluded */
  int32_t reserved;
} mpsfm_nms_info;           /* mpsfm_thin_dense_matches: rounds, launches and ms summed over its two passes, cells and
                               max_cell_points the larger of the two */

int mpsfm_radius_nms(int64_t n, const double* points /* [n][2] */, const double* scores /* [n] */,
                     const int64_t* order /* [n] or NULL */, double radius, int32_t device, uint8_t* keep /* [n] */,
                     int64_t* num_kept, mpsfm_nms_info* info /* may be NULL */);

int mpsfm_thin_dense_matches(int64_t n_sparse, const double* sparse0, const double* sparse1 /* [n_sparse][2] */, int64_t n_dense,
                             const double* dense0, const double* dense1 /* [n_dense][2] */, const double* dscores /* [n_dense] */,
                             double radius, int32_t reference_slice, int32_t device, uint8_t* keep /* [n_dense] */,
                             int64_t* num_kept, mpsfm_nms_info* info /* may be NULL */);

int mpsfm_assign_keypoints(int64_t n_query, const double* query /* [n_query][2] */, int64_t n_kps, const double* kps /* [n_kps][2] */,
                           double max_error, int32_t device, int64_t* ids /* [n_query] */, float* ms /* may be NULL */);

/* ---- descriptors to match lists: mutual nearest neighbours without the n0 x n1 similarity matrix
 *    (reference: mpsfm/extraction/pairwise/models/nearest_neighbor.py NearestNeighbor / find_nn / mutual_check and
 *    models/utils/featuremap.py NNs_sparse; the arithmetic contract and the tie rule: DESIGN.md section 4m).
 *
 *    Similarities are fp64 dot products of the fp32 (or, sampled, fp64) descriptor values, accumulated with k ascending on
 *    the matrix pipe; every element goes through the same operation sequence wherever it sits, so identical descriptors give
 *    bitwise identical similarities.  Nearest neighbour of a row: the maximum similarity, EQUAL SIMILARITIES GOING TO THE
 *    LOWEST INDEX; second nearest: the maximum over the remaining columns.  Decisions in fp64, every operation rounded on
 *    its own: dist = 2 (1 - sim); ratio test dist0 <= ratio^2 dist1 (skipped when either side holds a single descriptor);
 *    distance test dist0 <= distance^2; scores0[i] = (sim0 + 1) / 2 where both tests passed, else 0; matches0[i] = the
 *    nearest neighbour where both passed, else -1.  mutual_check: matches0[i] is kept only if the same tests in the other
 *    direction give matches1[matches0[i]] == i; as in the reference scores0 is NOT zeroed for a match only the mutual check
 *    (or the score threshold) removes.  score_threshold: matches with scores0 < score_threshold become -1 (after the mutual
 *    check, as NNs_sparse does).  A threshold <= 0 is off.
 *
 *    mpsfm_match_map_descriptors: the descriptors are bilinear samples (align_corners, zero padding, fp64 with every operation
 *    rounded on its own, the keypoint coordinates rounded to float32 first and taken as pixel coordinates) of channel-last
 *    fp32 maps [H][W][C] at the keypoints; the confidences are sampled the same way.  The samples stay fp64 on the device.
 *    scores0[i] = sqrt(conf0[i] * conf1[matches0[i]]) for matched rows, else 0.
 *
 *    inputs_on_device != 0: desc0 / desc1, or map0 / conf0 / map1 / conf1, are device pointers on `device` (checked).  The
 *    call records an event on `stream` (a hipStream_t: the stream that produced them) and its own stream waits for it;
 *    stream == NULL: the inputs must be complete when the call is made.  The library never works on the null stream.
 *    Keypoints and all outputs are host memory, complete on return; nothing is retained.
 *
 *    MPSFM_EINVAL before any device is touched: NULL pointers, negative counts, dim / C outside 1 .. 1024, more than 2^24
 *    descriptors on a side, H or W < 2, non-finite thresholds, non-finite values in host inputs (device inputs are scanned
 *    by a kernel: MPSFM_EINVAL after it).  Either side empty: matches0 all -1, scores0 all 0, no device needed.
 *    MPSFM_ENODEVICE without a device. ---- */
typedef struct mpsfm_match_options {
  double ratio_threshold;     /* <= 0: off */
  double distance_threshold;  /* <= 0: off */
  double score_threshold;     /* <= 0: off */
  int32_t mutual_check;
  int32_t inputs_on_device;
  void* stream;               /* hipStream_t of the caller, read only with inputs_on_device */
} mpsfm_match_options;

typedef struct mpsfm_match_info {
  int64_t num_matches;  /* rows with matches0 >= 0 */
  float ms;             /* device time from the first kernel to the last (HIP events), transfers excluded */
  int32_t column_ranges; /* workgroups that shared the columns of one strip of rows (results do not depend on it) */
} mpsfm_match_info;

/* the reference's defaults: thresholds off, mutual check on, host inputs */
void mpsfm_match_default_options(mpsfm_match_options* opts);

int mpsfm_match_descriptors(int64_t n0, int64_t n1, int32_t dim, const float* desc0 /* [n0][dim] */, const float* desc1 /* [n1][dim] */,
                            const mpsfm_match_options* opts /* NULL: defaults */, int32_t device, int32_t* matches0 /* [n0] */,
                            double* scores0 /* [n0] */, mpsfm_match_info* info /* may be NULL */);

int mpsfm_match_map_descriptors(const float* map0 /* [H0][W0][C] */, const float* conf0 /* [H0][W0] */, int32_t H0, int32_t W0,
                                const float* map1 /* [H1][W1][C] */, const float* conf1 /* [H1][W1] */, int32_t H1, int32_t W1, int32_t C,
                                int64_t n0, const double* kps0 /* [n0][2] x, y; host */, int64_t n1, const double* kps1 /* [n1][2] */,
                                const mpsfm_match_options* opts /* NULL: defaults */, int32_t device, int32_t* matches0 /* [n0] */,
                                double* scores0 /* [n0] */, mpsfm_match_info* info /* may be NULL */);

/* ---- descriptors to match lists for MANY image pairs in one call (reference mpsfm/extraction/pairwise/match_sparse.py
 *    match_from_paths, the loop over all retrieved pairs of a scene).  The descriptor sets of all images are
 *    given once, concatenated: image i owns the rows [image_start[i], image_start[i + 1]) of desc.  Pair k matches image
 *    pair_image0[k] (rows) against image pair_image1[k] (columns) and owns the rows [match_start[k], match_start[k + 1]) of
 *    matches0 / scores0, as many as its first image has descriptors.  One set of options serves all pairs.
 *
 *    Pair k's slice of matches0 / scores0 is IDENTICAL, matches equal and scores bitwise equal, to what mpsfm_match_descriptors
 *    returns for (image pair_image0[k], image pair_image1[k]) alone with the same options, whatever the other pairs, their
 *    order, the order of the images, column_ranges and pairs_per_group: both calls run the same device code on every element
 *    (csrc/sim_top2.h), and a row's top-2 is a function of the SET of its candidates under one total order.  The ratio test is
 *    skipped per pair when either of ITS sides holds a single descriptor.  (i, i) is allowed, and so is any pair listed twice;
 *    (i, j) and (j, i) are two pairs.  A pair whose first image is empty owns zero rows; a pair whose second image is empty gets
 *    -1 / 0; both take part in no launch, and if no other pair is left no device is touched.
 *
 *    The pairs that are launched are processed in GROUPS of consecutive launched pairs: per group one launch forms the top-2 of every
 *    strip of 64 rows of every pair in both directions from a host-built table of work items, one launch decides every output row.
 *    pairs_per_group 0: consecutive pairs while the group's top-2 tables (24 B per row and column range, both directions) stay
 *    under 256 MiB; an explicit value is used as given up to 4096.  column_ranges 0: per group, every strip's column tiles are
 *    shared out over ceil(8 CUs / (strips of the group, both directions)) workgroups, at most one per column tile, so a batch of
 *    many pairs runs with one workgroup per strip; an explicit value asks for that many per strip, clamped the same way.  Results
 *    depend on neither.  All groups are enqueued back to back on one stream and reuse the same tables in stream order; the
 *    descriptors of all images are uploaded once, matches and scores of the whole batch come down once, and the host waits
 *    ONCE per call (report->num_syncs == 1).  A batch whose descriptors do not fit the device returns MPSFM_ENOMEM: chunking a
 *    scene over images is the caller's business.
 *
 *    opts->inputs_on_device != 0: desc is a device pointer on `device` (checked), the event is recorded on opts->stream as
 *    in the single call, non-finite values are found by a kernel and reported as MPSFM_EINVAL after it.  image_start, the
 *    pair arrays, match_start and all outputs are host memory, complete on return; nothing is retained.
 *
 *    MPSFM_EINVAL before any HIP call, the message naming the image or pair: NULL pointers (opts, pair_num_matches and report
 *    may be NULL), negative counts, image_start[0] != 0 or a decreasing offset, an image of more than 2^24 descriptors, dim
 *    outside 1 .. 1024, a pair index outside [0, num_images), match_start[0] != 0 or a slice whose length is not its first
 *    image's size, negative column_ranges or pairs_per_group, non-finite thresholds, a non-finite host descriptor value.
 *    num_pairs == 0 returns 0 and touches nothing.  MPSFM_ENODEVICE without a device, but only when a pair needs one. ---- */
typedef struct mpsfm_match_batch_report {
  int64_t num_matches;     /* rows with matches0 >= 0, all pairs */
  int64_t num_groups;
  int64_t num_launches;    /* kernel launches of the call */
  int64_t num_syncs;       /* stream synchronisations of the call */
  int64_t num_workgroups;  /* workgroups of all similarity launches */
  float ms;                /* device time, first kernel to last (HIP events) */
  int32_t reserved;
} mpsfm_match_batch_report;
#ifdef __cplusplus
static_assert(sizeof(mpsfm_match_batch_report) == 48 && offsetof(mpsfm_match_batch_report, num_groups) == 8 &&
                  offsetof(mpsfm_match_batch_report, num_launches) == 16 && offsetof(mpsfm_match_batch_report, num_syncs) == 24 &&
                  offsetof(mpsfm_match_batch_report, num_workgroups) == 32 && offsetof(mpsfm_match_batch_report, ms) == 40,
              "ABI of mpsfm_match_batch_report");
#endif

int mpsfm_match_descriptors_batch(int32_t num_images, const int64_t* image_start /* [num_images + 1], image_start[0] == 0 */, int32_t dim,
                                  const float* desc /* [image_start[num_images]][dim]: the images' descriptor sets, concatenated */,
                                  int64_t num_pairs, const int32_t* pair_image0, const int32_t* pair_image1 /* [num_pairs] image indices */,
                                  const int64_t* match_start /* [num_pairs + 1], match_start[0] == 0 */,
                                  const mpsfm_match_options* opts /* NULL: defaults */, int32_t column_ranges /* 0: default rule */,
                                  int32_t pairs_per_group /* 0: default rule */, int32_t device,
                                  int32_t* matches0, double* scores0 /* [match_start[num_pairs]] */,
                                  int64_t* pair_num_matches /* [num_pairs], may be NULL */, mpsfm_match_batch_report* report /* may be NULL */);

/* ---- global descriptors to image pairs: the top num_select db images of every query image without the nq x nd similarity
 *    matrix (reference: mpsfm/extraction/pairs/hloc/pairs_from_retrieval.py, einsum + masked_fill + torch.topk; the contract,
 *    the tie rule, the kernels and the margins: DESIGN.md section 4r).
 *
 *    Similarities are fp64 dot products of the fp32 descriptor values, accumulated with k ascending on the matrix pipe; every
 *    element goes through the same operation sequence wherever it sits, so identical descriptors give bitwise identical
 *    similarities (the contract of mpsfm_match_descriptors).  CANDIDATES of query row i: every db column j but those a test
 *    removes, which are never offered and never occupy a slot:
 *      identity  query_id[i] == db_id[j], when both id arrays are given (the reference's `self` mask; ids stand for names, so a
 *                query may share its id with several db columns or with none);
 *      score     sim < min_score, when use_min_score != 0 (a similarity EQUAL to min_score stays, as with the reference's
 *                `scores < min_score`).
 *    RESULT of row i: the first num_select candidates under the order (similarity descending, index ascending), in that order:
 *    indices[i][0 .. counts[i]) and scores[i][0 .. counts[i]), counts[i] <= num_select, the rest of the row -1 / 0.  The result
 *    is a function of the SET of candidates only: it depends on neither column_ranges nor scheduling, and equal similarities
 *    go to the lowest index (the reference leaves ties to the torch build).
 *
 *    column_ranges 0: every strip's column tiles (64 columns each) are shared out over ceil(8 CUs / strips of 64 rows)
 *    workgroups, at most one per column tile and at most 4096; an explicit value asks for that many per strip, clamped the same
 *    way.  Results do not depend on it.
 *
 *    query == db is allowed and is the common case: the set is scanned and uploaded once.  inputs_on_device / stream: as for
 *    mpsfm_match_options (query and db are device pointers, checked; an event is recorded on `stream` and the call's own stream
 *    waits for it).  Ids, options and all outputs are host memory, complete on return; the host waits ONCE per call
 *    (info->num_syncs == 1); nothing is retained.
 *
 *    MPSFM_EINVAL before any device is touched: NULL pointers (opts NULL: defaults; info may be NULL), negative counts or
 *    column_ranges, dim outside 1 .. 65536, more than 2^24 rows on a side, num_select outside 1 .. 128 or greater than nd when
 *    nd > 0, one id array without the other, a non-finite min_score, a non-finite host value (device inputs are scanned by a
 *    kernel: MPSFM_EINVAL after it).  nq == 0 returns 0; nd == 0 gives all counts 0 (indices -1, scores 0); both without a
 *    device.  MPSFM_ENODEVICE without a device, but only when one is needed.  The lists of all column ranges
 *    (12 B x nq x column_ranges x num_select) live on the device during the call: MPSFM_ENOMEM when they do not fit. ---- */
typedef struct mpsfm_retrieval_options {
  int32_t num_select;        /* entries per query row, 1 .. 128 */
  int32_t use_min_score;     /* != 0: similarities below min_score are no candidates */
  double min_score;
  int32_t column_ranges;     /* 0: default rule */
  int32_t inputs_on_device;
  void* stream;              /* hipStream_t of the caller, read only with inputs_on_device */
} mpsfm_retrieval_options;

typedef struct mpsfm_retrieval_info {
  int64_t num_pairs;      /* listed pairs: the sum of counts */
  int64_t num_launches;   /* kernel launches of the call */
  int64_t num_syncs;      /* stream synchronisations of the call */
  float ms;               /* device time, first kernel to last (HIP events), transfers excluded */
  int32_t column_ranges;  /* workgroups that shared the columns of one strip of rows (results do not depend on it) */
} mpsfm_retrieval_info;
#ifdef __cplusplus
static_assert(sizeof(mpsfm_retrieval_options) == 32 && offsetof(mpsfm_retrieval_options, use_min_score) == 4 &&
                  offsetof(mpsfm_retrieval_options, min_score) == 8 && offsetof(mpsfm_retrieval_options, column_ranges) == 16 &&
                  offsetof(mpsfm_retrieval_options, inputs_on_device) == 20 && offsetof(mpsfm_retrieval_options, stream) == 24,
              "ABI of mpsfm_retrieval_options");
static_assert(sizeof(mpsfm_retrieval_info) == 32 && offsetof(mpsfm_retrieval_info, num_launches) == 8 &&
                  offsetof(mpsfm_retrieval_info, num_syncs) == 16 && offsetof(mpsfm_retrieval_info, ms) == 24 &&
                  offsetof(mpsfm_retrieval_info, column_ranges) == 28,
              "ABI of mpsfm_retrieval_info");
#endif

/* the reference's defaults: num_select 20, score test on at 0, host inputs */
void mpsfm_retrieval_default_options(mpsfm_retrieval_options* opts);

int mpsfm_retrieve_topk(int64_t nq, int64_t nd, int32_t dim, const float* query /* [nq][dim] */, const float* db /* [nd][dim] */,
                        const int32_t* query_id /* [nq] or NULL */, const int32_t* db_id /* [nd] or NULL: both or neither */,
                        const mpsfm_retrieval_options* opts /* NULL: defaults */, int32_t device,
                        int32_t* indices /* [nq][num_select] */, double* scores /* [nq][num_select] */, int32_t* counts /* [nq] */,
                        mpsfm_retrieval_info* info /* may be NULL */);

/* ---- dense reciprocal matches from descriptor maps: the dense leg of the reference's MASt3R matcher
 *    (mpsfm/extraction/pairwise/models/mast3r.py:119-170 merge_corres, extract_correspondences, with MASt3R's
 *    fast_reciprocal_NNs; the contract, the kernels and the measurements: DESIGN.md section 4p).
 *
 *    One search (A [H1][W1][C], B [H2][W2][C], subsample S, max_iter), channel-last float32 maps.  The descent rule is MASt3R's
 *    fast_nn.py (int subsample, pixel_tol 0, ret_basin False, dist "dot"), which is NOT part of the reference tree: the rule
 *    is INFERRED AND FROZEN BY TESTS.  Seeds are the pixels (y, x) with y = S/2, S/2 + S, ... < H1 and x = S/2, ... < W1,
 *    y-major; xy1 = y W1 + x, xy2 = -1, old1 = xy1, old2 = xy2, all seeds active.  While a seed is active:
 *      1. active seeds: xy2 = NN_B(A[xy1])            2. seeds with xy2 == old2 become inactive
 *      3. still active seeds: xy1 = NN_A(B[xy2])      4. seeds with xy1 == old1 become inactive
 *      5. one iteration is counted; at max_iter the loop ends   6. otherwise old1 = xy1, old2 = xy2
 *    The seeds inactive at the end have converged; the result is their (xy1, xy2), unique and sorted by (xy1, xy2) ascending.
 *    NN_X(d): the pixel of X with the largest fp64 dot product with d, accumulated with k ascending on the matrix pipe, every
 *    element through the same operation sequence (section 4m's contract); EQUAL SIMILARITIES GO TO THE LOWEST INDEX.  The
 *    result is a function of the inputs alone: bitwise the same from run to run and from host or device inputs.
 *
 *    mpsfm_recip_seed_count: the number of seeds of an H x W map, 0 for arguments below 1.
 *    mpsfm_reciprocal_nns: one search; idx1 / idx2 [capacity] receive *n_out pairs; capacity >= the seed count of (H1, W1).
 *    mpsfm_dense_correspondences: extract_correspondences.  The searches (feat11 -> feat21), (feat21 -> feat11),
 *    (feat12 -> feat22), (feat22 -> feat12) run in lockstep; per pair of searches idx1 = [fwd.xy1, bwd.xy2],
 *    idx2 = [fwd.xy2, bwd.xy1] with the float32 confidences QA[idx1], QB[idx2], (QA, QB) = (qonf11, qonf21), then
 *    (qonf12, qonf22); the two pairs are concatenated and made unique by (idx1 major, idx2 minor) ascending; a kept row's
 *    score is that of its FIRST occurrence, sqrtf(q1 * q2) in float32 with each operation rounded on its own.
 *    xy1 [n][2] = (idx1 % W1, idx1 / W1), xy2 likewise with W2.  feat11, feat12, qonf11, qonf12 are [H1][W1]([C]), the
 *    others [H2][W2]([C]).  capacity >= 2 (seeds of (H1, W1) + seeds of (H2, W2)).
 *    info of the four searches: counts summed, iterations the largest.
 *
 *    inputs_on_device / stream: as for mpsfm_match_options (maps and confidences are device pointers, checked; an event is
 *    recorded on `stream` and the call's own stream waits for it; the library never works on the null stream).  Outputs are
 *    host memory, complete on return; nothing is retained.
 *
 *    MPSFM_EINVAL before any device is touched: NULL pointers, C outside 1 .. 1024, H or W < 1, more than 2^24 pixels in a
 *    map, subsample < 1, max_iter outside 1 .. 1024, a capacity below the bound above, non-finite values in host inputs
 *    (device inputs are scanned by a kernel: MPSFM_EINVAL after it).  No seed (S/2 >= H or W on every seeded map): *n_out = 0,
 *    no device needed.  MPSFM_ENODEVICE without a device. ---- */
typedef struct mpsfm_recip_options {
  int32_t subsample;
  int32_t max_iter;
  int32_t inputs_on_device;
  void* stream;              /* hipStream_t of the caller, read only with inputs_on_device */
} mpsfm_recip_options;

typedef struct mpsfm_recip_info {
  int64_t n_seeds;
  int64_t n_converged;    /* seeds inactive at the end (before the pairs are made unique) */
  int64_t nn_queries;     /* nearest-neighbour queries: the active seeds summed over all half-steps */
  int32_t iterations;     /* iterations at whose start a seed was active */
  int32_t column_ranges;  /* workgroups that shared the columns of one strip of rows (results do not depend on it) */
  float ms;               /* device time from the first kernel to the last (HIP events), transfers excluded */
  int32_t reserved;
} mpsfm_recip_info;

/* the reference's use: subsample 8, max_iter 10, host inputs */
void mpsfm_recip_default_options(mpsfm_recip_options* opts);

int64_t mpsfm_recip_seed_count(int32_t H, int32_t W, int32_t subsample);

int mpsfm_reciprocal_nns(const float* A /* [H1][W1][C] */, int32_t H1, int32_t W1, const float* B /* [H2][W2][C] */, int32_t H2, int32_t W2,
                         int32_t C, const mpsfm_recip_options* opts /* NULL: defaults */, int32_t device, int64_t capacity,
                         int32_t* idx1 /* [capacity] */, int32_t* idx2 /* [capacity] */, int64_t* n_out, mpsfm_recip_info* info /* may be NULL */);

int mpsfm_dense_correspondences(const float* feat11, const float* feat21, const float* feat22, const float* feat12,
                                const float* qonf11, const float* qonf21, const float* qonf22, const float* qonf12,
                                int32_t H1, int32_t W1, int32_t H2, int32_t W2, int32_t C, const mpsfm_recip_options* opts /* NULL: defaults */,
                                int32_t device, int64_t capacity, int32_t* xy1 /* [capacity][2] x, y */, int32_t* xy2 /* [capacity][2] */,
                                float* scores /* [capacity] */, int64_t* n_out, mpsfm_recip_info* info /* may be NULL */);

/* ---- a dense matcher's warp to match lists: the post-network half of the reference's RoMa matcher
 *    (mpsfm/extraction/pairwise/models/roma.py:82-124 with models/utils/warp.py simple_nms, kpids_to_matches0,
 *    get_unique_matches, matches_to_matches0, assign_keypoints; contract, tie rule and kernels: DESIGN.md section 4n).
 *    Every decision below is a comparison of input values or of values rounded operation by operation: results are exact
 *    and do not depend on how the device schedules the work.
 *
 *    mpsfm_simple_nms: out = simple_nms(scores, radius) of a float32 map [H][W].  With pool(x)[i][j] the maximum of x over
 *    |di| <= radius, |dj| <= radius inside the map:  m = (s == pool(s));  twice { supp = any m in the window;
 *    ss = supp ? 0 : s;  m |= (ss == pool(ss)) & !supp };  out = m ? s : 0.  A plateau of equal values keeps all its pixels,
 *    radius 0 keeps everything, negative scores meet the zeros of suppressed pixels as they do in the reference.  The result
 *    is bitwise torch's.  inputs_on_device != 0: scores AND out are device pointers (overlapping ranges are MPSFM_EINVAL), else
 *    both are host memory.
 *
 *    mpsfm_kpids_to_matches0: a row i is valid when ids0[i] >= 0 and ids1[i] >= 0.  A valid row is kept iff it has the
 *    highest score among the valid rows with its ids0 AND among the valid rows with its ids1; EQUAL SCORES GO TO THE LOWEST
 *    ROW (-0.0 counts as +0.0; the reference's choice among equal scores is an accident of an unstable np.argsort).  For
 *    kept rows matches0[ids0] = ids1 and scores0[ids0] = score, elsewhere -1 and 0.  *n_kps0 = 1 + the largest ids0 of a
 *    kept row, 0 when none is kept: the LENGTH OF THE REFERENCE'S OUTPUT, which is not the number of keypoints.
 *    inputs_on_device != 0: ids0, ids1 and scores are device pointers; the outputs are host memory.
 *
 *    mpsfm_warp_matches: both legs of Roma._forward for one pair, selected by `mode` (MPSFM_WARP_DENSE | MPSFM_WARP_SPARSE).
 *    certainty [H][W] and warp [H W][4] = (xA, yA, xB, yB) in normalised coordinates, float32.  Pixel coordinates are
 *    px = fl32(fl32(W_img / 2) * fl32(x + 1)), py = fl32(fl32(H_img / 2) * fl32(y + 1)), each operation rounded on its own:
 *    what torch computes for `W / 2 * (coords[..., 0] + 1)` on a float32 tensor.  The formula is RoMa's to_pixel_coordinates,
 *    third-party code that is not part of the reference tree: it is TAKEN AS THE CONTRACT here, not pinned to RoMa's source.
 *      dense leg   the rows whose simple_nms(certainty, nms_radius) value is strictly greater than fl32(sample_thresh), in
 *                  row order: dkeypoints0 / dkeypoints1 [n_dense][2] pixels, dscores [n_dense] (capacity H W each).
 *      sparse leg  for EVERY row id0 = the keypoint of skpts0 nearest to (fp64(px_A) scale0[0], fp64(py_A) scale0[1]) and
 *                  strictly closer than max_error, as mpsfm_assign_keypoints decides it (lowest index among equidistant
 *                  ones); id1 the same with skpts1, scale1 and (px_B, py_B); then mpsfm_kpids_to_matches0 with the raw
 *                  certainty as score: smatches0 / sscores0 [n_s0], *n_kps0.
 *    skpts* and scale* are host memory, all outputs are host memory and complete on return; nothing is retained.
 *
 *    inputs_on_device / stream: as for mpsfm_match_options (an event is recorded on `stream` and the call's own stream waits
 *    for it; the library never works on the null stream).
 *
 *    MPSFM_EINVAL before any device is touched: NULL pointers, H or W < 1, H W or n above 2^27, negative counts, radius
 *    outside 0 .. 64, ids >= n0 / n1 or < -1, image sizes < 1, a mode without a leg, non-finite or negative max_error,
 *    a sample_thresh that is not finite as float32, non-finite scales, keypoints or host map / warp / score values, device
 *    ranges of scores and out that overlap.  Device inputs are scanned by a kernel: MPSFM_EINVAL after it.  No rows, no valid row among host rows, or (sparse leg) no keypoints on a side: all -1 / 0 /
 *    count 0 without a device.
 *    MPSFM_ENODEVICE without a device. ---- */
#define MPSFM_WARP_DENSE 1
#define MPSFM_WARP_SPARSE 2

typedef struct mpsfm_warp_options {
  double sample_thresh;  /* dense leg */
  double max_error;      /* sparse leg */
  double scale0[2];
  double scale1[2];
  int32_t nms_radius;    /* dense leg */
  int32_t inputs_on_device;
  void* stream;          /* hipStream_t of the caller, read only with inputs_on_device */
} mpsfm_warp_options;

typedef struct mpsfm_warp_info {
  int64_t num_dense;    /* rows the dense leg selected */
  int64_t num_valid;    /* rows with both ids >= 0 */
  int64_t num_matches;  /* rows kept by the unique-match rule */
  float ms;             /* device time from the first kernel to the last (HIP events), transfers excluded */
  int32_t reserved;
} mpsfm_warp_info;

/* the reference's default_conf: sample_thresh 0.1, nms_radius 8, max_error 2, scales 1, host inputs */
void mpsfm_warp_default_options(mpsfm_warp_options* opts);

int mpsfm_simple_nms(int32_t H, int32_t W, const float* scores /* [H][W] */, int32_t radius, int32_t inputs_on_device, void* stream,
                     int32_t device, float* out /* [H][W] */, mpsfm_warp_info* info /* may be NULL: ms */);

int mpsfm_kpids_to_matches0(int64_t n, const int64_t* ids0, const int64_t* ids1 /* [n], -1: none */, const float* scores /* [n] */,
                            int64_t n0, int64_t n1 /* ids0 < n0, ids1 < n1 */, int32_t inputs_on_device, void* stream, int32_t device,
                            int32_t* matches0 /* [n0] */, float* scores0 /* [n0] */, int64_t* n_kps0, mpsfm_warp_info* info /* may be NULL */);

int mpsfm_warp_matches(int32_t H, int32_t W, const float* certainty /* [H][W] */, const float* warp /* [H W][4] */, int32_t H_A, int32_t W_A,
                       int32_t H_B, int32_t W_B, int32_t mode, const mpsfm_warp_options* opts /* NULL: defaults */,
                       int64_t n_s0, const double* skpts0 /* [n_s0][2], host */, int64_t n_s1, const double* skpts1 /* [n_s1][2], host */,
                       int32_t device, float* dkeypoints0, float* dkeypoints1 /* [H W][2] */, float* dscores /* [H W] */, int64_t* n_dense,
                       int32_t* smatches0 /* [n_s0] */, float* sscores0 /* [n_s0] */, int64_t* n_kps0, mpsfm_warp_info* info /* may be NULL */);

/* ---- monocular depth and normal priors of many images in one call (reference mpsfm/sfm/scene/image/depth.py:34-130
 *    Depth._init, image/utils.py:6-36 get_continuity_mask, image/normals.py:12-246 Normals._init; looped per image by
 *    reconstruction/mixins/init_utils.py:53-64 initialize_mono_maps).  Images of one call may differ in source size, target
 *    size and in which optional inputs they carry; the configuration is per call.  Value maps are float64, or float32 with
 *    is_float32 (upcast on load: arithmetic is fp64, except the continuity test, which runs in the map's own precision);
 *    masks are one byte per pixel, non-zero = true.  Value outputs are float64, mask outputs uint8 (0 / 1).
 *    Resizing (OpenCV is restated): bilinear samples at (i + 0.5) (n_src / n_dst) - 0.5 per axis with a
 *    replicated border and the fraction rounded to float32, rows first, then columns; equal sizes copy; a mask resized
 *    bilinearly and tested == 1 is true iff every tap of non-zero weight is true; nearest takes source index
 *    min(floor(i n_src / n_dst), n_src - 1).  n_images == 0 is a no-op.  No input array is modified. ---- */
typedef struct mpsfm_depth_prior_conf { /* Depth.default_conf */
  double inherent_noise;
  double std_multiplier;
  double prior_std_multiplier;
  double max_std;               /* read with has_max_std */
  double depth_lim;             /* read with has_depth_lim */
  double fixed_uncertainty_val;
  double depth_uncertainty;     /* read with has_depth_uncertainty */
  int32_t has_max_std, has_depth_lim, has_depth_uncertainty; /* 0: the setting is None */
  int32_t use_continuity, fixed_uncertainty, prior_uncertainty, flip_consistency;
  int32_t reserved;
} mpsfm_depth_prior_conf;

typedef struct mpsfm_depth_prior_problem {
  int32_t height, width;           /* of depth, depth2, the variances, valid, valid2            */
  int32_t int_height, int_width;   /* camera.int_height / int_width: size of the outputs        */
  int32_t mask_height, mask_width; /* of mask (ignored when mask is NULL)                       */
  int32_t is_float32;              /* depth, depth2 and the variances are float32               */
  int32_t n_kps;
  const void* depth;               /* required                                                  */
  const void* depth2;              /* NULL: absent (required by flip_consistency)               */
  const void* depth_variance;      /* NULL: absent (required by prior_uncertainty)              */
  const void* depth_variance2;     /* NULL: absent (required by both together)                  */
  const uint8_t* valid;            /* NULL: absent                                              */
  const uint8_t* valid2;           /* NULL: absent                                              */
  const uint8_t* mask;             /* NULL: absent; [mask_height][mask_width]                   */
  const double* kps;               /* [n_kps][2] image coordinates; may be NULL with n_kps == 0 */
  double sx, sy;                   /* camera.sx / sy (keypoint -> map coordinates)              */
} mpsfm_depth_prior_problem;

typedef struct mpsfm_depth_prior_output {
  double* data_prior;         /* [int_height][int_width] */
  double* uncertainty;        /* [int_height][int_width] */
  uint8_t* valid;             /* [int_height][int_width] */
  uint8_t* continuity_mask;   /* [int_height][int_width]; all 1 without use_continuity */
  double* uncertainty_update; /* [n_kps]: the finished uncertainty at the keypoints (PriorUtils.uncertainty_at_kps) */
} mpsfm_depth_prior_output;

typedef struct mpsfm_normal_prior_conf { /* Normals.default_conf */
  double inherent_polar_noise;
  double std_multiplier;
  double lc_std_multiplier;
  double prior_std_multiplier;
  double downscale_factor;
  int32_t flip_consistency;
  int32_t reserved;
} mpsfm_normal_prior_conf;

typedef struct mpsfm_normal_prior_problem {
  int32_t height, width;           /* of normals, normals2 and the variances                    */
  int32_t int_height, int_width;   /* H, W of the full-size outputs                             */
  int32_t mask_height, mask_width; /* of mask (ignored when mask is NULL)                       */
  int32_t half_height, half_width; /* Hd, Wd the caller sized the half-size outputs for: checked */
  int32_t is_float32;              /* normals and variances are float32                         */
  int32_t reserved;
  const void* normals;             /* [height][width][3], required                              */
  const void* normals2;            /* NULL: absent (required by flip_consistency)               */
  const void* normals_variance;    /* [height][width], required                                 */
  const void* normals2_variance;   /* NULL: absent (required by flip_consistency)               */
  const uint8_t* mask;             /* NULL: absent; [mask_height][mask_width]                   */
  const uint8_t* continuity_mask;  /* NULL: absent; [int_height][int_width]                     */
} mpsfm_normal_prior_problem;

typedef struct mpsfm_normal_prior_output { /* Hd = int(H // downscale_factor), Wd = int(W // downscale_factor): Python's floor
                                            * division (fmod based, 77 // 1.1 == 69), not floor(H / f); a problem whose
                                            * half_height / half_width differ from that is refused                         */
  double* data;                   /* [H][W][3]      */
  double* uncertainty;            /* [H][W][3][3]   */
  double* data_downscaled;        /* [Hd][Wd][3]    */
  double* uncertainty_downscaled; /* [Hd][Wd][3][3] */
} mpsfm_normal_prior_output;

typedef struct mpsfm_prior_summary {
  float ms;          /* device time of the launches (HIP events), transfers excluded */
  int32_t n_images;
  int64_t n_pixels;  /* destination pixels over all images (full size) */
} mpsfm_prior_summary;
#ifdef __cplusplus
static_assert(sizeof(mpsfm_depth_prior_conf) == 88 && offsetof(mpsfm_depth_prior_conf, has_max_std) == 56 &&
                  offsetof(mpsfm_depth_prior_conf, flip_consistency) == 80,
              "ABI of mpsfm_depth_prior_conf");
static_assert(sizeof(mpsfm_depth_prior_problem) == 112 && offsetof(mpsfm_depth_prior_problem, depth) == 32 &&
                  offsetof(mpsfm_depth_prior_problem, kps) == 88 && offsetof(mpsfm_depth_prior_problem, sy) == 104,
              "ABI of mpsfm_depth_prior_problem");
static_assert(sizeof(mpsfm_depth_prior_output) == 40, "ABI of mpsfm_depth_prior_output");
static_assert(sizeof(mpsfm_normal_prior_conf) == 48 && offsetof(mpsfm_normal_prior_conf, flip_consistency) == 40,
              "ABI of mpsfm_normal_prior_conf");
static_assert(sizeof(mpsfm_normal_prior_problem) == 88 && offsetof(mpsfm_normal_prior_problem, half_height) == 24 &&
                  offsetof(mpsfm_normal_prior_problem, normals) == 40 && offsetof(mpsfm_normal_prior_problem, continuity_mask) == 80,
              "ABI of mpsfm_normal_prior_problem");
static_assert(sizeof(mpsfm_normal_prior_output) == 32, "ABI of mpsfm_normal_prior_output");
static_assert(sizeof(mpsfm_prior_summary) == 16 && offsetof(mpsfm_prior_summary, n_pixels) == 8, "ABI of mpsfm_prior_summary");
#endif

int mpsfm_depth_priors(int32_t n_images, const mpsfm_depth_prior_problem* problems /* [n_images] */,
                       const mpsfm_depth_prior_conf* conf, int32_t device, const mpsfm_depth_prior_output* outputs /* [n_images] */,
                       mpsfm_prior_summary* summary /* may be NULL */);

int mpsfm_normal_priors(int32_t n_images, const mpsfm_normal_prior_problem* problems /* [n_images] */,
                        const mpsfm_normal_prior_conf* conf, int32_t device, const mpsfm_normal_prior_output* outputs /* [n_images] */,
                        mpsfm_prior_summary* summary /* may be NULL */);

/* ---- the correspondence graph from the inlier matches of all image pairs, in one call (COLMAP 3.11 CorrespondenceGraph::
 *    AddCorrespondences + Finalize, restated as a set rule so that no result depends on arrival order; what consumes it:
 *    mpsfm_tri_graph; the design and the measurements: DESIGN.md section 4s).
 *
 *    Images i = 0 .. n_images - 1 with nkp(i) = kp_start[i + 1] - kp_start[i] keypoints; the global index of keypoint idx of
 *    image i is kp_start[i] + idx, n_kp = kp_start[n_images].  Match lists l = 0 .. n_lists - 1: the rows
 *    matches[list_start[l] .. list_start[l + 1])[2] are (point2D index in list_image0[l], point2D index in list_image1[l]);
 *    n_matches = list_start[n_lists].  The same image pair may occur in several lists and in either orientation.
 *
 *    match_status[m] of every match, tested in this order (COLMAP refuses a whole list of self matches before it looks at
 *    an index):
 *      2 self pair   list_image0 == list_image1
 *      1 invalid     an index outside [0, nkp(image))
 *      3 duplicate   an equal UNDIRECTED pair of global keypoints occurs among the matches of status 0 or 3 at a lower position
 *                    in `matches`, whatever the orientation of either list
 *      0 added       everything else.  A keypoint may keep several partners in one other image, as in COLMAP.
 *
 *    corr_start [n_kp + 1] / corr_kp [n_corr]: the layout of mpsfm_tri_graph.  Row k holds the global indices of the partners
 *    of keypoint k, ascending; *n_corr = 2 x the number of added matches.
 *    image_num_correspondences[i]: the entries of the rows of image i; image_num_observations[i]: its non-empty rows.
 *    kp_two_view[k] = 1 where row k has exactly one entry and that entry's row has exactly one (IsTwoViewObservation).
 *    The pair view: the *n_pairs distinct image pairs with an added match, pair_image0 < pair_image1, ascending by
 *    (image0, image1); the added matches of pair p are pair_matches[pair_start[p] .. pair_start[p + 1])[2], local indices
 *    (in image0, in image1), ascending by (idx0, idx1).
 *
 *    Capacities, all caller-allocated host memory: match_status [n_matches], corr_kp [2 n_matches], pair_image0 / pair_image1
 *    [n_lists], pair_start [n_lists + 1], pair_matches [n_matches][2]; what lies behind n_corr / n_pairs is set to 0.  Every
 *    output is a function of the input alone: bitwise the same from run to run.  Nothing is retained; the host waits ONCE per
 *    call (info->num_syncs == 1).
 *
 *    MPSFM_EINVAL before any device is touched: NULL pointers (info may be NULL; arrays of length 0 may be NULL), negative
 *    counts, kp_start[0] or list_start[0] != 0, a decreasing kp_start or list_start, a list image outside [0, n_images).
 *    MPSFM_EUNSUPPORTED: n_kp >= 2^31 or 2 n_matches >= 2^31.  No matches or no keypoints: the empty graph (every match a
 *    self pair or invalid) without a device.  MPSFM_ENODEVICE without a device, but only when one is needed. ---- */
typedef struct mpsfm_corr_graph_info {
  int64_t num_added, num_invalid, num_self_pairs, num_duplicates; /* matches per status */
  int64_t num_launches; /* kernel launches of the call, the library sorts and scans excluded */
  int64_t num_syncs;    /* stream synchronisations of the call */
  float ms;             /* device time from the first kernel to the last (HIP events), transfers excluded */
  int32_t reserved;
} mpsfm_corr_graph_info;
#ifdef __cplusplus
static_assert(sizeof(mpsfm_corr_graph_info) == 56 && offsetof(mpsfm_corr_graph_info, num_launches) == 32 &&
                  offsetof(mpsfm_corr_graph_info, ms) == 48,
              "ABI of mpsfm_corr_graph_info");
#endif

int mpsfm_corr_graph_build(int32_t n_images, const int64_t* kp_start /* [n_images + 1] */, int32_t n_lists,
                           const int32_t* list_image0, const int32_t* list_image1 /* [n_lists] image indices */,
                           const int64_t* list_start /* [n_lists + 1] */, const int32_t* matches /* [n_matches][2] */, int32_t device,
                           uint8_t* match_status /* [n_matches] */, int64_t* corr_start /* [n_kp + 1] */,
                           int64_t* corr_kp /* [2 n_matches] */, int64_t* n_corr, int32_t* image_num_correspondences /* [n_images] */,
                           int32_t* image_num_observations /* [n_images] */, uint8_t* kp_two_view /* [n_kp] */, int64_t* n_pairs,
                           int32_t* pair_image0, int32_t* pair_image1 /* [n_lists] */, int64_t* pair_start /* [n_lists + 1] */,
                           int32_t* pair_matches /* [n_matches][2] */, mpsfm_corr_graph_info* info /* may be NULL */);

/* ---- scene queries of the incremental loop: which image to register next, and the local bundle of an image (the design and the
 *    measurements: DESIGN.md section 4t).  Both read the arrays of mpsfm_tri_graph / mpsfm_tri_state; images, keypoints and
 *    points are addressed as there (global keypoint index kp_start[image] + point2D_idx).  Stateless; inputs and outputs are
 *    caller-allocated host memory; the host waits ONCE per call (info->num_syncs == 1).  The fork's COLMAP source is not in
 *    the reference tree: both rules are restated from upstream COLMAP 3.11, parity unpinned.
 *
 *    mpsfm_visibility_scores: COLMAP's per-image statistics num_visible_points3D and point3D_visibility_score
 *    (VisibilityPyramid::SetPoint applied to the set that ObservationManager maintains incrementally), stated on sets:
 *      keypoint k is VISIBLE when some entry p of its row corr_kp[corr_start[k] .. corr_start[k + 1]) has kp_point[p] >= 0
 *      (its own point does not count).  With D = 1 << num_levels, cx = clamp((int64) trunc((double) D * x / width), 0, D - 1),
 *      a negative or NaN operand giving 0, and cy likewise from height: level l = 1 .. num_levels has 2^l x 2^l cells, the
 *      visible keypoint occupies cell (cy >> (num_levels - l), cx >> (num_levels - l)) of it;
 *      score[i] = sum over l of occupied_cells(l) * 4^l, num_visible[i] = the number of visible keypoints of image i,
 *      kp_visible[k] = 1 / 0 (may be NULL).  num_levels: 6 is COLMAP's kNumPoint3DVisibilityPyramidLevels; 1 .. 8 are accepted.
 *      image_size [n_images][2]: width, height.  Every output is an integer: bitwise the same from run to run.
 *    MPSFM_EINVAL before any device is touched: NULL pointers (info and kp_visible may be NULL; arrays of length 0 may be NULL),
 *    a negative count, num_levels outside 1 .. 8, kp_start[0] or corr_start[0] != 0, a decreasing kp_start or corr_start, a
 *    corr_kp outside [0, n_kp), a width or height <= 0.  MPSFM_EUNSUPPORTED: n_kp >= 2^31.  No keypoints: zeros without a device.
 *
 *    mpsfm_local_bundles: IncrementalMapper::FindLocalBundle for n_refs reference images in one call (the same image may occur
 *    twice).  Keypoints of images that are not registered are ignored.  With m_r(p) the number of keypoints of reference r whose
 *    point is p:
 *      shared[r][j]   = sum over the keypoints k' of image j != r with a point p' of m_r(p'): track elements count with
 *                       multiplicity, as in COLMAP's map.  shared[r][r] = 0.
 *      overlapping images: shared > 0, ordered by shared descending, equal counts by ascending image index (COLMAP leaves
 *                       those to an unordered map).
 *      angle list of (r, j): ONE entry per keypoint k' of j with m_r(p') > 0, the triangulation angle of X_p' between the
 *                       projection centres C = -R^T t of r and j (CalculateTriangulationAngle, radians).
 *      angle75[r][j]  = the element of rank floor(0.75 (n - 1) + 0.5) of that list in ascending order (COLMAP's Percentile,
 *                       which rounds), -1 where shared == 0.  Exact: it does not depend on the order of the list.
 *      selection: N = num_images - 1, E = min(N, #overlapping).  If #overlapping == E all are taken in order.  Otherwise, with
 *                       T the number of keypoints of r with a point, the eight thresholds (min_tri_angle_rad / {1, 1.5, 2, 2.5,
 *                       3, 4, 5, 6}, {0.6, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.1} * T) are walked in turn, each over the overlapping
 *                       images in order: the walk of a threshold stops at the first image whose shared is below the second
 *                       number, images already taken are skipped, an image is taken when angle75 >= the first number;
 *                       everything stops at E images, and what is missing is filled with untaken images in order.
 *      bundle [n_refs][num_images - 1]: image indices, padded with -1; bundle_len [n_refs]; shared and angle75 [n_refs][n_images].
 *    MPSFM_EINVAL before any device is touched: NULL pointers, negative counts, kp_start as above, num_images < 1, a
 *    min_tri_angle_deg that is negative or not finite, a reference outside [0, n_images) or not registered, a kp_point
 *    outside [-1, n_points), a pose of a registered image or a point that is not finite.  Many references are worked off in
 *    groups that share one workspace (info->num_groups), still with one wait. ---- */
typedef struct mpsfm_scene_query_info {
  int64_t num_launches; /* kernel launches of the call */
  int64_t num_syncs;    /* stream synchronisations of the call */
  int64_t num_groups;   /* groups of reference images (mpsfm_local_bundles; 1 for mpsfm_visibility_scores) */
  float ms;             /* device time from the first kernel to the last (HIP events), transfers excluded */
  int32_t reserved;
} mpsfm_scene_query_info;
#ifdef __cplusplus
static_assert(sizeof(mpsfm_scene_query_info) == 32 && offsetof(mpsfm_scene_query_info, num_groups) == 16 &&
                  offsetof(mpsfm_scene_query_info, ms) == 24,
              "ABI of mpsfm_scene_query_info");
#endif

int mpsfm_visibility_scores(int32_t n_images, const int64_t* kp_start /* [n_images + 1] */, const double* kp_xy /* [n_kp][2] */,
                            const int64_t* corr_start /* [n_kp + 1] */, const int64_t* corr_kp /* [n_corr] */,
                            const int64_t* kp_point /* [n_kp] */, const int32_t* image_size /* [n_images][2] */, int32_t num_levels,
                            int32_t device, int32_t* num_visible /* [n_images] */, int64_t* score /* [n_images] */,
                            uint8_t* kp_visible /* [n_kp], may be NULL */, mpsfm_scene_query_info* info /* may be NULL */);

int mpsfm_local_bundles(int32_t n_images, const int64_t* kp_start /* [n_images + 1] */, const mpsfm_tri_state* state, int32_t n_refs,
                        const int32_t* ref_image /* [n_refs] */, int32_t num_images, double min_tri_angle_deg, int32_t device,
                        int32_t* bundle /* [n_refs][num_images - 1] */, int32_t* bundle_len /* [n_refs] */,
                        int32_t* shared /* [n_refs][n_images] */, double* angle75 /* [n_refs][n_images] */,
                        mpsfm_scene_query_info* info /* may be NULL */);

/* ---- the filter behind a bundle adjustment, over the scene's arrays (reference mpsfm/sfm/mapper/base.py:686-797: filter_bundle /
 *    filter_all; the design and the measurements: DESIGN.md section 4v).  ONE stateless call does what the mapper does through
 *    ObservationManager one filter at a time: filter_observations_with_negative_depth, the "risky" set of find_invalid_depth_points,
 *    filter_points3D on that set and filter_points3D on the bundle's points.  It reads kp_start, kp_xy and cam_intr of
 *    mpsfm_tri_graph (corr_* may be NULL) and the whole mpsfm_tri_state; it changes nothing: the caller applies the answer.  One
 *    host wait per call (info->num_syncs == 1); every output is the same bit for bit from run to run.
 *
 *    The rules (COLMAP 3.11 ObservationManager as sfm/scene/observations.py freezes it), per point p with the elements
 *    E = {k : kp_point[k] == p}, in ascending k.  A point index without an element is untouched and never counted.
 *      per element     with R, t of the image that owns k (R from the quaternion, C = -R^T t) and its fx fy cx cy:
 *                      (xc, yc, zc) = R X + t, front = zc >= 2^-52, sq_err = (fx xc / zc + cx - x)^2 + (fy yc / zc + cy - y)^2.
 *                      Every product and sum rounds on its own (no fused multiply-add), left to right.
 *      step 0          only with negative_depth.  n = |E|, m = the elements that are not in front.  m == 0: nothing.  n - m >= 2:
 *                      those m observations are removed, num_negative += m.  Otherwise the point dies, num_negative +=
 *                      max(n - 1, 1): the delete_observation calls up to and including the one that meets a track of length <= 2.
 *      risky set A     on what step 0 left: p is in A iff in_bundle and kp_invalid_depth are given, at least one image is in the
 *                      bundle, and every bundle image owns at least one surviving element of p with kp_invalid_depth == 1 (two
 *                      such keypoints of one image count once): set.intersection(*find_invalid_depth_points(optim_ids)).
 *      a pass (max_err, thr) on the current elements, L of them: bad = not in front, or sq_err > max_err^2 (strict; a NaN error is
 *                      not bad by itself).  L < 2 or |bad| >= L - 1: the point dies, changed += L.  Otherwise the bad observations
 *                      are removed, changed += |bad|, and the largest pairwise angle of the remaining elements is taken (b2 =
 *                      |C1 - C2|^2, r1 = |X - C1|^2, r2 = |X - C2|^2, den = 2 sqrt(r1 r2), 0 where den == 0, else a =
 *                      |acos(clamp((r1 + r2 - b2) / den))|, min(a, pi - a)); if !(angle >= thr) the point dies, changed += 1.
 *      order           pass A = pass(max_reproj_error, risky_min_tri_angle_rad) on the points of A (num_changed_a), then pass B =
 *                      pass(max_reproj_error, min_tri_angle_rad) on the points of point_sel that still exist (num_changed_b); a
 *                      point in both sets gets both.  point_sel == NULL selects every point: with no bundle that is filter_all.
 *                      Points in neither set do step 0 only.
 *    Outputs: kp_deleted [n_kp] 0, or 1 / 2 / 3 for an observation removed on its own in step 0 / pass A / pass B from a point that
 *    lives on (the observations that go with a whole point are not marked, whenever they left it).  point_fate [n_points] 0 untouched,
 *    1 kept with observations removed, 2 died in step 0, 3 / 4 died in pass A by reprojection / by angle, 5 / 6 the same in pass B.
 *    point_risky [n_points] 1 for the points of A.  point_max_angle [n_points] (may be NULL) the angle of the angle test run on the
 *    point, 0 where none ran.  kp_sq_err [n_kp] (may be NULL) sq_err of every keypoint with a point, 0 for the others.
 *    MPSFM_EINVAL before any device is touched: NULL pointers (in_bundle, kp_invalid_depth, point_sel, point_max_angle, kp_sq_err and
 *    info may be NULL; arrays of length 0 may be NULL), a negative count, kp_start[0] != 0 or decreasing, a kp_point outside
 *    [-1, n_points), a keypoint with a point in an image that is not registered, a pose of a registered image, a point or an
 *    intrinsic that is not finite, a max_reproj_error or an angle that is negative or not finite, a negative_depth other than 0 / 1.
 *    MPSFM_EUNSUPPORTED: 2^31 keypoints or points.  n_points == 0 or n_kp == 0: zeroed outputs, no device. ---- */
typedef struct mpsfm_scene_filter_options {
  double max_reproj_error;         /* pixels: filter_max_reproj_error x median(kp_std) */
  double min_tri_angle_rad;        /* pass B */
  double risky_min_tri_angle_rad;  /* pass A: the mapper's 1.5 degrees */
  int32_t negative_depth;          /* 1: step 0 runs */
  int32_t reserved;
} mpsfm_scene_filter_options;
typedef struct mpsfm_scene_filter_info {
  int64_t num_negative;           /* what filter_observations_with_negative_depth returns */
  int64_t num_changed_a;          /* what filter_points3D returns on the risky set */
  int64_t num_changed_b;          /* ... and on the selected points */
  int64_t n_points_deleted;       /* points with point_fate >= 2 */
  int64_t n_observations_deleted; /* keypoints with kp_deleted != 0 */
  int64_t num_syncs;              /* stream synchronisations of the call */
  float ms;                       /* device time from the first kernel to the last (HIP events), transfers excluded */
  float ms_tracks;                /* ... of which the track lists: image records, keys, sort, segment starts */
} mpsfm_scene_filter_info;
#ifdef __cplusplus
static_assert(sizeof(mpsfm_scene_filter_options) == 32 && sizeof(mpsfm_scene_filter_info) == 56 &&
                  offsetof(mpsfm_scene_filter_info, ms) == 48,
              "ABI of mpsfm_filter_scene");
#endif

int mpsfm_filter_scene(const mpsfm_tri_graph* graph, const mpsfm_tri_state* state, const uint8_t* in_bundle /* [n_images] or NULL */,
                       const uint8_t* kp_invalid_depth /* [n_kp] or NULL */, const uint8_t* point_sel /* [n_points] or NULL */,
                       const mpsfm_scene_filter_options* options, int32_t device, uint8_t* kp_deleted /* [n_kp] */,
                       uint8_t* point_fate /* [n_points] */, uint8_t* point_risky /* [n_points] */,
                       double* point_max_angle /* [n_points], may be NULL */, double* kp_sq_err /* [n_kp], may be NULL */,
                       mpsfm_scene_filter_info* info /* may be NULL */);

/* ---- 3D-3D alignment: rigid and similarity LO-RANSAC of two point sets, the least-squares fit on its own, and the RGB-D pair
 *    registration built on them (reference icp/main.py:105-193 with icp/depth_to_3d.py and icp/interpolate.py, the fork's only
 *    addition to upstream MP-SfM).  Loop, options and names are modelled on COLMAP 3.11's EstimateRigid3dRobust /
 *    EstimateSim3dRobust (LORANSAC over a closed-form 3-point solver) as recalled; parity with pycolmap is unpinned.  The fork's
 *    own loop (5000 fixed trials of np.random.choice, inliers counted by |q - (R p + t)| < 0.1, no local optimisation, no scale)
 *    is not reproduced trial by trial: its closed form (rigid_transform_3D) and its lifting are, see below.
 *
 *    mpsfm_align3d_estimate.  Model: tgt ~ s R src + t, s == 1 when with_scale == 0.  Residual: |tgt_i - (s R src_i + t)|^2,
 *    evaluated as written (s (R p) + t, no fused multiply-add); inlier: residual <= max_error^2, max_error in the units of tgt.
 *    Loop: LO-RANSAC with sample size 3, one model per trial; support measure, min_inlier_ratio cap, dynamic bound and stop test
 *    as in mpsfm_abs_pose_estimate (exponent 3).  Sampler: the counter recipe of mpsfm_abs_pose_estimate, the first three
 *    distinct indices.  Minimal solver: centroids, the 3 x 3 cross-covariance of the centred points, the rotation by Horn's
 *    quaternion method (always det R = +1: a mirrored set gets the best proper rotation, as the fork's reflection fix does);
 *    with_scale: s = sum (q - mq)^T R (p - mp) / sum |p - mp|^2 (Umeyama); t = mq - s R mp.  Rules of ours that COLMAP and
 *    the fork leave open: a sample gives no model when its three source points or its three target points are collinear
 *    (sin^2 of the angle at the first point <= 1e-20, P3P's test; it covers coincident points), or when its scale is not finite
 *    and positive.  Local estimator: a sample model that becomes the best with more than 3 inliers starts up to 10 rounds of the
 *    same closed form over its current inlier set, continued while the inlier count grows.  Its sums are reduced on the device
 *    in a fixed order in two passes, so the covariance is centred: count, sum p, sum q; then the 9 cross terms, the 6 + 6
 *    scatter terms of source and target and sum |p - mp|^2, with the inlier test evaluated from the incoming model inside the
 *    reduction.  The fit gives no model when fewer than 3 points are selected or when the source or the target scatter matrix has
 *    its second-largest eigenvalue <= 1e-12 x its largest (points on a line; a planar set is fine).
 *    tgt_from_src = [R | t] row-major with R orthonormal, det R = +1, and scale apart: tgt = scale R src + t.
 *    inlier_mask[i] = 1 for the inliers of the final model.  n < 3, n > INT32_MAX, NULL pointers, non-finite inputs and invalid
 *    options are MPSFM_EINVAL before any HIP call.  No model: result->success = 0 and return value 0.  Results are identical
 *    run to run and for every batch_trials.
 *
 *    mpsfm_align3d_fit: the local estimator on its own (the non-robust estimate_rigid3d / estimate_sim3d) over the points with
 *    mask[i] != 0 (mask NULL: all), same reductions, same degeneracy rule; num_inliers = the number of points used,
 *    num_models = 1 on success, the other counters 0.  Argument checks as above (no options).
 *
 *    mpsfm_lift_keypoints: icp/depth_to_3d.py + icp/interpolate.py in one launch, one thread per keypoint; the point map is never
 *    materialised.  The four corner points at (c, r) = (trunc(x) + {0, 1}, trunc(y) + {0, 1}) are ((c - cx) z) / fx,
 *    ((r - cy) z) / fy, z; with ax = x - trunc(x), ay = y - trunc(y) the result is
 *        a00 (1 - ax) (1 - ay) + a01 ax (1 - ay) + a10 (1 - ax) ay + a11 ax ay      (a01: column + 1, a10: row + 1)
 *    evaluated left to right without fused multiply-adds: bit for bit the fork's float64 result.  VALIDITY (the fork has no rule:
 *    it indexes out of range or interpolates zero depth; icp/save_pcd.py treats z == 0 as absent): a keypoint is valid iff
 *    x >= 0, y >= 0, trunc(x) + 1 <= W - 1, trunc(y) + 1 <= H - 1, all four corner depths are finite and > 0, and the lifted
 *    point is finite (no overflow).  A NaN coordinate is invalid.  An invalid keypoint gets xyz = 0 and valid = 0.
 *    MPSFM_EINVAL before any HIP call: NULL pointers, H or W < 1, H W > INT32_MAX, n < 0 or > INT32_MAX, intrinsics that are
 *    not finite or a zero focal length.  n == 0: no device.
 *
 *    mpsfm_depth_pair_register: everything of icp/main.py behind the matcher in one call.  Both ends of each match
 *    (matches[i] = {keypoint of image 0, keypoint of image 1}) are lifted; matches whose two ends are both valid are compacted on
 *    the device in match order (one host wait delivers their count) and mpsfm_align3d_estimate's loop runs on them, source =
 *    image 0, target = image 1; its mask is scattered back to the matches.  valid[i]: both ends valid; lifted0 / lifted1 [m][3]:
 *    the lifted ends (zeros where that end is invalid); inlier_mask[i] = 0 for invalid matches.  Fewer than 3 valid matches:
 *    success = 0.  The result equals, bit for bit, two mpsfm_lift_keypoints calls, a host compaction and mpsfm_align3d_estimate
 *    with the same options.  MPSFM_EINVAL before any HIP call: as mpsfm_lift_keypoints for both maps, a match index out of
 *    range, invalid options.  m == 0: success = 0, no device.  One PINHOLE pair per call. ---- */
/* defaults: max_error 0.1 (the fork's pts_bound), min_inlier_ratio 0.1, confidence 0.99, dyn_num_trials_multiplier 3.0,
 * min_num_trials 100, max_num_trials 5000 (the fork's trial count) */
typedef mpsfm_ransac_options mpsfm_align3d_options;

typedef struct mpsfm_align3d_result {
  double tgt_from_src[12];  /* [R | t] row-major; tgt = scale R src + t */
  double scale;             /* 1 for a rigid model */
  int64_t num_inliers;      /* mpsfm_align3d_fit: points used */
  int64_t num_trials;       /* LORANSAC's report.num_trials */
  int64_t max_num_trials;   /* after the min_inlier_ratio cap */
  int64_t num_models;       /* model slots scored (all batches, one per trial) */
  int32_t success;
  int32_t lo_rounds;        /* local estimates run */
  int32_t num_batches;
  float ms;                 /* device time of the launches (HIP events), transfers and host work excluded */
} mpsfm_align3d_result;
#ifdef __cplusplus
static_assert(sizeof(mpsfm_align3d_result) == 152 && offsetof(mpsfm_align3d_result, scale) == 96 &&
                  offsetof(mpsfm_align3d_result, success) == 136,
              "ABI of mpsfm_align3d_result");
#endif

int mpsfm_align3d_estimate(int64_t n, const double* src /* [n][3] */, const double* tgt /* [n][3] */, int32_t with_scale,
                           const mpsfm_align3d_options* options, int32_t device, uint8_t* inlier_mask /* [n] */,
                           mpsfm_align3d_result* result);

int mpsfm_align3d_fit(int64_t n, const double* src /* [n][3] */, const double* tgt /* [n][3] */, const uint8_t* mask /* [n] or NULL */,
                      int32_t with_scale, int32_t device, mpsfm_align3d_result* result);

int mpsfm_lift_keypoints(int32_t H, int32_t W, const double* depth /* [H][W] */, const double* intr /* PINHOLE fx fy cx cy */,
                         int64_t n, const double* xy /* [n][2] pixels of the map */, int32_t device, double* xyz /* [n][3] */,
                         uint8_t* valid /* [n] */);

int mpsfm_depth_pair_register(int32_t H0, int32_t W0, const double* depth0 /* [H0][W0] */, const double* intr0,
                              int32_t H1, int32_t W1, const double* depth1 /* [H1][W1] */, const double* intr1,
                              int64_t n0, const double* xy0 /* [n0][2] */, int64_t n1, const double* xy1 /* [n1][2] */,
                              int64_t m, const int32_t* matches /* [m][2] */, int32_t with_scale,
                              const mpsfm_align3d_options* options, int32_t device, uint8_t* valid /* [m] */,
                              uint8_t* inlier_mask /* [m] */, double* lifted0 /* [m][3] */, double* lifted1 /* [m][3] */,
                              mpsfm_align3d_result* result);

/* ---- Dense point-to-plane ICP of an RGB-D pair: the refinement behind mpsfm_depth_pair_register, over every depth pixel
 *    instead of a few hundred keypoints (the fork's icp/main.py stops at the RANSAC).  Projective association, one linearisation
 *    and one 6 x 6 solve per iteration, the whole loop enqueued without a host wait.  All f64, every expression rounded as
 *    written (no fused multiply-add).  PINHOLE intr = fx, fy, cx, cy.  Model: x1 = s (R x0) + t, mpsfm_depth_pair_register's
 *    tgt_from_src; s is an input held constant, the ICP refines R and t only.
 *
 *    Vertex of pixel (r, c): V = (((c - cx) z) / fx, ((r - cy) z) / fy, z), mpsfm_lift_keypoints' expression at integer
 *    coordinates; valid iff z is finite and > 0.
 *    Normal of an interior pixel: a = V(r, c + 1) - V(r, c - 1), b = V(r + 1, c) - V(r - 1, c), m = a x b, n = m / sqrt(m.m);
 *    valid iff the five vertices are valid, |z_nb - z_c| <= edge_ratio z_c for the four neighbours, m.m is finite and > 0 and
 *    n.V != 0; negated where n.V > 0, so it faces the camera.  Border pixels have no normal.  An invalid normal is stored as
 *    zeros.
 *    Source set: the pixels of map 0 with a valid normal and r % stride == 0 && c % stride == 0.
 *    Association at the pose (R, t): p' = s (R p) + t; p'_z > 0; u = (p'_x / p'_z) fx1 + cx1, v likewise; ci = floor(u + 0.5),
 *    ri = floor(v + 0.5), tested as doubles against 0 <= ci <= W1 - 1, 0 <= ri <= H1 - 1 (a NaN fails); the target pixel
 *    (ri, ci) needs a valid normal n1, its vertex is q; |p' - q|^2 <= max_distance^2; (R n0).n1 >= cos(max_angle_deg), the
 *    cosine formed once on the host.  A source pixel fails at the first test it does not pass; rejected[] counts the causes:
 *    0 not in front or outside the map, 1 no target normal, 2 distance, 3 angle.
 *    Linearisation: r = n1.(p' - q), J = [p' x n1, n1] for the left increment p' + w x p' + v; A = sum J J^T, b = - sum J r,
 *    sum r^2 and the counts, reduced in a fixed order without atomics: per workgroup, then the workgroups' rows in order.  The
 *    partition into threads and workgroups depends on H0, W0 and stride only.
 *    Step: A scaled symmetrically to unit diagonal and factored by Cholesky without pivoting; singular when a diagonal entry of
 *    A is <= 0 or a pivot of the scaled matrix is <= 1e-10.  Else xi = (w, v) = A^-1 b, R <- exp(w) R, t <- exp(w) t + v by
 *    Rodrigues' formula (I + [w]x below |w| = 1e-12).
 *    Endings (status): CONVERGED |w| <= eps_rotation and |v| <= eps_translation after the step is applied; TOO_FEW_PAIRS the
 *    pair count is < min_pairs, the pose of the previous iteration is kept; SINGULAR the pose is kept; MAX_ITERATIONS otherwise.
 *    iterations counts the linearisations formed, the one that ended the loop included; info, rhs, num_pairs, rejected and
 *    rmse = sqrt(sum r^2 / num_pairs) (0 without pairs) are those of the last one.
 *    trace (may be NULL) [options->max_iterations][4]: pair count, rmse, |w|, |v| per iteration (|w| = |v| = 0 where no step
 *    was taken), zeros past `iterations`.
 *
 *    mpsfm_depth_normals: the normal map on its own; normals [H][W][3], valid [H][W].
 *    mpsfm_depth_pair_icp: the loop from init [12] = [R | t] row-major and scale.  One host wait per call.
 *    mpsfm_depth_pair_register_dense: mpsfm_depth_pair_register, then, when it found a model, mpsfm_depth_pair_icp from that
 *    model on the maps already on the device: bit for bit the two calls one after the other.  No model (or m == 0): success = 0
 *    and *icp zeroed.
 *    MPSFM_EINVAL before any HIP call: NULL pointers (trace excepted), H or W < 3 (mpsfm_depth_normals: < 1), H W > INT32_MAX,
 *    intrinsics that are not finite or a zero focal length, init or scale not finite, scale <= 0, options out of range
 *    (max_distance > 0, 0 <= max_angle_deg <= 180, edge_ratio >= 0, eps >= 0, all finite; 1 <= max_iterations <= 64;
 *    min_pairs >= 6; stride >= 1).  Non-finite or non-positive depths are data: holes.  One PINHOLE pair per call. ---- */
#define MPSFM_ICP_MAX_ITERATIONS 64
enum { MPSFM_ICP_CONVERGED = 0, MPSFM_ICP_MAX_ITERATIONS_REACHED = 1, MPSFM_ICP_TOO_FEW_PAIRS = 2, MPSFM_ICP_SINGULAR = 3 };

/* defaults: max_distance 0.1 (the fork's pts_bound), max_angle_deg 30, edge_ratio 0.05, eps_rotation 1e-6, eps_translation 1e-6,
 * max_iterations 30, min_pairs 100, stride 1 */
typedef struct mpsfm_icp_options {
  double max_distance;     /* units of the depth maps */
  double max_angle_deg;
  double edge_ratio;
  double eps_rotation;     /* radians */
  double eps_translation;
  int32_t max_iterations;  /* 1 .. MPSFM_ICP_MAX_ITERATIONS */
  int32_t min_pairs;       /* >= 6 */
  int32_t stride;          /* >= 1 */
  int32_t reserved;
} mpsfm_icp_options;

typedef struct mpsfm_icp_result {
  double tgt_from_src[12];  /* [R | t] row-major; tgt = scale R src + t */
  double scale;             /* the input scale */
  double info[36];          /* A of the last linearisation formed, row-major, order (w, v) */
  double rhs[6];            /* b of the last linearisation formed */
  double rmse;
  int64_t num_pairs;
  int64_t rejected[4];
  int32_t iterations;
  int32_t status;           /* MPSFM_ICP_* */
  float ms;                 /* device time of the launches (HIP events), transfers excluded */
  int32_t reserved;
} mpsfm_icp_result;
#ifdef __cplusplus
static_assert(sizeof(mpsfm_icp_result) == 504 && offsetof(mpsfm_icp_result, scale) == 96 && offsetof(mpsfm_icp_result, iterations) == 488,
              "ABI of mpsfm_icp_result");
#endif

int mpsfm_depth_normals(int32_t H, int32_t W, const double* depth /* [H][W] */, const double* intr, double edge_ratio, int32_t device,
                        double* normals /* [H][W][3] */, uint8_t* valid /* [H][W] */);

int mpsfm_depth_pair_icp(int32_t H0, int32_t W0, const double* depth0 /* [H0][W0] */, const double* intr0, int32_t H1, int32_t W1,
                         const double* depth1 /* [H1][W1] */, const double* intr1, const double* init /* [12] */, double scale,
                         const mpsfm_icp_options* options, int32_t device, double* trace /* [max_iterations][4] or NULL */,
                         mpsfm_icp_result* result);

int mpsfm_depth_pair_register_dense(int32_t H0, int32_t W0, const double* depth0 /* [H0][W0] */, const double* intr0,
                                    int32_t H1, int32_t W1, const double* depth1 /* [H1][W1] */, const double* intr1,
                                    int64_t n0, const double* xy0 /* [n0][2] */, int64_t n1, const double* xy1 /* [n1][2] */,
                                    int64_t m, const int32_t* matches /* [m][2] */, int32_t with_scale,
                                    const mpsfm_align3d_options* options, const mpsfm_icp_options* icp_options, int32_t device,
                                    uint8_t* valid /* [m] */, uint8_t* inlier_mask /* [m] */, double* lifted0 /* [m][3] */,
                                    double* lifted1 /* [m][3] */, mpsfm_align3d_result* result,
                                    double* trace /* [max_iterations][4] or NULL */, mpsfm_icp_result* icp);

#ifdef __cplusplus
}
#endif
#endif /* MPSFM_HIP_H */
