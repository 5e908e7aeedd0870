/*
 * sqrtlm.h — C ABI of the MI355X square-root Levenberg–Marquardt
 * bundle-adjustment backend (libsqrtlm.so).
 *
 * Drop-in seam: the reference dispatches every BA call through the static
 * façade `Optimizer` (include/backend/Optimizer.h:42-71, solver switch
 * src/backend/Optimizer.cc:26-28) into `g2oOptimizer`, which assembles a g2o
 * graph and calls `SparseOptimizer::optimize`. A host adapter (see
 * INTEGRATION.md) replaces that g2o graph with the plain arrays below and
 * calls this library instead; the Tracking / LocalMapping / LoopClosing
 * threads are untouched.
 *
 * Conventions (all mirror the g2o path):
 *   - poses are T_cw as SE3Quat: q = (qx,qy,qz,qw) unit, qw >= 0, t (3);
 *     tangent order [omega; upsilon], left update T <- exp(d) T
 *     (Thirdparty/g2o/g2o/types/types_six_dof_expmap.h:73-76);
 *   - observations are EdgeSE3ProjectXYZ in insertion order (edge id = index);
 *     error = obs - project(T X) (types_six_dof_expmap.h:90-95);
 *     information = I * info; Huber delta per edge, 0 = no robust kernel;
 *   - every call is FP64 end to end.
 * Error model: every entry point returns an int status (SQLM_OK = 0, < 0 on
 * error); nothing throws across the ABI. A non-SPD damped system is NOT an
 * error: the LM step is rejected, as g2o does (levenberg.cpp:126-127).
 * Threading: one context per calling thread (LBA, loop-closing and GBA threads
 * may each own one); a context owns its HIP stream and device memory.
 */
#ifndef SQRTLM_H
#define SQRTLM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SQLM_OK 0
#define SQLM_ERR_INVALID_ARG (-1)
#define SQLM_ERR_HIP (-2)
#define SQLM_ERR_NOT_SPD (-3)
#define SQLM_ERR_OOM (-4)
#define SQLM_ERR_ABORTED (-5)
#define SQLM_ERR_NO_DEVICE (-6)
#define SQLM_ERR_STATE (-7)
#define SQLM_ERR_UNSUPPORTED (-8)
#define SQLM_ERR_COMM (-9)

#define SQLM_TRACE_MAX 256

typedef struct sqlm_ctx sqlm_ctx;

/* Per optimize() statistics; field meaning follows g2o's loop
 * (sparse_optimizer.cpp:354-419, optimization_algorithm_levenberg.cpp:61-164). */
typedef struct sqlm_stats {
  int iterations;     /* value SparseOptimizer::optimize returns               */
  int trials;         /* inner LM trials, all iterations                         */
  int result;         /* last SolverResult: 0 OK, 1 Terminate, 2 Fail          */
  int n_active_edges;
  double chi2_begin;  /* robust chi2 at the start of iteration 0               */
  double chi2_end;    /* currentChi after the last iteration                   */
  double lambda_end;
  int trace_len;
  double trace_chi2[SQLM_TRACE_MAX];
  double trace_lambda[SQLM_TRACE_MAX];
  int trace_trials[SQLM_TRACE_MAX];
  /* wall time split (ms, host clock around stream syncs) */
  double ms_total, ms_setup, ms_linearize, ms_trials;
} sqlm_stats;

const char *sqlm_version(void);
const char *sqlm_status_string(int status);

/* Context / device. Replaces `new g2o::SparseOptimizer` + solver setup
 * (g2oOptimizer.cc:784-798). device_id < 0 picks the current HIP device. */
int sqlm_ctx_create(int device_id, sqlm_ctx **out);
int sqlm_ctx_destroy(sqlm_ctx *ctx);

/* Graph assembly: replaces the addVertex/addEdge loops of
 * g2oOptimizer::LocalBundleAdjustment (g2oOptimizer.cc:805-912) and
 * ::BundleAdjustment (:142-296). Arrays are copied (caller keeps ownership).
 *   pose_q [n_pose][4], pose_t [n_pose][3], pose_fixed [n_pose], intr [n_pose][4]
 *   pt [n_pt][3]
 *   obs_pose/obs_pt [n_obs], obs_uv [n_obs][2], obs_info [n_obs] (invSigma2),
 *   obs_delta [n_obs] Huber delta (0 = none; NULL = none), obs_level [n_obs] (NULL = 0). */
int sqlm_set_problem(sqlm_ctx *ctx, int n_pose, const double *pose_q, const double *pose_t,
                     const uint8_t *pose_fixed, const double *intr, int n_pt, const double *pt,
                     int64_t n_obs, const int32_t *obs_pose, const int32_t *obs_pt, const double *obs_uv,
                     const double *obs_info, const double *obs_delta, const uint8_t *obs_level);

/* EdgeStereoSE3ProjectXYZ (types_six_dof_expmap.h:112-145): edges with
 * obs_ur[e] >= 0 become stereo edges, error (u, v, u_right) - cam_project
 * (float invz, float bf*invz, .cpp:150-157), information info*I3; the Huber
 * delta set for the edge applies to its 3-D chi2. pose_bf [n_pose] = mbf.
 * obs_ur = NULL (or all < 0) makes every edge mono again. Call after
 * sqlm_set_problem (which resets it). GBA stereo branch: g2oOptimizer.cc:247-281. */
int sqlm_set_stereo(sqlm_ctx *ctx, const double *obs_ur, const double *pose_bf);

/* EdgeLidarFlatPoint unary pose edges (types_six_dof_expmap.h:206-234), added
 * after the mono edges (g2oOptimizer.cc:1062-1070). Level 0, no kernel. */
int sqlm_set_lidar(sqlm_ctx *ctx, int64_t n, const int32_t *pose, const double *p_cam,
                   const double *p_world, const double *normal, const double *info);

/* e->setLevel / e->setRobustKernel for every mono edge (NULL delta = none). */
int sqlm_set_edge_level(sqlm_ctx *ctx, const uint8_t *level);
int sqlm_set_robust(sqlm_ctx *ctx, const double *delta);
int sqlm_set_lidar_level(sqlm_ctx *ctx, const uint8_t *level);
/* The kind of every LiDAR edge, kind [n_lid]: 0 EdgeLidarFlatPoint e = (T_cw p_w - p_c) . n,
 * 1 EdgeLidarCornerPoint e = |T_cw p_w - p_c| (types_six_dof_expmap.h:237-262; its normal is
 * ignored, as in sqlm_pose_refine_lidar); both 1-D with scalar information, no robust kernel,
 * numeric Jacobian (central differences through oplus, delta 1e-9). NULL = every edge flat.
 * Called after sqlm_set_lidar, like sqlm_set_lidar_level: sqlm_set_problem, sqlm_set_lidar
 * and sqlm_set_lidar_from_clouds reset every edge to flat. A value above 1 is
 * SQLM_ERR_INVALID_ARG, a call before a problem is set SQLM_ERR_STATE. */
int sqlm_set_lidar_kind(sqlm_ctx *ctx, const uint8_t *kind);

/* optimizer.initializeOptimization(level); optimizer.optimize(iterations).
 * user_lambda > 0 mirrors setUserLambdaInit. stop mirrors setForceStopFlag
 * (polled before each iteration and each trial; may be NULL).
 * *n_iter receives optimize()'s return value. */
int sqlm_optimize(sqlm_ctx *ctx, int level, int iterations, double user_lambda,
                  const volatile uint8_t *stop, sqlm_stats *stats, int *n_iter);

/* The whole g2oOptimizer::LocalBundleAdjustment schedule on the set problem
 * (g2oOptimizer.cc:923-1136): pass 1 optimize(5) with the set Huber kernels;
 * unless stopped, tag chi2 > 5.991 || depth <= 0 edges to level 1, drop the
 * kernels, pass 2 optimize(10); pass 3 optimize(20) with the LiDAR edges of either kind;
 * outlier[n_obs] receives the final erase tags. *ran = 0 when the stop flag
 * was already set (the reference returns before pass 1). */
int sqlm_local_ba(sqlm_ctx *ctx, const volatile uint8_t *stop, uint8_t *outlier,
                  sqlm_stats stats[3], int *ran);

/* g2oOptimizer::BundleAdjustment core (g2oOptimizer.cc:299-301): optimize
 * level 0 for `iterations`, kernels as set. */
int sqlm_global_ba(sqlm_ctx *ctx, int iterations, const volatile uint8_t *stop, sqlm_stats *stats,
                   int *n_iter);

/* Essential graph: g2oOptimizer::OptimizeEssentialGraph (g2oOptimizer.cc:1212-1534).
 * Vertices VertexSim3Expmap (types_seven_dof_expmap.h:48-94), one per keyframe in
 * g2o id order: Siw [n_kf][8] = qx qy qz qw tx ty tz s (Sim3 S_iw), fixed [n_kf]
 * (the loop keyframe), fix_scale = bFixScale (VertexSim3Expmap::_fix_scale).
 * Edges EdgeSim3 (:99-122) in insertion order: vertex 0 = edge_i, vertex 1 =
 * edge_j, measurement Sji [n_edge][8], error log(S_ji * S_i * S_j^-1),
 * information info [n_edge][49] row-major (NULL = identity, as the reference).
 * Numeric Jacobians (central differences, delta 1e-9, base_binary_edge.hpp:131-205). */
int sqlm_eg_set_problem(sqlm_ctx *ctx, int n_kf, const double *Siw, const uint8_t *fixed, int fix_scale,
                        int64_t n_edge, const int32_t *edge_i, const int32_t *edge_j, const double *Sji,
                        const double *info);
/* optimizer.setUserLambdaInit(user_lambda) (the reference: 1e-16); optimize(iterations). */
int sqlm_eg_optimize(sqlm_ctx *ctx, int iterations, double user_lambda, const volatile uint8_t *stop,
                     sqlm_stats *stats, int *n_iter);
int sqlm_eg_get_poses(sqlm_ctx *ctx, double *Siw);
/* e->chi2() from the last computed error (g2o semantics). */
int sqlm_eg_get_edge_chi2(sqlm_ctx *ctx, double *chi2);
/* The numeric Jacobians EdgeSim3::linearizeOplus computes at the current
 * estimates (BaseBinaryEdge, base_binary_edge.hpp:131-205: central differences
 * through oplus, delta 1e-9), on the GPU with the arithmetic of the optimizer's
 * k_eg_linearize: J [n_edge][2][7][7] row-major, [e][0] = d e / d S_i,
 * [e][1] = d e / d S_j, zero for a fixed vertex. Diagnostics / parity tests. */
int sqlm_eg_get_jacobians(sqlm_ctx *ctx, double *J);
/* The linear system of the most recent LM trial of the last sqlm_eg_optimize
 * (introspection for tests; no reference counterpart), in g2o's sign
 * convention (H + lambda I) dx = b with b = -J^T Omega e: the right-hand side
 * b [7 n_free] and the solution dx [7 n_free] the trial applied as
 * S <- Sim3(dx) S, both in free-vertex (hessianIndex, i.e. id) order whatever
 * layout the solver chose. SQLM_ERR_STATE before any trial has run. */
int sqlm_eg_get_last_step(sqlm_ctx *ctx, double *b, double *dx);
/* What the last sqlm_eg_optimize ran: out[0] = solve path, 1 band by cyclic
 * reduction + border complement, 2 arrow Cholesky, 3 dense Cholesky; out[1] =
 * n_free; out[2] = 112-row band blocks p (0 on the dense layout); out[3] =
 * border vertices; out[4] = nc, the padded order of the border complement,
 * out[5] = R, the padded count of cyclic-reduction right-hand sides, out[6] =
 * n_last, the rows factored in the complement's last block (all 0 off path
 * 1, n_last 0 without a border); out[7] = 1 if an information matrix was
 * given. SQLM_ERR_STATE before any optimize with a free vertex. */
int sqlm_eg_get_exec_info(sqlm_ctx *ctx, int out[8]);

/* Sim3 alignment of a loop candidate: g2oOptimizer::OptimizeSim3
 * (g2oOptimizer.cc:1560-1793), n_prob independent problems in one call (the
 * reference's call is n_prob = 1). One free VertexSim3Expmap S12 per problem
 * and, per surviving correspondence ("pair"), an EdgeSim3ProjectXYZ
 * e12 = obs1 - cam_map1(project(S12.map(X2c))) and an EdgeInverseSim3ProjectXYZ
 * e21 = obs2 - cam_map2(project(S12^-1.map(X1c))) (types_seven_dof_expmap.h:
 * 130-171), information info * I2, Huber delta (float)sqrt(th2), numeric
 * Jacobians (central differences through oplus, delta 1e-9). Schedule: stage 1
 * optimize(iters[0]); pairs with chi2 > th2 on either edge are removed
 * (pair_state 1, n_bad of them); fewer than 10 left: n_inliers = 0 and S12_out
 * = S12; otherwise a fresh initializeOptimization and optimize(n_bad > 0 ?
 * iters[1] : iters[2]); pairs failing the same check get pair_state 2, the
 * others (state 0) are counted in n_inliers. The two checks read the plain
 * chi2 of the last computed error (it may belong to a rejected trial).
 * The whole schedule of every problem runs in one kernel launch. */
#define SQLM_SIM3_TRACE_MAX 16
typedef struct sqlm_sim3_stats {
  int n_corr, n_bad;
  int iterations[2], trials[2], result[2]; /* per stage, as in sqlm_stats */
  double chi2_begin[2], chi2_end[2], lambda_end[2];
  int trace_len[2];
  double trace_chi2[2][SQLM_SIM3_TRACE_MAX];
  double trace_lambda[2][SQLM_SIM3_TRACE_MAX];
  int trace_trials[2][SQLM_SIM3_TRACE_MAX];
} sqlm_sim3_stats;
int sqlm_sim3_optimize(sqlm_ctx *ctx, int n_prob,
    const double *S12,            /* [n_prob][8] qx qy qz qw tx ty tz s, the ABI's Sim3 layout        */
    const double *intr1, const double *intr2,   /* [n_prob][4] fx fy cx cy of KF1 / KF2              */
    const uint8_t *fix_scale, const double *th2,/* [n_prob]                                            */
    const int64_t *pair_off,      /* [n_prob+1] CSR offsets into the pair arrays                       */
    const double *X1c, const double *X2c,       /* [n_pair][3] pMP1 in camera 1, pMP2 in camera 2    */
    const double *obs1, const double *obs2,     /* [n_pair][2] kpUn1.pt, kpUn2.pt                     */
    const double *info1, const double *info2,   /* [n_pair] invSigma2 of each keypoint's octave       */
    const int32_t iters[3],       /* NULL = {5, 10, 5}: stage 1, stage 2 if nBad>0, stage 2 otherwise  */
    double user_lambda,           /* 0 = g2o's computeLambdaInit (the reference); >0 for tests         */
    double *S12_out, int32_t *n_inliers, uint8_t *pair_state, sqlm_sim3_stats *stats);
/* Introspection of the last sqlm_sim3_optimize of the context (tests; no
 * reference counterpart); SQLM_ERR_STATE before any call.
 * chi2 [n_pair][2 checks][2 edges]: the e->chi2() values the check after
 * stage 1 and the final check read (e12, e21); a pair removed after stage 1
 * keeps its stage-1 values in check 1.
 * e [n_pair][2][2], J [n_pair][2][2][7]: error and numeric Jacobian of e12 and
 * e21 at the input S12.
 * The last LM trial of problem `prob`, in g2o's convention (H + lambda I) dx
 * = b with b = -J^T rho' Omega e: H [49] row-major (undamped), b [7], dx [7]
 * (zero if the damped system met a non-positive pivot); SQLM_ERR_STATE if the
 * problem ran no trial. */
int sqlm_sim3_get_pair_chi2(sqlm_ctx *ctx, double *chi2);
int sqlm_sim3_get_linearization(sqlm_ctx *ctx, double *e, double *J);
int sqlm_sim3_get_last_step(sqlm_ctx *ctx, int prob, double *H, double *b, double *dx);

/* Sim3 RANSAC of loop candidates: Sim3Solver (src/algorithm/Sim3Solver.cc),
 * every hypothesis of n_prob candidates in one launch. A problem follows the
 * conventions of sqlm_sim3_optimize: its pairs are the correspondences the
 * constructor keeps (:78-127), X1c / X2c are the two map points in their own
 * cameras (float values carried in doubles, rounded to float on entry), the
 * targets mvP1im1 / mvP2im2 are the library's own projections of those points
 * (FromCameraToImage, :543-562). max_err1 / max_err2 are mvnMaxError1/2 as
 * stored: the reference keeps 9.210 * sigma2 in a std::vector<size_t>, so the
 * caller truncates to an integer and the test err < maxErr compares a float
 * with that integer converted to float.
 * Hypothesis h of a problem with N pairs uses draws[h][0..2], the raw
 * DUtils::Random::RandomInt(0, size-1) values of :243, draws[h][i] in
 * [0, N-1-i]; the library maps them to pair indices as the swap-remove of
 * :236-256 does. Per hypothesis: ComputeSim3 (:319-458) and CheckInliers
 * (:462-490) in float, one rule for what the source leaves to OpenCV (products
 * and sums in double, one rounding per stored element), and the eigenvector of
 * step 4 by a fixed-sweep cyclic Jacobi iteration in double instead of
 * cv::eigen + cv::Rodrigues. A NaN or Inf transform has 0
 * inliers. Then, per problem, the sequential bookkeeping of iterate()
 * (:264-284) over the counts c_h with a running best b (initially 0):
 * flags[h] bit 0 = hypothesis h updates the best (c_h >= b), bit 1 = it also
 * returns (c_h > min_inliers); b carries on across returns. first_return is
 * the first returning hypothesis of the problem or -1, best the last one that
 * updated the best (-1 without hypotheses); both count from the problem's
 * first hypothesis. A problem with hypotheses and fewer than 3 pairs, a
 * negative threshold or a draw out of range is SQLM_ERR_INVALID_ARG. */
int sqlm_sim3_ransac(sqlm_ctx *ctx, int n_prob,
    const double *intr1, const double *intr2,   /* [n_prob][4] fx fy cx cy of KF1 / KF2              */
    const uint8_t *fix_scale,     /* [n_prob]                                                          */
    const int32_t *min_inliers,   /* [n_prob] mRansacMinInliers                                        */
    const int64_t *pair_off,      /* [n_prob+1] CSR offsets into the pair arrays                       */
    const double *X1c, const double *X2c,       /* [n_pair][3]                                        */
    const int32_t *max_err1, const int32_t *max_err2, /* [n_pair], >= 0                                */
    const int64_t *hyp_off,       /* [n_prob+1] CSR offsets into the per-hypothesis arrays             */
    const int32_t *draws,         /* [n_hyp][3]                                                        */
    int32_t *n_inliers,           /* [n_hyp] mnInliersi                                                */
    uint8_t *flags,               /* [n_hyp]                                                           */
    float *R12, float *t12, float *s12,         /* [n_hyp][9] row-major, [n_hyp][3], [n_hyp]          */
    int32_t *first_return, int32_t *best);      /* [n_prob]                                           */
/* Of the last sqlm_sim3_ransac of the context (SQLM_ERR_STATE before any):
 * mvbInliersi of hypothesis `hyp` of problem `prob`, mask [N] of 0 / 1; and the
 * three pair indices it drew with the float T12 and T21 (4x4 row-major) that
 * CheckInliers used (any of idx, T12, T21 may be NULL, not all). */
int sqlm_sim3_ransac_get_inliers(sqlm_ctx *ctx, int prob, int hyp, uint8_t *mask);
int sqlm_sim3_ransac_get_hypothesis(sqlm_ctx *ctx, int prob, int hyp, int32_t idx[3], float T12[16], float T21[16]);
/* Host only, no context. mRansacMaxIts after SetRansacParameters(probability,
 * min_inliers, max_iterations) on n_pair correspondences (:145-203), the
 * number of hypotheses of a problem: max(1, min(ceil(log(1-p) / log(1 -
 * pow((float)min_inliers / n_pair, 3))), max_iterations)), clamped in double
 * before the conversion to int; 1 if min_inliers == n_pair; 0 if n_pair <
 * min_inliers, where iterate() gives up at once (:214-218). */
int sqlm_sim3_ransac_max_its(int64_t n_pair, double probability, int min_inliers, int max_iterations);
/* Host only: the bookkeeping above on given counts; first_return / best may be NULL. */
int sqlm_sim3_ransac_scan(int64_t n_hyp, const int32_t *counts, int min_inliers, uint8_t *flags,
    int64_t *first_return, int64_t *best);
/* Host only: one hypothesis of one problem evaluated on the CPU by the source
 * text the kernel is compiled from (diagnostics and CPU tests). */
int sqlm_sim3_ransac_hypothesis_host(int n_pair, const double intr1[4], const double intr2[4], int fix_scale,
    const double *X1c, const double *X2c, const int32_t *max_err1, const int32_t *max_err2, const int32_t draws[3],
    int32_t idx[3], float R12[9], float t12[3], float *s12, float T12[16], float T21[16], uint8_t *mask,
    int32_t *n_inliers);

/* PnP RANSAC of relocalization candidates: PnPsolver
 * (src/algorithm/PnPsolver.cc), EPnP inside RANSAC, every hypothesis of n_prob
 * candidates in one launch and the Refine() of the record-breaking ones in a
 * second. A problem's pairs are the correspondences the constructor keeps
 * (:131-153): Xw the float world position, uv the undistorted keypoint, max_err
 * mvMaxError as stored (the float product mvSigma2 * th2, :226); intr is fu fv
 * uc vc. Hypothesis h of a problem with N pairs uses draws[h][0..3], the raw
 * DUtils::Random::RandomInt(0, size-1) values of :286, draws[h][i] in
 * [0, N-1-i]; the library maps them to pair indices as the swap-remove of
 * :281-297 does. Per hypothesis: compute_pose on the four points and
 * CheckInliers (:430-467) in the precisions written there. The scalar code of
 * EPnP is the reference's in double; what it hands to OpenCV is the library's
 * own, deterministic definition: fixed-sweep cyclic Jacobi for
 * the two symmetric eigenproblems, the inverse of CC from its orthogonal
 * columns, the reference's qr_solve for the 6x4, 6x3 and 6x5 systems, a
 * one-sided Jacobi SVD for R = U V^T. A NaN or Inf pose has 0 inliers.
 * Then, per problem, the bookkeeping of iterate() (:308-344) over the counts
 * c_h with a running best b (initially 0): flags[h] bit 0 = it qualifies
 * (c_h >= min_inliers), bit 1 = it is also a new best (c_h > b; a "record"),
 * bit 2 = it returns: it qualifies and the Refine() of the best mask so far,
 * i.e. of the latest record, found more than min_inliers inliers. first_return
 * is the first returning hypothesis or -1, best the last record or -1; both
 * count from the problem's first hypothesis. Tcw / n_refined are mRefinedTcw
 * (4x4 row-major float) and mnRefinedInliers at first_return (identity and 0
 * without one). A problem with hypotheses and fewer than 4 or fewer than
 * min_inliers pairs, or a draw out of range, is SQLM_ERR_INVALID_ARG. */
int sqlm_pnp_ransac(sqlm_ctx *ctx, int n_prob,
    const double *intr,           /* [n_prob][4] fu fv uc vc                                           */
    const int32_t *min_inliers,   /* [n_prob] mRansacMinInliers after SetRansacParameters              */
    const int64_t *pair_off,      /* [n_prob+1] CSR offsets into the pair arrays                       */
    const float *Xw,              /* [n_pair][3]                                                       */
    const float *uv,              /* [n_pair][2]                                                       */
    const float *max_err,         /* [n_pair]                                                          */
    const int64_t *hyp_off,       /* [n_prob+1] CSR offsets into the per-hypothesis arrays             */
    const int32_t *draws,         /* [n_hyp][4]                                                        */
    int32_t *n_inliers,           /* [n_hyp] mnInliersi                                                */
    uint8_t *flags,               /* [n_hyp]                                                           */
    double *R, double *t,         /* [n_hyp][9] row-major, [n_hyp][3]: mRi, mti                        */
    int32_t *first_return, int32_t *best,       /* [n_prob]                                           */
    float *Tcw, int32_t *n_refined);            /* [n_prob][16], [n_prob]                             */
/* Of the last sqlm_pnp_ransac of the context (SQLM_ERR_STATE before any):
 * mvbInliersi of hypothesis `hyp` of problem `prob`, mask [N] of 0 / 1; the
 * Refine() of a record's mask (SQLM_ERR_STATE for a hypothesis that is no
 * record: the reference never refines its mask); and diagnostics of a
 * hypothesis: the four pair indices, the 12x12 ut (rows by descending
 * eigenvalue) with its eigenvalues, the three beta vectors after Gauss-Newton
 * (the reference's N = 4, 2, 3 order), their reprojection errors and the
 * chosen candidate 0..2. Any output pointer but mask of get_inliers may be NULL. */
int sqlm_pnp_ransac_get_inliers(sqlm_ctx *ctx, int prob, int hyp, uint8_t *mask);
int sqlm_pnp_ransac_get_refined(sqlm_ctx *ctx, int prob, int hyp, double R[9], double t[3], uint8_t *mask,
    int32_t *n_inliers, double ut[144], double eig[12], double betas[12], double rep_err[3], int32_t *chosen);
int sqlm_pnp_ransac_get_hypothesis(sqlm_ctx *ctx, int prob, int hyp, int32_t idx[4], double ut[144], double eig[12],
    double betas[12], double rep_err[3], int32_t *chosen);
/* Host only, no context. SetRansacParameters(probability, min_inliers,
 * max_iterations, min_set, epsilon, .) on n_pair correspondences (:178-227):
 * *min_inliers_out = max((int)(n_pair * epsilon) as a float product,
 * min_inliers, min_set); the return value is mRansacMaxIts = max(1,
 * min(ceil(log(1-p) / log(1 - pow(max(epsilon, (float)that / n_pair), 3))),
 * max_iterations)), clamped in double before the conversion to int; 1 if that
 * count == n_pair; 0 if n_pair is below it, where iterate() gives up at once
 * (:257-261). */
int sqlm_pnp_ransac_max_its(int64_t n_pair, double probability, int min_inliers, int max_iterations, int min_set,
    float epsilon, int *min_inliers_out);
/* Host only: the bookkeeping above on given counts. refined[0 .. n_refined)
 * are the refined inlier counts of the records in their order; a record past
 * them (or refined == NULL) counts as a failed refine. flags, first_return,
 * best and n_record (the number of records) may be NULL. */
int sqlm_pnp_ransac_scan(int64_t n_hyp, const int32_t *counts, const int32_t *refined, int64_t n_refined,
    int min_inliers, uint8_t *flags, int64_t *first_return, int64_t *best, int64_t *n_record);
/* Host only: one hypothesis and one refine (EPnP on the pairs with in_mask != 0,
 * then CheckInliers) of one problem on the CPU by the source text the kernels
 * are compiled from. sweeps, if not NULL, replaces the Jacobi sweep counts of
 * the 3x3, the 12x12 and the polar factor where > 0 (the CPU test that keeps
 * the library's counts converged). The diagnostic outputs may be NULL. */
int sqlm_pnp_ransac_hypothesis_host(int n_pair, const double intr[4], const float *Xw, const float *uv,
    const float *max_err, const int32_t draws[4], const int32_t sweeps[3], int32_t idx[4], double R[9], double t[3],
    uint8_t *mask, int32_t *n_inliers, double ut[144], double eig[12], double betas[12], double rep_err[3],
    int32_t *chosen);
int sqlm_pnp_ransac_refine_host(int n_pair, const double intr[4], const float *Xw, const float *uv,
    const float *max_err, const uint8_t *in_mask, const int32_t sweeps[3], double R[9], double t[3], uint8_t *mask,
    int32_t *n_inliers, double ut[144], double eig[12], double betas[12], double rep_err[3], int32_t *chosen);

/* Motion-only bundle adjustment: g2oOptimizer::PoseOptimization
 * (g2oOptimizer.cc:385-679), n_prob independent problems in one call (Tracking's
 * call is n_prob = 1, Relocalization's candidates are a batch). One free
 * VertexSE3Expmap per problem and one EdgeSE3ProjectXYZOnlyPose per monocular
 * correspondence ("edge"): e = uv - cam_project(T_cw Xw), information info * I2,
 * analytic Jacobian, Huber delta (double)(float)sqrt(th2).
 * sqlm_pose_optimize runs the vision schedule. Fewer than 3 edges: n_inliers =
 * 0, the pose is returned unchanged, flags 0. Otherwise four rounds; round r
 * restarts from the INPUT pose, runs optimize(iters[r]) over the level-0 edges
 * (no such edge or iters[r] = 0: no trial, no error computed) and then
 * classifies every edge: a level-1 edge is evaluated at the round's estimate,
 * a level-0 edge keeps the error last computed (it may belong to a rejected
 * trial); (float)chi2 > (float)th2 puts the edge on level 1 (outlier), else on
 * level 0. Rounds 0-2 run with the Huber kernel, round 3 without; with fewer
 * than 10 edges only round 0 runs. The final classification reads the errors
 * in the same way and tests (double)(float)chi2 > th2: outlier[] holds its
 * flags, n_inliers = n_corr - their number; the pose is the last round's.
 * sqlm_pose_refine_lidar is the optional LiDAR stage (:560-641) and the final
 * classification after it: one optimize(iters) from the given pose (the
 * caller passes it after its own float round trip, SetPose / toSE3Quat) over
 * the mono edges with outlier_in = 0 plus every LiDAR edge on the same
 * vertex: kind 0 EdgeLidarFlatPoint e = (T_cw pw - pc) . n, kind 1
 * EdgeLidarCornerPoint e = |T_cw pw - pc| (lid_n ignored); scalar information,
 * no robust kernel, numeric Jacobians (central differences through oplus,
 * delta 1e-9). robust_on[p] = 1 keeps the Huber kernel on problem p's mono
 * edges (fewer than 10 correspondences never reach the round that removes it).
 * The whole schedule of every problem runs in one kernel launch. */
#define SQLM_POSE_STAGES 5 /* rounds 0-3, LiDAR stage */
#define SQLM_POSE_CHECKS 5 /* the checks after rounds 0-3, the final classification */
typedef struct sqlm_pose_stats {
  int n_corr, rounds; /* edges of the problem; rounds run (0, 1 or 4; 0 from a refine) */
  int n_bad[4];       /* level-1 edges after each round's check */
  int n_lidar, n_bad_final;
  int iterations[SQLM_POSE_STAGES], trials[SQLM_POSE_STAGES], result[SQLM_POSE_STAGES]; /* as in sqlm_stats */
  int active[SQLM_POSE_STAGES];                        /* level-0 edges the stage optimized (LiDAR edges included) */
  double chi2_begin[SQLM_POSE_STAGES], chi2_end[SQLM_POSE_STAGES], lambda_end[SQLM_POSE_STAGES];
} sqlm_pose_stats;
int sqlm_pose_optimize(sqlm_ctx *ctx, int n_prob,
    const double *pose_q, const double *pose_t, /* [n_prob][4] qx qy qz qw, [n_prob][3]: T_cw                */
    const double *intr,           /* [n_prob][4] fx fy cx cy                                           */
    const int64_t *obs_off,       /* [n_prob+1] CSR offsets into the edge arrays                       */
    const double *Xw,             /* [n_obs][3] pMP->GetWorldPos()                                     */
    const double *uv,             /* [n_obs][2] kpUn.pt                                                */
    const double *info,           /* [n_obs] mvInvLevelSigma2[kpUn.octave]                             */
    const int32_t iters[4],       /* NULL = {10, 10, 10, 10}                                           */
    double th2,                   /* 5.991 in the reference                                            */
    double user_lambda,           /* 0 = g2o's computeLambdaInit (the reference); >0 for tests         */
    double *pose_q_out, double *pose_t_out, int32_t *n_inliers, uint8_t *outlier, sqlm_pose_stats *stats);
int sqlm_pose_refine_lidar(sqlm_ctx *ctx, int n_prob,
    const double *pose_q, const double *pose_t, const double *intr, const int64_t *obs_off,
    const double *Xw, const double *uv, const double *info,
    const uint8_t *outlier_in,    /* [n_obs] 1 = level-1 edge (sqlm_pose_optimize's outlier)           */
    const uint8_t *robust_on,     /* [n_prob]                                                          */
    const int64_t *lid_off,       /* [n_prob+1] CSR offsets into the LiDAR arrays                      */
    const uint8_t *lid_kind,      /* [n_lid] 0 flat, 1 corner                                          */
    const double *lid_pc, const double *lid_pw, const double *lid_n, /* [n_lid][3] point in the camera
                                     frame, its nearest map point in the world, the flat point's normal */
    const double *lid_info,       /* [n_lid]                                                           */
    const int32_t *iters,         /* one value >= 1, NULL = 10                                         */
    double th2, double user_lambda,
    double *pose_q_out, double *pose_t_out, int32_t *n_inliers, uint8_t *outlier, sqlm_pose_stats *stats);
/* Introspection of the context's last sqlm_pose_optimize / sqlm_pose_refine_lidar
 * (tests; no reference counterpart); SQLM_ERR_STATE before any call.
 * chi2 [n_obs][SQLM_POSE_CHECKS]: the e->chi2() value each check read (a check
 * that did not run leaves 0; a refine fills the last column only).
 * e [n_obs][2], J [n_obs][2][6] of the mono edges and lid_e [n_lid], lid_J
 * [n_lid][6] of the LiDAR edges (refine only) at the input pose; any may be NULL.
 * The last LM trial of problem `prob`, in g2o's convention (H + lambda I) dx
 * = b with b = -J^T rho' Omega e: H [36] row-major (undamped), b [6], dx [6]
 * (zero if the damped system met a non-positive pivot); SQLM_ERR_STATE if the
 * problem ran no trial. */
int sqlm_pose_get_edge_chi2(sqlm_ctx *ctx, double *chi2);
int sqlm_pose_get_linearization(sqlm_ctx *ctx, double *e, double *J, double *lid_e, double *lid_J);
int sqlm_pose_get_last_step(sqlm_ctx *ctx, int prob, double *H, double *b, double *dx);

/* LiDAR association: the kd-tree search of g2oOptimizer.cc:978-1073 / :560-630 as an exact
 * brute-force 1-NN on the device.
 * World transform (pcl::transformPointCloud with an Eigen::Affine3d whose entries are the
 * float entries of Twc, :985-1010): per coordinate out = (float)(((m0 x + m1 y) + m2 z) + m3)
 * in double, no FMA. Distance: FLANN's L2_Simple<float>, d = query - map per coordinate in
 * float, ((dx dx) + dy dy) + dz dz in float, no FMA. The neighbour is the exact minimum over
 * the concatenated map (cloud order, then point order); equal float distances resolve to the
 * lowest global index (the reference's tie order depends on FLANN's traversal and is
 * unpinned). A query is accepted when (double)d2 < dist_sq_threshold, strictly (:1045).
 * An empty map gives index -1, distance +inf, point 0 and no pair for every query (the
 * reference would crash). Non-finite coordinates, and distances that overflow a float, are
 * undefined behaviour of the search (PCL asserts on them); no memory is touched out of bounds.
 * Twc is the float 4x4 the caller computed, Converter::toCvMat(estimate).inv(): cv::Mat::inv()
 * is not restated here. */
int sqlm_lidar_associate(sqlm_ctx *ctx,
    int n_map_clouds, const int64_t *map_off /*[n_map_clouds+1]*/,
    const float *map_xyz /*[n_map][3], each cloud in its own sensor frame*/,
    const float *map_Twc /*[n_map_clouds][16] row-major, NULL = the clouds are already in the world*/,
    int64_t n_query, const float *query_xyz /*[n_query][3]*/, const float *query_Twc /*[16]*/,
    double dist_sq_threshold,
    int32_t *nn_index /*[n_query] global map index, -1 on an empty map*/,
    float *nn_sq_dist /*[n_query]*/, float *nn_xyz /*[n_query][3] the world map point*/,
    uint8_t *accepted /*[n_query]*/, int64_t *n_pairs);   /* any output may be NULL */

/* The same search, then the accepted pairs become the context's EdgeLidarFlatPoint edges on
 * pose `pose_index` (replacing any set before), exactly as sqlm_set_lidar with the pairs in
 * query order would: p_cam = the query's sensor-frame xyz, p_world = the transformed float map
 * point, normal = the query's normal, all widened, information `info` (:1062-1070); n_pairs
 * out. For the call between pass 2 and pass 3. SQLM_ERR_STATE before sqlm_set_problem;
 * pose_index out of range or naming a fixed pose is SQLM_ERR_INVALID_ARG. */
int sqlm_set_lidar_from_clouds(sqlm_ctx *ctx, int32_t pose_index,
    int n_map_clouds, const int64_t *map_off, const float *map_xyz, const float *map_Twc,
    int64_t n_query, const float *query_xyz, const float *query_Twc,
    const float *query_normal /*[n_query][3]*/, double info, double dist_sq_threshold, int64_t *n_pairs);

/* Local BA pass 3 with both kinds of LiDAR edge (g2oOptimizer.cc:1034-1107): n_sets searches,
 * each exactly that of sqlm_set_lidar_from_clouds (same transform, distance, tie rule and
 * strict threshold) on its own map and queries. The context's LiDAR edges become set 0's
 * accepted pairs in query order, then set 1's, and so on -- the reference inserts the flat
 * edges, then the corner edges -- each with its set's kind (0 flat, 1 corner) and info;
 * edges set before are replaced. query_normal may be NULL for a corner set. n_pairs [n_sets]
 * (may be NULL) receives the pairs of each set. With more than one set, a set with an empty
 * map or without queries contributes no edge and launches nothing; sqlm_lidar_get_exec_info
 * describes the last set that launched a search. n_sets = 1 with kind 0 is
 * sqlm_set_lidar_from_clouds. Errors as there; a kind other than 0 or 1 is
 * SQLM_ERR_INVALID_ARG, and no set reaches the device unless all are valid. */
typedef struct sqlm_lidar_set {
  int32_t kind;
  int32_t n_map_clouds;
  const int64_t *map_off;    /* [n_map_clouds+1] */
  const float *map_xyz;      /* [n_map][3] */
  const float *map_Twc;      /* [n_map_clouds][16], NULL = world */
  int64_t n_query;
  const float *query_xyz;    /* [n_query][3] */
  const float *query_Twc;    /* [16] */
  const float *query_normal; /* [n_query][3] */
  double info;
  double dist_sq_threshold;
} sqlm_lidar_set;
int sqlm_set_lidar_from_cloud_sets(sqlm_ctx *ctx, int32_t pose_index, int n_sets, const sqlm_lidar_set *sets,
                                   int64_t *n_pairs);

/* What the context's last association ran (tests and tools; no reference counterpart):
 * out[0] = n_map, out[1] = n_query, out[2] = map segments searched by separate workgroups
 * (0: empty map or no query, nothing launched), out[3] = map points per LDS tile T,
 * out[4] = n_pairs, out[5] = queries per workgroup W, out[6..7] = 0. SQLM_ERR_STATE before
 * any association. */
int sqlm_lidar_get_exec_info(sqlm_ctx *ctx, int out[8]);

/* LiDAR flat-feature extraction: the flat-point path of Frame::lidarProcess (Frame.cc:1243;
 * CalculateRingAndTime :473, PointToImage :548, PrepareRing_flat :704, PrepareSubregion_flat
 * :797, ExtractFeaturePoints :834 with using_flat_point = 1, using_sharp_point = 0) and the
 * final transform of the clouds (:461-466), for a batch of sweeps. What a sweep yields depends
 * on that sweep and the parameters alone. All arithmetic is IEEE, no FMA, in the precision and
 * order the reference writes it (C++'s usual conversions); the reference's float atan / atan2 /
 * sqrt calls are f(x) = (float)F((double)x) with F = sqlm_libm.h's atan / atan2 /
 * the IEEE sqrt. Whether that equals glibc's atanf / atan2f on every input is unpinned (the
 * reference cannot be built against); sqrt is exact either way. PI is M_PI.
 *
 * Per point i of a sweep (x, y, z float):
 *   dropped when a coordinate is not finite (removeNaNFromPointCloud);
 *   s = sqrtf(x x + y y), ang = (float)((double)(atanf(z / s) * 180.0f) / PI);
 *   ring = ang >= -8.83 ? int((double)(2.0f - ang) * 3.0 + 0.5)
 *                       : 32 + int((-8.83 - (double)ang) * 2.0 + 0.5);
 *   dropped when ang is NaN (x = y = z = 0; the reference's conversion is undefined) or ring is
 *   outside [0, 63]. The other points are the kept points, in input order.
 *   azi = -atan2f(y, x).
 * Per sweep: first / last = the first and last kept point;
 *   startOri = (float)((double)azi[first] + PI), endOri = (float)((double)azi[last] + 3.0 PI),
 *   then endOri = (float)(endOri - 2 PI) when endOri - startOri (float) > 3 PI, else
 *   (float)(endOri + 2 PI) when it is < PI.
 *   For a kept point, A(i) is the reference's not-yet-passed branch (:568-572): a = azi;
 *   a < startOri - PI/2 -> a = (float)(a + 2 PI); else a > startOri + PI 3/2 -> a = (float)(a - 2 PI).
 *   half = the lowest kept i with A(i) - startOri (float) > PI. A kept point i <= half uses
 *   a = A(i); a later one the passed branch (:577-582) against endOri. halfPassed is thus a
 *   minimum over indices, not a loop state.
 *   col = (int((double)(a - startOri) / (2 PI) * col_num) + col_num) % col_num, row = ring;
 *   a point with row >= row_num or col outside [0, col_num) claims no cell.
 * Range image: a cell's occupant is the claiming point of least d = sqrtf((x x + y y) + z z),
 *   the lowest input index among equal d (:617 is strict). A row's scan order is arrival order:
 *   the cell's index is the rank, among the row's occupied cells, of the lowest input index
 *   that claims the cell; the scan point at that index is the cell's occupant.
 * A row (ring) r with n scan points is processed when ring_enabled[r] and
 *   n - 1 > 2 max(num_curvature_regions_flat, num_curvature_regions_corner) (:846-854). With
 *   c = num_curvature_regions_flat, the mask is the OR over i in [c, n - c) of the range each i
 *   writes (:714-736): [i - c, i] or [i + 1, i + c]. Subregion j = 0 .. num_scan_subregions - 1
 *   is [sp, ep] as :1053-1056, skipped when ep <= sp. Inside one, the curvature of scan point i
 *   is :808-826 in float, the sums in j order; a neighbourhood int(25.0 / d + 0.5) + 1 that is
 *   NaN or not below 2^30 takes the fallback like any that does not fit the scan. The
 *   subregion's candidates are ordered by (curvature bits, index): non-negative floats order as
 *   their bits, so this is std::sort's order of the pairs and independent of the algorithm.
 * A candidate in that order is rejected as masked, then when not (double)curv < surf_curv_th;
 *   else cw = int((double)d 0.01 / (deg_diff / 180.0 PI (double)d) + 0.5) (0 when NaN, at most
 *   8), the search points are gathered in the order of :1088-1138 (the gather does not wrap
 *   around the columns), fewer than 5 reject; the near points are those with
 *   (double)CalcSquaredDiff < max_sq_dis, in gather order, at most 3 (2 cw + 1) = 51.
 * Plane fit: the least-squares solution of A n = -1 (rows = near points, widened) by a
 *   column-pivoted Householder QR in double with this fixed order. For k = 0, 1, 2: the squared
 *   norm of every remaining column over rows k.. (summed in row order) is taken, the largest
 *   becomes column k (the first of equals); when it is not above 1e-24 times the largest initial
 *   squared column norm the fit is degenerate. beta = -sign(a_kk) sqrt(norm2) (sign(0) = +),
 *   v = column / (a_kk - beta) below the diagonal, tau = (beta - a_kk) / beta; every later
 *   column and the right side get w = tau (a_k + sum_s v_s a_s), a_k -= w, a_s -= v_s w in row
 *   order. Back substitution x2 = c2 / r22, x1 = (c1 - r12 x2) / r11,
 *   x0 = ((c0 - r01 x1) - r02 x2) / r00, unpermuted. Fewer than 3 near points are degenerate
 *   too. Eigen's colPivHouseholderQr is not restated: it differs in rounding, and on a
 *   rank-deficient neighbourhood it returns a minimum-norm-like answer where this rejects.
 *   nrm = sqrt((x0 x0 + x1 x1) + x2 x2), d0 = 1 / nrm, n = x / nrm; the plane is invalid when
 *   fabs(((n0 X + n1 Y) + n2 Z) + d0) > 0.1 for a near point (:1196-1205). The normal is
 *   (float)n.
 * Pick: the valid candidates of a subregion in sorted order; the first max_surf_less_flat are
 *   less-flat points and the first max_surf_flat of those are flat points too. The reference's
 *   break only stops early: every candidate after the one that fills the less-flat cap (with
 *   a cap of 0: the first valid candidate and every later one) has reason OVER_CAP whatever
 *   its own evaluation would give.
 * Output order is the reference's push order: ring, subregion, sorted rank. Every output
 *   point p and every normal n, as a point, translation included (:465-466 do that), goes
 *   through `extrinsic` as sqlm_lidar_associate defines pcl::transformPointCloud:
 *   (float)(((m0 x + m1 y) + m2 z) + m3) in double per coordinate. NULL is the identity and
 *   copies the floats.
 * A sweep without a kept point gives empty outputs (the reference would read points[0]).
 * Coordinates whose squares overflow a float are undefined; no memory is touched out of bounds.
 *
 * Limits: row_num in [1, 128], col_num in [1, 4096], the neighbourhood half-width
 * int(0.01 / (deg_diff / 180 PI) + 0.5) + 1 <= 8, using_sharp_point = 0 (the corner branch,
 * :861-1038, is sqlm_lidar_features_all's, below): beyond them
 * SQLM_ERR_UNSUPPORTED, before the device is touched. num_scan_subregions < 1,
 * num_curvature_regions_flat < 1, a negative corner width or cap, deg_diff <= 0 and a sweep
 * of 2^31 points or more are SQLM_ERR_INVALID_ARG. */
#define SQLM_LF_MAX_ROWS 128
#define SQLM_LF_MAX_COLS 4096
#define SQLM_LF_MAX_HALF_WIDTH 8
#define SQLM_LF_NONE 0      /* no candidate: the scan point lies in no processed subregion */
#define SQLM_LF_MASKED 1
#define SQLM_LF_CURVATURE 2
#define SQLM_LF_FEW_SEARCH 3 /* fewer than 5 search points */
#define SQLM_LF_DEGENERATE 4 /* fewer than 3 near points or a pivot below the tolerance */
#define SQLM_LF_PLANE_INVALID 5
#define SQLM_LF_OVER_CAP 6
#define SQLM_LF_PICKED 7
typedef struct sqlm_lidar_feat_params {
  int32_t row_num, col_num;
  int32_t num_scan_subregions;
  int32_t num_curvature_regions_flat, num_curvature_regions_corner;
  int32_t max_surf_flat, max_surf_less_flat;
  int32_t using_sharp_point;
  double surf_curv_th, max_sq_dis, deg_diff;
  uint8_t ring_enabled[SQLM_LF_MAX_ROWS]; /* ring r (0-based) takes part in :1041-1045 */
} sqlm_lidar_feat_params;

/* The intermediate state of a call (tests and tools). Caller-allocated; any pointer may be
 * NULL. n = sweep_off[n_sweep], S = n_sweep row_num. Scan points are numbered sweep by sweep,
 * row by row, in scan order: row (s, r) owns [scan_off[s row_num + r], scan_off[.. + 1]). */
typedef struct sqlm_lidar_feat_state {
  int32_t *ring;        /* [n] ring of every input point, -1 for a dropped point */
  int64_t *scan_off;    /* [S + 1] */
  int32_t *scan_src;    /* [n] (first scan_off[S] used) the occupant's index within its sweep */
  int32_t *scan_col;    /* [n] its column; its row is the scan's */
  int32_t *image_index; /* [S][col_num] the cell's index within its row's scan, -1 = unoccupied */
  uint8_t *mask;        /* [n] the ring mask, 0 on a row that is not processed */
  float *curvature;     /* [n] 0 outside the processed subregions */
  int32_t *neighbours;  /* [n] the curvature half-width used, 0 outside */
  int32_t *sorted;      /* [n] at position row start + sp + k: the in-scan index of the subregion's rank k; -1 outside */
  uint8_t *reason;      /* [n] SQLM_LF_* of every scan point */
} sqlm_lidar_feat_state;

/* Outputs are packed sweep after sweep: sweep s owns [flat_off[s], flat_off[s + 1]) of the
 * flat arrays and likewise for less-flat; every array has room for n entries. */
int sqlm_lidar_features(sqlm_ctx *ctx, int n_sweep, const int64_t *sweep_off /*[n_sweep+1]*/,
    const float *xyz /*[n][3]*/, const sqlm_lidar_feat_params *params,
    const double *extrinsic /*[16] row-major, NULL = identity*/,
    int64_t *flat_off /*[n_sweep+1]*/, float *flat_xyz /*[n][3]*/, float *flat_normal /*[n][3]*/,
    int64_t *less_off /*[n_sweep+1]*/, float *less_xyz /*[n][3]*/, float *less_normal /*[n][3]*/,
    int32_t *less_row_col /*[n][2]*/);
/* The same text compiled for the CPU; no context, no device. `state` may be NULL. */
int sqlm_lidar_features_host(int n_sweep, const int64_t *sweep_off, const float *xyz,
    const sqlm_lidar_feat_params *params, const double *extrinsic,
    int64_t *flat_off, float *flat_xyz, float *flat_normal,
    int64_t *less_off, float *less_xyz, float *less_normal, int32_t *less_row_col,
    sqlm_lidar_feat_state *state);
/* The state of the context's last sqlm_lidar_features, read back from the device; the arrays
 * are sized by that call's arguments. SQLM_ERR_STATE before any call. */
int sqlm_lidar_features_get_state(sqlm_ctx *ctx, sqlm_lidar_feat_state *state);
/* out[0] = SQLM_LF_MAX_ROWS, out[1] = SQLM_LF_MAX_COLS, out[2] = kernel launches of the last
 * call (0: nothing reached the device), out[3] = the largest subregion, out[4] = candidates
 * (scan points in processed subregions), out[5] = candidates evaluated before the caps stopped
 * their subregions (in steps of 64 per subregion), out[6] = less-flat points picked,
 * out[7] = SQLM_LF_MAX_HALF_WIDTH. ctx may be NULL (the limits alone). */
int sqlm_lidar_features_info(const sqlm_ctx *ctx, int32_t out[8]);
/* Test probe of sqlm_libm.h's atan / atan2 as this library compiled them: out[i] =
 * atan2 of (y[i], x[i]), or atan of y[i] where x is NULL. */
int sqlm_lidar_feat_trig_probe(int64_t n, const double *y, const double *x, double *out);

/* ---- LiDAR corner-feature extraction of a fusion frame ----
 * The corner branch of Frame::ExtractFeaturePoints (src/data_structure/Frame.cc:861-1038 with
 * PrepareRing_corner :647 and PrepareSubregion_corner :756; line numbers are that file's), beside
 * the flat branch above: sqlm_lidar_features_all runs both on one range image. Ring assignment,
 * columns, cell occupants, scan order and image_index are those of sqlm_lidar_features. Float
 * and double expressions are evaluated as written with C++'s usual conversions, no FMA;
 * acos / sin / cos / atan2 are sqlm_libm.h's.
 *
 * Cell state (int32 per range-image cell): -3 when unoccupied; -1 (ground) when the final
 *   occupant has (double)z < ground_z_bound; else 0. :596-626 rewrite the state at every change
 *   of occupant, so it follows the occupant of least distance and is order-free.
 * Corner rings: ring r (0-based) takes part when corner_ring_enabled[r], which the caller
 *   builds as lower_ring_num_sharp_point <= r + 1 && r < upper_ring_num_sharp_point, and when
 *   its scan passes the short-scan test of the flat path (:846-854, the same min over both
 *   widths).
 * Corner mask (:647-701), c = num_curvature_regions_corner, for i in [c, n - c): the two
 *   depth-jump rules of the flat mask with c ([i - c, i] or [i + 1, i + c]); only when neither
 *   fired for i: mask[i] = 1 when (double)diff_next2 > 0.0002 (double)dis2 &&
 *   (double)diff_prev2 > 0.0002 (double)dis2, with diff_next2 = CalcSquaredDiff(p_i, p_i+1),
 *   diff_prev2 = CalcSquaredDiff(p_i, p_i-1), dis2 = (x x + y y) + z z in float. The mask is
 *   the OR of every i's writes.
 * Corner curvature (:766-780): half-width c always; dx = -(float)(2c) x, then
 *   dx += x[i + j] + x[i - j] for j = 1 .. c (likewise y, z), curvature =
 *   ((dx dx + dy dy) + dz dz) / (float)(2c). Subregion j is [sp, ep] of :871-874 (the flat
 *   formula with c), skipped when ep <= sp. Its candidates are sorted ascending on
 *   (curvature bits, index) and walked from the highest rank down: among equal curvatures the
 *   higher index comes first.
 * Edge predicate between two occupied, non-ground cells with occupants p1, p2 (:963-975), in
 *   double: n = sqrt((x x + y y) + z z), dot = (x1 x2 + y1 y2) + z1 z2 (Eigen's own summation
 *   order is unpinned); d1 = (float)max(n1, n2), d2 = (float)min(n1, n2);
 *   alpha = (float)acos(dot / (n1 n2));
 *   angle = (float)atan2((double)(d2 sinf(alpha)), (double)(d1 - d2 cosf(alpha))) with
 *   sinf(a) = (float)sin((double)a), cosf likewise, the products and the difference in float.
 *   The edge exists when angle > 1.0f; a NaN (an acos argument that rounds above 1) gives no
 *   edge. The predicate is bit-symmetric in its cells.
 * Neighbourhood (:929-957), directed, six distinct offsets (row, col) numbered
 *   0 (-1, 0), 1 (1, 0), 2 (0, -1), 3 (0, 1), 4 (-1, -1), 5 (1, -1). A row outside
 *   [0, row_num) has no target; a column < 0 becomes col_num - 1, one >= col_num becomes 0.
 *   A cell's edge mask has bit k set when offset k has a target, both cells are occupied and
 *   not ground, and the edge exists.
 * Growth from a seed cell of state 0: S = the cells reachable from the seed along edge-mask
 *   bits through cells whose state is 0 when the growth starts, the seed included (the set does
 *   not depend on the traversal). lineCount = the number of distinct rows among S \ {seed}
 *   (:980 flags the row of every pushed cell, never the seed's own push). lineCount >= 3: every
 *   cell of S gets the current label and the label counter, 1 at the start of each sweep, goes
 *   up by one. Otherwise every cell of S becomes -2.
 * Walk (:861-1037), per sweep, corner rings ascending, subregions ascending, ranks descending,
 *   num = 0 per subregion. Per candidate: cell state -1 -> GROUND. Else mask set -> MASKED;
 *   else !((double)curvature > sharp_curv_th) -> CURVATURE. Else, if the cell state is 0, grow
 *   from it; if the state is then < 1 -> UNSTABLE (whether the -2 is this growth's or an
 *   earlier one's; a cell an earlier seed labelled passes without growing). Else, if
 *   num < max_corner_less_sharp, the point is PICKED: a less-sharp point with its cell's
 *   label, a sharp point too if num < max_corner_sharp, ++num; with a cap of 0 it is OVER_CAP.
 *   If then num >= max_corner_less_sharp the subregion stops: every lower rank is OVER_CAP
 *   whatever its own evaluation would give, and is not grown.
 * Outputs per sweep in push order, through `extrinsic` as the flat clouds: sharp xyz;
 *   less-sharp xyz, label (what :1016 leaves in the point's intensity) and (row, col).
 *   less_sharp_ and feature_state are not provided (nothing outside that loop reads them), nor
 *   is the label :1016 leaves in the intensity of flat points inside a picked segment.
 * The flat branch reads point_state only as != -3 and the corner branch never makes or
 *   removes a -3, so the flat outputs do not depend on the corner branch. */
#define SQLM_LC_NONE 0
#define SQLM_LC_GROUND 1
#define SQLM_LC_MASKED 2
#define SQLM_LC_CURVATURE 3
#define SQLM_LC_UNSTABLE 4
#define SQLM_LC_OVER_CAP 5
#define SQLM_LC_PICKED 6
typedef struct sqlm_lidar_corner_params {
  int32_t max_corner_sharp, max_corner_less_sharp;
  double sharp_curv_th, ground_z_bound;
  uint8_t corner_ring_enabled[SQLM_LF_MAX_ROWS];
} sqlm_lidar_corner_params;

/* The intermediate state of the corner branch. Caller-allocated; any pointer may be NULL.
 * Scan points are numbered as in sqlm_lidar_feat_state, whose scan_off applies. */
typedef struct sqlm_lidar_corner_state {
  int32_t *cell_state; /* [S][col_num] final: -3, -2, -1, 0 or a label */
  uint8_t *mask;       /* [n] the corner mask, 0 on a row that takes no part */
  float *curvature;    /* [n] 0 outside the corner subregions */
  int32_t *sorted;     /* [n] as sqlm_lidar_feat_state.sorted, ascending rank */
  uint8_t *reason;     /* [n] SQLM_LC_* */
  uint8_t *edge;       /* [S][col_num] the 6-bit edge mask */
  float *angle;        /* [S][col_num][6] the angle of every offset; NaN where the offset has no
                          target or either cell is unoccupied or ground */
} sqlm_lidar_corner_state;

/* Both branches on one upload and one range image. The flat outputs are those of
 * sqlm_lidar_features; when all seven are NULL the flat stage is skipped. params->using_sharp_point
 * is ignored. corner == NULL runs no corner stage (the six corner outputs are not touched) and
 * equals sqlm_lidar_features bit for bit. The corner arrays have room for n entries, the offsets
 * for n_sweep + 1. Limits as sqlm_lidar_features; with corner != NULL,
 * num_curvature_regions_corner < 1, a negative cap and a non-finite threshold or ground bound
 * are SQLM_ERR_INVALID_ARG, reported before the device is touched. */
int sqlm_lidar_features_all(sqlm_ctx *ctx, int n_sweep, const int64_t *sweep_off, const float *xyz,
    const sqlm_lidar_feat_params *params, const sqlm_lidar_corner_params *corner,
    const double *extrinsic,
    int64_t *flat_off, float *flat_xyz, float *flat_normal,
    int64_t *less_off, float *less_xyz, float *less_normal, int32_t *less_row_col,
    int64_t *sharp_off /*[n_sweep+1]*/, float *sharp_xyz /*[n][3]*/,
    int64_t *less_sharp_off /*[n_sweep+1]*/, float *less_sharp_xyz /*[n][3]*/,
    int32_t *less_sharp_label /*[n]*/, int32_t *less_sharp_row_col /*[n][2]*/);
/* The same text on the CPU; either state may be NULL. */
int sqlm_lidar_features_all_host(int n_sweep, const int64_t *sweep_off, const float *xyz,
    const sqlm_lidar_feat_params *params, const sqlm_lidar_corner_params *corner,
    const double *extrinsic,
    int64_t *flat_off, float *flat_xyz, float *flat_normal,
    int64_t *less_off, float *less_xyz, float *less_normal, int32_t *less_row_col,
    int64_t *sharp_off, float *sharp_xyz, int64_t *less_sharp_off, float *less_sharp_xyz,
    int32_t *less_sharp_label, int32_t *less_sharp_row_col,
    sqlm_lidar_feat_state *flat_state, sqlm_lidar_corner_state *corner_state);
/* The state of the context's last sqlm_lidar_features_all, read back from the device; either
 * may be NULL. The angle array is recomputed by a launch of its own. corner_state after a call
 * without a corner stage is SQLM_ERR_STATE. */
int sqlm_lidar_features_all_get_state(sqlm_ctx *ctx, sqlm_lidar_feat_state *flat_state,
    sqlm_lidar_corner_state *corner_state);
/* Of the last sqlm_lidar_features_all: out[0] = kernel launches, out[1] = seeds grown,
 * out[2] = cells labelled, out[3] = cells set unstable, out[4] = the largest segment (cells of
 * one growth), out[5] = the most BFS levels of one growth, out[6] = less-sharp points,
 * out[7] = sharp points. */
int sqlm_lidar_features_all_info(const sqlm_ctx *ctx, int32_t out[8]);
/* Test probe of sqlm_libm.h's acos (which = 0), sin (1) and cos (2) as this library compiled them. */
int sqlm_lidar_corner_trig_probe(int64_t n, int which, const double *x, double *out);
/* Test probe of the edge predicate: out[i] = the float angle of p1[i], p2[i] (float xyz). */
int sqlm_lidar_corner_angle_probe(int64_t n, const float *p1, const float *p2, float *out);

/* ---- LiDAR depth image and keypoint depth association of a fusion frame ----
 * The other LiDAR half of the reference's Frame constructor
 * (src/data_structure/Frame.cc:290-313 and :333-408; line numbers below are that file's): the
 * sweep is projected into the double depth image Depthimg_, and every ORB keypoint gets a
 * class_id and an mvDepth from an 8 x 14 pixel patch of that image. A batch of frames shares
 * rows, cols, the 3x4 `intrinsic` and the 4x4 `extrinsic` (double, row-major); frame f owns
 * the points [sweep_off[f], sweep_off[f+1]) of xyz and the keypoints [key_off[f], key_off[f+1])
 * of key_xy (mvKeys[i].pt, the distorted coordinates). The reference's loops overwrite, break
 * and sort; each is restated as a rule that does not depend on an order of evaluation, and
 * the arithmetic is IEEE in the order written here, nothing contracted into an FMA.
 *
 * Projection (:293-313). M = intrinsic extrinsic is formed once on the host,
 *   M[r][c] = ((a0 b0 + a1 b1) + a2 b2) + a3 b3 (a = row r of intrinsic, b = column c of
 *   extrinsic). Per point, (x, y, z) widened to double: zu, zv, zw = rows 0, 1, 2 of M applied
 *   to (x, y, z, 1) and depth = row 2 of extrinsic applied to it, each
 *   ((m0 x + m1 y) + m2 z) + m3, as sqlm_lidar_associate defines pcl::transformPointCloud.
 *   How Eigen groups or fuses intrinsicMatrix*extrinsicMatrix*P_lidar is unpinned (the
 *   reference cannot be built against).
 *   u = int(zu / zw), v = int(zv / zw), truncating toward zero: a quotient in (-1, 0) lands
 *   on 0. The point writes pixel (v, u) iff x, y, z are finite, x > SQLM_LD_MIN_X (:295 and
 *   :308 together: x == 1 passes the first test and fails the second), and the quotients qu,
 *   qv satisfy -1 < qu < cols and -1 < qv < rows, which is 0 <= u <= cols - 1 and
 *   0 <= v <= rows - 1 for every quotient that converts to int32 and false for NaN, the
 *   infinities and everything beyond int32 (the reference's int() of those is undefined; on
 *   x86-64 it gives INT_MIN, which fails its bound test, so dropping them gives the same
 *   image). A point with zw < 0 whose quotients land inside writes its negative depth, as
 *   the reference does. A point with a non-finite coordinate is dropped (the reference's
 *   cloud has been through removeNaNFromPointCloud by then, or would convert a NaN).
 * Image. A pixel's occupant is the writing point of greatest input index (the loop
 *   overwrites), its value that point's depth; unwritten pixels hold 0.0. n_written counts
 *   writing points (depthpixel_num, :310), n_occupied distinct written pixels.
 * min_v (:341-353) = the lowest row holding a pixel > 0.0 (as double), 0 when there is none:
 *   a negative depth does not count, a depth in (0, 1) does.
 * The patch's "seen" test (:366-367) reads the double into a uchar. With
 *   t = (int32)trunc(depth) when |depth| < 2^31, else INT_MIN, a cell is seen iff
 *   (t & 255) != 0: what cvttsd2si followed by taking the low byte gives. The C++ conversion
 *   is defined on (-1, 256) only; outside that range this is a rule of ours and unpinned. So
 *   a return with depth in [0, 1) or [256, 257) is invisible to the patch (yet counts for
 *   min_v when positive), and a depth of -3.2 is seen.
 * Per keypoint (:355-401), pt = (px, py) float: py < (float)min_v gives class 0, depth -1.0f.
 *   Otherwise the cells of dx = -SQLM_LD_HALF_W .. SQLM_LD_HALF_W - 1 (outer loop),
 *   dy = -SQLM_LD_HALF_H .. SQLM_LD_HALF_H - 1 (inner) are row = int(py + (float)dy),
 *   col = int(px + (float)dx): the add in float, the conversion truncating toward zero (a sum
 *   in (-1, 0) is cell 0, and px = 3.5 reaches column 0 with dx = -4 and with dx = -3). A cell
 *   outside the image (a sum that is NaN, <= -1 or >= the size) is empty; the reference reads
 *   out of bounds there, which its extractor rules out (keypoints stay 16 px inside,
 *   ORBextractor.cc:1058-1061). Over the seen cells: min and max depth (the reference's sort
 *   serves front() and back() only) and the nearest cell, the one of least key
 *   (dx dx + dy dy, (dx + SQLM_LD_HALF_W) 2 SQLM_LD_HALF_H + (dy + SQLM_LD_HALF_H)): :373 is
 *   strict, so among equal distances the first in scan order wins, and distinct small integers
 *   have distinct double square roots, so comparing the integers equals comparing the sqrt.
 *   No seen cell: class 0, depth -1. max - min > SQLM_LD_MAX_RANGE (double): class 2,
 *   depth -1. Otherwise class 1 and depth = (float)image[nearest]. nearest_uv = (col, row) of
 *   the nearest cell, (-1, -1) when there is none (classes 0) - it is reported for class 2 too.
 *   n_with_depth counts keypoints with depth > 0 (:404-408).
 * Camera-frame point (Frame::UnprojectStereo, :1710-1723), when key_un_xy (mvKeysUn[i].pt),
 *   cam = (fx, fy, cx, cy) and xyz_cam are all given: for z = depth > 0, in float,
 *   x = ((u - cx) z) (1.0f / fx), y = ((v - cy) z) (1.0f / fy), and z; zeros otherwise. The
 *   world transform of :1725 is a cv::Mat float product whose rounding cannot be pinned here;
 *   it stays with the caller. xyz_cam without key_un_xy or cam is SQLM_ERR_INVALID_ARG.
 * A depth that overflows to a NaN (coordinates times matrix entries beyond double) is stored
 *   as some NaN; it is never seen and never positive. No memory is touched out of bounds for
 *   any finite or non-finite input.
 *
 * Empty sweeps, empty keypoint lists, frames with either one empty and n_frame = 0 are fine.
 * Limits: rows, cols in [1, SQLM_LD_MAX_DIM], n_frame rows cols <= SQLM_LD_MAX_CELLS, fewer
 * than 2^31 points and fewer than 2^27 keypoints in the batch: beyond them
 * SQLM_ERR_UNSUPPORTED before the device (or any array) is touched. SQLM_ERR_INVALID_ARG: a
 * NULL required pointer, n_frame < 0, rows or cols < 1, offsets that do not start at 0 or
 * decrease, a sweep of 2^31 - 1 points or more, a non-finite matrix entry. */
#define SQLM_LD_HALF_W 4        /* half_patch_width, :339 */
#define SQLM_LD_HALF_H 7        /* half_patch_height, :340 */
#define SQLM_LD_MIN_X 1.0f      /* :295, :308 */
#define SQLM_LD_MAX_RANGE 2.0   /* :386 */
#define SQLM_LD_MAX_DIM 4096
#define SQLM_LD_MAX_CELLS (1 << 25)
/* Outputs are packed like the inputs: keypoint k of the batch owns class_id[k], depth[k],
 * nearest_uv[2k..], xyz_cam[3k..]. stats[f] = (min_v, n_written, n_occupied, n_with_depth).
 * depth_image, when given, receives double [n_frame][rows][cols]; it is not read back from
 * the device otherwise. */
int sqlm_lidar_depth(sqlm_ctx *ctx, int n_frame, const int64_t *sweep_off /*[n_frame+1]*/,
    const float *xyz /*[n][3]*/, const int64_t *key_off /*[n_frame+1]*/, const float *key_xy /*[m][2]*/,
    const float *key_un_xy /*[m][2], NULL ok*/, int rows, int cols,
    const double *intrinsic /*[12]*/, const double *extrinsic /*[16]*/, const float *cam /*[4], NULL ok*/,
    int32_t *class_id /*[m]*/, float *depth /*[m]*/, int32_t *nearest_uv /*[m][2]*/,
    float *xyz_cam /*[m][3], NULL ok*/, int32_t *stats /*[n_frame][4]*/, double *depth_image /*NULL ok*/);
/* The same text compiled for the CPU; no context, no device. The two trailing arrays are the
 * intermediate state (NULL ok): pixel [n] = v cols + u of a writing point, -1 otherwise;
 * winner [n_frame][rows][cols] = the occupant's index within its sweep plus one, 0 = unwritten. */
int sqlm_lidar_depth_host(int n_frame, const int64_t *sweep_off, const float *xyz,
    const int64_t *key_off, const float *key_xy, const float *key_un_xy, int rows, int cols,
    const double *intrinsic, const double *extrinsic, const float *cam,
    int32_t *class_id, float *depth, int32_t *nearest_uv, float *xyz_cam, int32_t *stats,
    double *depth_image, int32_t *pixel, int32_t *winner);
/* The state of the context's last sqlm_lidar_depth, read back from the device, sized by that
 * call's arguments; any pointer may be NULL. SQLM_ERR_STATE before any call. */
int sqlm_lidar_depth_get_state(sqlm_ctx *ctx, int32_t *pixel, int32_t *winner, double *depth_image);
/* out[0] = SQLM_LD_MAX_DIM, out[1] = SQLM_LD_MAX_CELLS, out[2] = kernel launches of the last
 * call (0: nothing reached the device), out[3] = SQLM_LD_HALF_W, out[4] = SQLM_LD_HALF_H,
 * out[5] = lanes per keypoint, out[6] = points and out[7] = keypoints of the last call
 * (saturated at INT32_MAX). ctx may be NULL (the limits alone). */
int sqlm_lidar_depth_info(const sqlm_ctx *ctx, int32_t out[8]);

/* Results (write-back inputs, g2oOptimizer.cc:1167-1189, :306-360). */
int sqlm_get_poses(sqlm_ctx *ctx, double *pose_q, double *pose_t);
int sqlm_get_points(sqlm_ctx *ctx, double *pt);
/* e->chi2() from the last computed error (g2o semantics: may belong to a
 * rejected trial, and level-1 edges keep their pass-1 value). */
int sqlm_get_edge_chi2(sqlm_ctx *ctx, double *chi2);
/* The _error of every LiDAR edge of either kind from the last computed error,
 * err [n_lid] in the caller's edge order (introspection for tests; no
 * reference counterpart): (T_cw p_w - p_c) . n of a flat edge, |T_cw p_w - p_c|
 * of a corner edge, at the state of the last trial whose errors were computed,
 * accepted or not. An edge that was inactive in
 * the last optimize() (fixed pose, other level) keeps the value of the last
 * optimize() in which it was active, 0 if there was none since the edges were
 * set -- what the oracle's lid_err holds (oracle/g2o_ref.c computes the error
 * of active edges only). Completes a pending device-to-host transfer of the
 * errors like sqlm_get_edge_chi2; adds no work to a trial.
 * SQLM_ERR_INVALID_ARG on a NULL argument, SQLM_ERR_STATE before a problem is
 * set or before an optimize() has run on the current LiDAR edges. */
int sqlm_get_lidar_error(sqlm_ctx *ctx, double *err);
/* e->isDepthPositive() evaluated at the current estimate. */
int sqlm_get_edge_depth_positive(sqlm_ctx *ctx, uint8_t *positive);
int sqlm_get_edge_level(sqlm_ctx *ctx, uint8_t *level);

/* Layout the last optimize() chose for the reduced camera system S (the
 * replacement of SimplicialLDLT + AMD, linear_solver_eigen.h:60-75):
 * out[0] = 0 none (no free camera), 1 banded (block cyclic reduction),
 * 2 band + border (loop closure: cameras coupled far off the band eliminated
 * last, launch_arrow_solve), 3 dense Cholesky; out[1] = cameras per
 * superblock B, out[2] = superblocks p, out[3] = superblock rows n,
 * out[4] = border cameras, out[5] = border rows (16-padded), out[6] = free
 * cameras, out[7] = superblocks carrying band-border coupling. */
int sqlm_get_rcs_layout(sqlm_ctx *ctx, int out[8]);

/* Device paths the last optimize() ran (introspection for tests and tools; no
 * reference counterpart): out[0] = 1 if the observation inputs (u, v,
 * invSigma2, Huber delta) were all float32 values and travelled as float4,
 * 0 if they took the double arrays; out[1] = reduced-camera solve: 0 none,
 * 1 cyclic reduction (per-level launches), 3 band + border, 4 dense
 * Cholesky (2 and 5 retired); out[2] = kernel that forms the reduced camera
 * system's partial sums: 0 none, 1 row fallback (launch_rcs: some landmark
 * window wider than 24 free cameras), 2 k_rcs_tile mono, 3 k_rcs_tile stereo,
 * 4 producer / consumer k_rcs_tile_p; out[3] = bitmask of the tile classes
 * with at least one tile (bit NT, NT = ceil(6 cp / 16) accumulator tiles for
 * a window of cp free cameras: 3, 4, 6, 8, 9); out[4] / out[5] = S blocks / g
 * rows summed by a whole workgroup (more than 24 tile partials: n_long_s /
 * n_long_g); out[6] = 1 if some landmark is observed twice by one camera
 * (tile_dups); out[7] = longest track (tile_maxk). */
int sqlm_get_exec_info(sqlm_ctx *ctx, int out[8]);

/* The reduced camera system of the most recent LM trial the last optimize()
 * launched (introspection for tests; no reference counterpart), in g2o's sign
 * convention H dx = b with b = -J^T W r (block_solver.hpp:420-470): g
 * [6 n_free] = b_p - sum_l H_pl (H_ll + lambda I)^-1 b_l, the Schur
 * complement's right-hand side, and dx [6 n_free] = the camera step the trial
 * applied as T <- exp(dx) T (zero if the solve met a non-positive pivot), both
 * in free-camera (hessianIndex) order, tangent order [omega; upsilon].
 * Synchronises the context stream. SQLM_ERR_STATE without a prepared problem
 * or before any trial has run.
 * On a sharded context (every rank indexes the same free cameras): rank 0, and
 * the one-rank self-loop, return the system it solved -- g summed over the
 * ranks -- and its solution; a rank >= 1 returns in dx the step rank 0
 * broadcast (the same bits) and in g its own share of the right-hand side as
 * it was sent to rank 0, meaningful only inside that rank's row range (the
 * free cameras its own edges touch; zero elsewhere). */
int sqlm_get_last_step(sqlm_ctx *ctx, double *g, double *dx);

/* Converter::toSE3Quat / toCvMat(SE3Quat) (src/utils/Converter.cc:55-79,98-109):
 * float32 row-major 4x4 T_cw <-> (q, t). */
void sqlm_pose_from_Tcw_f32(const float T[16], double q[4], double t[3]);
void sqlm_pose_to_Tcw_f32(const double q[4], const double t[3], float T[16]);

/* Multi-GPU: landmark-sharded global BA, one context per rank. Each rank
 * calls sqlm_set_problem with ALL poses and ITS landmarks/observations; the
 * reduced camera system, gradient and scalars are summed over RCCL (xGMI).
 * Rank 0 creates the id; the caller broadcasts it (e.g. torch.distributed). */
int sqlm_comm_id_size(void);
int sqlm_comm_get_unique_id(char *id_out);
int sqlm_ctx_set_comm(sqlm_ctx *ctx, const char *unique_id, int rank, int nranks);
/* What the context's exchange actually runs on: *transport = SQLM_COMM_NONE,
 * _RCCL, _RCCL_SELFLOOP or _HOST; for RCCL *rank / *nranks are the ones the
 * communicator itself reports (ncclCommUserRank / ncclCommCount), otherwise
 * the ones the caller set. No reference counterpart (bench / test hook). */
#define SQLM_COMM_NONE 0
#define SQLM_COMM_RCCL 1
#define SQLM_COMM_RCCL_SELFLOOP 2
#define SQLM_COMM_HOST 3
int sqlm_ctx_comm_info(const sqlm_ctx *ctx, int *transport, int *rank, int *nranks);
/* RCCL transport checks on ONE GPU (no reference counterpart; test hooks).
 * sqlm_ctx_set_comm_selfloop: a one-rank RCCL communicator on which the
 * context takes the sharded code path (every all-reduce, the rank-0 gather and
 * the dx broadcast run through RCCL with one rank).
 * sqlm_comm_selftest: on `device`, a one-rank communicator drives the three
 * exchange primitives — a grouped send/recv to self of `count` doubles, an
 * in-place broadcast and sum / max all-reduces (f64, i32, u8) — and writes
 * the largest deviation from the expected buffers to *max_err. */
int sqlm_ctx_set_comm_selfloop(sqlm_ctx *ctx, const char *unique_id);
int sqlm_comm_selftest(int device, const char *unique_id, int64_t count, double *max_err);

/* Same sharded algorithm over a caller-provided host collective (for example
 * torch.distributed gloo): the library stages each exchange through host
 * memory and calls fn(user, buf, count, dtype, op), which must all-reduce
 * `count` elements of `buf` in place across the ranks and return 0. Used to
 * run several ranks on one GPU (tests); production uses sqlm_ctx_set_comm.
 * LiDAR unary edges, with their kinds, are owned by rank 0 (ignored on other ranks). */
#define SQLM_DT_F64 0
#define SQLM_DT_U8 1
#define SQLM_DT_I32 2
#define SQLM_OP_SUM 0
#define SQLM_OP_MAX 1
typedef int (*sqlm_allreduce_fn)(void *user, void *buf, int64_t count, int dtype, int op);
int sqlm_ctx_set_host_comm(sqlm_ctx *ctx, int rank, int nranks, sqlm_allreduce_fn fn, void *user);
/* Point-to-point half of the host transport (the per-trial gather of the
 * reduced camera system to rank 0 and the broadcast of its solution):
 * fn(user, buf, count, dtype, peer, op) with op SQLM_P2P_SEND (buf -> peer),
 * SQLM_P2P_RECV (peer -> buf) or SQLM_P2P_BCAST (in place from root = peer).
 * Required with sqlm_ctx_set_host_comm for nranks > 1; set it first. */
#define SQLM_P2P_SEND 0
#define SQLM_P2P_RECV 1
#define SQLM_P2P_BCAST 2
typedef int (*sqlm_p2p_fn)(void *user, void *buf, int64_t count, int dtype, int peer, int op);
int sqlm_ctx_set_host_p2p(sqlm_ctx *ctx, sqlm_p2p_fn fn, void *user);

/* Device-resident benchmarking hooks: time `n` LM iterations on the set
 * problem with data already in HBM (bench.py). Per-kernel averaged durations
 * (HIP events on the context stream) are returned through kernel_ms
 * [SQLM_NKERNEL_TIMERS] when non-NULL. */
#define SQLM_NKERNEL_TIMERS 9
int sqlm_bench_iterations(sqlm_ctx *ctx, int warmup, int n, double *ms_per_iter, double *kernel_ms,
                          sqlm_stats *stats);
const char *sqlm_kernel_timer_name(int i);
/* Diagnostic: the cyclic reduction this process launched last on the plain
 * band solve: out[0] = index of the first superblock (1, or 0 with
 * SQLM_CR_LO0=1), out[1] = elimination levels, out[2] = the top superblock. */
int sqlm_debug_cr_levels(int out[3]);

#ifdef __cplusplus
}
#endif
#endif
