/*
 * cgmr.h -- C ABI of libcgmr.so: the MI355X-native pose-graph optimiser and scan matcher
 * behind cg_mrslam's hot path.
 *
 * The reference has no FFI layer; its seams are C++ member functions.  Every
 * entry point below names the reference interface it replaces (file:line in
 * mtlazaro/cg_mrslam).  INTEGRATION.md shows the adapter a maintainer adds on the reference
 * side (flatten the g2o containers, call these, write the results back).
 *
 * Conventions
 *   - plain C, flat caller-owned arrays, no global state except the opaque context, which is
 *     bound to one HIP device and one HIP stream;
 *   - return value: 0 = OK, < 0 = error (cgmr_last_error() has the text); like the reference
 *     (which swallows g2o's status, src/slam/graph_slam.cpp:565) a failed Cholesky is *also*
 *     reported through the return value, never through an exception;
 *   - poses are (x, y, theta) triples of doubles; information matrices are the 6 doubles
 *     I11 I12 I13 I22 I23 I33 of the EDGE_SE2 line;
 *   - vertices are addressed by *index* into the pose array; mapping g2o ids to indices is
 *     the adapter's job (ids are robot*10000+k, src/slam/graph_slam.cpp:95,155);
 *   - calls on one context must be serialised by the caller, exactly like calls on one
 *     GraphSLAM instance are serialised by graphMutex (src/slam/graph_slam.h:119);
 *   - there is NO CPU fallback: every compute entry point fails with CGMR_E_NO_DEVICE when no
 *     gfx950 device is usable.
 */
#ifndef CGMR_H
#define CGMR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGMR_OK 0
#define CGMR_E_INVALID (-1)      /* bad argument / index out of range */
#define CGMR_E_NO_DEVICE (-2)    /* no usable HIP device */
#define CGMR_E_HIP (-3)          /* HIP runtime error */
#define CGMR_E_ALLOC (-4)
#define CGMR_E_TIMEOUT (-5)      /* a bounded in-kernel wait ran out (a device-side hand-off that never arrived): NOT a numerical failure */
#define CGMR_E_CHOLESKY_BASE (-100) /* Cholesky failed in GN iteration it: returns CGMR_E_CHOLESKY_BASE - it */

typedef struct cgmr_ctx cgmr_ctx;

int cgmr_version(void);

/* Create a context on HIP device `device`.  `hip_stream` may be an existing hipStream_t (e.g.
 * torch.cuda.current_stream().cuda_stream) or NULL to let the context own a stream. */
int cgmr_ctx_create(int device, void* hip_stream, cgmr_ctx** out);
void cgmr_ctx_destroy(cgmr_ctx* ctx);
const char* cgmr_last_error(const cgmr_ctx* ctx);
/* The context's hipStream_t (the one given to cgmr_ctx_create, or the one the context owns): for a caller that
 * orders its own streams against the context's work with events instead of blocking the host. */
void* cgmr_ctx_stream(const cgmr_ctx* ctx);

/* Block until everything queued on the context's stream has finished. */
int cgmr_ctx_synchronize(cgmr_ctx* ctx);

/* ------------------------------------------------------------------------------------------
 * Gauss-Newton optimisation.
 * Replaces: void GraphSLAM::optimize(int nrunnings)            src/slam/graph_slam.cpp:561-575
 *           the 1-iteration pre-solve in findConstraints       src/slam/graph_slam.cpp:392-393
 * i.e. g2o's initializeOptimization() + optimize(n) with the solver configured at
 * src/slam/graph_slam.cpp:44-56 (Gauss-Newton, no damping, no stopping rule, exactly n
 * iterations unless the Cholesky fails).
 *
 *   poses_xyt   [nV*3] in/out  estimates
 *   fixed       [nV]           1 = vertex is fixed (g2o setFixed)
 *   from_idx/to_idx [nE]       vertex indices of each EdgeSE2
 *   meas_xyt    [nE*3]         edge measurements
 *   info_upper  [nE*6]         edge information matrices
 *   chi2_out    [iters+1]      (nullable) chi2 before each iteration and after the last
 * Host-pointer variant: copies in, runs on the GPU, copies poses and chi2 back.
 * Limit: a front of the elimination tree may have at most 10 890 border poses (16-bit row maps in LDS); a graph
 * whose nested-dissection separators are wider is rejected with CGMR_E_INVALID (none of the BASELINE.json
 * configurations comes near: C2 has 74, a 100k-vertex / 300k-edge graph about 800).
 * An edge from a vertex to itself (from_idx[k] == to_idx[k]) is accepted and is the chain rule's term: its error is
 * z^-1 (xi^-1 xi), its one Jacobian Ji + Jj, so H_ii += (Ji + Jj)^T Omega (Ji + Jj) and b_i likewise.  That error does not
 * depend on xi and Ji + Jj is exactly zero: the edge adds its constant to chi2 and nothing to H or b (a vertex with no
 * other edge is left without a pivot, as in any system that does not determine it).  The same holds on every path that
 * linearises (Levenberg-Marquardt, dogleg, marginals, condensed graphs).                          */
int cgmr_gn_optimize(cgmr_ctx* ctx, int nV, double* poses_xyt, const uint8_t* fixed, int nE,
                     const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt,
                     const double* info_upper, int iters, double* chi2_out);

/* Device-resident variant: d_poses / d_meas / d_info are device pointers on the context's
 * device (poses updated in place); the graph *structure* (fixed, from, to) stays in host
 * memory because the ordering / symbolic analysis runs on the host, as it does in g2o.
 * Asynchronous on the context's stream except for the final chi2 / status read-back. */
int cgmr_gn_optimize_dev(cgmr_ctx* ctx, int nV, double* d_poses_xyt, const uint8_t* fixed, int nE,
                         const int32_t* from_idx, const int32_t* to_idx, const double* d_meas_xyt,
                         const double* d_info_upper, int iters, double* chi2_out);

/* Levenberg-Marquardt optimisation (C ABI version >= 104): g2o's OptimizationAlgorithmLevenberg [g2o-recalled], the
 * alternative the reference's map tool includes (ros_map_publisher/graph2occupancy.h:19).  Outer iteration i linearises
 * once; its trials solve (H + lambda I) dx = b on the Gauss-Newton path's factorisation (fixed and inactive vertices stay
 * outside the system and take no lambda), evaluate chi2 at x (+) dx and keep the step when
 *   rho = (chi2(x) - chi2(x')) / (dx^T (lambda dx + b) + 1e-3) > 0
 * (lambda *= max(lower, min(upper, 1 - (2 rho - 1)^3)), nu = 2); a rejected trial restores the poses bit for bit and
 * retries with lambda *= nu, nu *= 2.  A failed factorisation is a rejected trial.  The call terminates early when an
 * iteration runs max_trials trials, when rho == 0, or when lambda is no longer finite.  lambda starts, on the first trial of
 * every call, at initial_lambda if > 0, else at tau * max |H_jj| over the free diagonal.
 *   params      nullable: g2o's defaults (tau 1e-5, initial_lambda -1, max_trials 10, 1/3, 2/3)
 *   chi2_out    [iters+1] nullable: chi2 at the start and after each iteration (after the last run: repeated)
 *   lambda_out  [iters]   nullable: lambda at the end of each iteration (0 past iters_done)
 *   trials_out  [iters]   nullable: trials (factorisations) of each iteration (0 past iters_done)
 *   iters_done  nullable: iterations run, a terminating one included (g2o's optimize() return value)
 * Returns CGMR_OK (also on termination: iters_done < iters unless it came in the last iteration), CGMR_E_INVALID,
 * CGMR_E_HIP / _ALLOC, or CGMR_E_TIMEOUT when a bounded in-kernel wait runs out twice (after the first time the trial is
 * repeated with one launch per kernel and level).  Never CGMR_E_CHOLESKY_*.  Shares the analysis cache with
 * cgmr_gn_optimize*.  The device keeps the state: the host queues iters - (iterations run) trials and waits once per
 * such round (one wait when every first trial is accepted).  CGMR_GRAPH capture does not apply to this path. */
typedef struct cgmr_lm_params {
  double tau;
  double initial_lambda;
  int32_t max_trials;
  double good_step_lower;
  double good_step_upper;
} cgmr_lm_params;
int cgmr_lm_optimize(cgmr_ctx* ctx, int nV, double* poses_xyt, const uint8_t* fixed, int nE, const int32_t* from_idx,
                     const int32_t* to_idx, const double* meas_xyt, const double* info_upper, int iters,
                     const cgmr_lm_params* params, double* chi2_out, double* lambda_out, int32_t* trials_out,
                     int32_t* iters_done);
/* Device-resident variant (d_poses / d_meas / d_info on the context's device, as cgmr_gn_optimize_dev). */
int cgmr_lm_optimize_dev(cgmr_ctx* ctx, int nV, double* d_poses_xyt, const uint8_t* fixed, int nE,
                         const int32_t* from_idx, const int32_t* to_idx, const double* d_meas_xyt,
                         const double* d_info_upper, int iters, const cgmr_lm_params* params, double* chi2_out,
                         double* lambda_out, int32_t* trials_out, int32_t* iters_done);
/* The last cgmr_lm_optimize* call on this context: out[0] = host waits for the device, out[1] = trials run. */
int cgmr_lm_last_stats(const cgmr_ctx* ctx, int64_t out[2]);

/* Robust kernels (C ABI version >= 105; g2o's edge->setRobustKernel(new RobustKernelX) with setDelta(delta)) [g2o-recalled].  An edge with error e
 * and information O at the linearisation point has e2 = e^T O e; its kernel maps e2 to (rho0, rho1).  The edge then adds
 * J^T (rho1 O) J to H and -rho1 J^T O e to b (g2o's robustInformation; the second-order term is left out, as in g2o), and
 * rho0 to the objective.  The chi2 of the robust entry points is the robust chi2, the sum of rho0 over the edges (g2o's
 * activeRobustChi2); it equals the plain chi2 when every edge is CGMR_RK_NONE.  With d2 = delta * delta:
 *   CGMR_RK_NONE          rho0 = e2, rho1 = 1
 *   CGMR_RK_HUBER         e2 <= d2: (e2, 1); else (2 delta sqrt(e2) - d2, delta / sqrt(e2))
 *   CGMR_RK_PSEUDO_HUBER  a = sqrt(1 + e2 / d2): (2 d2 (a - 1), 1 / a)
 *   CGMR_RK_CAUCHY        a = 1 + e2 / d2: (d2 log(a), 1 / a)
 *   CGMR_RK_WELSCH        a = exp(-e2 / d2): (d2 (1 - a), a)
 *   CGMR_RK_TUKEY         sqrt(e2) <= delta, a = 1 - e2 / d2: (d2 (1 - a^3) / 3, a^2); else (d2 / 3, 0)
 *   CGMR_RK_SATURATED     e2 <= d2: (e2, 1); else (d2, 0)
 *   CGMR_RK_DCS           delta = phi, s = 2 phi / (phi + e2): s >= 1: (e2, 1); else (s^2 e2, s^2)
 * delta must be finite and > 0 for every kind but CGMR_RK_NONE; anything else (an unknown kind included) is CGMR_E_INVALID,
 * returned before anything is queued.  g2o's Fair and GemanMcClure kernels are not offered: their formulas are not recalled
 * reliably enough to pin them down.
 * A zero weight (Tukey, Saturated, Welsch underflowing) can leave a free vertex whose edges all weigh 0: its block of H is
 * singular, as in g2o.  Gauss-Newton then returns CGMR_E_CHOLESKY_BASE - it with the poses at the last good update;
 * Levenberg-Marquardt rejects the trial.
 * The marginals and the condensed graphs take the robust H through their own entry points (cgmr_marginals_robust,
 * cgmr_marginals_all_robust, cgmr_covariance_estimate_robust, cgmr_condense_robust; the robot graph: cgmr_graph_set_condensed_robust),
 * as g2o's computeMarginals inverts the H of the last buildSystem, robust weights included [g2o-recalled].  rho1 is taken at
 * the linearisation point of the H that is inverted: the poses passed in for the marginals; for cgmr_covariance_estimate_robust
 * and cgmr_condense_robust, the spanning-tree initial guess their one Gauss-Newton iteration starts from.  There the robust H
 * drives the iteration's step as well as the marginals, so a condensed edge's measurement can change, not its information
 * alone.  At that guess every spanning-tree edge has a zero residual (to rounding) and weight 1 under every kind: an outlier
 * is down-weighted only when it is off the tree, and how much depends on the residual it shows at the guess, not at the
 * optimum. */
#define CGMR_RK_NONE 0
#define CGMR_RK_HUBER 1
#define CGMR_RK_PSEUDO_HUBER 2
#define CGMR_RK_CAUCHY 3
#define CGMR_RK_WELSCH 4
#define CGMR_RK_TUKEY 5
#define CGMR_RK_SATURATED 6
#define CGMR_RK_DCS 7
typedef struct cgmr_robust {
  const uint8_t* kind;      /* [nE] nullable: every edge takes default_kind (host memory, device memory for the _dev entry points) */
  const double* delta;      /* [nE] nullable: every edge takes default_delta (the same memory as kind) */
  int32_t default_kind;
  double default_delta;
  double* edge_chi2_out;    /* [nE] host, nullable: e^T O e of every edge at the returned estimate */
  double* weight_out;       /* [nE] host, nullable: rho1 there */
} cgmr_robust;
/* cgmr_gn_optimize / cgmr_lm_optimize and their _dev variants with robust kernels.  rk == NULL: the plain call, bit for bit.
 * The statistics are those of the estimate the call returns (Gauss-Newton: also after a failed Cholesky, at the poses as
 * left).  The _dev variants read kind / delta back once to check them. */
int cgmr_gn_optimize_robust(cgmr_ctx* ctx, int nV, double* poses_xyt, const uint8_t* fixed, int nE, const int32_t* from_idx,
                            const int32_t* to_idx, const double* meas_xyt, const double* info_upper, int iters,
                            double* chi2_out, const cgmr_robust* rk);
int cgmr_gn_optimize_robust_dev(cgmr_ctx* ctx, int nV, double* d_poses_xyt, const uint8_t* fixed, int nE,
                                const int32_t* from_idx, const int32_t* to_idx, const double* d_meas_xyt,
                                const double* d_info_upper, int iters, double* chi2_out, const cgmr_robust* rk);
int cgmr_lm_optimize_robust(cgmr_ctx* ctx, int nV, double* poses_xyt, const uint8_t* fixed, int nE, const int32_t* from_idx,
                            const int32_t* to_idx, const double* meas_xyt, const double* info_upper, int iters,
                            const cgmr_lm_params* params, double* chi2_out, double* lambda_out, int32_t* trials_out,
                            int32_t* iters_done, const cgmr_robust* rk);
int cgmr_lm_optimize_robust_dev(cgmr_ctx* ctx, int nV, double* d_poses_xyt, const uint8_t* fixed, int nE,
                                const int32_t* from_idx, const int32_t* to_idx, const double* d_meas_xyt,
                                const double* d_info_upper, int iters, const cgmr_lm_params* params, double* chi2_out,
                                double* lambda_out, int32_t* trials_out, int32_t* iters_done, const cgmr_robust* rk);

/* Dogleg optimisation (C ABI version 105, added later under the same number: callers find it by its symbols): g2o's
 * OptimizationAlgorithmDogleg [g2o-recalled: recalled from g2o, not read from its source; the contract is
 * tests/ref_dogleg.py], the third algorithm of the optimisation-algorithm factory the reference includes (graph_slam.h:36,
 * "dl_var").  At the start of a call delta = initial_delta, currentLambda = initial_lambda, wasPD = true.  Outer iteration i
 * linearises once (currentChi = the (robust) chi2 at x, H and b = -J^T Omega e; fixed and inactive vertices stay out) and:
 *   alpha = |b|^2 / (b^T H b), hsd = alpha b;
 *   hgn solves H hgn = b -- H + currentLambda I on the free diagonal once any factorisation of the call has failed (wasPD
 *   false); then an ok solve sets currentLambda = max(1e-12, currentLambda / (0.5 lambda_factor)), a failed one multiplies it
 *   by lambda_factor and repeats, and above 1e3 the call fails (g2o's Fail);
 *   trials: |hgn| < delta: h = hgn (CGMR_DL_STEP_GN); |hsd| > delta: h = delta / |hsd| hsd (_SD); else h = hsd + beta (hgn -
 *   hsd) with |h| = delta (_DL); rho = (currentChi - chi2(x (+) h)) / (-h^T H h + 2 b^T h) (a gain below 1e-12 in magnitude
 *   counts as 1e-12); rho > 0 keeps the step, otherwise x is restored bit for bit; rho > 0.75: delta = max(delta, 3 |h|),
 *   rho < 0.25: delta *= 0.5; repeat while no step was good and the trials are fewer than max_trials.
 * The call terminates (g2o's Terminate) after an iteration that ran max_trials trials -- even when its last one was good --
 * or had no good step; that iteration counts as run.  H is never damped for alpha or the gain.  A rejected trial needs no
 * new factorisation: its retry mixes the same hgn and hsd for the smaller delta.
 *   params      nullable: g2o's defaults (initial_delta 1e4, max_trials 100, initial_lambda 1e-7, lambda_factor 10);
 *               max_trials >= 1, the rest finite and > 0, lambda_factor > 1, or CGMR_E_INVALID before anything is queued
 *   chi2_out    [iters+1] nullable: chi2 at the start and after each iteration (after the last one run: repeated)
 *   delta_out   [iters]   nullable: delta at the end of each iteration (0 past iters_done)
 *   trials_out  [iters]   nullable: trials of each iteration (0 past iters_done)
 *   step_out    [iters]   nullable: CGMR_DL_STEP_* of each iteration's last trial (0 past iters_done)
 *   iters_done  nullable: iterations run, a terminating one included
 *   rk          nullable: the plain call; otherwise the robust rules of cgmr_robust above (robust chi2 and H)
 * Returns CGMR_OK (also on termination), CGMR_E_CHOLESKY_BASE - i on g2o's Fail in iteration i (the poses at the last
 * accepted step, the records of iterations 0 .. i-1, *iters_done = i), CGMR_E_INVALID, CGMR_E_HIP / _ALLOC, or
 * CGMR_E_TIMEOUT when a bounded in-kernel wait runs out twice.  Shares the analysis cache with cgmr_gn_optimize*.  The device
 * keeps the state; the host queues rounds and waits once per round: one wait when every first trial is accepted and H stays
 * positive definite. */
typedef struct cgmr_dl_params {
  double initial_delta;
  int32_t max_trials;
  double initial_lambda;
  double lambda_factor;
} cgmr_dl_params;
#define CGMR_DL_STEP_SD 1
#define CGMR_DL_STEP_GN 2
#define CGMR_DL_STEP_DL 3
int cgmr_dl_optimize(cgmr_ctx* ctx, int nV, double* poses_xyt, const uint8_t* fixed, int nE, const int32_t* from_idx,
                     const int32_t* to_idx, const double* meas_xyt, const double* info_upper, int iters,
                     const cgmr_dl_params* params, double* chi2_out, double* delta_out, int32_t* trials_out,
                     int32_t* step_out, int32_t* iters_done, const cgmr_robust* rk);
/* Device-resident variant (d_poses / d_meas / d_info, and rk's kind / delta, on the context's device). */
int cgmr_dl_optimize_dev(cgmr_ctx* ctx, int nV, double* d_poses_xyt, const uint8_t* fixed, int nE,
                         const int32_t* from_idx, const int32_t* to_idx, const double* d_meas_xyt,
                         const double* d_info_upper, int iters, const cgmr_dl_params* params, double* chi2_out,
                         double* delta_out, int32_t* trials_out, int32_t* step_out, int32_t* iters_done,
                         const cgmr_robust* rk);
/* The last cgmr_dl_optimize* call on this context: out[0] = host waits for the device, out[1] = trials run, out[2] =
 * factorisations that served an iteration (failed damped ones included). */
int cgmr_dl_last_stats(const cgmr_ctx* ctx, int64_t out[3]);

/* Typed factors: point landmarks and priors, g2o's slam2d types (present in C ABI version 105 libraries that export these
 * symbols) [g2o-recalled].  Every vertex still owns three doubles of the pose array and a 3x3 block column of H; every edge
 * still has meas_xyt [3] and info_upper [6].
 *   vertex kinds  CGMR_VERTEX_SE2 (0)  a pose (x, y, theta)
 *                 CGMR_VERTEX_XY  (1)  a point (x, y): its third double is 0.0 on input and exactly 0.0 on output
 *   edge kinds    CGMR_EDGE_SE2 (0)           EDGE_SE2            pose i -> pose j, as everywhere above
 *                 CGMR_EDGE_SE2_XY (1)        EDGE_SE2_XY         pose i -> point l: e = R(theta_i)^T (l - t_i) - z           (2)
 *                 CGMR_EDGE_BEARING_SE2_XY (2) EDGE_BEARING_SE2_XY pose i -> point l: e = normalize(atan2(ry, rx) - z0),
 *                                                                 (rx, ry) = R(theta_i)^T (l - t_i)                          (1)
 *                 CGMR_EDGE_PRIOR_SE2 (3)     EDGE_PRIOR_SE2      from == to == i: e = (R(z_theta)^T (t_i - z_t),
 *                                                                 normalize(theta_i - z_theta))                              (3)
 *                 CGMR_EDGE_PRIOR_SE2_XY (4)  EDGE_PRIOR_SE2_XY   from == to == i: e = t_i - z                               (2)
 * A 2-dimensional factor reads its first two measurements and the entries I11 I12 I22 (positions 0, 1, 3) of info_upper;
 * the rest is ignored; the 1-dimensional bearing reads meas_xyt[0] and info_upper[0] alone.  With the point on the pose
 * (rx = ry = 0) a bearing's error is normalize(-z0) and its Jacobians are zero.  A robust kernel sees e^T Omega e of the factor's own dimension.  CGMR_E_INVALID, with a message that
 * names the edge and before the device is touched, for: a kind-1 edge whose from is not a pose or whose to is not a point;
 * a kind-0, 3 or 4 edge that touches a point; a prior with from != to; any kind above 4; a vertex kind above 1 (kind 2 has kind 1's rule).
 * A prior makes its vertex a live column: a graph with no fixed vertex and one CGMR_EDGE_PRIOR_SE2 is a regular system.
 * A point's third unknown is carried as a decoupled dummy (pivot = a copy of the block's H_xx, right-hand side 0; a kind-1
 * edge whose H_xx is not positive contributes 1.0 instead, a bearing always its own H_xx, which is 0 along the world's x
 * axis: a point needs two bearings, or one kind-1 observation, to be determined at all): its step is exactly zero, the Levenberg-Marquardt start tau * max |H_jj| and every chi2 are those of the true-dimension system.
 * types == NULL, a null member, or kinds that are all zero: the plain / robust call, bit for bit (the same launches).  rk is
 * nullable as in the robust entry points.  vertex_kind / edge_kind are host memory in the _dev variants too (they are
 * structure, like fixed / from_idx / to_idx).  The typed path adds one small launch per linearisation that has priors;
 * CGMR_GRAPH capture is not supported on it (as for Levenberg-Marquardt).  Joint / pairwise marginals and the
 * gate of a landmark observation: cgmr_marginals_joint_typed, cgmr_marginals_pairs_typed, cgmr_observation_covariance below.
 * Not offered for condensed graphs and the robot graph (cgmr_graph_*): the multi-robot protocol has no landmarks.
 * cgmr_marginals_typed / cgmr_marginals_all_typed: cgmr_marginals_robust / cgmr_marginals_all_robust on the typed H.  A
 * point's 3x3 block comes back with its third row and column zero; so does the third column of the cross block of a
 * kind-1 edge (rows: the pose, columns: the point). */
#define CGMR_VERTEX_SE2 0
#define CGMR_VERTEX_XY 1
#define CGMR_EDGE_SE2 0
#define CGMR_EDGE_SE2_XY 1
#define CGMR_EDGE_BEARING_SE2_XY 2
#define CGMR_EDGE_PRIOR_SE2 3
#define CGMR_EDGE_PRIOR_SE2_XY 4
typedef struct cgmr_factor_types {
  const uint8_t* vertex_kind;   /* [nV] host, nullable: every vertex is a pose */
  const uint8_t* edge_kind;     /* [nE] host, nullable: every edge is an EDGE_SE2 */
} cgmr_factor_types;
int cgmr_gn_optimize_typed(cgmr_ctx* ctx, int nV, double* poses_xyt, const uint8_t* fixed, int nE, const int32_t* from_idx,
                           const int32_t* to_idx, const double* meas_xyt, const double* info_upper, int iters,
                           double* chi2_out, const cgmr_factor_types* types, const cgmr_robust* rk);
int cgmr_gn_optimize_typed_dev(cgmr_ctx* ctx, int nV, double* d_poses_xyt, const uint8_t* fixed, int nE,
                               const int32_t* from_idx, const int32_t* to_idx, const double* d_meas_xyt,
                               const double* d_info_upper, int iters, double* chi2_out, const cgmr_factor_types* types,
                               const cgmr_robust* rk);
int cgmr_lm_optimize_typed(cgmr_ctx* ctx, int nV, double* poses_xyt, const uint8_t* fixed, int nE, const int32_t* from_idx,
                           const int32_t* to_idx, const double* meas_xyt, const double* info_upper, int iters,
                           const cgmr_lm_params* params, double* chi2_out, double* lambda_out, int32_t* trials_out,
                           int32_t* iters_done, const cgmr_factor_types* types, const cgmr_robust* rk);
int cgmr_lm_optimize_typed_dev(cgmr_ctx* ctx, int nV, double* d_poses_xyt, const uint8_t* fixed, int nE,
                               const int32_t* from_idx, const int32_t* to_idx, const double* d_meas_xyt,
                               const double* d_info_upper, int iters, const cgmr_lm_params* params, double* chi2_out,
                               double* lambda_out, int32_t* trials_out, int32_t* iters_done,
                               const cgmr_factor_types* types, const cgmr_robust* rk);
int cgmr_dl_optimize_typed(cgmr_ctx* ctx, int nV, double* poses_xyt, const uint8_t* fixed, int nE, const int32_t* from_idx,
                           const int32_t* to_idx, const double* meas_xyt, const double* info_upper, int iters,
                           const cgmr_dl_params* params, double* chi2_out, double* delta_out, int32_t* trials_out,
                           int32_t* step_out, int32_t* iters_done, const cgmr_factor_types* types, const cgmr_robust* rk);
int cgmr_dl_optimize_typed_dev(cgmr_ctx* ctx, int nV, double* d_poses_xyt, const uint8_t* fixed, int nE,
                               const int32_t* from_idx, const int32_t* to_idx, const double* d_meas_xyt,
                               const double* d_info_upper, int iters, const cgmr_dl_params* params, double* chi2_out,
                               double* delta_out, int32_t* trials_out, int32_t* step_out, int32_t* iters_done,
                               const cgmr_factor_types* types, const cgmr_robust* rk);
/* Max-mixture edges (same ABI version: callers find the entry points by their symbols): an edge is one of K Gaussian
 * alternatives (z_k, Omega_k, w_k) and every linearisation keeps the most likely one at the estimate it linearises at, after
 * Olson and Agarwal's max-mixtures [recalled: from memory, not read from the paper's or vertigo's text; the contract is
 * tests/ref_mixture.py].  For an edge with components k = 1..K:
 *   r_k = e(z_k)^T Omega_k e(z_k), in the factor's own dimension (as the typed entry points form it)
 *   a_k = 2 ln w_k + ln det Omega_k, the determinant over the factor's own dimension: 3x3 for kinds 0 and 3, the leading 2x2
 *         (I11 I12 I22) for kinds 1 and 4, info[0] for a bearing
 *   c_k = max_j a_j - a_k >= 0
 *   the edge contributes min_k (r_k + c_k); the selected component is the argmin, ties to the lowest index.
 * The cost is continuous and non-negative, and for K = 1 it is the plain chi2 (c = 0; Omega may be singular, nothing of it is
 * checked).  H, b and the chi2 of a linearisation are those of the selected (z, Omega), the chi2 with c added; a chi-only pass
 * (a Levenberg-Marquardt or dogleg trial point) selects afresh, so the gain ratios compare this cost between points.
 * Worked example: z equal, Omega_1 = I, Omega_2 = 0.01 I, w = (1/2, 1/2) gives c = (0, 6 ln 10); the second component (a null
 * hypothesis: same z, inflated covariance) wins exactly when r_1 > 6 ln 10 / 0.99.
 *   comp_ptr     [nE + 1]: edge k owns the components [comp_ptr[k], comp_ptr[k + 1]); nC = comp_ptr[nE]
 *   comp_meas    [3 nC], comp_info [6 nC] (upper triangle), comp_weight [nC]
 *   selected_out [nE], nullable: every edge's selected component (its index within the edge), from the call's final chi-only
 *                pass at the returned poses
 * All five are host memory, in the _dev variants too.  meas_xyt / info_upper hold every edge's first component: a null
 * mixture, a null comp_ptr, or one component on every edge is the typed / plain call on them, bit for bit (the same
 * launches; selected_out is all zero); on the mixture path they are not read.  The arguments are those of the typed entry
 * points without rk: a mixture is not combined with cgmr_robust, nor offered for GNC, chordal initialisation, the robot
 * graph, condensed graphs or batches; every component of an edge has the edge's vertices and kind.  CGMR_E_INVALID, with a
 * message that names the edge and before the device is touched: a comp_ptr that does not increase from 0 (an edge without a
 * component); on an edge with K > 1, a weight that is not finite and > 0, or an own-dimension det Omega that is not finite and
 * > 0.  One launch per linearisation as before: K components cost the edge's thread K + 1 error evaluations.  CGMR_GRAPH
 * capture is not supported on this path (as for the typed one).
 * cgmr_mixture_select: the chi2 (chi2_out [1]) and the selection at the given poses -- one chi-only pass, poses untouched; bit
 * for bit the first (last) chi2 of an optimise call that starts (ends) there. */
typedef struct cgmr_mixture {
  const int32_t* comp_ptr;      /* [nE + 1] host */
  const double* comp_meas;      /* [3 nC] host */
  const double* comp_info;      /* [6 nC] host */
  const double* comp_weight;    /* [nC] host */
  int32_t* selected_out;        /* [nE] host, nullable */
} cgmr_mixture;
int cgmr_gn_optimize_mixture(cgmr_ctx* ctx, int nV, double* poses_xyt, const uint8_t* fixed, int nE, const int32_t* from_idx,
                             const int32_t* to_idx, const double* meas_xyt, const double* info_upper, int iters,
                             double* chi2_out, const cgmr_factor_types* types, const cgmr_mixture* mixture);
int cgmr_gn_optimize_mixture_dev(cgmr_ctx* ctx, int nV, double* d_poses_xyt, const uint8_t* fixed, int nE,
                                 const int32_t* from_idx, const int32_t* to_idx, const double* d_meas_xyt,
                                 const double* d_info_upper, int iters, double* chi2_out, const cgmr_factor_types* types,
                                 const cgmr_mixture* mixture);
int cgmr_lm_optimize_mixture(cgmr_ctx* ctx, int nV, double* poses_xyt, const uint8_t* fixed, int nE, const int32_t* from_idx,
                             const int32_t* to_idx, const double* meas_xyt, const double* info_upper, int iters,
                             const cgmr_lm_params* params, double* chi2_out, double* lambda_out, int32_t* trials_out,
                             int32_t* iters_done, const cgmr_factor_types* types, const cgmr_mixture* mixture);
int cgmr_lm_optimize_mixture_dev(cgmr_ctx* ctx, int nV, double* d_poses_xyt, const uint8_t* fixed, int nE,
                                 const int32_t* from_idx, const int32_t* to_idx, const double* d_meas_xyt,
                                 const double* d_info_upper, int iters, const cgmr_lm_params* params, double* chi2_out,
                                 double* lambda_out, int32_t* trials_out, int32_t* iters_done,
                                 const cgmr_factor_types* types, const cgmr_mixture* mixture);
int cgmr_dl_optimize_mixture(cgmr_ctx* ctx, int nV, double* poses_xyt, const uint8_t* fixed, int nE, const int32_t* from_idx,
                             const int32_t* to_idx, const double* meas_xyt, const double* info_upper, int iters,
                             const cgmr_dl_params* params, double* chi2_out, double* delta_out, int32_t* trials_out,
                             int32_t* step_out, int32_t* iters_done, const cgmr_factor_types* types,
                             const cgmr_mixture* mixture);
int cgmr_dl_optimize_mixture_dev(cgmr_ctx* ctx, int nV, double* d_poses_xyt, const uint8_t* fixed, int nE,
                                 const int32_t* from_idx, const int32_t* to_idx, const double* d_meas_xyt,
                                 const double* d_info_upper, int iters, const cgmr_dl_params* params, double* chi2_out,
                                 double* delta_out, int32_t* trials_out, int32_t* step_out, int32_t* iters_done,
                                 const cgmr_factor_types* types, const cgmr_mixture* mixture);
int cgmr_mixture_select(cgmr_ctx* ctx, int nV, const double* poses_xyt, const uint8_t* fixed, int nE, const int32_t* from_idx,
                        const int32_t* to_idx, const double* meas_xyt, const double* info_upper,
                        const cgmr_factor_types* types, const cgmr_mixture* mixture, double* chi2_out);
/* Graduated non-convexity (same ABI version: callers find the entry points by their symbols): outlier rejection by the
 * method of Yang, Antonante, Tzoumas and Carlone (RA-L 2020) as GTSAM's GncOptimizer runs it [recalled: from memory, not read
 * from the paper's or GTSAM's text; the contract is tests/ref_gnc.py].  A truncated-least-squares (TLS) or Geman-McClure (GM)
 * cost is reached from a convex surrogate by stepping a parameter mu; every outer iteration re-weights the edges from their
 * residuals and runs inner_iters Gauss-Newton iterations on the weighted system.  The result is an estimate and a weight per
 * edge (TLS: 0 = rejected).
 *   r_k = e_k^T Omega_k e_k, in the factor's own dimension for a typed edge; c_k = barc_sq[k]; F = the edges not marked
 *   known_inlier (those always have weight 1).
 *   Start, r at the poses passed in:  TLS  mu0 = min over k in F with 2 r_k - c_k > 0 of c_k / (2 r_k - c_k)
 *                                     GM   mu0 = max over k in F of 2 r_k / c_k
 *   Nothing to reject (TLS: no such k; GM: mu0 <= 1; F empty): every weight is 1, one outer iteration runs, mu_out[0] = 0,
 *   *outer_done = 1, and the poses are bit-identical to cgmr_gn_optimize (cgmr_gn_optimize_typed) with iters = inner_iters.
 *   Outer iteration t, at poses x_t with mu_t: weights from r(x_t) --
 *     TLS  up = (mu + 1) / mu c, lo = mu / (mu + 1) c:  w = 0 if r >= up, 1 if r <= lo, else sqrt(c mu (mu + 1) / r) - mu
 *     GM   w = (mu c / (r + mu c))^2
 *   then inner_iters Gauss-Newton iterations with Omega_k replaced by w_k Omega_k, the weights frozen.
 *     mu_out[t] = mu_t; cost_out[t] = sum w_k r_k at x_t; partial_out[t] = number of k in F with 0 < w_k < 1.
 *   Last iteration: TLS the first t with partial_out[t] == 0, GM the t that ran with mu = 1, t = max_outer - 1 at the latest;
 *   *outer_done = t + 1.  Otherwise mu_(t+1) = mu_t mu_factor (TLS), max(1, mu_t / mu_factor) (GM).
 *   End: weight_out = the weights of the last outer iteration (not recomputed), edge_chi2_out = r at the returned poses,
 *   cost_out[outer_done] = sum w r there; mu_out / partial_out behind outer_done are zero, cost_out repeats its last value.
 * A non-positive pivot in inner iteration i, counted over the whole call, returns CGMR_E_CHOLESKY_BASE - i with the poses at
 * the last good update (TLS weights of 0 on every edge of a free vertex do that); the iteration it happened in counts in
 * *outer_done, and weight_out / edge_chi2_out are still written.  CGMR_E_INVALID, before the device is touched: an unknown
 * loss, mu_factor <= 1 or not finite, max_outer / inner_iters / outer_per_wait < 1, a barc_sq that is not finite and > 0, bad
 * kinds (as the typed entry points).  CGMR_E_TIMEOUT as cgmr_lm_optimize.  With one Gauss-Newton step per mu the estimate lags
 * behind mu: at the chi2 0.99 quantile a few true inliers of a graph with many gross outliers are rejected too; a larger
 * barc_sq or more inner iterations avoid that.  The device keeps mu, the weights and the stop test; the host queues
 * outer_per_wait outer iterations per wait, and the result does not depend on that number.  Not combined with cgmr_robust;
 * CGMR_GRAPH capture does not apply to this path. */
#define CGMR_GNC_TLS 0
#define CGMR_GNC_GM 1
typedef struct cgmr_gnc_params {
  int32_t loss;                 /* CGMR_GNC_TLS or CGMR_GNC_GM */
  double mu_factor;             /* > 1; default 1.4 */
  int32_t max_outer;            /* >= 1; default 100 */
  int32_t inner_iters;          /* >= 1; default 1 */
  int32_t outer_per_wait;       /* >= 1; default 8 */
  const double* barc_sq;        /* [nE] host, nullable: default_barc_sq for every edge */
  double default_barc_sq;       /* <= 0: the chi2 0.99 quantile of the factor's dimension (11.344866730144373, 9.21034037197618, 6.634896601021213 for 3, 2, 1) */
  const uint8_t* known_inlier;  /* [nE] host, nullable: none */
  double* weight_out;           /* [nE] host, nullable */
  double* edge_chi2_out;        /* [nE] host, nullable */
} cgmr_gnc_params;
/* TLS, 1.4, 100, 1, 8, no arrays, default_barc_sq 0 (by dimension) */
cgmr_gnc_params cgmr_gnc_params_default(void);
/*   params   nullable: the defaults;  types  nullable: every vertex a pose, every edge an EDGE_SE2
 *   mu_out [max_outer], cost_out [max_outer + 1], partial_out [max_outer], outer_done: nullable */
int cgmr_gnc_optimize(cgmr_ctx* ctx, int nV, double* poses_xyt, const uint8_t* fixed, int nE, const int32_t* from_idx,
                      const int32_t* to_idx, const double* meas_xyt, const double* info_upper, const cgmr_factor_types* types,
                      const cgmr_gnc_params* params, double* mu_out, double* cost_out, int32_t* partial_out, int32_t* outer_done);
/* Device-resident variant (d_poses / d_meas / d_info on the context's device; the per-edge parameter arrays stay host memory):
 * bit-identical to the host variant. */
int cgmr_gnc_optimize_dev(cgmr_ctx* ctx, int nV, double* d_poses_xyt, const uint8_t* fixed, int nE, const int32_t* from_idx,
                          const int32_t* to_idx, const double* d_meas_xyt, const double* d_info_upper,
                          const cgmr_factor_types* types, const cgmr_gnc_params* params, double* mu_out, double* cost_out,
                          int32_t* partial_out, int32_t* outer_done);
/* The last cgmr_gnc_optimize* call on this context: out[0] = host waits for the device, out[1] = inner iterations run. */
int cgmr_gnc_last_stats(const cgmr_ctx* ctx, int64_t out[2]);
/* Chordal initialisation (same ABI version: callers find the entry points by their symbols): a starting point from two linear
 * least-squares problems, as GTSAM's InitializePose and LAGO do [recalled: from memory, not read from either source; the
 * contract is tests/ref_chordal.py].  Linear problems have no basin of attraction: the result does not depend on the estimates
 * passed in, up to rounding.  All information is read from the edge's own 3x3 Omega; the cross terms between translation and
 * heading are ignored by design.
 *   stages bit 0, the rotation stage: unknown r_i = (c_i, s_i) per free pose, omega = Omega(2,2) --
 *     CGMR_EDGE_SE2 (i, j)   omega || r_j - R(z_theta) r_i ||^2
 *     CGMR_EDGE_PRIOR_SE2    omega || r_i - (cos z_theta, sin z_theta) ||^2
 *     every other kind       nothing
 *   A fixed pose is the constant (cos theta, sin theta).  Then theta_i = atan2(s_i, c_i); c_i^2 + s_i^2 = 1 is not imposed.  A
 *   solved (c_i, s_i) of length exactly zero, or not finite, leaves the pose its heading and counts as degenerate.
 *   stages bit 1, the translation stage: unknown t_i per free pose and l per free point, the headings held at their current
 *   values (the rotation stage's when both bits are set), weight Omega[0:2, 0:2] --
 *     CGMR_EDGE_SE2          e = R(z_theta)^T (R_i^T (t_j - t_i) - z_t)
 *     CGMR_EDGE_SE2_XY       e = R_i^T (l - t_i) - z
 *     CGMR_EDGE_PRIOR_SE2    e = R(z_theta)^T (t_i - z_t)
 *     CGMR_EDGE_PRIOR_SE2_XY e = t_i - z
 *     CGMR_EDGE_BEARING_SE2_XY  nothing
 * A vertex that no term of a stage touches -- a point in the rotation stage, a point seen by bearings only, a vertex all of
 * whose information entries for the stage are zero, an isolated vertex -- is left out of that stage and keeps its estimate.
 *   stages       1, 2 or 3; anything else is CGMR_E_INVALID
 *   chi2_out     [2], nullable: the SE(2) chi2 (cgmr_gn_optimize's, cgmr_gn_optimize_typed's) at the estimates passed in and at the result
 *   counts_out   [3], nullable: vertices solved in the rotation stage, in the translation stage, degenerate headings
 * A stage without a gauge -- no fixed pose and no prior reaches some connected component -- is singular: the call returns
 * CGMR_E_CHOLESKY_BASE - p, p the stage's place among the requested ones (0 or 1), and the estimates are those from before
 * that stage; its count and the later stage's are 0.  Chordal relaxation is not robust to wrong loop closures: it is no start
 * for cgmr_gnc_optimize on a graph with outliers.  One host wait; the _dev variants read d_info_upper back once before it (which
 * terms are all zero is decided on the host) and are otherwise bit-identical to the host variants.  CGMR_E_TIMEOUT as
 * cgmr_gn_optimize.  Not offered for the robot graph, condensed graphs or batches. */
#define CGMR_CHORDAL_ROTATION 1
#define CGMR_CHORDAL_TRANSLATION 2
int cgmr_chordal_initialize(cgmr_ctx* ctx, int nV, double* poses_xyt, const uint8_t* fixed, int nE, const int32_t* from_idx,
                            const int32_t* to_idx, const double* meas_xyt, const double* info_upper, int stages,
                            double* chi2_out, int32_t* counts_out);
int cgmr_chordal_initialize_dev(cgmr_ctx* ctx, int nV, double* d_poses_xyt, const uint8_t* fixed, int nE,
                                const int32_t* from_idx, const int32_t* to_idx, const double* d_meas_xyt,
                                const double* d_info_upper, int stages, double* chi2_out, int32_t* counts_out);
/* types nullable (or all zero): the plain call */
int cgmr_chordal_initialize_typed(cgmr_ctx* ctx, int nV, double* poses_xyt, const uint8_t* fixed, int nE,
                                  const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt,
                                  const double* info_upper, int stages, double* chi2_out, int32_t* counts_out,
                                  const cgmr_factor_types* types);
int cgmr_chordal_initialize_typed_dev(cgmr_ctx* ctx, int nV, double* d_poses_xyt, const uint8_t* fixed, int nE,
                                      const int32_t* from_idx, const int32_t* to_idx, const double* d_meas_xyt,
                                      const double* d_info_upper, int stages, double* chi2_out, int32_t* counts_out,
                                      const cgmr_factor_types* types);
/* g2o's SparseOptimizer::computeInitialGuess with unit edge cost [g2o-recalled]: breadth-first from the fixed vertices that
 * have an edge, over the edges in their order, x_to = x_from * z or x_from = x_to * z^-1; a vertex it does not reach keeps its
 * estimate.  Host arrays in and out (poses_xyt in place), no device work, no context.  CGMR_E_INVALID: a null or negative
 * argument, an edge index out of range. */
int cgmr_initial_guess(int nV, double* poses_xyt, const uint8_t* fixed, int nE, const int32_t* from_idx, const int32_t* to_idx,
                       const double* meas_xyt);
int cgmr_marginals_typed(cgmr_ctx* ctx, int nV, const double* poses_xyt, const uint8_t* fixed, int nE,
                         const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt, const double* info_upper,
                         int nK, const int32_t* query_idx, double* cov_out, const cgmr_factor_types* types,
                         const cgmr_robust* rk);
int cgmr_marginals_all_typed(cgmr_ctx* ctx, int nV, const double* poses_xyt, const uint8_t* fixed, int nE,
                             const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt,
                             const double* info_upper, double* cov_out, double* cross_out,
                             const cgmr_factor_types* types, const cgmr_robust* rk);

/* The ordering + symbolic analysis + structure upload of the last analysed edge list stay on the context and are
 * reused by every later call (cgmr_gn_optimize*, cgmr_marginals, cgmr_covariance_estimate, cgmr_condense*) whose
 * (nV, from_idx, to_idx) are exactly the same -- the fixed flags are applied numerically and do not enter the
 * analysis, so the pre-solve, the covariance estimate and the optimize(n) of one key frame
 * (src/slam/graph_slam.cpp:392-393, 315-320; src/srslam.cpp:211) share one analysis.  Results are bit-identical
 * with the cache on or off.  on = 0 switches the reuse off (every call analyses, as g2o does); default on.
 * A graph that GROWS -- the cached edge list plus vertices / edges appended at the end, the key-frame pattern of
 * src/slam/graph_slam.cpp:197-267 and of a multi-robot round -- keeps its ordering: the new vertices are inserted into the
 * cached nested-dissection tree (into the leaf their neighbours live in, or the separator above them), everything
 * downstream of the ordering is rebuilt; after a quarter of the graph has been inserted that way the ordering is computed
 * from scratch again.  Same results as a from-scratch analysis to rounding (another elimination order).
 * cgmr_symbolic_cache_stats (ABI of version 100, two values): out[0] = calls served from the cache, out[1] = calls that
 * analysed (from scratch or by extending the cached ordering).  cgmr_symbolic_cache_stats3 (version >= 101) splits the
 * second: out[1] = analysed from scratch, out[2] = analysed by extending the cached ordering.               */
int cgmr_set_symbolic_cache(cgmr_ctx* ctx, int on);
int cgmr_symbolic_cache_stats(const cgmr_ctx* ctx, int64_t out[2]);
int cgmr_symbolic_cache_stats3(const cgmr_ctx* ctx, int64_t out[3]);
/* The chained backward solve waits, inside one launch, for values other workgroups produce; every wait is bounded.  When
 * one runs out the call does not report a Cholesky failure: cgmr_gn_optimize* repeats the iterations that were not applied
 * with one backward launch per tree level (no in-kernel waits) and returns CGMR_OK; the batched condensed-graph /
 * marginals paths return CGMR_E_TIMEOUT.  cgmr_gn_timeouts: how often that has happened on this context.           */
int64_t cgmr_gn_timeouts(const cgmr_ctx* ctx);
/* The environment switches (same ABI version: callers find the entry point by its symbol).  A context reads every
 * context-scoped CGMR_* variable once, when it is created, and works by those values for its whole life; the process-scoped
 * ones (the host threads, the RCCL library) are read once per process.  cgmr_switches writes one line per switch into buf,
 * "name<TAB>scope<TAB>value<TAB>effect\n", scope = context or process, a flag's value 0 or 1, a path that is not set empty:
 * with a context the values it holds (and the process' own for the process-scoped ones), with a null context the defaults.
 * Returns the bytes the whole listing needs, the terminating zero included; buf (cap bytes, may be null with cap 0) holds as
 * much of it as fits, terminated.  tools/README.md has the table.                                                       */
int cgmr_switches(const cgmr_ctx* ctx_or_null, char* buf, int cap);

/* The host threads behind the symbolic analysis (no reference counterpart: g2o's analysis is one thread).
 * out[0] = threads an analysis uses, the caller included (CGMR_HOST_THREADS, default by core count); out[1] = 1 if the
 * helper threads are pinned around one last-level cache (CGMR_HOST_PIN=0 or an affinity mask that excludes the cores: 0);
 * out[2] = the CPU the caller is held on while it analyses (-1: nowhere); out[3] = CPUs the process may run on;
 * out[4] = times the pool has moved to another cache group because its helpers kept losing their cores to other
 * processes (CGMR_HOST_MOVE=0: never).                                                                                     */
int cgmr_host_threads_info(int32_t out[5]);

/* Host-only: run the ordering / symbolic analysis and report its shape (no GPU needed).
 * out[0]=poses in the system (every vertex with an edge; `fixed` is ignored: fixed vertices are masked numerically)
 * [1]=off-diagonal H blocks  [2]=fronts  [3]=tree levels
 * [4]=doubles in L   [5]=doubles in update matrices  [6]=max border (poses)
 * [7]=factor flops   [8]=ordering microseconds  [9]=structure microseconds
 * [10]=max children of a front  [11]=max children of a front with 1..32 border poses
 * [12]=doubles of the fronts' assembled panels (F11, border rows, rhs row; every copy): what the factor kernel reads
 * [13]=tree levels that are launched one by one: the last fronts of the root's chain are handled together by one extra
 *   launch, the "top block"  [14]=fronts of the top block  [15]=its scalar columns
 * perm_out (nullable, nV entries): permuted block column of each vertex or -1.          */
int cgmr_gn_symbolic_info(int nV, const uint8_t* fixed, int nE, const int32_t* from_idx,
                          const int32_t* to_idx, int64_t out[16], int32_t* perm_out);

/* Host-only: the analysis of a graph that grows.  The first (nV0, nE0) vertices / edges are analysed from scratch, then
 * step k extends the analysis to the first (nV_step[k], nE_step[k]) of them the way cgmr_gn_optimize* does for a context
 * whose cached edge list is a prefix of the new one; out / perm_out describe the last analysis, n_extended_out counts the
 * steps that re-used the ordering (the others fell back to a from-scratch ordering). */
int cgmr_gn_symbolic_info_grown(int nV0, int nE0, int n_steps, const int32_t* nV_step, const int32_t* nE_step,
                                const int32_t* from_idx, const int32_t* to_idx, int64_t out[16], int32_t* perm_out,
                                int32_t* n_extended_out);

/* Timing of the last cgmr_gn_optimize* call on this context, seconds:
 * out[0]=host ordering  [1]=host structure  [2]=upload+alloc  [3]=device GN iterations (stream time,
 * measured with HIP events)  [4]=total wall.                                             */
int cgmr_gn_last_timing(const cgmr_ctx* ctx, double out[5]);

/* Per-kernel-class device time of GN runs made while profiling is on: a HIP event pair around every launch,
 * recorded on the context's stream without synchronising (the stream stays busy, so a pair brackets the kernel,
 * not an idle-to-busy launch latency) and read back after the call's final synchronisation.  At most 2048
 * launches per call are timed.  bench.py uses it for the roofline figure.
 * classes: 0 linearize 1 assemble 2 chi2 3 front_factor 4 front_update 5 top_block (the forward solve rides
 * through front_factor) 6 solve_bwd 7 update
 * seconds_out[8], launches_out[8] are accumulated since profiling was switched on.       */
int cgmr_set_profiling(cgmr_ctx* ctx, int on);
int cgmr_gn_kernel_times(const cgmr_ctx* ctx, double seconds_out[8], int64_t launches_out[8]);
/* ... with the classes added since: 8 front_level = a tree level's factorisation AND its update tiles in one launch
 * (k_front_level, round 6: the levels whose launch is certainly resident at once); 9..11 cgmr_closure_consistency's:
 * 9 the forward solve and the Gram tiles, 10 k_closure_consistency[_inter], 11 the bit words and the clique (cgmr_max_clique_greedy:
 * the clique alone; the exact calls: the exact solver's launches with it) -- zero in a library that does not export
 * those symbols.                                                                                                       */
int cgmr_gn_kernel_times_ex(const cgmr_ctx* ctx, double seconds_out[12], int64_t launches_out[12]);

/* ------------------------------------------------------------------------------------------
 * Correlative scan matcher.
 * Replaces: ScanMatcher::{initializeKernel, initializeGrid, resetGrid, closeScanMatching}
 *           src/matcher/scan_matcher.h:45-53, src/matcher/scan_matcher.cpp:38-189
 *           and underneath CharGrid::{addAndConvolvePoints, subsample, greedySearch}
 *           src/matcher/chargrid.h:127-216, src/matcher/chargrid.cpp:61-308
 * (there is no Matcher::match() in the reference).
 *
 * cgmr_matcher_config mirrors the state a ScanMatcher holds after GraphSLAM::init
 * (src/slam/graph_slam.cpp:58-62) plus the laser description of RobotLaser / LaserParameters.
 * cgmr_matcher_config_close() fills in the reference's close-matcher defaults:
 * grid [-15,15]^2 at 0.025 m, kernel range 0.2 m, kscale 128, window +/-(0.3 m, 0.3 m, 0.2 rad),
 * theta step 0.00625, result bins (0.5, 0.5, 0.2), query subsampling 0.1 m.
 *
 * Limits (every one refused with CGMR_E_INVALID and a message before or by the launch; tests/test_matcher_config_gpu.py
 * holds each of them with a configuration beyond it and, where the limit is a size -- bins, angles, directory, table values,
 * table radius, beams --, one inside it that must match the oracle):
 *   - resolution, theta_res, bin_x / bin_y / bin_theta and subsample_res positive and finite; kscale > 0; the window, the
 *     corners, max_range, min_range and the maxScore of a call finite (to accept every candidate pass a large finite
 *     maxScore); grid_ur beyond grid_ll in both coordinates;
 *   - the grid fits the tile directory: (ceil(nx / 8) + 2) * (ceil(ny / 8) + 7) <= 152 * 157, i.e. 1200 x 1200 cells or a
 *     non-square grid of the same directory size (1400 x 1000);
 *   - the kernel table: radius int(kernel_range / resolution) <= 15 cells, and every value of it fits a signed char as in
 *     the reference (`char distance = K1 * sqrt(..)`): int(resolution * kscale) * sqrt(2) * radius < 128 (which implies
 *     int(kernel_range * kscale) <= 127);
 *   - at most 80 search angles: (2 win_theta) / theta_res + 2 <= 80; at most 128 result bins inside a window;
 *   - n_beams <= 1088.
 * Inside these limits every configuration is bit-identical to the reference's arithmetic; which device code serves it
 * (cgmr_match_last_launch_shape, cgmr_match_last_path_counts) depends on the configuration: the fast search needs cell counts
 * that are multiples of 8 and a fill value int(kernel_range * kscale) <= 63.                */
typedef struct cgmr_matcher_config {
  float grid_ll_x, grid_ll_y, grid_ur_x, grid_ur_y;   /* initializeGrid(lowerLeft, upperRight, res) */
  double resolution;                                  /* grid resolution and kernel resolution      */
  double kernel_range;                                /* initializeKernel(resolution, kernelRange)  */
  int kscale;                                         /* 128 (scan_matcher.cpp:35)                  */
  double win_x, win_y, win_theta;                     /* half widths of the search window           */
  double theta_res;
  double bin_x, bin_y, bin_theta;                     /* resultsDiscretization                      */
  double subsample_res;
  /* laser */
  int n_beams;
  double angle_min, angle_inc, max_range, min_range;
  double laser_pose[3];                               /* laserParams().laserPose (x, y, theta)      */
} cgmr_matcher_config;

void cgmr_matcher_config_close(cgmr_matcher_config* cfg, int n_beams, double angle_min, double angle_inc,
                               double max_range);

/* Batched bool ScanMatcher::closeScanMatching(vset, origin, current, SE2* trel, double maxScore)
 * (src/matcher/scan_matcher.cpp:112-189) for n_pairs independent (reference scan, current scan) pairs,
 * each with a single-scan reference set whose vertex is the origin vertex:
 *   ranges_ref / ranges_qry [n_pairs * n_beams] float32   raw laser ranges (sensor_msgs/LaserScan order)
 *   guess_xyt  [n_pairs * 3]   origin^-1 * current (the odometry guess)
 *   out_xyt    [n_pairs * 3]   matched relative pose (mresvec[0]); zeros when not found
 *   out_score  [n_pairs]       score of that result
 *   out_found  [n_pairs]       the bool return value
 *   out_nresults (nullable) [n_pairs]  number of entries mresvec would have had (the reference only prints it,
 *                              scan_matcher.cpp:155-157).  NULL -- the reference's call -- selects the pruned search:
 *                              candidates that provably cannot be mresvec[0] are dropped early, xyt / score / found
 *                              are the exhaustive search's bit for bit; with a pointer every candidate is evaluated.
 * Host-pointer variant copies in and out; the _dev variant takes device pointers for every array.   */
int cgmr_match_close_batch(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, int n_pairs, const float* ranges_ref,
                           const float* ranges_qry, const double* guess_xyt, double max_score, double* out_xyt,
                           double* out_score, uint8_t* out_found, int32_t* out_nresults);
int cgmr_match_close_batch_dev(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, int n_pairs,
                               const float* d_ranges_ref, const float* d_ranges_qry, const double* d_guess_xyt,
                               double max_score, double* d_out_xyt, double* d_out_score, uint8_t* d_out_found,
                               int32_t* d_out_nresults);
/* The same with the reference's real call shape: GraphSLAM::addDataSM / findConstraints always pass the last vertex
 * and up to 5 predecessors as the reference set (src/slam/graph_slam.cpp:230-244; scan_matcher.cpp:119-127 rasterises
 * all of them into one grid).  Every pair has n_ref_scans (1..6) reference scans; a set with fewer is padded with
 * all-zero scans (no valid beam).
 *   ranges_ref   [n_pairs * n_ref_scans * n_beams]
 *   ref_rel_xyt  [n_pairs * n_ref_scans * 3]   origin^-1 * v_k of every scan (zeros for the origin vertex itself)
 * The _dev variant takes, instead of ref_rel_xyt, d_ref_xform [n_pairs * n_ref_scans * 4] = (cos, sin, tx, ty) of
 * (origin^-1 * v_k) * laserPose as cgmr_scan_transforms() (host, libm -- what applyTransfToScan uses) computes them. */
int cgmr_match_close_vset_batch(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, int n_pairs, int n_ref_scans,
                                const float* ranges_ref, const double* ref_rel_xyt, const float* ranges_qry,
                                const double* guess_xyt, double max_score, double* out_xyt, double* out_score,
                                uint8_t* out_found, int32_t* out_nresults);
int cgmr_match_close_vset_batch_dev(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, int n_pairs, int n_ref_scans,
                                    const float* d_ranges_ref, const double* d_ref_xform, const float* d_ranges_qry,
                                    const double* d_guess_xyt, double max_score, double* d_out_xyt, double* d_out_score,
                                    uint8_t* d_out_found, int32_t* d_out_nresults);
int cgmr_scan_transforms(const cgmr_matcher_config* cfg, int n, const double* rel_xyt, double* xform_out);
/* out[0] = pairs of the last batched close-matching launch, out[1] = those whose grid tiles did not fit the LDS pool
 * (they take the slower generic search path; same results) */
int cgmr_match_last_stats(const cgmr_ctx* ctx, int64_t out[2]);
/* Pairs of the last batched close-matching launch that the kernel instance built for the common shape (one reference scan, the
 * shipped grid and kernel) handed to the general kernel (same results; such a pair is prepared twice).  0 when the general
 * kernel ran alone (CGMR_MATCH_LEAN=0, reference sets of several scans, single calls). */
int cgmr_match_last_redo_pairs(const cgmr_ctx* ctx, int64_t* out);
/* How the pairs of the last batched close-matching launch were searched, beyond the common case: out[0] = pairs whose reference
 * scan claimed more grid tiles than the LDS pool holds and borrowed half of the point lists for them (half the wavefronts search;
 * beyond that come the "slow pairs" of cgmr_match_last_stats); out[1..3] = the pairs of cgmr_match_last_redo_pairs by cause:
 * [1] the reference grid (tiles beyond LDS, or a cell off the grid whose stamp reaches in), [2] the search window or the point
 * count (more than 32 offsets along an axis, more points than one list holds), [3] an angle whose point lists did not fit. */
int cgmr_match_last_path_counts(const cgmr_ctx* ctx, int64_t out[4]);
/* What the host chose for the last batched close-matching launch from the configuration and the batch size (read-only):
 * out[0] = 1 the distance-transform rasteriser / 0 the compare-and-swap stamping one (kernel radius above 8 cells, or a table
 * that is not a non-decreasing function of the squared distance); out[1] = 1 32-bit / 0 64-bit subsample sort keys;
 * out[2] = 1 when the lean kernel instance ran in front of the general one; out[3] = workgroups per pair (split). */
int cgmr_match_last_launch_shape(const cgmr_ctx* ctx, int64_t out[4]);
/* Device time (HIP events on the context's stream) of the last matcher launch, seconds. */
int cgmr_match_last_kernel_seconds(const cgmr_ctx* ctx, double* seconds);

/* ------------------------------------------------------------------------------------------
 * Marginal covariances and condensed measurements.
 *
 * cgmr_marginals: 3x3 diagonal blocks of H^-1 for the query vertices, H linearised at poses_xyt with
 * the given fixed flags.  Replaces SparseOptimizer::computeMarginals(spinv, {(h,h)}) as called at
 * src/slam/graph_manipulator.cpp:134-142.  Fixed / inactive query vertices get zeros.  cov_out [nK*9].
 *
 * cgmr_covariance_estimate: CovarianceEstimator::{setVertices,setGauge,compute,getCovariance}
 * (src/slam/graph_manipulator.cpp:128-157; caller GraphSLAM::checkCovariance, src/slam/graph_slam.cpp:311-354):
 * push state, fix exactly the gauge, spanning-tree initial guess over all edges, one GN iteration, marginals
 * of that iteration's Hessian, pop state (the caller's poses are never modified).
 *
 * cgmr_condense: CondensedGraphCreator::{setVertices,setGauge,setEdges,compute,getCondensedGraph}
 * (src/mrslam/condensed_graph/condensed_graph_creator.cpp:33-66): the same manipulation restricted to the
 * given (own) edges, then one star edge gauge -> v per other query vertex, labelled by g2o_hierarchical's
 * EdgeLabeler: measurement = relative pose after the iteration, information = inverse of the unscented-
 * transformed marginal covariance.  query_idx holds nK vertex indices *including* the gauge; outputs are
 * written for the nK-1 others in query order: to_out [nK-1], est_out [(nK-1)*3], info_upper_out [(nK-1)*6],
 * cov_out (nullable) [(nK-1)*9].  Returns the number of edges (>= 0) or an error (< 0).            */
int cgmr_marginals(cgmr_ctx* ctx, int nV, const double* poses_xyt, const uint8_t* fixed, int nE,
                   const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt, const double* info_upper,
                   int nK, const int32_t* query_idx, double* cov_out);
/* cgmr_marginals_all: the covariance of every pose, and of every edge's pair of poses, in one call -- what
 * SparseOptimizer::computeMarginals over all vertices gives [g2o-recalled].  H is linearised at poses_xyt with the given
 * fixed flags, as for cgmr_marginals; the caller's poses are not modified.
 *   cov_out   [nV*9]            cov_out[v] = the 3x3 block Sigma_vv of H^-1, row-major (x, y, theta).
 *   cross_out [nE*9] nullable   cross_out[e] = the block Sigma_{from,to}: rows index the from vertex, columns the to vertex.
 * Fixed and inactive vertices get exact zeros, and so does every edge with such an endpoint; duplicate edges get
 * identical blocks.  Computed by selected inversion (the Takahashi recurrence) on the supernodal factor, top-down over the
 * elimination tree: device memory grows with the factor (every front keeps its dense block of H^-1 on its own rows,
 * (3 (block columns + border block rows))^2 doubles each), not with the number of poses asked for.  Shares the analysis
 * cache with the other entry points (a call right after cgmr_gn_optimize on the same edge list is a hit).  Returns
 * CGMR_OK, CGMR_E_INVALID for a bad argument, CGMR_E_CHOLESKY_BASE when the factorisation fails, CGMR_E_TIMEOUT as
 * cgmr_marginals does.                                                                                                   */
int cgmr_marginals_all(cgmr_ctx* ctx, int nV, const double* poses_xyt, const uint8_t* fixed, int nE,
                       const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt,
                       const double* info_upper, double* cov_out, double* cross_out);
int cgmr_covariance_estimate(cgmr_ctx* ctx, int nV, const double* poses_xyt, int nE, const int32_t* from_idx,
                             const int32_t* to_idx, const double* meas_xyt, const double* info_upper, int gauge_idx,
                             int nK, const int32_t* query_idx, double* cov_out);
int cgmr_condense(cgmr_ctx* ctx, int nV, const double* poses_xyt, int nE, const int32_t* from_idx,
                  const int32_t* to_idx, const double* meas_xyt, const double* info_upper, int gauge_idx, int nK,
                  const int32_t* query_idx, int32_t* to_out, double* est_out, double* info_upper_out, double* cov_out);
/* The four calls above with robust kernels (cgmr_robust; present in C ABI version 105 libraries that export these symbols):
 * every edge's information is scaled by rho1 at the linearisation point of the H that is inverted (see cgmr_robust above: the
 * poses given for the marginals, the spanning-tree guess for covariance_estimate / condense).  edge_chi2_out / weight_out
 * receive e2 and rho1 there (not written when no pass runs: no free vertex, or no query left).  rk == NULL: the plain call,
 * bit for bit; so is a description whose kinds are all CGMR_RK_NONE.  A bad kind or delta is CGMR_E_INVALID before anything
 * is queued.  A zero weight that leaves a free vertex's block singular (Tukey, Saturated) gives CGMR_E_CHOLESKY_BASE, as a
 * singular H does in the plain calls; the bounded-wait time-out is handled as there. */
int cgmr_marginals_robust(cgmr_ctx* ctx, int nV, const double* poses_xyt, const uint8_t* fixed, int nE,
                          const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt, const double* info_upper,
                          int nK, const int32_t* query_idx, double* cov_out, const cgmr_robust* rk);
int cgmr_marginals_all_robust(cgmr_ctx* ctx, int nV, const double* poses_xyt, const uint8_t* fixed, int nE,
                              const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt,
                              const double* info_upper, double* cov_out, double* cross_out, const cgmr_robust* rk);
int cgmr_covariance_estimate_robust(cgmr_ctx* ctx, int nV, const double* poses_xyt, int nE, const int32_t* from_idx,
                                    const int32_t* to_idx, const double* meas_xyt, const double* info_upper, int gauge_idx,
                                    int nK, const int32_t* query_idx, double* cov_out, const cgmr_robust* rk);
int cgmr_condense_robust(cgmr_ctx* ctx, int nV, const double* poses_xyt, int nE, const int32_t* from_idx,
                         const int32_t* to_idx, const double* meas_xyt, const double* info_upper, int gauge_idx, int nK,
                         const int32_t* query_idx, int32_t* to_out, double* est_out, double* info_upper_out, double* cov_out,
                         const cgmr_robust* rk);

/* Joint and pairwise marginal covariances, and the uncertainty of a relative pose (present in C ABI version 105 libraries that
 * export these symbols).  cgmr_marginals gives Sigma_vv, cgmr_marginals_all Sigma_ij for the graph's edges; these give
 * Sigma_ij for ANY two poses -- SparseOptimizer::computeMarginals(spinv, blockIndices) with arbitrary (i, j) [g2o-recalled].
 * H is linearised at poses_xyt with the given fixed flags, exactly as for cgmr_marginals; the caller's poses are not
 * modified.  rk (nullable, last): robust kernels as for cgmr_marginals_robust; NULL is the plain call.  All three share the
 * analysis cache and the bounded-wait fall-back of cgmr_marginals, and return CGMR_OK, CGMR_E_INVALID (null context, null
 * or negative argument, an index outside [0, nV), too many query vertices -- all before anything is queued),
 * CGMR_E_CHOLESKY_BASE (outputs zeroed), CGMR_E_TIMEOUT, CGMR_E_HIP / _ALLOC.  Two calls give identical bytes.
 *
 * The work is Y = L^-1 E for 4 columns per UNIQUE query vertex (the forward solve of cgmr_marginals), then the 16x16 tiles of
 * Y^T Y that hold a requested block.  Device memory: Y takes 32 bytes x 3 x free poses per unique query vertex; the Gram
 * tiles of the dense joint call take (u / 4)(u / 4 + 1) KiB for u unique vertices.  CGMR_JOINT_MAX_QUERIES bounds u in all
 * three calls: at the limit Y is 64 KiB per row of H (1.8 GiB for 10 000 poses) and the dense tiles are 257 MiB.
 *
 * cgmr_marginals_joint: cov_out [(3 nK)^2], row-major, the joint covariance of the query vertices in query order: block
 *   (k, l) = Sigma_{query[k], query[l]}.  Exactly symmetric.  Fixed / inactive queries give exact zero rows and columns, a
 *   vertex listed twice gives identical rows and columns.  nK == 0: CGMR_OK, nothing written.
 * cgmr_marginals_pairs: for pair p the blocks Sigma_aa, Sigma_ab (rows index pair_a[p], columns pair_b[p]) and Sigma_bb,
 *   each output [nP * 9] and nullable.  The unique vertices of the pairs form the query set; only the tiles that hold a
 *   requested block are contracted.  A pair with a fixed / inactive end gives a zero Sigma_ab; pair (a, a) gives
 *   aa == ab == bb.  nP == 0: CGMR_OK, nothing written.
 * cgmr_relative_covariance: for pair p, rel_xyt_out [nP * 3] = z = x_a^-1 x_b at poses_xyt and rel_cov_out [nP * 9] =
 *   Sigma_z = J_a Sigma_aa J_a^T + J_a Sigma_ab J_b^T + J_b Sigma_ab^T J_a^T + J_b Sigma_bb J_b^T, J_a / J_b the Jacobians of
 *   z for the additive (x, y, theta) update (EdgeSE2's, zero measurement).  With a hypothesis per pair -- hyp_meas_xyt
 *   [nP * 3] and hyp_info_upper [nP * 6] (nullable: no measurement noise) -- d2_out [nP] = e^T (J_e Sigma_z J_e^T +
 *   Omega^-1)^-1 e, e the EdgeSE2 error of the hypothesis at z: the squared Mahalanobis distance a closure candidate is
 *   gated on; NaN where that 3x3 matrix is not positive definite.  rel_xyt_out, rel_cov_out, d2_out are nullable; d2_out
 *   needs hyp_meas_xyt.                                                                                                 */
#define CGMR_JOINT_MAX_QUERIES 2048
int cgmr_marginals_joint(cgmr_ctx* ctx, int nV, const double* poses_xyt, const uint8_t* fixed, int nE,
                         const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt, const double* info_upper,
                         int nK, const int32_t* query_idx, double* cov_out, const cgmr_robust* rk);
int cgmr_marginals_pairs(cgmr_ctx* ctx, int nV, const double* poses_xyt, const uint8_t* fixed, int nE,
                         const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt, const double* info_upper,
                         int nP, const int32_t* pair_a, const int32_t* pair_b, double* cov_aa_out, double* cov_ab_out,
                         double* cov_bb_out, const cgmr_robust* rk);
int cgmr_relative_covariance(cgmr_ctx* ctx, int nV, const double* poses_xyt, const uint8_t* fixed, int nE,
                             const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt, const double* info_upper,
                             int nP, const int32_t* pair_a, const int32_t* pair_b, double* rel_xyt_out, double* rel_cov_out,
                             const double* hyp_meas_xyt, const double* hyp_info_upper, double* d2_out, const cgmr_robust* rk);

/* The same on typed factors (cgmr_factor_types above; present in C ABI version 105 libraries that export these symbols).
 * cgmr_marginals_joint_typed / cgmr_marginals_pairs_typed: the plain calls' arguments, then types and rk as the other typed
 * entry points take them; the kinds are checked as there (CGMR_E_INVALID names the edge) before the device is touched.  A
 * point's third row and column are exactly zero in every block (the joint matrix's rows and columns 3 k + 2; aa, ab, bb);
 * the joint matrix stays exactly symmetric; two calls give identical bytes.  types == NULL, a null member or all-zero kinds:
 * the plain call bit for bit.  Limits, errors and zero rules are those of the plain calls.
 *
 * cgmr_observation_covariance: data association.  Pair p is predicted as a factor of kind obs_kind[p] (host, [nP]; NULL: all 0)
 * from pose pair_a[p] to vertex pair_b[p], at poses_xyt, with the covariance S = J Sigma J^T of that prediction:
 *   0  b a pose: exactly cgmr_relative_covariance (with types == NULL on a pose graph, bit for bit)
 *   1  b a point: z = R_a^T (l - t_a); J = [A rows 0-1 | R_a^T] (2x5), A as in EdgeSE2PointXY; Sigma the 5x5 joint covariance
 *      of (x_a, l).  Hypothesis: e = z - zh (hyp_meas_xyt[0, 1]), Omega from hyp_info_upper[0, 1, 3]
 *   2  b a point: z = atan2(ry, rx); J the 1x5 bearing row; e = normalize(z - zh[0]); Omega = hyp_info_upper[0].  With the
 *      point on the pose (rx = ry = 0): z = 0, S and d2 are NaN
 * d2_out [nP] = e^T (S + Omega^-1)^-1 e in the factor's own dimension (hyp_info_upper NULL: no Omega term); NaN where that
 * matrix is not positive definite (a pair with both ends fixed and no Omega, for one).  z_out [nP * 3] and cov_out [nP * 9] are
 * padded with exact zeros outside the factor's dimension.  Nullability as in cgmr_relative_covariance.  CGMR_E_INVALID, naming
 * the pair and before anything is queued: an obs_kind above 2, pair_a[p] a point, kind 0 with b a point, kind 1 / 2 with b a
 * pose.  One thread per pair after the pairs' blocks of cgmr_marginals_pairs_typed, which stay on the device. */
int cgmr_marginals_joint_typed(cgmr_ctx* ctx, int nV, const double* poses_xyt, const uint8_t* fixed, int nE,
                               const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt,
                               const double* info_upper, int nK, const int32_t* query_idx, double* cov_out,
                               const cgmr_factor_types* types, const cgmr_robust* rk);
int cgmr_marginals_pairs_typed(cgmr_ctx* ctx, int nV, const double* poses_xyt, const uint8_t* fixed, int nE,
                               const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt,
                               const double* info_upper, int nP, const int32_t* pair_a, const int32_t* pair_b,
                               double* cov_aa_out, double* cov_ab_out, double* cov_bb_out, const cgmr_factor_types* types,
                               const cgmr_robust* rk);
int cgmr_observation_covariance(cgmr_ctx* ctx, int nV, const double* poses_xyt, const uint8_t* fixed, int nE,
                                const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt,
                                const double* info_upper, int nP, const int32_t* pair_a, const int32_t* pair_b,
                                const uint8_t* obs_kind, double* z_out, double* cov_out, const double* hyp_meas_xyt,
                                const double* hyp_info_upper, double* d2_out, const cgmr_factor_types* types,
                                const cgmr_robust* rk);

/* Pairwise consistency maximisation (PCM) of closure candidates (present in C ABI version 105 libraries that export these
 * symbols).  Where cgmr_relative_covariance gates one hypothesis at a time, these ask whether two candidates agree with EACH
 * OTHER, given what the graph knows about the poses between them, and keep the largest set whose members all agree pairwise:
 * what LoopClosureChecker::check (src/slam/closure_checker.cpp) decides by making each candidate exact in turn and counting
 * the others' chi2 under a constant information.  Pose graphs only.
 *
 * Candidate k = (cl_a[k], cl_b[k], z_k = cl_meas_xyt[3 k ..], Omega_k = cl_info_upper[6 k ..]) measures x_a^-1 x_b; the
 * candidates are not edges of the graph.  With (+) the SE(2) composition on (x, y, theta), theta normalised to (-pi, pi], the
 * loop residual of the pair l < k is
 *   eps_kl = z_k (+) (x_bk^-1 (+) x_bl) (+) z_l^-1 (+) (x_al^-1 (+) x_ak)            (the identity when both agree with the graph)
 * with the first-order covariance
 *   S_kl = J_x Sigma J_x^T + J_zk Omega_k^-1 J_zk^T + J_zl Omega_l^-1 J_zl^T
 * Sigma the 12x12 joint covariance of (x_ak, x_bk, x_al, x_bl) at poses_xyt with the given fixed flags, exactly as
 * cgmr_marginals_joint returns it (cross-covariances included; shared, repeated, fixed and inactive vertices as there), the
 * Jacobians for additive (x, y, theta) updates.  d2_out [nC * nC], row-major: d2[k][l] = d2[l][k] = eps_kl^T S_kl^-1 eps_kl,
 * computed once per unordered pair; NaN where S_kl is not finite or not positive definite; exactly 0 on the diagonal.
 * Adjacency: k ~ l iff k != l and d2[k][l] < gamma (NaN is not adjacent).  adj_out [nC * W], W = (nC + 63) / 64: bit (l & 63)
 * of word k * W + (l >> 6); padding bits are zero.
 *
 * The clique (deterministic): from a seed s, C = {s} and P = A[s]; while P is not empty, the u in P with the largest
 * |A[u] & P| (ties: the lowest index) joins C and P &= A[u].  The result is the C of largest size over all seeds (ties: the
 * lowest seed): clique_out [nC] its members ascending, -1 behind them, clique_size_out [1], seed_out [1].  A graph without
 * an edge gives size 1 from seed 0.  This is the greedy heuristic that PCM implementations use: the set is a maximal clique,
 * NOT necessarily a maximum one -- it is not an exact solver.
 *
 * cgmr_closure_consistency: the nine graph arguments of cgmr_marginals, then the candidates (all four arrays required),
 *   gamma (a chi2 quantile with 3 degrees of freedom: 11.344866730144373 for 0.99), the outputs -- d2_out and adj_out nullable,
 *   the clique's three nullable together -- and rk (nullable, last) as for cgmr_marginals_joint.  The work is that call's over
 *   the unique endpoints (at most 2 nC <= CGMR_JOINT_MAX_QUERIES; its device memory: Y and every lower Gram tile, which stay
 *   on the device), one thread per pair on the tiles, one workgroup per seed; plus 8 nC^2 bytes of d2.  Analysis cache,
 *   bounded-wait fall-back, return codes and their order as for cgmr_marginals_joint (CGMR_E_CHOLESKY_BASE: outputs zeroed,
 *   size 0).  The caller's poses are not modified; two calls give identical bytes.
 * cgmr_max_clique_greedy: the clique alone on a caller's adjacency words adj_bits (host, [n * W], the layout above).
 * Both return CGMR_E_INVALID, naming the closure or the word in cgmr_last_error and before anything is queued, for: a null
 * context or a null required pointer, a negative count, nC or n above CGMR_PCM_MAX_CLOSURES, an endpoint outside [0, nV), a
 * gamma that is not finite or <= 0; for cgmr_max_clique_greedy a set diagonal bit, an asymmetric bit or a set padding bit.
 * nC == 0 / n == 0: CGMR_OK, clique_size_out = 0 (where given) and nothing else written. */
#define CGMR_PCM_MAX_CLOSURES 1024   /* 2 nC unique endpoints <= CGMR_JOINT_MAX_QUERIES */
int cgmr_closure_consistency(cgmr_ctx* ctx, int nV, const double* poses_xyt, const uint8_t* fixed, int nE,
                             const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt, const double* info_upper,
                             int nC, const int32_t* cl_a, const int32_t* cl_b, const double* cl_meas_xyt,
                             const double* cl_info_upper, double gamma, double* d2_out, uint64_t* adj_out,
                             int32_t* clique_out, int32_t* clique_size_out, int32_t* seed_out, const cgmr_robust* rk);
int cgmr_max_clique_greedy(cgmr_ctx* ctx, int n, const uint64_t* adj_bits, int32_t* clique_out, int32_t* clique_size_out,
                           int32_t* seed_out);

/* The exact maximum clique, as published PCM keeps it (present in C ABI version 105 libraries that export these symbols).
 * cgmr_max_clique_exact is cgmr_max_clique_greedy, and cgmr_closure_consistency_exact is cgmr_closure_consistency, with a
 * branch and bound behind the greedy clique; arguments, checks, error texts and their order are the greedy pair's, with
 * proven_out in seed_out's place and node_limit <= 0 refused as CGMR_E_INVALID as well.  The result is never smaller than the
 * greedy call's.
 *
 * The search (deterministic; csrc/clique_exact_kernels.hip).  The greedy clique G of the call above is the lower bound.  The
 * vertices are ordered by ascending degree, ties by ascending index.  One sub-problem per root vertex r: C = {r}, P = the
 * neighbours of r later in the order.  A node (C, P) is expanded as follows.  P empty: C is kept if larger than the best
 * known to this root (at first |G|, or the round's bound below).  Otherwise P is coloured greedily -- the uncoloured vertices
 * are taken from the last in the order to the first; a vertex joins the current class unless adjacent to one already in it;
 * when none is left to try, the next class opens -- and the node is left if |C| + classes <= best.  Else the last vertex
 * coloured, v, joins: the child (C + v, P & A[v]) is expanded, and then the node itself again with P - v.  Every root stops
 * after node_limit nodes, its own root node counted; a stopped root keeps the best clique it has found.  Two rounds: in the
 * first every root runs with the bound |G|; in the second the roots that were stopped run again from their root node, with
 * the largest size of the first round as the bound.  Bounds pass between rounds only, never between the roots of a round.
 * The result: the largest clique over roots, ties to the root first in the order; of one root the second round's, and in a
 * round the first of its final size that the search met; G itself when no root found a larger one.  This need not be the
 * lexicographically smallest maximum clique.
 *   clique_out [n] the members ascending, -1 behind them; clique_size_out [1];
 *   proven_out [1]: 1 when no root was stopped in its last round -- the size is the clique number --, else 0: the set is
 *     still a clique and still at least as large as the greedy one;
 *   nodes_out [1] (nullable): the nodes expanded over all roots and rounds, at most 2 n node_limit.
 * Work: one wavefront per root, at most 2 n node_limit nodes per call; device memory 8 n^2 W bytes of search stack (one set
 * per root and depth; 128 MiB at n = 1024) beside the greedy call's.  Two calls give identical bytes in every output.
 * CGMR_EXACT_DEFAULT_NODE_LIMIT is what the Python binding passes: the largest power of two for which a call in which every
 * one of 1024 roots is stopped in both rounds stays under 0.5 s on an MI355X.  Measured: a node costs one
 * colouring of its candidate set, so the rate falls with the graph's density -- 4.1e7 nodes/s over a call on G(1024, 0.5),
 * 1.0e6 on G(1024, 0.995), where the slowest workgroup expands 3.9e3 nodes/s and spends its whole budget: 265 ms of device
 * time at node_limit 512, 524 ms at 1024.  The closure sets of DESIGN.md 2.14 are proven at the root nodes (N nodes). */
#define CGMR_EXACT_DEFAULT_NODE_LIMIT 512
int cgmr_closure_consistency_exact(cgmr_ctx* ctx, int nV, const double* poses_xyt, const uint8_t* fixed, int nE,
                                   const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt,
                                   const double* info_upper, int nC, const int32_t* cl_a, const int32_t* cl_b,
                                   const double* cl_meas_xyt, const double* cl_info_upper, double gamma, double* d2_out,
                                   uint64_t* adj_out, int64_t node_limit, int32_t* clique_out, int32_t* clique_size_out,
                                   int32_t* proven_out, const cgmr_robust* rk);
int cgmr_max_clique_exact(cgmr_ctx* ctx, int n, const uint64_t* adj_bits, int64_t node_limit, int32_t* clique_out,
                          int32_t* clique_size_out, int32_t* proven_out, int64_t* nodes_out);

/* Inter-robot PCM: the two-graph form of the test, as published PCM states it (present in C ABI version 105 libraries that
 * export these symbols).  A candidate between this robot and a peer ends at a vertex that is in no graph until it is accepted,
 * so cgmr_closure_consistency cannot take it.  Here candidate k = (cl_a[k], p_k = peer_pose_xyt[3 k ..], z_k, Omega_k): cl_a[k]
 * an own vertex (an index into the graph), p_k the peer vertex's pose as the peer sent it, in the peer's frame, z_k a
 * measurement of x_a^-1 x_p.  The loop residual of the pair l < k is
 *   eps_kl = z_k (+) (p_k^-1 (+) p_l) (+) z_l^-1 (+) (x_al^-1 (+) x_ak)
 * -- cgmr_closure_consistency's with x_b replaced by p; only the peer's relative pose enters, so its frame does not matter --
 * with the first-order covariance
 *   S_kl = J_a Sigma_a J_a^T + J_p Sigma_p J_p^T + J_zk Omega_k^-1 J_zk^T + J_zl Omega_l^-1 J_zl^T
 * Sigma_a the 6x6 joint covariance of (x_ak, x_al) exactly as cgmr_marginals_joint returns it (shared, repeated, fixed and
 * inactive vertices as there), Sigma_p the 6x6 sub-matrix at candidates (k, l) of peer_cov [3 nC * 3 nC] (host, row-major,
 * indexed by candidate: rows 3 k .. 3 k + 2 are p_k's; two candidates at one peer vertex repeat its rows).  Only the lower
 * triangle of peer_cov is read, so (i, j) and (j, i) are the same double.  The two graphs share no factor: no cross term
 * between Sigma_a and Sigma_p; correlations between the own graph and peer vertices already accepted into it are ignored.
 * peer_cov == NULL: Sigma_p = 0, the peer's poses are taken as exact -- how LoopClosureChecker treats them, and all that the
 * reference's wire format allows (a peer's vertices arrive as bare poses).  This UNDER-states S, so the gate d2 < gamma is
 * stricter than the data justify: consistent candidates may be refused; inconsistent ones are not let in by it.  A null
 * peer_cov and an all-zero one give identical bytes.
 * d2_out, the adjacency, the clique (greedy; _exact: the branch and bound behind it), output nullability, nC == 0, the limit
 * CGMR_PCM_MAX_CLOSURES, analysis cache, bounded-wait fall-back, return codes and their order, the zeroed outputs on
 * CGMR_E_CHOLESKY_BASE and the launch classes 9..11 are those of cgmr_closure_consistency[_exact]; class 10 is
 * k_closure_consistency_inter.  Device memory: cgmr_marginals_joint's at the unique own endpoints (at most nC, where the
 * single-graph call has up to 2 nC), plus 8 nC^2 bytes of d2, plus 72 nC^2 bytes when peer_cov is given.
 * CGMR_E_INVALID, before anything is queued and with the candidate named in cgmr_last_error, for every reason
 * cgmr_closure_consistency[_exact] refuses a call (cl_a[k] outside [0, nV) among them), a null peer_pose_xyt with nC > 0, a
 * peer pose that is not finite, a peer_cov with an entry in its lower triangle that is not finite, or with a negative
 * diagonal entry. */
int cgmr_closure_consistency_inter(cgmr_ctx* ctx, int nV, const double* poses_xyt, const uint8_t* fixed, int nE,
                                   const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt,
                                   const double* info_upper, int nC, const int32_t* cl_a, const double* peer_pose_xyt,
                                   const double* peer_cov, const double* cl_meas_xyt, const double* cl_info_upper, double gamma,
                                   double* d2_out, uint64_t* adj_out, int32_t* clique_out, int32_t* clique_size_out,
                                   int32_t* seed_out, const cgmr_robust* rk);
int cgmr_closure_consistency_inter_exact(cgmr_ctx* ctx, int nV, const double* poses_xyt, const uint8_t* fixed, int nE,
                                         const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt,
                                         const double* info_upper, int nC, const int32_t* cl_a, const double* peer_pose_xyt,
                                         const double* peer_cov, const double* cl_meas_xyt, const double* cl_info_upper,
                                         double gamma, double* d2_out, uint64_t* adj_out, int64_t node_limit,
                                         int32_t* clique_out, int32_t* clique_size_out, int32_t* proven_out,
                                         const cgmr_robust* rk);

/* Joint-compatibility data association of landmark observations: Neira and Tardos' joint compatibility branch and bound, JCBB
 * (present in C ABI version 105 libraries that export these symbols).  cgmr_observation_covariance gates every (measurement,
 * landmark) pair on its own; the innovations of one scan share the pose error, so two pairings that each pass can fail
 * together.  These return the assignment.
 *
 * Observation i = 0 .. nM - 1 is made from a pose a_i in dimension d_i (2: EDGE_SE2_XY, 1: EDGE_BEARING_SE2_XY) with the
 * measurement zh_i and the noise covariance R_i; the candidates j = 0 .. nL - 1 are distinct point landmarks.  Pair (i, j) has
 * the innovation e_ij = z(a_i, l_j) - zh_i (a bearing's normalised), the Jacobian J_ij (d_i x 5) with respect to (x_ai, l_j)
 * exactly as in cgmr_observation_covariance, and the individual distance ic_ij = e^T (J Sigma J^T + R_i)^-1 e.  A hypothesis
 * h[i] in {-1} or [0, nL) is injective on its pairings.  Its joint distance d2_H = e_H^T C_H^-1 e_H: e_H stacks the paired
 * innovations in observation order (dof D = the sum of their d_i); C_H has for paired i, k the block
 * J_i Sigma_{(ai, h[i]), (ak, h[k])} J_k^T from the four cross blocks of Sigma, plus R_i on the diagonal blocks.  A test passes
 * iff the distance is finite and < gamma_by_dof[dof] (host, [2 nM + 1], entry 0 unused; the caller owns the confidence
 * level); NaN or a pivot of the Cholesky factorisation of C_H that is not positive and finite fails.  A hypothesis is
 * ADMISSIBLE iff every pairing passes on its own (ic_ij < gamma[d_i]) and, for every i, its restriction to the observations
 * 0 .. i passes jointly -- JCBB's prefix rule: the admissible set does not depend on the traversal, and it is smaller than
 * "every jointly compatible subset".  The result is an admissible hypothesis with the most pairings, among those one with the
 * smallest d2_H.
 *
 * The search (deterministic; csrc/jcbb_kernels.hip).  The candidates of observation i are its individually compatible
 * landmarks in ascending (ic, j).  The greedy hypothesis is the lower bound: observations in order, each takes its first
 * candidate that is unused and keeps the hypothesis jointly compatible, else none.  One sub-problem per root, an individually
 * compatible pair (i0, j): the observations before i0 unpaired, i0 with j, depth-first over i0 + 1 .. nM - 1, candidates in list
 * order, "unpaired" last.  A hypothesis is kept as soon as its last pairing passes when it has more pairings than the bound,
 * or as many and a smaller d2; a subtree is left when the pairings it can still reach (one per observation left that has a
 * candidate) are fewer than the bound's, or as many with d2 -- which never decreases along a branch -- not below the bound's.
 * A node is one joint test, the root's own included; a root stops in front of test node_limit + 1 and keeps its best.  Two
 * rounds: every root with the greedy hypothesis as the bound, then the stopped roots again with the best of the first round.
 * Ties (equal count and bit-equal d2): within a root the hypothesis met first stays; over roots the lowest root i0 * nL + j,
 * then the earlier round; the greedy hypothesis unless strictly beaten.
 *   ic_d2_out [nM * nL] (nullable): ic_ij, NaN where not positive definite
 *   assign_out [nM]: h (cgmr_jcbb_dense: the landmark's position j; cgmr_joint_compatibility: its vertex index), or -1
 *   count_out, d2_out, dof_out [1]: the pairings, d2_H and D of the result
 *   proven_out [1]: 1 when no root was stopped in its last round -- the result is the optimum --, else 0: the hypothesis is
 *     still admissible and no worse than the greedy one
 *   nodes_out [1] (nullable): the tests made over all roots and rounds, at most roots * CGMR_JC_ROUNDS (2) * node_limit
 *
 * cgmr_jcbb_dense: the caller's own Sigma and predictions.  obs_pose_slot [nM] in [0, nA), obs_dim [nM] 1 or 2; sigma
 *   [(3 nA + 2 nL)^2] row-major, the nA poses first (3 each), then the nL landmarks (2 each), only the lower triangle is read;
 *   e [nM * nL * 2], J [nM * nL * 2 * 5] (a bearing: e[0] and row 0 alone are read), R_upper [nM * 3] = (R00, R01, R11).
 * cgmr_joint_compatibility: the nine graph arguments of cgmr_observation_covariance, then the observations -- obs_pose [nM]
 *   vertex indices (poses), obs_kind [nM] 1 or 2, obs_meas_xyt [nM * 3] and obs_info_upper [nM * 6] read as that call reads a
 *   hypothesis (nullable: R = 0) -- and the candidates landmark_idx [nL] (distinct points); types and rk last.  Sigma is that
 *   of cgmr_marginals_joint_typed over the unique observing poses and the candidates (at most CGMR_JOINT_MAX_QUERIES), kept
 *   on the device; analysis cache, bounded-wait fall-back, Cholesky / timeout / HIP / allocation codes as there
 *   (CGMR_E_CHOLESKY_BASE: outputs zeroed, count 0).  The caller's poses are not modified; the other entry points' bytes do
 *   not change.
 * nM == 0 or nL == 0: CGMR_OK, count 0, proven 1, every assign_out -1.  CGMR_E_INVALID, before anything is queued and naming
 * the observation or the landmark in cgmr_last_error: a null context or required pointer, a negative count, nM above
 * CGMR_JC_MAX_OBS, nL above CGMR_JC_MAX_LANDMARKS, node_limit <= 0, a kind or dimension outside {1, 2}, a pose slot outside
 * [0, nA), an observing vertex that is a point or out of range, a candidate that is a pose or out of range, a repeated
 * candidate, a gamma_by_dof[1 .. 2 nM] that is not finite or not increasing, an entry of sigma's lower triangle or of R_upper that is not finite (a non-finite e or J only makes its pair
 * incompatible).
 * Work: one wavefront per root, the Cholesky factor of C_H (at most 64 x 64 doubles, 32 KiB) in LDS, four roots per workgroup;
 * two calls give identical bytes in every output.  CGMR_JC_DEFAULT_NODE_LIMIT is what the Python binding passes: the largest
 * power of two for which the slowest call found at the cap shape (32 x 256) stays at or under 0.27 s on an MI355X, the figure
 * CGMR_EXACT_DEFAULT_NODE_LIMIT was chosen against.  Measured (tools/gpu_jcbb_time.py): a row of landmarks
 * 0.5 m apart with a pose variance of 1e4 along it and a decoy that leaves the greedy hypothesis one pairing, so that all 8192
 * roots search in the first round and half of the two rounds' budget is spent: 75 ms of device time at node_limit 512, 128 ms
 * at 1024, 229 ms at 2048, 417 ms at 4096.  Tests per second over a call: 6e7 there (every root busy, mostly shallow tests),
 * 7.5e5 .. 1.2e6 where only the few hundred roots of observation 0 search and descend to D = 64. */
#define CGMR_JC_MAX_OBS 32
#define CGMR_JC_MAX_LANDMARKS 256
#define CGMR_JC_DEFAULT_NODE_LIMIT 2048
int cgmr_jcbb_dense(cgmr_ctx* ctx, int nM, int nL, int nA, const int32_t* obs_pose_slot, const int32_t* obs_dim,
                    const double* sigma, const double* e, const double* J, const double* R_upper, const double* gamma_by_dof,
                    int64_t node_limit, double* ic_d2_out, int32_t* assign_out, int32_t* count_out, double* d2_out,
                    int32_t* dof_out, int32_t* proven_out, int64_t* nodes_out);
int cgmr_joint_compatibility(cgmr_ctx* ctx, int nV, const double* poses_xyt, const uint8_t* fixed, int nE,
                             const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt, const double* info_upper,
                             int nM, const int32_t* obs_pose, const uint8_t* obs_kind, const double* obs_meas_xyt,
                             const double* obs_info_upper, int nL, const int32_t* landmark_idx, const double* gamma_by_dof,
                             int64_t node_limit, double* ic_d2_out, int32_t* assign_out, int32_t* count_out, double* d2_out,
                             int32_t* dof_out, int32_t* proven_out, int64_t* nodes_out, const cgmr_factor_types* types,
                             const cgmr_robust* rk);

/* Condensed graphs as spanning trees of relative poses (present in C ABI version 105 libraries that export these symbols).
 *
 * cgmr_condense labels a star gauge -> v from Sigma_vv alone, as CondensedGraphCreator::compute does, and drops every
 * cross-covariance between the requested vertices.  cgmr_condense_tree keeps the edge count, the edge type and the wire record
 * and chooses which pairs the edges join: the nodes are the gauge (node 0) and the unique requested vertices other than the
 * gauge (nodes 1 .. nq, in order of first appearance), every unordered pair (a, b) is a candidate edge of weight
 *     w(a, b) = log det Sigma_z(a, b),
 * Sigma_z the first-order covariance of z = x_a^-1 x_b, a < b, under the joint covariance of the two vertices
 * (cgmr_relative_covariance's formula; Sigma_aa = Sigma_ab = 0 for the gauge), at the estimates after the completed iteration,
 * the determinant from a 3x3 Cholesky factor; a pivot that is not positive and finite, or a NaN, gives +inf, and so does every
 * pair of a requested vertex that no edge touches (it has no covariance: it is not known exactly, it is not known).  The condensed
 * graph is the minimum spanning tree under the total order (w, max(a, b), min(a, b)), compared lexicographically -- unique
 * whichever algorithm finds it -- rooted at the gauge: one edge per node 1 .. nq, in node order, from = the node's parent, to =
 * the node.  On a chain of odometry edges the tree is the chain and its labels are the odometry's, whichever vertex is the gauge.
 *
 *   the pass: cgmr_condense's (the gauge alone fixed, the spanning-tree guess, one iteration solved and applied), then the
 *   forward solve and every lower Gram tile of cgmr_marginals_joint over the nq vertices (their device memory: as there).
 *   est_out [3 nq]: x_parent^-1 x_child at the estimates after the iteration.  info_upper_out [6 nq]: g2o's EdgeLabeler -- a
 *   parent that is the gauge: cgmr_condense's labelling (7 sigma points of Sigma_cc); otherwise sampleUnscented at dimension 6
 *   (alpha 1e-3, beta 2, lambda = alpha^2 6): 13 sigma points of [Sigma_pp Sigma_pc; Sigma_cp Sigma_cc], each applied to both
 *   vertices by the additive (x, y, theta) update, the edge error in the measurement's frame, weighted mean and covariance, 3x3
 *   inverse.
 *   from_out / to_out [nq]: vertex indices.  weight_out [nq] (nullable): the chosen edge's w.  flags_out [nq] (nullable): 0, 1
 *   (no Cholesky factor: identity information, as cgmr_condense leaves it), 2 (every weight of the node was +inf: it hangs on
 *   the gauge, identity information).
 *   rk: as cgmr_condense_robust (null: the plain call).
 * Returns the edge count nq (0 with no requested vertex besides the gauge, or no free vertex), or a negative code:
 * CGMR_E_INVALID before anything is queued for a null required pointer, an index out of range, or more than
 * CGMR_TREE_MAX_NODES nodes (the weight matrix: 8 n^2 bytes, 8.4 MB at the limit); otherwise as cgmr_condense.
 * Pose graphs only.  Deterministic: no atomics, two calls give identical bytes.
 *
 * cgmr_min_spanning_tree: the combinatorial half on a caller's dense symmetric matrix weights [n * n] (host, row-major; only
 * the lower triangle is read, a NaN counts as +inf): parent_out [n] of the tree of the same total order rooted at `root`,
 * parent_out[root] = -1.  CGMR_E_INVALID for n < 1, n > CGMR_TREE_MAX_NODES or a root outside [0, n).  In profiling mode its
 * one launch is counted in class 11 of cgmr_gn_kernel_times_ex. */
#define CGMR_TREE_MAX_NODES 1025
int cgmr_condense_tree(cgmr_ctx* ctx, int nV, const double* poses_xyt, int nE, const int32_t* from_idx, const int32_t* to_idx,
                       const double* meas_xyt, const double* info_upper, int gauge_idx, int nK, const int32_t* query_idx,
                       int32_t* from_out, int32_t* to_out, double* est_out, double* info_upper_out, double* weight_out,
                       int32_t* flags_out, const cgmr_robust* rk);
int cgmr_min_spanning_tree(cgmr_ctx* ctx, int n, const double* weights, int root, int32_t* parent_out);

/* Vertex removal: marginalise vertices out of a pose graph into spanning trees of relative-pose edges (present in C ABI version
 * 105 libraries that export this symbol).
 *
 * Every other entry point makes the graph grow or reads it.  cgmr_remove_nodes computes what replaces the edges of each vertex
 * of remove_idx once the vertex is gone -- generic-linear-constraint node removal with a Chow-Liu-style tree -- from the edges
 * incident to that vertex alone; estimates are not an input.  Pose graphs only (every edge an EdgeSE2 between two different
 * poses).  For a removed vertex v with the distinct neighbours n_1 < .. < n_m (by vertex index; the nodes 1 .. m):
 *   1. the local configuration: v at the identity, n at z_vn of the lowest-index edge between v and n, inverted where that edge
 *      is stored n -> v: the exact optimum of the star of those edges.
 *   2. H = sum J^T Omega J over all incident edges at that configuration, EdgeSE2's Jacobians with each measurement's own
 *      rotation.  A parallel edge adds its term there; its residual against the first edge is dropped.
 *   3. n_1 is fixed; the rest is factored by Cholesky, v first, and the trailing 3 (m - 1) block inverted: the covariance of
 *      n_2 .. n_m with v marginalised out, zero blocks for n_1.
 *   4. w(a, b) = log det Sigma_z(a, b) for every pair of nodes as in cgmr_condense_tree (a 3x3 Cholesky factor; a pivot that is
 *      not positive and finite gives +inf).  Sigma_z does not depend on which neighbour is fixed.
 *   5. the minimum spanning tree under cgmr_condense_tree's total order (w, max, min), rooted at n_1.
 *   6. each tree edge parent -> child: meas = x_p^-1 x_c at the local configuration (= z_vp^-1 (+) z_vc), information =
 *      (R(meas.theta)^T Sigma_z R(meas.theta))^-1, first order.  With two neighbours this is exactly the composed edge.
 *   7. m - 1 new edges in order of the child's node; m = 0 or 1: none.
 * flags_out [nR]: 0 removed; 1 H has no Cholesky factor; 2 more than CGMR_REMOVE_MAX_DEGREE distinct neighbours; 3 a tree
 * edge's Sigma_z has no factor (its weight is +inf).  A vertex flagged 1, 2 or 3 is to be left in place and gets no edges.
 * off_out [nR + 1]: the edges of remove_idx[r] are off_out[r] .. off_out[r + 1] - 1 of from_out / to_out (vertex indices),
 * meas_out [3 per edge], info_upper_out [6 per edge] and weight_out (nullable: the edge's w).
 * Returns the number of new edges (0 for nR == 0), or CGMR_E_INVALID, before anything is queued and with the reason in
 * cgmr_last_error, for: a null required pointer (the edge outputs are required with cap_out > 0) or a negative count, an
 * index out of range, a repeated remove_idx, a self edge on a removed vertex, two removed vertices joined by an edge (one call
 * removes an independent set), cap_out smaller than the sum of max(m_v - 1, 0) over the vertices within the degree limit;
 * CGMR_E_HIP / _ALLOC.  One launch on the context's stream, one 64-lane workgroup per vertex (in profiling mode counted in class
 * 11 of cgmr_gn_kernel_times_ex).  Deterministic: no atomics, two calls give identical bytes. */
#define CGMR_REMOVE_MAX_DEGREE 16
int cgmr_remove_nodes(cgmr_ctx* ctx, int nV, int nE, const int32_t* from_idx, const int32_t* to_idx, const double* meas_xyt,
                      const double* info_upper, int nR, const int32_t* remove_idx, int cap_out, int32_t* off_out, int32_t* from_out,
                      int32_t* to_out, double* meas_out, double* info_upper_out, double* weight_out, int32_t* flags_out);

/* ------------------------------------------------------------------------------------------
 * Generic correlative search (loop-closure / hierarchical / global matching).
 *
 * cgmr_match_greedy replaces CharGrid::greedySearch(mresvec, points, regions, params)
 * (src/matcher/chargrid.cpp:208-308) preceded by resetGrid + addAndConvolvePoints of the reference points
 * (src/matcher/scan_matcher.cpp:206-210): the building block of ScanMatcher::scanMatchingLC (scan_matcher.cpp:201-294),
 * CharGrid::hierarchicalSearch (chargrid.cpp:310-413) and ScanMatcher::globalMatching (scan_matcher.cpp:366-428),
 * whose region bookkeeping is host logic (cg_mrslam_amd/matcher.py mirrors it).
 *   cfg            grid geometry + kernel (e.g. the LC matcher: [-35,35]^2 at 0.1 m, kernel range 0.5, graph_slam.cpp:61-62)
 *   ref_pts_xy     [n_ref*2]  reference points already in the reference vertex' frame (transformPointsFromVSet)
 *   qry_pts_xy     [n_qry*2]  query points (already subsampled, scan_matcher.cpp:216-217)
 *   regions        [n_regions*6] float32: lower (x, y, theta), upper (x, y, theta)  (struct Region, chargrid.h:87-91)
 *   step_x/step_y  searchStep; theta_res; max_score; dx/dy/dth resultsDiscretization (MatchingParameters, chargrid.h:94-99)
 *   results_out    up to cap results {x, y, theta, score}, ascending score (ties: result-map order); *n_out = total found
 * The reference's <= 4 per-thread result maps are reproduced (a bin can appear once per map).            */
typedef struct cgmr_match_result { double x, y, theta, score; } cgmr_match_result;
int cgmr_match_greedy(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, int n_ref, const double* ref_pts_xy, int n_qry,
                      const double* qry_pts_xy, int n_regions, const float* regions, double step_x, double step_y,
                      double theta_res, double max_score, double dx, double dy, double dth,
                      cgmr_match_result* results_out, int cap, int* n_out);

/* ------------------------------------------------------------------------------------------
 * The ScanMatcher member functions (src/matcher/scan_matcher.h:45-78) on flat scan sets.
 *
 * A cgmr_scan_set is the flat form of the (OptimizableGraph::VertexSet&, OptimizableGraph::Vertex* reference)
 * argument pairs of the reference: the RobotLaser ranges and the VertexSE2 estimates of the set's vertices, in
 * the order the caller iterates its set (the reference iterates a std::set<Vertex*>, i.e. in address order; the
 * rasterised grid and the searches do not depend on that order, the concatenated point list does), and which of
 * them is the reference vertex.  The laser description and laserParams().laserPose come from the config.
 * All of these run the region / transform bookkeeping on the host with the reference's arithmetic (Vector3f
 * regions in float, SE2 products in double with libm) and every search on the GPU.
 *
 *   cgmr_close_scan_matching   bool closeScanMatching(vset, originVertex, currentVertex, SE2* trel, maxScore)
 *                              scan_matcher.cpp:112-189 with the reference's real call shape: the last vertex and up
 *                              to 5 predecessors (src/slam/graph_slam.cpp:230-244); window / steps / bins from cfg
 *   cgmr_scan_matching_lc      bool scanMatchingLC(vset, ref, currvset, current, vector<SE2>& trel, maxScore)
 *                              scan_matcher.cpp:191-294 (the single-vertex overload :191-199 is a set of one):
 *                              trel_out [2*3], *n_out = 0..2 results; the bool is *n_out > 0
 *   cgmr_global_matching       bool globalMatching(vset, ref, currvset, current, SE2* trel, maxScore)
 *                              scan_matcher.cpp:358-428 (+ the single-vertex overload): 4-level hierarchical search
 *                              over +/-(10 m, 5 m, pi)
 *   cgmr_scan_matching_lc_hierarchical  bool scanMatchingLChierarchical(vset, ref, currvset, current, vector<SE2>& trel, maxScore)
 *                              scan_matcher.cpp:296-356 (the reference's only call of it, :197, is commented out): one region
 *                              of +/-(2 m, 2 m, 1 rad) around reference^-1 * current, 3-level hierarchical search, best result
 *   cgmr_verify_matching       bool verifyMatching(vset1, ref1, vset2, ref2, SE2 trel12, double* score)
 *                              scan_matcher.cpp:430-505; *accepted_out = score <= 40
 *   cgmr_match_hierarchical    CharGrid::hierarchicalSearch(mresvec, points, regions, params, nLevels)
 *                              chargrid.cpp:310-413 on explicit point lists (see cgmr_match_greedy for the arguments)
 *   cgmr_transform_points_from_vset  ScanMatcher::transformPointsFromVSet, scan_matcher.cpp:89-110 (host only);
 *                              returns the number of points written to pts_out [cap*2], or < 0          */
typedef struct cgmr_scan_set {
  int n_scans;
  const float* ranges;          /* [n_scans * cfg->n_beams] */
  const double* poses_xyt;      /* [n_scans * 3] vertex estimates */
  int ref_index;                /* the reference (origin) vertex of the set */
} cgmr_scan_set;
int cgmr_close_scan_matching(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, const cgmr_scan_set* vset,
                             const float* cur_ranges, const double cur_pose_xyt[3], double max_score, double trel_out[3],
                             int* found_out);
int cgmr_scan_matching_lc(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, const cgmr_scan_set* ref_set,
                          const cgmr_scan_set* cur_set, double max_score, double* trel_out, int* n_out);
int cgmr_global_matching(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, const cgmr_scan_set* ref_set,
                         const cgmr_scan_set* cur_set, double max_score, double trel_out[3], int* found_out);
int cgmr_scan_matching_lc_hierarchical(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, const cgmr_scan_set* ref_set,
                                       const cgmr_scan_set* cur_set, double max_score, double trel_out[3], int* found_out);
int cgmr_verify_matching(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, const cgmr_scan_set* set1, const cgmr_scan_set* set2,
                         const double trel12[3], double* score_out, int* accepted_out);
int cgmr_match_hierarchical(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, int n_ref, const double* ref_pts_xy, int n_qry,
                            const double* qry_pts_xy, int n_regions, const float* regions, double theta_res, double max_score,
                            double dx, double dy, double dth, int n_levels, cgmr_match_result* results_out, int cap,
                            int* n_out);
int cgmr_transform_points_from_vset(const cgmr_matcher_config* cfg, const cgmr_scan_set* vset, double* pts_out, int cap);
/* Batched forms: n_jobs independent calls in one go -- the loop-closure matcher tries every
 * candidate set of a key frame (graph_slam.cpp:388-485), the inter-robot matcher every candidate vertex of every peer
 * (mr_graph_slam.cpp:213-220, 287-295).  All jobs of a call share cfg; every search level is ONE kernel launch that
 * serves all jobs (each job's grid is rasterised by the workgroups assigned to it), results are those of the single
 * calls.  trel_out: [n_jobs*6] (LC: up to 2 results each) / [n_jobs*3]; n_out / found_out / score_out / accepted_out
 * [n_jobs]; trel12 [n_jobs*3]. */
int cgmr_scan_matching_lc_batch(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, int n_jobs, const cgmr_scan_set* ref_sets,
                                const cgmr_scan_set* cur_sets, double max_score, double* trel_out, int* n_out);
int cgmr_global_matching_batch(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, int n_jobs, const cgmr_scan_set* ref_sets,
                               const cgmr_scan_set* cur_sets, double max_score, double* trel_out, int* found_out);
int cgmr_scan_matching_lc_hierarchical_batch(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, int n_jobs, const cgmr_scan_set* ref_sets,
                                             const cgmr_scan_set* cur_sets, double max_score, double* trel_out, int* found_out);
int cgmr_verify_matching_batch(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, int n_jobs, const cgmr_scan_set* sets1,
                               const cgmr_scan_set* sets2, const double* trel12, double* score_out, int* accepted_out);

/* ------------------------------------------------------------------------------------------
 * Scan-match covariance from the correlative search's response surface (C ABI version 105, added later under the same
 * number: callers find it by its symbols).  The reference declares MatcherResult::informationMatrix
 * (src/matcher/chargrid.h:50-60) and leaves it at identity; GraphSLAM::addDataSM writes the constant _SMinf onto every
 * scan-match edge (src/slam/graph_slam.cpp:246-249).  These calls deliver the information matrix of the match itself.
 *
 * Definition.
 * The inputs are the same as for `cgmr_match_greedy`, with exactly one region per job: reference points, query points, the region, `step_x`, `step_y` and `theta_res`. Two more inputs are added: a temperature `T > 0` in metres of score, and the winner `(x*, y*, θ*, s*)` that the preceding search returned.
 *
 * The candidates are exactly those of `CharGrid::greedySearch` (`chargrid.cpp:237-287`):
 *
 * - the angles `t = lower.θ; t < upper.θ; t += theta_res`, accumulated in double (the host's existing angle table);
 * - the cells `i, j` from `world2grid(lower)` to `world2grid(upper)` in steps `xSteps`, `ySteps`;
 * - the kept-point rule of `:246-256`.
 *
 * A candidate's score `s_c` is the reference's float32 `dsum`, read as double. Candidates with `k == 0` are left out. No `maxScore` cut is applied.
 *
 * With `w_c = exp(-(s_c - s*) / T)` and `d_c = (x_c - x*, y_c - y*, t_c - θ*)`, where `x_c`, `y_c` are the reference's float `grid2world` values read as double:
 *
 * - `mass = Σ w_c`
 * - `u = Σ w_c d_c / mass`
 * - `cov = Σ w_c d_c d_cᵀ / mass − u uᵀ`; centring the moments at the winner keeps this subtraction harmless
 * - `mean = (x*, y*, θ*) + u`
 * - `border_mass` is the share of `mass` on candidates whose `i`, `j` or angle index is the first or last of its range.
 * - `floor = diag((xSteps·res)²/12, (ySteps·res)²/12, theta_res²/12)`, the variance of the search's own quantisation.
 * - `info = (J (cov + floor) Jᵀ)⁻¹` with `J = blockdiag(R(θ*)ᵀ, 1)`. g2o's `EdgeSE2` error lives in the frame of the measurement's end, so the translation block is rotated into it.
 *
 * The output also carries `n_candidates` and a status: 0 means ok, 1 means no candidate was counted, and 2 means the job was skipped because the search found nothing. A job with status ≠ 0 returns zeros and never NaN.
 *
 * (`res` is the grid's float32 resolution read as double, as in grid2world.  Status 1 also covers a mass that is zero or not
 * finite -- a winner whose score lies far from every candidate's -- and a matrix that cannot be inverted in double.)  `T` has no
 * default: it is a modelling parameter to be calibrated on real scans.  cov and info are 3x3, row-major.  The same
 * call made twice returns identical bits (no floating-point atomics; fixed summation order).
 *
 *   cgmr_match_response             one job: region [6] float32 as in cgmr_match_greedy, winner [4] = (x*, y*, theta*, s*)
 *   cgmr_match_response_batch       n_jobs in one launch of each kernel; a job with found == 0 is skipped (status 2); n_regions
 *                                   must be 1 (the field exists so that a caller's region list can be passed as it is)
 *   cgmr_close_scan_matching_cov    cgmr_close_scan_matching, then the response over the window that search used (same host
 *                                   arithmetic for the region and the points); info_out = the response's info, zeros when nothing
 *                                   was found or the status is not 0; resp_out nullable
 *   cgmr_match_response_information host only: info_out = (J (cov + floor) J^T)^-1 from cov, theta*, the steps in metres and
 *                                   theta_res -- the finishing arithmetic of the calls above (CGMR_E_INVALID: not invertible)   */
struct cgmr_match_response {
  double mean[3], cov[9], info[9];
  double mass, border_mass;
  int64_t n_candidates;
  int32_t status, reserved;
};
typedef struct cgmr_response_job {
  int n_ref; const double* ref_pts_xy;
  int n_qry; const double* qry_pts_xy;
  int n_regions; const float* regions;       /* exactly one region */
  double winner[4];
  int found;
} cgmr_response_job;
int cgmr_match_response(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, int n_ref, const double* ref_pts_xy, int n_qry,
                        const double* qry_pts_xy, const float region[6], double step_x, double step_y, double theta_res, double T,
                        const double winner[4], struct cgmr_match_response* out);
int cgmr_match_response_batch(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, int n_jobs, const cgmr_response_job* jobs,
                              double step_x, double step_y, double theta_res, double T, struct cgmr_match_response* out);
int cgmr_close_scan_matching_cov(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, const cgmr_scan_set* vset,
                                 const float* cur_ranges, const double cur_pose_xyt[3], double max_score, double T,
                                 double trel_out[3], int* found_out, double info_out[9], struct cgmr_match_response* resp_out);
int cgmr_match_response_information(const double cov[9], double theta_star, double step_x_m, double step_y_m, double theta_res,
                                    double info_out[9]);

/* ------------------------------------------------------------------------------------------
 * Refining a match below the grid's resolution (C ABI version 105, added later under the same number: callers find it by
 * its symbols).  closeScanMatching returns the best cell of CharGrid::greedySearch (src/matcher/chargrid.cpp:237-287): a
 * multiple of the grid's resolution and of theta_res, and GraphSLAM::addDataSM (src/slam/graph_slam.cpp:230-249) puts that
 * rounding onto every scan-match edge.  These calls move the winner to where the distance field says the minimum is.  They
 * promise a pose whose cost is not higher than the winner's, inside a stated bound; they do not promise accuracy (a field
 * with gaps has a local minimum at every reference point: DESIGN.md 3.2).  Nothing else changes: the searches return the
 * bits they returned before.
 *
 * Definition.
 * Inputs: as for `cgmr_match_response` without the region -- config, reference points, query points, `step_x`, `step_y`,
 * `theta_res` --, the winner `(x*, y*, θ*, s*)` with its `found` flag, and a parameter struct.
 *
 * Field.
 * - `res`, `ll_x`, `ll_y` are the grid's float32 values read as double.
 * - Node `(i, j)` lies at the world position `(ll_x + res·i, ll_y + res·j)`. This is `grid2world`, and the search's `world2grid` rounds to the nearest node.
 * - The node carries `F[i][j] = cell(i, j) / kscale` metres.
 * - `cell` is the rasterised grid of the reference points, exactly as the searches build it.
 *
 * Residual of a query point.
 * - For query point `q` under pose `(x, y, θ)`: `w = R(θ) q + (x, y)`, `u = (w_x − ll_x) / res`, `v` likewise.
 * - `i0 = floor(u)`, `a = u − i0`, `j0 = floor(v)`, `b = v − j0`.
 * - The point is *inside* iff `0 ≤ i0`, `i0 + 1 ≤ nx − 1`, `0 ≤ j0`, `j0 + 1 ≤ ny − 1`.
 * - Inside: `r` is the bilinear interpolation of the four nodes, and `∇r` is its exact gradient, `(∂r/∂u, ∂r/∂v) / res`.
 * - Outside: `r = int(kernel_range·kscale) / kscale` and the gradient is zero.
 * - This differs from the reference's `isInside`. `grid_cell` returns 0 off the grid, so the inside test comes before any cell is read.
 * - Every query point counts. There is no kept-point rule and no `maxScore`.
 * - `J_q = ∇rᵀ · [1 0 −(s q_x + c q_y); 0 1 (c q_x − s q_y)]`.
 *
 * Sums at a pose.
 * - `cost = Σ r²`
 * - `b = Σ J_qᵀ r`
 * - `H = Σ J_qᵀ J_q`
 * - `score = Σ r / n_qry`. This is comparable with the search's score but not equal to it.
 * - `n_active` = the number of points with a non-zero gradient.
 *
 * Iteration.
 * - Start at the winner, with `bound = bound_steps · (step_x_m, step_y_m, theta_res)`; `step_x_m = xSteps·res` as for the response.
 * - Repeat up to `max_iters` times.
 * - Form `μ = ridge · trace(H) / 3`.
 * - Solve `d = −(H + μ I)⁻¹ b` directly in double.  A `d` that is not finite (a singular system) stops with code 2.
 * - If `max_k |d_k| / bound_k < step_tol`, stop with code 1.
 * - Otherwise try up to `max_halvings + 1` candidates `c = clip(pose + d, winner − bound, winner + bound)`, halving `d` after each failure.
 * - If a `c` equals the current pose in all three coordinates exactly, stop with code 3.
 * - If `cost(c) < cost`, move to `c`. Its sums are already known.
 * - If no candidate is taken, stop with code 2.
 * - If the iterations run out, stop with code 0.
 * - The pose is kept as winner + offset and the offset is what is clipped, so that the `at_bound` test below is exact.
 *
 * Output (`struct cgmr_match_refined`).
 * - `pose[3]`, `cost0` (at the winner), `cost`, `score0`, `score`.
 * - `hessian[9]` = `H` at the final pose, row-major, without the ridge.
 * - `n_active` at the final pose, `n_iters` (moves taken), `n_halvings` (candidates turned down), `stop`.
 * - `at_bound`: bit k is set when `|pose_k − winner_k| == bound_k`.
 * - `status`: 0 ok; 1 nothing to refine (`n_qry == 0` or `trace(H) == 0` at the winner); 2 skipped (`found == 0`).
 * - With status ≠ 0, `pose` is the winner as given and everything else is zero. Never NaN.
 * - The same call twice returns identical bits.
 *
 * Parameters.
 * - `cgmr_refine_params { int32 max_iters; int32 max_halvings; double ridge, step_tol, bound_steps; }`.
 * - `cgmr_refine_params_default()` fills in 10, 4, 1e-6, 1e-6, 1.0. These are numerical settings, not calibration.
 * - Refused with `CGMR_E_INVALID` and a message: `max_iters` outside 1..64, `max_halvings` outside 0..16, a `ridge` that is
 *   negative or not finite, a `step_tol` or `bound_steps` that is not positive and finite, a winner that is not finite.
 *
 *   cgmr_match_refine                 one job: winner [4] = (x*, y*, theta*, s*), found = the search's flag
 *   cgmr_match_refine_batch           n_jobs in one launch, one workgroup each; a job with found == 0 is skipped (status 2)
 *   cgmr_close_scan_matching_refined  cgmr_close_scan_matching, then the refinement with the points and steps
 *                                     cgmr_close_scan_matching_cov uses: trel_out = the refined pose (the search's winner when
 *                                     the status is not 0), trel_search_out (nullable) = the search's winner, found_out = the
 *                                     search's flag, refined_out nullable                                                     */
typedef struct cgmr_refine_params {
  int32_t max_iters, max_halvings;
  double ridge, step_tol, bound_steps;
} cgmr_refine_params;
struct cgmr_match_refined {
  double pose[3];
  double cost0, cost, score0, score;
  double hessian[9];
  int32_t n_active, n_iters, n_halvings, stop, at_bound, status;
};
typedef struct cgmr_refine_job {
  int n_ref; const double* ref_pts_xy;
  int n_qry; const double* qry_pts_xy;
  double winner[4];
  int found;
} cgmr_refine_job;
cgmr_refine_params cgmr_refine_params_default(void);
int cgmr_match_refine(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, int n_ref, const double* ref_pts_xy, int n_qry,
                      const double* qry_pts_xy, double step_x, double step_y, double theta_res, const double winner[4], int found,
                      const cgmr_refine_params* params, struct cgmr_match_refined* out);
int cgmr_match_refine_batch(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, int n_jobs, const cgmr_refine_job* jobs, double step_x,
                            double step_y, double theta_res, const cgmr_refine_params* params, struct cgmr_match_refined* out);
int cgmr_close_scan_matching_refined(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, const cgmr_scan_set* vset,
                                     const float* cur_ranges, const double cur_pose_xyt[3], double max_score,
                                     const cgmr_refine_params* params, double trel_out[3], double trel_search_out[3],
                                     int* found_out, struct cgmr_match_refined* refined_out);

/* ------------------------------------------------------------------------------------------
 * Polishing a search's results: refinement and response behind one rasterisation (C ABI version 105, added later under the
 * same number: callers find it by its symbols).  The loop-closure and global matchers return the best cell of a 0.1 m grid with
 * 0.025 rad steps; the two sections above can be pointed at such a match with the generic calls, at the price of one
 * rasterisation of the job's grid per call and per result.  These calls rasterise a job's grid once, then run the refinement
 * ("Refining a match") for each of the job's winners in order, then take the response ("Scan-match covariance") over a window
 * around each winner in order.  Neither part reads what the other writes.  No new arithmetic: both parts are the definitions above.
 *
 * - A job has reference points, query points and `n_winners` in 0..CGMR_POLISH_MAX_WINNERS winners `(x, y, θ, s)`.
 * - Refinement (`refine == 1`): `refined` holds the bits `cgmr_match_refine_batch` returns for the same points, winner, steps and
 *   `refine_params`.
 * - Response (`T > 0`): one region per winner, `lower = (float)(w − h)`, `upper = (float)(w + h)` with `w` the winner as the search
 *   produced it (before any angle normalisation) and `h = window`; the sums are formed in double and narrowed once.  It is taken
 *   around the search's winner, not the refined pose.  One workgroup sums all candidates of a window, in a partition of its own:
 *   the result agrees with `cgmr_match_response_batch` on the same region to rounding, not to the bit.
 * - Status codes are those of the two parts, and 3: not asked for.  A part with status 3 is all zeros, except `refined.pose`,
 *   which holds the winner.  Entries beyond `n_winners` have status 2 in both parts (`refined.pose` zero).  Never NaN.
 * - Refused with `CGMR_E_INVALID` and a message: what `cgmr_match_refine_batch` and `cgmr_match_response_batch` refuse; a `T`
 *   that is negative or not finite; a half-width that is not positive and finite; `refine` other than 0 or 1; `n_winners` outside
 *   0..4; a winner that is not finite; with `T > 0`, a window with more than 65 536 candidates (angles × cells).  Without a
 *   response (`T == 0`) the window is checked for being positive and finite and is otherwise not used: no region is built for it.
 * - The same call twice returns identical bits.
 *
 *   cgmr_match_polish_batch               n_jobs in ONE launch, one workgroup each; out holds CGMR_POLISH_MAX_WINNERS entries per job
 *   cgmr_scan_matching_lc_polished_batch  cgmr_scan_matching_lc_batch (trel_out, n_out: the same bits), then every returned result
 *                                         polished in one launch on the same prepared points with the search's own score,
 *                                         step = (float)resolution and theta_res = 0.025: polished_out[j * 2 + k] belongs to
 *                                         trel_out[j * 6 + 3 k].  The kernel works on the raw winner; response.mean[2] and
 *                                         refined.pose[2] are normalised on the way out, as the search's own angle is.
 *   cgmr_global_matching_polished_batch   cgmr_global_matching_batch (trel_out, found_out: the same bits), then the same for every
 *                                         job's result: polished_out[j]
 *   cgmr_scan_matching_lc_polished, cgmr_global_matching_polished: a batch of one                                               */
#define CGMR_POLISH_MAX_WINNERS 4
typedef struct cgmr_polish_params {
  double T;              /* > 0: take the response at this temperature (no default); 0: no response */
  double window[3];      /* half-widths (x, y, theta) of the response window around a winner */
  int32_t refine;        /* 1: refine with refine_params; 0: no refinement */
  int32_t reserved;
  cgmr_refine_params refine_params;
} cgmr_polish_params;
struct cgmr_match_polished {
  struct cgmr_match_response response;
  struct cgmr_match_refined refined;
};
typedef struct cgmr_polish_job {
  int n_ref; const double* ref_pts_xy;
  int n_qry; const double* qry_pts_xy;
  int n_winners;
  double winners[CGMR_POLISH_MAX_WINNERS][4];
} cgmr_polish_job;
int cgmr_match_polish_batch(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, int n_jobs, const cgmr_polish_job* jobs, double step_x,
                            double step_y, double theta_res, const cgmr_polish_params* params,
                            struct cgmr_match_polished* out /* [n_jobs * CGMR_POLISH_MAX_WINNERS] */);
int cgmr_scan_matching_lc_polished_batch(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, int n_jobs, const cgmr_scan_set* ref_sets,
                                         const cgmr_scan_set* cur_sets, double max_score, const cgmr_polish_params* params,
                                         double* trel_out /* [n_jobs * 6] */, int* n_out,
                                         struct cgmr_match_polished* polished_out /* [n_jobs * 2] */);
int cgmr_scan_matching_lc_polished(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, const cgmr_scan_set* ref_set,
                                   const cgmr_scan_set* cur_set, double max_score, const cgmr_polish_params* params,
                                   double* trel_out /* [6] */, int* n_out, struct cgmr_match_polished* polished_out /* [2] */);
int cgmr_global_matching_polished_batch(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, int n_jobs, const cgmr_scan_set* ref_sets,
                                        const cgmr_scan_set* cur_sets, double max_score, const cgmr_polish_params* params,
                                        double* trel_out /* [n_jobs * 3] */, int* found_out,
                                        struct cgmr_match_polished* polished_out /* [n_jobs] */);
int cgmr_global_matching_polished(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, const cgmr_scan_set* ref_set,
                                  const cgmr_scan_set* cur_set, double max_score, const cgmr_polish_params* params,
                                  double trel_out[3], int* found_out, struct cgmr_match_polished* polished_out);

/* Host helpers with the reference's exact arithmetic (no GPU): RawLaser::cartesian [g2o-recalled] and
 * CharGrid::subsample (src/matcher/chargrid.cpp:61-122).  Both return the number of points written. */
int cgmr_scan_cartesian(int n_beams, const float* ranges, double angle_min, double angle_inc, double max_range,
                        double min_range, double* pts_out);
int cgmr_subsample(int n, const double* pts_xy, double res, double* pts_out);

/* Numeric core of bool ScanMatcher::verifyMatching(vset1, ref1, vset2, ref2, trel12, double* score)
 * (src/matcher/scan_matcher.cpp:430-505): rasterise pts2 (vset2 moved into the frame of reference vertex 1 by
 * trel12), collect the points of pts1 the map does not explain (cell/kscale > nonmatched_score, 0.3 in the
 * reference; CharGrid::searchNonMatchedPoints chargrid.cpp:444-455), rasterise those into a fresh grid and average
 * its cells over the window [lower, upper) (CharGrid::countPoints chargrid.cpp:417-441).  The caller applies the
 * reference's threshold (score <= 40).  *n_nonmatched_out (nullable) receives the number of unexplained points. */
int cgmr_match_verify(cgmr_ctx* ctx, const cgmr_matcher_config* cfg, int n2, const double* pts2_xy, int n1,
                      const double* pts1_xy, double nonmatched_score, const float lower_xy[2], const float upper_xy[2],
                      double* score_out, int* n_nonmatched_out);

/* ------------------------------------------------------------------------------------------
 * Robot graph: one robot's pose graph resident in HBM -- the multi-robot path.
 *
 * Replaces, for one robot (= one rank = one GPU), the part of MRGraphSLAM that touches numbers:
 *   the g2o SparseOptimizer the robot grows key frame by key frame         src/slam/graph_slam.cpp:87-122,197-267
 *   GraphSLAM::optimize                                                    src/slam/graph_slam.cpp:561-575
 *   CondensedGraphBuffer::{insertInClosure, insertOutClosure, getMyEdges, selectGaugeCentroid, computeCondensedGraph,
 *     insertEdgesFromRobot}          src/mrslam/condensed_graph/condensed_graph_buffer.cpp:131-170,318-366,437-510
 *   CondensedGraphCreator::compute                  src/mrslam/condensed_graph/condensed_graph_creator.cpp:33-66
 *   MRGraphSLAM::addInterRobotData (messages in)                           src/mrslam/mr_graph_slam.cpp:331-395
 *   the wire structs (44 B / edge, float32)                                src/mrslam/msg_factory.h:78-112,200-238
 * Vertices and edges are addressed by g2o *id* here (robot * baseId + k, graph_slam.cpp:95,155): messages carry ids.
 * The structure (ids, end points, closure lists) is host state; poses, measurements, information matrices, received
 * edges and the wire buffers are device state.  A graph created with ctx == NULL does the bookkeeping only (CPU
 * tests, no numeric entry point works).  Calls on one graph must be serialised by the caller (graphMutex).
 *
 * Round protocol (C5: every 50 new vertices):
 *   cgmr_graph_optimize(g, 5)                      local solve on own + received level-0 edges
 *   cgmr_graph_compute_condensed[_async](g, -1)    one star of condensed edges per peer that asked (own edges only)
 *   cgmr_graph_pack(g, send)                       my message: edges for every peer + my closure requests
 *   cgmr_allgather_condensed(ctx, comm, ...)       one RCCL all-gather on a side stream (overlaps the next solve)
 *   cgmr_comm_wait + cgmr_graph_ingest(g, recv)    requests -> out-closures; newest edge set per peer replaces the old
 *
 * Wire buffer of one rank, cgmr_graph_wire_bytes() bytes:
 *   int32 robot, n_robots, n_edges[R], n_closures[R];  {int32 from, to; float est[3]; float info[6]} edges[R][cap];
 *   int32 closures[R][cap]          (slice p = what is addressed to robot p)                                   */
typedef struct cgmr_graph cgmr_graph;
typedef struct cgmr_comm cgmr_comm;

int cgmr_graph_create(cgmr_ctx* ctx, int robot_id, int n_robots, int base_id, int cap_edges_per_peer, cgmr_graph** out);
void cgmr_graph_destroy(cgmr_graph* g);
const char* cgmr_graph_last_error(const cgmr_graph* g);
/* ids must be new; fixed nullable (all free).  Edges: both end points must exist; these are the robot's OWN level-0
 * edges (odometry, scan matching, inter-robot closures it found itself). */
int cgmr_graph_add_vertices(cgmr_graph* g, int n, const int32_t* ids, const double* poses_xyt, const uint8_t* fixed);
int cgmr_graph_add_edges(cgmr_graph* g, int n, const int32_t* from_ids, const int32_t* to_ids, const double* meas_xyt,
                         const double* info_upper);
/* out[0] = vertices, [1] = own edges, [2] = received edges currently in the graph, [3] = peers with out-closures */
/* debugging aid: the level-0 edge list (vertex indices) the solver sees, own edges first; returns their number */
int cgmr_graph_debug_edges(const cgmr_graph* g, int cap, int32_t* from_out, int32_t* to_out, int32_t* n_own_out);
int cgmr_graph_counts(const cgmr_graph* g, int32_t out[4]);
/* GraphSLAM::optimize(iters); chi2_out nullable [iters+1]; returns like cgmr_gn_optimize */
int cgmr_graph_optimize(cgmr_graph* g, int iters, double* chi2_out);
/* The optimiser cgmr_graph_optimize uses: CGMR_ALG_GAUSS_NEWTON (default, the reference's) or CGMR_ALG_LEVENBERG with
 * params (nullable: g2o's defaults), run as cgmr_lm_optimize does; a Levenberg call never returns CGMR_E_CHOLESKY_*.
 * cgmr_graph_lm_last: the records of the last Levenberg solve -- lambda_out / trials_out [cap] (nullable), returns the
 * iterations run (0 after a Gauss-Newton solve).
 * CGMR_ALG_DOGLEG (params must be NULL, else CGMR_E_INVALID) runs as cgmr_dl_optimize does, with the parameters of
 * cgmr_graph_set_dogleg_params (checked there; default g2o's); it returns CGMR_E_CHOLESKY_BASE - i on g2o's Fail.
 * cgmr_graph_dl_last: the records of the last dogleg solve -- delta_out / trials_out / step_out [cap] (nullable), returns
 * the iterations run (0 after another algorithm's solve). */
#define CGMR_ALG_GAUSS_NEWTON 0
#define CGMR_ALG_LEVENBERG 1
#define CGMR_ALG_DOGLEG 2
int cgmr_graph_set_algorithm(cgmr_graph* g, int algorithm, const cgmr_lm_params* params);
int cgmr_graph_set_dogleg_params(cgmr_graph* g, const cgmr_dl_params* params);
int cgmr_graph_dl_last(const cgmr_graph* g, int cap, double* delta_out, int32_t* trials_out, int32_t* step_out);
/* Robust kernels of the robot graph (cgmr_robust above), applied by cgmr_graph_optimize under either algorithm: own edges
 * [first, first + n) by insertion index take kind[k] / delta[k] (host arrays; delta nullable: 1.0, which only kind 0 may
 * keep); own edges added later take CGMR_RK_NONE.  The received edges take one class, set by cgmr_graph_set_received_robust
 * (default CGMR_RK_NONE).  The condensed graphs stay plain unless cgmr_graph_set_condensed_robust(g, 1) is called (default
 * off): then every condensed graph the robot builds (cgmr_graph_compute_condensed, _async, the optimal gauge's candidates)
 * scales its own edges' information by rho1 at its spanning-tree guess, as cgmr_condense_robust does; the received edges are
 * switched off in those passes, so their class never enters.  Switched off, the condensed graphs are the plain ones byte for
 * byte.  cgmr_graph_edge_stats: e^T O e and rho1 of every level-0 edge at
 * the estimate of the last cgmr_graph_optimize, own edges first, then the received ones (the order of cgmr_graph_debug_edges);
 * returns that edge count, 0 when that solve ran with no kernel set. */
int cgmr_graph_set_edge_robust(cgmr_graph* g, int first, int n, const uint8_t* kind, const double* delta);
int cgmr_graph_set_received_robust(cgmr_graph* g, int kind, double delta);
int cgmr_graph_edge_stats(const cgmr_graph* g, int cap, double* edge_chi2_out, double* weight_out);
int cgmr_graph_set_condensed_robust(cgmr_graph* g, int on);
/* Graduated non-convexity on the robot graph (same ABI version: found by symbol).  cgmr_graph_optimize_gnc is cgmr_gnc_optimize
 * above -- the same contract, tests/ref_gnc.py -- on the system cgmr_graph_optimize would solve now: own edges, then the received
 * ones (the order of cgmr_graph_debug_edges), Gauss-Newton inside, the received stars' gauge vertices as hubs of the ordering.
 *   cgmr_graph_set_edge_gnc      barc_sq / known_inlier of own edges [first, first + n) by insertion index (host arrays).  A null
 *                                pointer: the default for the range -- the chi2 0.99 quantile of dimension 3, or the call's
 *                                default_barc_sq; free.  Edges never named, and edges added later, are default.  A value that is
 *                                not finite and > 0, a range beyond the own edges: CGMR_E_INVALID.
 *   cgmr_graph_set_received_gnc  one class for every received edge; barc_sq == 0: the default.
 *   cgmr_graph_optimize_gnc      params nullable (the defaults); its per-edge pointers (barc_sq, known_inlier, weight_out,
 *                                edge_chi2_out) must be null -- the graph holds those -- else CGMR_E_INVALID; also refused while an
 *                                own edge or the received class carries a robust kernel other than CGMR_RK_NONE.  mu_out
 *                                [max_outer], cost_out [max_outer + 1], partial_out [max_outer], outer_done: nullable.  Like
 *                                cgmr_graph_optimize it brings the host copy of the estimates along in its final wait;
 *                                cgmr_graph_edge_stats then returns r and w of every edge of this solve.  On a Cholesky code the
 *                                poses are those of the last good update and the stored weights stay what they were.
 *   cgmr_graph_gnc_weights       the stored weight of every own edge (returns their count; weight_out [cap]): 1 before any GNC
 *                                solve and for edges added since the last one, else the last outer iteration's weights of the
 *                                last cgmr_graph_optimize_gnc that returned CGMR_OK.  Received edges keep no weight between
 *                                calls: their set is replaced every round.
 *   cgmr_graph_keep_gnc_weights  on: cgmr_graph_optimize with Gauss-Newton scales every own edge's information by its stored
 *                                weight (received edges: 1) -- a key-frame loop's solves between two GNC calls.  With Levenberg
 *                                or dogleg selected, or a robust kernel set, that call returns CGMR_E_INVALID.  With every weight
 *                                1 its result is the plain call's bit for bit.  Default off: nothing changes.
 *   cgmr_graph_set_condensed_gnc on: every condensed graph the robot builds is that of its own-edge graph without the edges of
 *                                stored weight w < drop_below or w == 0, the others' information scaled by w: the spanning-tree
 *                                guess does not walk a removed edge (a vertex it no longer reaches keeps its estimate) and the
 *                                pass gets exact zeros from it.  drop_below in [0, 1]; Geman-McClure never gives an exact zero, so
 *                                drop_below is what removes its outliers.  A batch works from the weights as they are when it is
 *                                queued (cgmr_graph_compute_condensed_async: a later cgmr_graph_optimize_gnc does not reach it).  A
 *                                vertex left with no kept edge fails its pass with the Cholesky code, handled like any failed pass.
 *                                Refused while cgmr_graph_set_condensed_robust is on, and that one while this is on.  Default off.
 * A graph without a context takes the setters and answers cgmr_graph_optimize_gnc with CGMR_E_NO_DEVICE. */
int cgmr_graph_set_edge_gnc(cgmr_graph* g, int first, int n, const double* barc_sq, const uint8_t* known_inlier);
int cgmr_graph_set_received_gnc(cgmr_graph* g, double barc_sq, int known_inlier);
int cgmr_graph_optimize_gnc(cgmr_graph* g, const cgmr_gnc_params* params, double* mu_out, double* cost_out, int32_t* partial_out,
                            int32_t* outer_done);
int cgmr_graph_gnc_weights(const cgmr_graph* g, int cap, double* weight_out);
int cgmr_graph_keep_gnc_weights(cgmr_graph* g, int on);
int cgmr_graph_set_condensed_gnc(cgmr_graph* g, int on, double drop_below);
int cgmr_graph_lm_last(const cgmr_graph* g, int cap, double* lambda_out, int32_t* trials_out);
/* estimates of vertices first .. first+n-1 in insertion order */
int cgmr_graph_get_poses(cgmr_graph* g, int first, int n, double* poses_out);
int cgmr_graph_set_poses(cgmr_graph* g, int first, int n, const double* poses_xyt);
int cgmr_graph_insert_in_closure(cgmr_graph* g, int peer, int n, const int32_t* vertex_ids);
int cgmr_graph_insert_out_closure(cgmr_graph* g, int peer, int n, const int32_t* vertex_ids);
/* which = 0: out-closures (my ids `peer` asked for), 1: in-closures (ids I ask `peer` for); returns the count */
int cgmr_graph_closures(const cgmr_graph* g, int peer, int which, int cap, int32_t* ids_out);
/* computeCondensedGraph for `peer`, or for every peer with out-closures when peer < 0; returns the number built */
int cgmr_graph_compute_condensed(cgmr_graph* g, int peer);
/* The same, queued on the context's SIDE stream and not waited for: returns once the passes are queued; they run beside
 * whatever the caller does next on the context's stream -- the next round's grow, structure analysis and solve (the
 * reference builds its condensed graphs on the communication thread, src/mrslam/graph_comm.cpp:195-207, beside the main
 * loop).  The batch works on a snapshot (the estimates and own edges as they are at the call); cgmr_graph_pack,
 * cgmr_allgather_condensed and cgmr_graph_deliver order themselves behind it on the device; an entry point that hands
 * results to the HOST (cgmr_graph_get_condensed, _pack_host, _message_for, the next _compute_condensed*) waits for it.
 * A failed pass (Cholesky, time-out) is reported by cgmr_graph_condensed_wait or by the next call that waits; the message
 * packed meanwhile then carries no edges for the batch's peers (the counts are taken back on the device).
 * cgmr_graph_set_async(g, 1) before the first solve announces the use (the chained backward solves of the two streams then
 * share the workgroups that are certainly resident together from the start).  Same results as the synchronous call. */
int cgmr_graph_compute_condensed_async(cgmr_graph* g, int peer);
int cgmr_graph_condensed_wait(cgmr_graph* g);
int cgmr_graph_set_async(cgmr_graph* g, int on);
/* optimal = 1: pick the gauge with selectOptimalGauge (condensed_graph_buffer.cpp:252-288: every requested vertex in turn,
 * smallest sum of det(information^-1) over the star wins) instead of selectGaugeCentroid; the reference's default is 0 */
int cgmr_graph_set_optimal_gauge(cgmr_graph* g, int optimal);
/* the condensed graph built for `peer` in double precision: returns its edge count; outputs nullable */
int cgmr_graph_get_condensed(cgmr_graph* g, int peer, int cap, int32_t* from_id_out, int32_t* to_ids_out, double* est_out,
                             double* info_upper_out);
/* install a condensed graph from host data in wire precision (tests, or a caller that labels edges itself) */
int cgmr_graph_set_condensed(cgmr_graph* g, int peer, int n, int32_t from_id, const int32_t* to_ids, const float* est,
                             const float* info_upper);
int64_t cgmr_graph_wire_bytes(const cgmr_graph* g);
/* device buffers owned by the graph: wire_bytes / n_robots * wire_bytes */
/* Messages this robot left out of its wire buffer, did not build, or dropped on receipt because they exceed
 * cap_edges_per_peer -- the reference's ComboMessage::toCharArray returns 0 for a message beyond MAX_LENGTH_MSG and
 * GraphComm::send skips it (src/mrslam/graph_comm.cpp:112-122, msg_factory.h:115); never an error. */
int64_t cgmr_graph_skipped_messages(const cgmr_graph* g);
/* Asynchronous batches of condensed graphs (cgmr_graph_compute_condensed_async) that failed -- Cholesky, or a bounded device-side
 * wait that ran out -- since the graph was created.  The peers of such a batch get no edges in that round's message (like a lost
 * UDP packet); the next batch is built regardless, and after a time-out this graph's batches solve level by level. */
int64_t cgmr_graph_failed_batches(const cgmr_graph* g);
void* cgmr_graph_send_buffer(cgmr_graph* g);
void* cgmr_graph_recv_buffer(cgmr_graph* g);
/* d_send_out NULL = the graph's own send buffer; d_recv NULL = the graph's own receive buffer */
int cgmr_graph_pack(cgmr_graph* g, void* d_send_out);
/* In-process transport for robots that share a device (loopback runs; several robots of one node in one process): src's
 * packed message (cgmr_graph_pack(src, NULL) first) is copied into slot src->robot of dst's own receive buffer on dst's
 * stream, behind src's pack -- what the all-gather does between ranks.  No host wait; dst's matching
 * cgmr_graph_ingest_delivered and src's next write into its send buffer are ordered behind the copy. */
int cgmr_graph_deliver(cgmr_graph* src, cgmr_graph* dst);
/* the ingest that goes with cgmr_graph_deliver: the k-th call digests the k-th message every peer has delivered (two
 * receive buffers take turns, so a robot may deliver round t before the destination has ingested round t - 1) */
int cgmr_graph_ingest_delivered(cgmr_graph* g, int32_t* n_edges_out);
int cgmr_graph_ingest(cgmr_graph* g, const void* d_recv, int32_t* n_edges_out);
/* the same through host memory (gloo; CPU tests on a graph without a device) */
int cgmr_graph_pack_host(cgmr_graph* g, void* send_out);
int cgmr_graph_ingest_host(cgmr_graph* g, const void* recv, int32_t* n_edges_out);
/* One peer's share of the round message as the reference's CondensedGraphMessage carries it
 * (MRGraphSLAM::constructCondensedGraphMessage, src/mrslam/mr_graph_slam.cpp:607-670): edges44_out receives
 * {int32 from, to; float est[3]; float info[6]} records.  Returns 1 = there is a message, 0 = nothing to send, < 0 error.
 * A message beyond cap_edges_per_peer, or whose byte string (24 + 44 * edges + 4 * closure ids) would exceed the
 * reference's MAX_LENGTH_MSG = 100000, is not sent: 0 with both counts 0, and one more cgmr_graph_skipped_messages. */
int cgmr_graph_message_for(cgmr_graph* g, int peer, int cap_edges, void* edges44_out, int32_t* n_edges_out, int cap_closures,
                           int32_t* closure_ids_out, int32_t* n_closures_out);
/* MRGraphSLAM::addInterRobotData(CondensedGraphMessage*) (src/mrslam/mr_graph_slam.cpp:331-395) for one message from
 * `sender`: requests -> out-closures + the condensed graph for `sender` rebuilt; edges replace the previous set. */
int cgmr_graph_message_from(cgmr_graph* g, int sender, int n_edges, const void* edges44, int n_closures,
                            const int32_t* closure_ids, int32_t* n_accepted_out);
/* the edges currently held from `peer`: returns their count; outputs nullable */
int cgmr_graph_received_edges(cgmr_graph* g, int peer, int cap, int32_t* from_ids_out, int32_t* to_ids_out, double* meas_out,
                              double* info_upper_out);
/* Test support, in the manner of cgmr_graph_debug_edges.
 * cgmr_graph_debug_received_segment: the numbers of the received edges as the SOLVER reads them -- the compact second edge
 * segment the ingest kernels fill, peer order (the order of cgmr_graph_debug_edges behind the own edges); meas_out [cap * 3],
 * info_upper_out [cap * 6], both nullable; returns the number of received edges.  (cgmr_graph_received_edges reads the staging.)
 * cgmr_wire_narrow_edges: the kernel that writes a condensed graph's 44-byte wire records (double -> float32, the ids
 * vertex_ids[to_vertex[k]]), run on host arrays: to_vertex [n] indices into vertex_ids [n_vertices], est [n * 3],
 * info_upper [n * 6]; edges44_out receives n records.  The solver never hands that kernel a float32 subnormal, a tie or an
 * overflow; this is the way in for them.
 * cgmr_wire_narrow_edges_batched: the same kernel as a batch of condensed-graph passes launches it, once for njobs jobs: job j
 * has nq[j] edges and the gauge id gauge_id[j], reads its vertex indices at to_vertex + j * marg_stride bytes and -- by its
 * output slot -- est / info_upper at out_slot[j] * est_stride / info_stride bytes, and writes its records at
 * wire_inout + out_slot[j] * wire_stride bytes.  to_vertex holds njobs * marg_stride bytes; est, info_upper and wire_inout
 * hold n_slots strides each.  wire_inout goes to the device as it is and comes back whole, so bytes the kernel must not
 * touch keep the caller's value.  Every index and stride is checked on the host (CGMR_E_INVALID). */
int cgmr_graph_debug_received_segment(cgmr_graph* g, int cap, double* meas_out, double* info_upper_out);
int cgmr_wire_narrow_edges(cgmr_ctx* ctx, int n, int32_t from_id, const int32_t* to_vertex, int n_vertices, const int32_t* vertex_ids,
                           const double* est, const double* info_upper, void* edges44_out);
int cgmr_wire_narrow_edges_batched(cgmr_ctx* ctx, int njobs, const int32_t* nq, const int32_t* gauge_id, const int32_t* out_slot,
                                   int n_slots, long long marg_stride, long long est_stride, long long info_stride,
                                   long long wire_stride, const void* to_vertex, int n_vertices, const int32_t* vertex_ids,
                                   const void* est, const void* info_upper, void* wire_inout);
/* wall seconds of the last cgmr_graph_optimize / cgmr_graph_compute_condensed */
int cgmr_graph_last_seconds(const cgmr_graph* g, double out[2]);

/* Exchange (replaces GraphComm's pairwise UDP, src/mrslam/graph_comm.cpp:103-208, by one collective per round).
 * A communicator wraps an RCCL communicator over the ranks' GPUs (xGMI inside a node) and a side stream:
 *   rank 0: cgmr_comm_unique_id(id) -> distribute the 128 bytes out of band -> every rank: cgmr_comm_create.
 * cgmr_allgather_condensed queues ncclAllGather(d_send, d_recv, bytes_per_rank) on the communicator's stream behind
 * everything already queued on the context's stream -- and on its side stream (a batch of condensed graphs queued with
 * cgmr_graph_compute_condensed_async, the message packed behind it) -- and returns; cgmr_comm_wait makes the context's
 * stream wait for it.  cgmr_ctx_join_side: everything queued on the context's stream from now on runs after what is on
 * its side stream (for a caller that moves the send buffer with a transport of its own). */
int cgmr_comm_unique_id(void* id_out_128);
/* CGMR_OK if librccl resolves in this process: the check of the ranks that do NOT create the unique id (the root alone calls
 * cgmr_comm_unique_id) before everybody enters the collective cgmr_comm_create */
int cgmr_comm_probe(void);
int cgmr_comm_create(cgmr_ctx* ctx, int n_ranks, int rank, const void* unique_id_128, cgmr_comm** out);
void cgmr_comm_destroy(cgmr_comm* comm);
int cgmr_allgather_condensed(cgmr_ctx* ctx, cgmr_comm* comm, const void* d_send, size_t bytes_per_rank, void* d_recv);
int cgmr_ctx_join_side(cgmr_ctx* ctx);
int cgmr_comm_wait(cgmr_ctx* ctx, cgmr_comm* comm);
/* What the communicator says it is: out[0] = ranks (ncclCommCount), out[1] = this rank (ncclCommUserRank), out[2] = 1 if librccl
 * answered, 0 if the values are the ones given to cgmr_comm_create.  For a multi-GPU run's own report. */
int cgmr_comm_info(cgmr_comm* comm, int32_t out[3]);
int cgmr_comm_last_seconds(cgmr_comm* comm, double* seconds);

/* ------------------------------------------------------------------ occupancy map
 * cgmr_occupancy_map replaces, for all scans of a graph at once, FrequencyMap::integrateScan + fillRobotPose
 * (src/ros_map_publisher/frequency_map.cpp:27-103) over GridLineTraversal::gridLine
 * (src/ros_map_publisher/grid_line_traversal.cpp:31-154) -- the loop of Graph2occupancy::computeMap
 * (src/ros_map_publisher/graph2occupancy.cpp:120-122) -- and the frequency -> image conversion (:128-147).
 * The map geometry (bounding box, size, offset; graph2occupancy.cpp:44-118) is host logic, see
 * cg_mrslam_amd/occupancy.py.
 *   cfg              FrequencyMap(resolution, offset, size); integrateScan's maxRange / usableRange /
 *                    infinityFillingRange / gain / squareSize (negative ranges take the reference's defaults);
 *                    LaserParameters (first beam angle, angular step, max range, laser pose on the robot);
 *                    occupied / free thresholds
 *   ranges           [n_scans * n_beams] float32
 *   robot_poses_xyt  [n_scans * 3]       the (base-transformed) vertex estimates
 *   hits_out, misses_out  [rows * cols] int32, cell (x, y) at x * cols + y (nullable)
 *   image_out        [rows * cols] uint8: 0 free, 100 occupied, 255 unknown (nullable)
 *   kernel_seconds_out    HIP-event time of the two kernels (nullable)                                      */
typedef struct cgmr_occupancy_config {
  float resolution, offset_x, offset_y;
  int32_t rows, cols;
  float max_range, usable_range, infinity_filling_range;
  int32_t gain, square_size;
  double first_beam_angle, angular_step, laser_max_range;
  double laser_pose[3];
  float threshold, free_threshold;
} cgmr_occupancy_config;
int cgmr_occupancy_map(cgmr_ctx* ctx, const cgmr_occupancy_config* cfg, int n_scans, int n_beams, const float* ranges,
                       const double* robot_poses_xyt, int32_t* hits_out, int32_t* misses_out, uint8_t* image_out,
                       double* kernel_seconds_out);

/* ------------------------------------------------------------------ scan ranking and greedy pruning
 * Which key frames is the map worth keeping for?  After Kretzschmar and Stachniss, "Information-theoretic compression of pose
 * graphs for laser-based SLAM": a scan is worth what it tells the occupancy map, and scans are discarded greedily, each time
 * the one whose loss raises the map's entropy least.  Everything is over the FrequencyMap counters exactly as
 * cgmr_occupancy_map produces them (same cfg, same arguments, the same ray walk on the device).
 *
 *   cell entropy      f(h, m) = -p ln p - (1 - p) ln(1 - p), p = (h + 1) / (h + m + 2), in nats and in double: the Bernoulli
 *                     entropy of the posterior mean under a uniform prior; f(0, 0) = ln 2
 *   map entropy       H(T) = sum over all rows * cols cells of f(H_c, M_c), T the totals of all scans
 *   a scan's counts   (h_s,c, m_s,c): what integrateScan + fillRobotPose of scan s alone adds to cell c
 *   information       dH_s(T) = sum over the cells with h_s,c + m_s,c > 0 of f(H_c - h_s,c, M_c - m_s,c) - f(H_c, M_c): the
 *                     entropy the map gains if s is dropped; negative for a scan that contradicts the others
 *   greedy pruning    all scans alive, T their sum; each round takes, among the alive scans with protected[s] == 0, the
 *                     minimum of dH_s(T) under the total order (dH, s) -- unless max_remove scans are gone, there is no
 *                     candidate, or max_entropy_increase >= 0 and the sum of the taken deltas plus this one exceeds it: then
 *                     the loop stops before taking it.  Taking: order[k] = s, delta[k] = dH_s, T loses the scan's counts.
 *
 * cgmr_scan_information: for every scan dH_s against the totals of all (delta_out [n_scans]), the cells it touches (cells_out
 * [n_scans] int32), the sums of its hits and misses (hit_sum_out, miss_sum_out [n_scans] int64), the totals (hits_out,
 * misses_out [rows * cols], equal to cgmr_occupancy_map's) and H(T) (map_entropy_out).  Every output is nullable.
 * n_scans == 0: CGMR_OK, zero totals, map_entropy = rows * cols * ln 2.
 *
 * cgmr_scan_prune: the greedy loop, resident on the device (per round: the dH pass, one workgroup that picks and applies the
 * stop rules, the subtraction; all rounds queued at once, one wait).  protected_or_null [n_scans] uint8; order_out, delta_out
 * [min(max_remove, n_scans)], the first *n_removed_out written; entropy_before_out = H(all scans), entropy_after_out = H of the
 * final totals, recomputed from them; hits_out / misses_out the final totals: bit for bit cgmr_occupancy_map over the kept
 * scans.  n_removed_out is required, order_out and delta_out when min(max_remove, n_scans) > 0; the rest is nullable.
 *
 * Scratch.  Every scan counts into a window of its own: the bounding box of the map cells its walk visits, 8 bytes a cell.  A
 * pre-pass finds the boxes (one read-back).  scratch_bytes_limit bounds the windows that exist at one time; 0 means
 * CGMR_SCAN_INFO_DEFAULT_SCRATCH.  cgmr_scan_information works through the scans in chunks of consecutive scans (each chunk
 * filled, in scan order, until the next window would not fit); the result does not depend on the chunks.  cgmr_scan_prune needs
 * all windows at once and returns CGMR_E_ALLOC, with the bytes needed in cgmr_last_error, when they do not fit -- after the
 * pre-pass, before anything of the selection is queued and with every output untouched.  So does either call when one window
 * alone exceeds the limit.  cgmr_scan_info_last_stats: out[0] the bytes of all windows of the last successful call on this
 * context, out[1] its chunks, out[2] its largest window in bytes, out[3] the greedy rounds it queued.
 *
 * CGMR_E_INVALID, before anything is queued and with the outputs untouched: what cgmr_occupancy_map refuses, gain < 0,
 * scratch_bytes_limit < 0, max_remove < 0, a NaN max_entropy_increase, a required pointer that is null.  Deterministic: the
 * counts are integer sums, every floating-point sum has a fixed order that depends on a cell's place in its window only, and
 * there are no floating-point atomics -- two calls give identical bytes, two identical scans identical dH (the lower index is
 * taken first).  kernel_seconds_out: HIP-event time of the pre-pass plus everything queued after it. */
#define CGMR_SCAN_INFO_DEFAULT_SCRATCH ((int64_t)1 << 30)
int cgmr_scan_information(cgmr_ctx* ctx, const cgmr_occupancy_config* cfg, int n_scans, int n_beams, const float* ranges,
                          const double* robot_poses_xyt, int64_t scratch_bytes_limit, double* delta_out, int32_t* cells_out,
                          int64_t* hit_sum_out, int64_t* miss_sum_out, int32_t* hits_out, int32_t* misses_out,
                          double* map_entropy_out, double* kernel_seconds_out);
int cgmr_scan_prune(cgmr_ctx* ctx, const cgmr_occupancy_config* cfg, int n_scans, int n_beams, const float* ranges,
                    const double* robot_poses_xyt, const uint8_t* protected_or_null, int max_remove, double max_entropy_increase,
                    int64_t scratch_bytes_limit, int32_t* order_out, double* delta_out, int32_t* n_removed_out,
                    double* entropy_before_out, double* entropy_after_out, int32_t* hits_out, int32_t* misses_out,
                    double* kernel_seconds_out);
int cgmr_scan_info_last_stats(const cgmr_ctx* ctx, int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* CGMR_H */
