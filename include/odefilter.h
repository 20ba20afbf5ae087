/* libodefilter_hip.so -- C ABI of the MI355X (gfx950) Gaussian ODE-filter hot path.
 *
 * Drop-in boundary for the Kalman predict / measure / calibrate / update / smooth path of
 * ProbNumDiffEq.jl v0.1.5 (nathanaelbosch/ODEFilters.jl).  Citations are file:line in the
 * reference tree.  A Julia host (`julia/ODEFilterHIP.jl`) binds these
 * entry points with `ccall`; the Python host mirror (`odefilters.jl_amd/host.py`) binds the
 * same symbols with ctypes.  Plain pointers and sizes only; no callbacks into the host.
 *
 * What each entry point replaces in the reference:
 *   odef_create / odef_destroy      alg_cache(alg::GaussianODEFilter, ...)        src/caches.jl:42-114
 *                                   (A, Q, Precond, Proj, work arrays; EK0/EK1 kwargs src/algorithms.jl:23-51)
 *   odef_set_problem*               ODEProblem(f,u0,tspan,p) x EnsembleProblem prob_func; initialize! +
 *                                   initial_update!                              src/perform_step.jl:2-12,
 *                                                                                src/state_initialization.jl:2-53
 *   odef_solve_fixed                solve(prob, alg; adaptive=false, dt) = loop of perform_step!
 *                                                                                src/perform_step.jl:27-93
 *                                   incl. predict!/update!                       src/filtering.jl:17-48,79-91
 *                                   measure!                                     src/perform_step.jl:95-132
 *                                   estimate_diffusion                           src/diffusions.jl:11-36,71-80
 *                                   savevalues!                                  src/integrator_utils.jl:33-48
 *   odef_solve_adaptive             same + estimate_errors                       src/perform_step.jl:78-84,148-158
 *                                   + PI controller (exponents src/alg_utils.jl:23-24; loop is OrdinaryDiffEq's)
 *   odef_smooth                     postamble! -> smooth_all! -> smooth!         src/integrator_utils.jl:2-30,
 *                                                                                src/smoothing.jl:4-63
 *   ODEF_IEKS contexts              IEKS, solve_ieks: odef_solve_fixed + odef_smooth, repeated  src/ieks.jl:2-61
 *                                   measure! with J = f.jac(linearize_at(t).mu)  src/perform_step.jl:111-113
 *   odef_dense_output               sol(t), GaussianODEFilterPosterior            src/solution.jl:165-214
 *   odef_sample                     sample_states / sample                        src/solution_sampling.jl:15-62
 *   odef_dense_sample               dense_sample_states / dense_sample            src/solution_sampling.jl:63-75
 *   odef_rhs_compile                the user's f / f.jac closure (compiled, not called) src/perform_step.jl:106,116-121
 *   odef_get / odef_get_device      sol.t, sol.x_filt, sol.x_smooth, sol.diffusions, sol.log_likelihood,
 *                                   sol.destats, sol.retcode                     src/solution.jl:8-24
 *   odef_predict / odef_update /
 *   odef_smooth_step                predict!, update!, smooth (pure functions)   src/filtering.jl:17,79,136
 *   odef_ibm / odef_preconditioner  ibm(d,q), preconditioner(T,d,q)              src/priors.jl:7-59,
 *                                                                                src/preconditioning.jl:1-17
 *   odef_errors_field ids           sol.errors, sol.u_analytic                    src/solution.jl:10-11,68-74,129-130
 *   odef_data_field ids             nothing in this version of the reference (later ones ship it as fenrir_data_loglik): the
 *                                   marginal log-likelihood of noisy observations under the posterior, per trajectory
 *   odef_event_field ids            nothing in the reference itself: what a ContinuousCallback with the condition u[c] - level
 *                                   answers in the SciML interface it plugs into, asked of the finished posterior
 *   odef_summary_field ids          nothing in the reference: per-time mean and covariance of the ensemble's Gaussian mixture,
 *                                   reduced on the device and read with odef_get (see odef_summary_field)
 *   odef_quantile_field ids         nothing in the reference: per-time quantiles of the ensemble's posterior means (median,
 *                                   credible bands), selected on the device (see odef_quantile_field)
 *   odef_wsummary_field ids         nothing in the reference: the summary with a weight per trajectory -- what the ensemble
 *                                   predicts given data --, the effective sample size and the log evidence (see odef_wsummary_field)
 *   odef_group_* / odef_allgather   nothing in the reference (it has no ensemble and no distributed code):
 *                                   the EnsembleProblem axis sharded over the GPUs of one node by ONE host process, the
 *                                   per-trajectory path above unchanged on every shard, one RCCL all-gather at the end
 *
 * Error convention: every function returns 0 on success, <0 on API / HIP failure with a
 * message in odef_last_error().  Numerical trouble is per trajectory (RETCODE field) and
 * never aborts the batch (the reference throws / asserts: src/numerics_tricks.jl:1-6,
 * src/smoothing.jl:25).
 *
 * Device data layout (all double unless noted), N = n_traj, D = d*(order+1), TRI = D(D+1)/2,
 * trajectory index fastest so that one 64-lane wavefront (one lane per trajectory) stores
 * 512 contiguous bytes per field element:
 *   MEAN        [n_save][D][N]     state ordering derivative-major (src/caches.jl:63-64)
 *   COV_TRIL    [n_save][TRI][N]   packed lower triangle, element (i,j), i>=j at i(i+1)/2+j, of
 *                                  Sigma = L L'  (`SquarerootMatrix.mat`, src/squarerootmatrix.jl:16)
 *   DIFFUSION   [n_save][N]        entry s = global diffusion of the step that produced save s (s>=1); [0]=0
 *               [n_save][d][N]     MV models (:dynamicMV / :fixedMV): the diagonal of that global diffusion; [0][.]=0
 *   T           [n_save] (fixed)   or [n_save][N] (adaptive)
 *   LOGLIK      [N]                sum of per-accepted-step log-likelihoods (src/perform_step.jl:66,91)
 *   NACCEPT, NREJECT, NF, NJAC     int32 [N]   (destats)
 *   NSAVED      int32 [N]          number of valid saves of a trajectory (adaptive)
 *   RETCODE     int32 [N]          odef_retcode
 *   SMOOTH_MEAN / SMOOTH_COV_TRIL  as MEAN / COV_TRIL after odef_smooth
 *   LINEARIZE_AT [n_save][d][N]    IEKS only: the u part of a mean per save; step s -> s+1 reads row s+1, row 0 is unused.
 *                                  Empty after odef_create, odef_set_problem* and odef_bind_device(ctx, F, NULL, 0): the step
 *                                  is EK1.  Bound with odef_bind_device: caller memory, read only, at least n_t*d*N doubles
 *                                  (IEKS(linearize_at = sol)).  Set by odef_smooth after a fixed-grid solve: rows 0..d-1 of
 *                                  every SMOOTH_MEAN save, owned (a bound buffer is let go, never written), valid for that
 *                                  grid only (alg.linearize_at = sol) -- odef_solve_fixed on another grid refuses it.
 * odef_get copies a field to host memory in exactly this layout.
 */
#ifndef ODEFILTER_H
#define ODEFILTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ODEF_VERSION 100

typedef struct odef_ctx odef_ctx;

/* EK0 / EK1 (src/algorithms.jl:23-51) and IEKS, the iterated extended Kalman smoother (src/ieks.jl:2-61): an EK1 context whose
 * step evaluates the Jacobian at ODEF_F_LINEARIZE_AT when that field holds data (src/perform_step.jl:111-125), at the
 * prediction (= EK1) when it is empty.  IEKS always smooths: odef_create refuses smooth = 0, the MV diffusion models and fields
 * on the workgroup-per-trajectory kernels (Pleiades, Lorenz-96, run-time fields with d(q+1) > 20 or d > 10).  On an IEKS context
 * odef_smooth after odef_solve_fixed sets ODEF_F_LINEARIZE_AT to the smoothed u on that grid, so that repeating
 * odef_solve_fixed + odef_smooth is solve_ieks (src/ieks.jl:52-61); odef_solve_adaptive runs while the field is empty only. */
typedef enum { ODEF_EK0 = 0, ODEF_EK1 = 1, ODEF_IEKS = 2 } odef_alg;
/* diffusionmodel = :dynamic / :fixed / :fixedMAP / :dynamicMV / :fixedMV (src/caches.jl:89-96, src/diffusions.jl:11-36, 46-68,
 * 71-80, 83-153).  The MV ("multivariate") models calibrate one diffusion per state component, Sigma = diag(sigma_1..sigma_d);
 * they require EK0 and run on the lane kernels only (state dimension d(q+1) <= 20 and d <= 10: not Pleiades, not Lorenz-96),
 * odef_create refuses anything else.  Their ODEF_F_DIFFUSION field is [n_save][d][N]. */
typedef enum {
  ODEF_DIFFUSION_DYNAMIC = 0,
  ODEF_DIFFUSION_FIXED = 1,
  ODEF_DIFFUSION_FIXED_MAP = 2,
  ODEF_DIFFUSION_DYNAMIC_MV = 3,
  ODEF_DIFFUSION_FIXED_MV = 4
} odef_diffusion;
typedef enum {
  ODEF_RHS_FHN = 0,            /* u' = (c(u1 - u1^3/3 + u2), -(u1 - a - b u2)/c), p = (a,b,c) */
  ODEF_RHS_LORENZ63 = 1,       /* p = (sigma, rho, beta) */
  ODEF_RHS_LOTKA_VOLTERRA = 2, /* u' = (a u1 - b u1 u2, -c u2 + d u1 u2), p = (a,b,c,d) */
  ODEF_RHS_VANDERPOL = 3,      /* u' = (u2, mu((1-u1^2)u2 - u1)), p = (mu) */
  ODEF_RHS_LINEAR = 4,         /* u_i' = p_i u_i, d = 2 */
  ODEF_RHS_PLEIADES = 5,       /* 7-body, d = 28, no parameters; workgroup-per-trajectory kernels (matrix cores) */
  ODEF_RHS_LORENZ96 = 6,       /* u_i' = (u_{i+1} - u_{i-2}) u_{i-1} - u_i + F, d = 16, p = (F); workgroup-per-trajectory kernels */
  ODEF_RHS_FORCED = 7          /* time-dependent: u' = (p0 u1 + p1 t, p2 t u2), d = 2, p = (p0, p1, p2); has an `analytic` */
} odef_rhs;
typedef enum { ODEF_SAVE_FINAL = 0, ODEF_SAVE_EVERYSTEP = 1 } odef_save_mode;
typedef enum {
  ODEF_RET_SUCCESS = 0,
  ODEF_RET_MAXITERS = 1,
  ODEF_RET_DT_LESS_THAN_MIN = 2,
  ODEF_RET_UNSTABLE = 3,       /* NaN/Inf in the state */
  ODEF_RET_NEGATIVE_VARIANCE = 4
} odef_retcode;
typedef enum {
  ODEF_F_MEAN = 0,
  ODEF_F_COV_TRIL = 1,
  ODEF_F_DIFFUSION = 2,
  ODEF_F_T = 3,
  ODEF_F_LOGLIK = 4,
  ODEF_F_NACCEPT = 5,
  ODEF_F_NREJECT = 6,
  ODEF_F_NF = 7,
  ODEF_F_NJAC = 8,
  ODEF_F_NSAVED = 9,
  ODEF_F_RETCODE = 10,
  ODEF_F_SMOOTH_MEAN = 11,
  ODEF_F_SMOOTH_COV_TRIL = 12,
  ODEF_F_U0 = 13,              /* [d][N] initial values as held on the device */
  ODEF_F_DENSE_MEAN = 14,      /* [n_q][D][N]   result of odef_dense_output */
  ODEF_F_DENSE_COV_TRIL = 15,  /* [n_q][TRI][N] */
  ODEF_F_SAMPLES = 16,         /* [n_save][D][n_samples][N] result of odef_sample */
  ODEF_F_LINEARIZE_AT = 17,    /* [n_save][d][N] IEKS linearisation points (see odef_alg) */
  ODEF_F_COUNT_
} odef_field;

/* Derived outputs and their caches.  Six families of fields are computed from the records on the device when first asked for --
 * the ensemble summary (odef_summary_field), the solution errors (odef_errors_field), the data log-likelihood
 * (odef_data_field) the event times (odef_event_field), the ensemble quantiles (odef_quantile_field) and the weighted ensemble summary (odef_wsummary_field) -- and cached; odef_field_bytes, odef_get and odef_get_device serve them like any other field.  One rule says
 * when a cached result is dropped, so that the next request computes it again.  The context tracks nine things that can change:
 *   the filter records    MEAN, COV_TRIL, DIFFUSION, T                 source 0
 *   the smoothed records  SMOOTH_MEAN, SMOOTH_COV_TRIL                 source 1
 *   the dense records     DENSE_MEAN, DENSE_COV_TRIL                   source 2
 *   the problem           u0, p, t0
 *   the bound truth       ODEF_E_REFERENCE
 *   the observations      ODEF_L_OBS_SAVE / COMPONENT / VALUE / NOISE / TIME
 *   the event spec        ODEF_EV_SPEC / ODEF_EV_LEVEL
 *   the probabilities     ODEF_Q_PROBS
 *   the log-weights       ODEF_W_LOGWEIGHT
 * and what is derived from what:
 *   the summary of source k       its record set; a new problem drops it as well
 *   the errors of source k        its record set, the bound truth, the problem
 *   the data log-likelihood       the filter records, the observations, the problem
 *   the events of source k        its record set, the filter records (both sources predict from them), the event spec, the problem
 *   the quantiles of source k     its record set, the problem (as for the summary), the probabilities
 *   the weighted summary of source k   its record set, the problem (as for the summary), the log-weights
 *   the filter records that odef_solve_fixed leaves staged for odef_smooth (the workgroup-per-trajectory path)   the filter records
 * A record set changes when an entry point writes it -- odef_solve_* all three (every summary includes its trajectories by the
 * RETCODE of the solve), odef_smooth the smoothed, odef_dense_output / odef_dense_sample the dense records -- and when the caller
 * may: odef_bind_device of one of its fields replaces the buffer, and odef_get_device of one hands out a WRITABLE pointer, so both
 * count as a change of the whole set.  odef_set_problem* change the problem, a bind of ODEF_E_REFERENCE the truth, a bind of an
 * ODEF_L_OBS_* the observations, a bind of ODEF_EV_SPEC or ODEF_EV_LEVEL the event spec, a bind of ODEF_Q_PROBS the probabilities, a bind of ODEF_W_LOGWEIGHT the log-weights.  odef_get, the host copy, changes nothing.  Records edited through a pointer taken EARLIER are not
 * seen: take the pointer again (or bind) after writing. */

/* Ensemble summary per time, reduced on the device (nothing in the reference: it has no ensemble).  For one time and the n
 * trajectories that are INCLUDED there -- RETCODE == ODEF_RET_SUCCESS and the d solution entries of the mean at that time finite --
 * with mu_i the solution part of the posterior mean (rows 0..d-1 of a record) and Sigma_i the d x d solution block of its covariance:
 *   COUNT        n                                              int64  [n_t]
 *   MEAN         m = (1/n) sum_i mu_i                           double [n_t][d]
 *   COV_WITHIN   W = (1/n) sum_i Sigma_i                        double [n_t][d(d+1)/2] packed lower triangle, (k,l), k>=l at k(k+1)/2+l
 *   COV_BETWEEN  B = (1/n) sum_i (mu_i - m)(mu_i - m)'          double [n_t][d(d+1)/2]
 * m and W + B are the mean and covariance of the equal-weight mixture of the trajectories' Gaussian posteriors.  The divisor is n;
 * with n = 0 the three moments are NaN.  Field id = ODEF_S_BASE + 8 * source + quantity, source 0: the filter records (n_t =
 * odef_n_save), 1: the smoothed records, 2: the last odef_dense_output / odef_dense_sample result (n_t = n_q).  odef_field_bytes,
 * odef_get and odef_get_device accept these ids (odef_bind_device does not).  The first request for a source after its records
 * changed runs the reduction on the context's stream (two passes, the covariance of the means is centred before it is squared;
 * deterministic, no floating-point atomics) and caches the four arrays (dropped as "Derived outputs and their caches" above
 * says).  Refused with a message: any source before a solve, source 1 before
 * odef_smooth, source 2 before a dense output, sources 0 / 1 after an ADAPTIVE solve (the records of one save index lie at
 * different times per trajectory: evaluate odef_dense_output at common times and use source 2).  With ODEF_SAVE_FINAL source 0
 * summarises the one record.  odef_kernel_time_ms / odef_kernel_name report the last reduction as which = 2. */
typedef enum {
  ODEF_S_BASE = 64,
  ODEF_S_FILTER_COUNT = 64,
  ODEF_S_FILTER_MEAN = 65,
  ODEF_S_FILTER_COV_WITHIN = 66,
  ODEF_S_FILTER_COV_BETWEEN = 67,
  ODEF_S_SMOOTH_COUNT = 72,
  ODEF_S_SMOOTH_MEAN = 73,
  ODEF_S_SMOOTH_COV_WITHIN = 74,
  ODEF_S_SMOOTH_COV_BETWEEN = 75,
  ODEF_S_DENSE_COUNT = 80,
  ODEF_S_DENSE_MEAN = 81,
  ODEF_S_DENSE_COV_WITHIN = 82,
  ODEF_S_DENSE_COV_BETWEEN = 83
} odef_summary_field;

/* Solution errors per trajectory, reduced on the device: sol.errors and sol.u_analytic of the reference (src/solution.jl:10-11,
 * 68-74, 129-130; test/specific_problems.jl:25-37).  For trajectory i over its own saves k = 0..n-1, e_k = u_k - u*_k in R^d with u_k
 * rows 0..d-1 of the mean and Sigma_k the d x d solution block of the covariance:
 *   FINAL       mean_a |e_{n-1,a}|                              double [N]   (DiffEqBase calculate_solution_errors!, :final)
 *   L2          sqrt(mean_{k,a} e_{k,a}^2)                      double [N]   (:l2)
 *   LINF        max_{k,a} |e_{k,a}|                             double [N]   (:l-infinity)
 *   CHI2        mean_k e_k' Sigma_k^+ e_k / d                   double [N]   nothing in the reference: ~ 1 for a calibrated posterior.
 *                                                               Saves whose block is exactly zero (the initial record; u' = 0) are
 *                                                               left out; NaN when none is left.  A non-positive pivot of the
 *                                                               factorisation drops its direction.
 *   NUSED       number of saves in L2 / LINF                    int64  [N]   adaptive solves: the zero-length repeats of rejected
 *                                                               attempts are skipped, NUSED = accepted steps + 1
 *   U_ANALYTIC  u* at the trajectory's own save times           double [n_save][d][N], computed when asked for
 * Field id = ODEF_E_BASE + 8 * source + quantity, source 0: the filter records, 1: the smoothed records (the reference's sol.u after
 * smooth = true).  odef_field_bytes, odef_get and odef_get_device accept these ids.  The truth u* comes from
 *   (a) the vector field's `analytic(u0, p, t, out)` member (ODEF_RHS_LINEAR has one; a run-time compiled field may), or
 *   (b) a reference buffer [n_save][d][N] in device memory bound with odef_bind_device(ctx, ODEF_E_REFERENCE, ptr, bytes) -- read
 *       only, never written, fixed grids only; (ptr = NULL lets it go).  A bound reference takes precedence; U_ANALYTIC is then
 *       that buffer.
 * The first request for a source runs the pass on the context's stream (deterministic, no floating-point atomics: two requests
 * agree bit for bit) and caches the five small arrays (dropped as "Derived outputs and their caches" above says).  Refused
 * with a message: before a solve, source 1 before odef_smooth, a field without
 * `analytic` and nothing bound, a bound reference after an ADAPTIVE solve (per-trajectory times: use `analytic`).  A trajectory
 * whose RETCODE is not Success still gets numbers over the saves it has; non-finite entries propagate as NaN.
 * odef_kernel_time_ms / odef_kernel_name report the last pass as which = 3. */
typedef enum {
  ODEF_E_BASE = 128,
  ODEF_E_FINAL = 128,
  ODEF_E_L2 = 129,
  ODEF_E_LINF = 130,
  ODEF_E_CHI2 = 131,
  ODEF_E_NUSED = 132,
  ODEF_E_U_ANALYTIC = 133,
  ODEF_E_SMOOTH_FINAL = 136,
  ODEF_E_SMOOTH_L2 = 137,
  ODEF_E_SMOOTH_LINF = 138,
  ODEF_E_SMOOTH_CHI2 = 139,
  ODEF_E_SMOOTH_NUSED = 140,
  ODEF_E_SMOOTH_U_ANALYTIC = 141,
  ODEF_E_REFERENCE = 144 /* odef_bind_device only */
} odef_errors_field;

/* Data log-likelihood of noisy observations per trajectory, on the device (nothing leaves it but 16 N bytes).  The filter records
 * (m_k, Sigma_k) of a FIXED grid and the backward transitions of the RTS smoother define a Gauss-Markov posterior over the path;
 * the marginal likelihood of observations y_j = H x(t_{k_j}) + N(0, R) under it is one backward sweep (the "Fenrir" likelihood of
 * Tronarp, Bosch and Hennig 2022), k = n_save - 1 down to the first observed save, xi starting as the last filter record:
 *     k < n_save - 1, h = t_{k+1} - t_k != 0, in the coordinates preconditioned with P(h) as odef_smooth does:
 *         B = A Sigma_k A' + sigma2_k Q;  G = Sigma_k A' B^-1;  xi.m <- m_k + G (xi.m - A m_k);  xi.P <- Sigma_k + G (xi.P - B) G'
 *         (sigma2_k: DIFFUSION[k + 1], the value odef_smooth uses for that step; a non-positive pivot of B drops its direction)
 *     k = k_j:  v = y_j - H xi.m;  S = H xi.P H' + R;  l += -1/2 (v' S^-1 v + log det S + o log 2 pi);  q += v' S^-1 v
 *               K = xi.P H' S^-1;  xi.m += K v;  xi.P -= K S K'
 *   ODEF_L_DATA_LOGLIK       l  double [N]     odef_field_bytes / odef_get / odef_get_device
 *   ODEF_L_DATA_MAHALANOBIS  q  double [N]     chi^2 with M o degrees of freedom for a calibrated model
 * Inputs, device memory bound with odef_bind_device (read only, never written; NULL lets one go); M and o follow from the byte counts:
 *   ODEF_L_OBS_SAVE       int64  [M]           observed save indices k_1 < ... < k_M in 0 .. n_save - 1 (save 0 may be observed)
 *   ODEF_L_OBS_COMPONENT  int64  [o]           observed state components c_1 < ... < c_o in 0 .. d - 1: H is those rows of E0
 *   ODEF_L_OBS_VALUE      double [M][o]        shared by the ensemble, or [M][o][N] per trajectory (told by the byte count, as for p)
 *   ODEF_L_OBS_NOISE      double [o]           variances r > 0, R = diag r
 * The first request runs the pass on the context's stream (one launch, one lane per trajectory; SAVE, COMPONENT and NOISE are copied
 * to the host and validated there) and caches both outputs (dropped as "Derived outputs and their caches" above says); two
 * requests agree bit for bit.  Refused with a message: before a solve; after an ADAPTIVE solve (observation times are per ensemble, the
 * grid per trajectory); the MV diffusion models; a (d, q) without a kernel (built for d <= 4, q <= 5, d (q + 1) <= 20); an input
 * missing; byte counts that do not agree; saves or components that are not strictly increasing or out of range; a noise variance
 * that is not finite and positive; a context that kept only the final state.  A non-positive pivot of S or a NaN in a record the
 * sweep reads gives NaN for that trajectory only; a trajectory whose RETCODE is not Success still gets a number.
 * odef_kernel_time_ms / odef_kernel_name report the last pass as which = 4; its n_launches counts the passes launched since the
 * context was created (a request served from the cache leaves it unchanged).
 *
 * Observations at ARBITRARY TIMES, after fixed-grid and after adaptive solves: bind
 *   ODEF_L_OBS_TIME       double [M]           times tau_1 < ... < tau_M, t0 <= tau_1 (fixed grid: tau_M <= the last save time)
 * INSTEAD of ODEF_L_OBS_SAVE (COMPONENT, VALUE, NOISE as above).  The sweep then runs per trajectory over its own records
 * t_0 .. t_{n-1} (n = n_save on a fixed grid, NSAVED[i] with the times T after an adaptive solve) plus one node per tau_j that is
 * none of its save times: for t_k < tau_j < t_{k+1} the filter's prediction from record k over h1 = tau_j - t_k, in the
 * coordinates of P(h1), with sigma2 = DIFFUSION[k + 1] -- what odef_dense_output forms for the filter source; two nodes of one
 * step are both predicted from record k.  A node takes the RTS step above against xi with h2 = (time of xi) - tau_j in the
 * coordinates of P(h2) and the same DIFFUSION[k + 1], and is then observed; tau_j == t_k is observed at save k.  A tau_j above a
 * trajectory's own last save (an adaptive solve whose RETCODE is not Success) gives NaN for that trajectory only.  Which pass runs:
 * OBS_TIME bound and OBS_SAVE not, this one (odef::data_loglik_times_kernel, named by which = 4); OBS_SAVE bound and OBS_TIME
 * not, the one above, unchanged; both bound, refused.  Refused in addition: a (d, q) outside d <= 4, q <= 5, d (q + 1) <= 12
 * (the pairs odef_dense_output serves per lane) and the workgroup-per-trajectory path; times that are not finite, not strictly
 * increasing, below t0 or, on a fixed grid, above the last save.  TIME, COMPONENT and NOISE are validated on the host. */
typedef enum {
  ODEF_L_BASE = 192,
  ODEF_L_DATA_LOGLIK = 192,
  ODEF_L_DATA_MAHALANOBIS = 193,
  ODEF_L_OBS_SAVE = 200,      /* odef_bind_device only */
  ODEF_L_OBS_COMPONENT = 201, /* odef_bind_device only */
  ODEF_L_OBS_VALUE = 202,     /* odef_bind_device only */
  ODEF_L_OBS_NOISE = 203,     /* odef_bind_device only */
  ODEF_L_OBS_TIME = 204       /* odef_bind_device only */
} odef_data_field;

/* Event location per trajectory, on the device: the times at which component c of the posterior mean crosses a level -- what a
 * ContinuousCallback with the condition u[c] - level answers in a SciML-style solver, here asked of the finished posterior (the solve
 * is not stopped and the state not modified).  Per trajectory i over its own saves t_0 .. t_{n-1} (n = odef_n_save on a fixed grid,
 * NSAVED[i] after an adaptive solve), with g_k = m_c[k] - level_i, m the mean record of the source:
 *   bracket   an interval k -> k + 1 with t_{k+1} > t_k is an UP bracket if g_k < 0 && g_{k+1} >= 0, a DOWN bracket if g_k > 0 &&
 *             g_{k+1} <= 0; direction +1 / -1 keeps the up / down brackets, 0 both.  A zero-length interval (a repeated tstop, the
 *             repeat of a rejected attempt) holds no event; a NaN (record or level) makes every comparison false: no event; g_0 == 0
 *             is not an event.  A crossing that does not show at the two ends of a step (a double root inside one step) is NOT
 *             detected.  A trajectory whose RETCODE is not Success is scanned over the records it has.
 *   COUNT     the brackets of the whole trajectory (may exceed K); the first min(COUNT, K) in time order are located
 *   root      g_{k+1} == 0: t* = t_{k+1}, every output is the stored record, NEVAL = 0.  Otherwise the root in (t_k, t_{k+1}) of
 *             E[u_c(t)] - level_i under the source's dense posterior (the semantics of odef_dense_output), by bracketed Newton with
 *             the slope E[u'_c(t)], entry d + c of the same evaluation: start at the secant point of the bracket's ends, shrink the
 *             bracket by the sign of g after each evaluation, replace an iterate outside the closed bracket (or a zero / non-finite
 *             slope) by the midpoint, stop at g == 0 or a step of at most 2^-40 (t_{k+1} - t_k); at most 64 evaluations, at the cap
 *             the current iterate is returned.  The outputs are one dense evaluation at t*.  Source 0 only: the filter's dense mean on
 *             (t_k, t_{k+1}) is the prediction from save k and jumps at t_{k+1} by the measurement update, so a bracket of the stored
 *             means may hold no root.  The first evaluation is therefore the left limit at t_{k+1}; if it has not passed the level
 *             the crossing lies inside the update: t* = t_{k+1}, every output is the stored record, NEVAL = 1.  (The smoothed
 *             interpolant is continuous at the saves.)
 * Field id = ODEF_EV_BASE + 8 * source + quantity, source 0: the filter posterior, 1: the smoothed posterior; slot s of K:
 *   COUNT      int32  [N]
 *   TIME       double [K][N]      t*
 *   TIME_VAR   double [K][N]      Var u_c(t*) / (E u'_c(t*))^2, the first-order variance of the event time (plain IEEE: zero slope -> inf)
 *   U          double [K][d][N]   E[u(t*)]
 *   DIRECTION  int32  [K][N]      +1 up, -1 down
 *   SAVE       int32  [K][N]      k, the left save of the bracket (a raw record index after an adaptive solve)
 *   NEVAL      int32  [K][N]      dense evaluations spent (distinct times, the one at t* included)
 * Unused slots hold NaN in the doubles, 0 in DIRECTION and NEVAL, -1 in SAVE.  odef_field_bytes, odef_get and odef_get_device accept
 * these ids.  Inputs, device memory bound with odef_bind_device (read only, never written; NULL lets one go):
 *   ODEF_EV_SPEC   int64  [3]          {component c, direction, K}
 *   ODEF_EV_LEVEL  double [1] or [N]   shared, or per trajectory (told by the byte count, as for p)
 * The first request for a source copies the three spec words to the host, validates them, runs the pass on the context's stream
 * (two launches: a scan of row c of the mean records, then the refinement, one lane per trajectory and slot) and caches all outputs
 * of that source (dropped as "Derived outputs and their caches" above says); two requests agree bit for bit.  Refused with a
 * message: before a solve; source 1 before odef_smooth; a context that kept only the final state; the MV diffusion models; a (d, q)
 * without a kernel (built for d <= 4, q <= 5, d (q + 1) <= 12); an input missing; ODEF_EV_SPEC not 24 bytes; a level of neither 8
 * nor 8 N bytes; a component outside 0 .. d - 1; a direction outside {-1, 0, 1}; K < 1, K > 65535, or K N max(d, 1) 8 bytes at or
 * above 2 GiB.  odef_kernel_time_ms / odef_kernel_name report the last pass as which = 5; its n_launches counts the launches since
 * the context was created (a request served from the cache leaves it unchanged). */
typedef enum {
  ODEF_EV_BASE = 256,
  ODEF_EV_COUNT = 256,
  ODEF_EV_TIME = 257,
  ODEF_EV_TIME_VAR = 258,
  ODEF_EV_U = 259,
  ODEF_EV_DIRECTION = 260,
  ODEF_EV_SAVE = 261,
  ODEF_EV_NEVAL = 262,
  ODEF_EV_SMOOTH_COUNT = 264,
  ODEF_EV_SMOOTH_TIME = 265,
  ODEF_EV_SMOOTH_TIME_VAR = 266,
  ODEF_EV_SMOOTH_U = 267,
  ODEF_EV_SMOOTH_DIRECTION = 268,
  ODEF_EV_SMOOTH_SAVE = 269,
  ODEF_EV_SMOOTH_NEVAL = 270,
  ODEF_EV_SPEC = 280, /* odef_bind_device only */
  ODEF_EV_LEVEL = 281 /* odef_bind_device only */
} odef_event_field;

/* Ensemble quantiles per time, selected on the device: the order statistics that the ensemble summary leaves out (SciML's
 * EnsembleSummary: med, qlow, qhigh; nothing in the reference, it has no ensemble).  For one time s, one component a < d and
 * probabilities p_1..p_P (1 <= P <= 8, each finite and in [0, 1]; they need not be sorted or distinct), with x_(0) <= ... <=
 * x_(n-1) the sorted values of row a of the mean over the n trajectories INCLUDED at s by the rule of the summary (RETCODE ==
 * ODEF_RET_SUCCESS and the d solution entries of the mean at s finite):
 *   h = (double)(n-1) p,  lo = min(floor(h), n-1),  hi = min(lo+1, n-1),  g = h - lo,
 *   Q = x_(lo) if g == 0, else x_(lo) + g (x_(hi) - x_(lo))      difference, product and sum rounded once each, no FMA
 * -- the type-7 rule of Julia's quantile and numpy's default.  With n = 0 every Q is NaN.
 *   ODEF_Q_FILTER / _SMOOTH / _DENSE              double [n_t][P][d]   source 0 (n_t = odef_n_save) / 1 / 2 (n_t = n_q)
 *   ODEF_Q_COUNT_FILTER / _SMOOTH / _DENSE        int64  [n_t]         the n used; equals ODEF_S_*_COUNT
 *   ODEF_Q_PROBS   double [P]   odef_bind_device only: device memory that stays the caller's (read only; copied to the host and
 *                               validated there; P follows from the byte count); NULL lets it go
 * Field id = ODEF_Q_BASE + 8 * source + quantity.  odef_field_bytes, odef_get and odef_get_device accept the six output ids
 * (odef_bind_device does not).  The first request for a source after its records or the probabilities changed runs the pass on
 * the context's stream -- exact radix selection on order-preserving 64-bit keys, integer counts only, no floating-point atomics:
 * the result is the order statistic itself and two requests agree bit for bit; the pass synchronises the stream once per slab of
 * 1024 / d times, to read back how many digit passes the slab needs -- and caches both arrays (dropped as "Derived
 * outputs and their caches" above says).  Refused with a message: everything the summary refuses (any source before a solve,
 * source 1 before odef_smooth, source 2 before a dense output, sources 0 / 1 after an ADAPTIVE solve: evaluate odef_dense_output
 * at common times and use source 2); no probabilities bound; a byte count that is not 8 P with 1 <= P <= 8; a probability that
 * is NaN or outside [0, 1]; d > 32.  odef_kernel_time_ms / odef_kernel_name report the last pass as which = 6 (its n_launches:
 * the launches of that pass). */
typedef enum {
  ODEF_Q_BASE = 320,
  ODEF_Q_FILTER = 320,
  ODEF_Q_COUNT_FILTER = 321,
  ODEF_Q_SMOOTH = 328,
  ODEF_Q_COUNT_SMOOTH = 329,
  ODEF_Q_DENSE = 336,
  ODEF_Q_COUNT_DENSE = 337,
  ODEF_Q_PROBS = 344 /* odef_bind_device only */
} odef_quantile_field;

/* Weighted ensemble summary per time, reduced on the device: the ensemble summary with a weight per trajectory -- the
 * importance-weighted mixture that answers "what does the ensemble predict given the data" when the weights are
 * exp(data log-likelihood + log prior) -- with the effective sample size and the log evidence (nothing in the reference: it
 * has no ensemble).
 *   ODEF_W_LOGWEIGHT   double [N]   odef_bind_device only: the unnormalised log-weights l_i in device memory that stays the
 *                                   caller's (read only, never written; NULL lets it go; a byte count other than 8 N is
 *                                   refused).  They are not copied to the host and not validated there: a value that is not
 *                                   finite (NaN, +-inf: what ODEF_L_DATA_LOGLIK holds for a trajectory it could not score)
 *                                   EXCLUDES its trajectory.
 * Independent of the time: L = max l_i over the trajectories with RETCODE == ODEF_RET_SUCCESS and l_i finite; v_i = exp(l_i - L)
 * for those and 0 for every other.  If no trajectory qualifies, every time has n = 0.  Trajectory i is INCLUDED at time s when
 * the rule of the summary holds (RETCODE == ODEF_RET_SUCCESS and the d solution entries of the mean at s finite) and l_i is
 * finite.  With Z = sum v_i over the included, w_i = v_i / Z, and mu_i, Sigma_i as for the summary:
 *   COUNT         n, the included trajectories (one whose v_i underflowed to 0 still counts)   int64  [n_t]
 *   MEAN          m = sum_i w_i mu_i                                                           double [n_t][d]
 *   COV_WITHIN    W = sum_i w_i Sigma_i                                                        double [n_t][d(d+1)/2] packed as for the summary
 *   COV_BETWEEN   B = sum_i w_i (mu_i - m)(mu_i - m)'                                          double [n_t][d(d+1)/2]
 *   LOG_EVIDENCE  L + log Z - log n = log((1/n) sum_i exp l_i): with trajectories drawn from the prior and l the data
 *                 log-likelihood, the Monte-Carlo log marginal likelihood                      double [n_t]
 *   ESS           Z^2 / sum_i v_i^2, the effective sample size, in [1, n]                      double [n_t]
 * With n = 0 the three moments, ESS and LOG_EVIDENCE are NaN.  With n > 0 but Z == 0 -- the trajectory that carries L is not
 * included at s and every other weight underflowed -- plain IEEE arithmetic gives NaN moments, NaN ESS and LOG_EVIDENCE = -inf;
 * this is not special-cased.  Field id = ODEF_W_BASE + 8 * source + quantity, quantity 0..5 in the order above, sources as for
 * the summary.  odef_field_bytes, odef_get and odef_get_device accept the eighteen output ids (odef_bind_device does not).  The
 * first request for a source after its records or the log-weights changed runs the pass on the context's stream -- the shift
 * and the weights once per request (one exp per trajectory), then the two passes of the summary, the covariance of the means
 * centred with the final m before it is squared; deterministic, no floating-point atomics: two requests agree bit for bit --
 * and caches the six arrays (dropped as "Derived outputs and their caches" above says).  Refused with a message: everything
 * the summary refuses (any source before a solve, source 1 before odef_smooth, source 2 before a dense output, sources 0 / 1
 * after an ADAPTIVE solve: evaluate odef_dense_output at common times and use source 2); no log-weights bound; d > 32.
 * odef_kernel_time_ms / odef_kernel_name report the last pass as which = 7. */
typedef enum {
  ODEF_W_BASE = 384,
  ODEF_W_FILTER_COUNT = 384,
  ODEF_W_FILTER_MEAN = 385,
  ODEF_W_FILTER_COV_WITHIN = 386,
  ODEF_W_FILTER_COV_BETWEEN = 387,
  ODEF_W_FILTER_LOG_EVIDENCE = 388,
  ODEF_W_FILTER_ESS = 389,
  ODEF_W_SMOOTH_COUNT = 392,
  ODEF_W_SMOOTH_MEAN = 393,
  ODEF_W_SMOOTH_COV_WITHIN = 394,
  ODEF_W_SMOOTH_COV_BETWEEN = 395,
  ODEF_W_SMOOTH_LOG_EVIDENCE = 396,
  ODEF_W_SMOOTH_ESS = 397,
  ODEF_W_DENSE_COUNT = 400,
  ODEF_W_DENSE_MEAN = 401,
  ODEF_W_DENSE_COV_WITHIN = 402,
  ODEF_W_DENSE_COV_BETWEEN = 403,
  ODEF_W_DENSE_LOG_EVIDENCE = 404,
  ODEF_W_DENSE_ESS = 405,
  ODEF_W_LOGWEIGHT = 408 /* odef_bind_device only */
} odef_wsummary_field;

/* POD mirror of the reference's keyword structs (src/algorithms.jl:23-28,46-51) plus the
 * ensemble shape.  Zero-initialise, set struct_size = sizeof(odef_config). */
typedef struct {
  int32_t struct_size;
  int32_t alg;           /* odef_alg */
  int32_t order;         /* q, 1..ODEF_MAX_ORDER */
  int32_t diffusion;     /* odef_diffusion */
  int32_t smooth;        /* keep what odef_smooth needs (forces ODEF_SAVE_EVERYSTEP) */
  int32_t rhs_id;        /* odef_rhs */
  int32_t d;             /* must equal the registry's dimension for rhs_id */
  int32_t n_params;      /* must equal the registry's parameter count */
  int32_t params_shared; /* 1: one parameter vector for all trajectories; 0: p[N][n_params] */
  int32_t save_mode;     /* odef_save_mode */
  int32_t device;        /* HIP device ordinal, -1 = current device */
  int32_t want_loglik;   /* accumulate sol.log_likelihood (src/perform_step.jl:66) */
  int64_t n_traj;        /* N */
} odef_config;

/* OrdinaryDiffEq PI step-size controller (third-party defaults; exponents from
 * src/alg_utils.jl:23-24).  Pass NULL to odef_solve_adaptive for these defaults. */
typedef struct {
  double beta1, beta2, gamma, qmin, qmax, qsteady_min, qsteady_max, qoldinit, dtmin, dtmax;
} odef_controller;

#define ODEF_MAX_ORDER 5

int odef_version(void);
const char* odef_last_error(const odef_ctx* ctx); /* ctx may be NULL: last error of odef_create */

/* Run-time compiled vector field.  The reference calls the user's Julia closure f (and f.jac or ForwardDiff) in the
 * middle of every step (src/perform_step.jl:106,116-121); a device kernel cannot call back into the host, so the
 * vector field is handed over as HIP C++ SOURCE: the definition of a struct `name` with the interface of the
 * compiled-in registry (odefilters.jl_amd/csrc/rhs.h), placed inside namespace odef:
 *
 *     struct MyField {
 *       static constexpr int d = 3, np = 3;
 *       template <class T>   // T = double in the step, a truncated Taylor jet in the initialisation
 *       __device__ static void f(const T (&u)[3], const double* p, T (&du)[3]) { ... }
 *       __device__ static void jac(const double (&u)[3], const double* p, double (&J)[3][3]) { ... }  // optional:
 *           // without it EK1 differentiates f in forward mode (the reference's ForwardDiff fallback, :119-121)
 *       template <class T>   // optional: the closed-form solution at the absolute time t (f.analytic); with it the
 *       __device__ static void analytic(const T (&u0)[3], const double* p, T t, T (&out)[3]) { ... }  // odef_errors_field ids work
 *     };
 *
 * A TIME-DEPENDENT field f(u, p, t) (the reference evaluates f and f.jac at the step's new time, src/perform_step.jl:106,117)
 * opts in with `static constexpr bool has_time = true;` and takes the absolute time behind p, in the scalar type of u:
 *
 *       template <class T> __device__ static void f(const T (&u)[3], const double* p, T t, T (&du)[3]) { ... }
 *       __device__ static void jac(const double (&u)[3], const double* p, double t, double (&J)[3][3]) { ... }  // optional
 *       template <class T> __device__ static void analytic(const T (&u0)[3], const double* p, T t0, T t, T (&out)[3]) { ... }
 *           // optional; (any field's analytic may take the initial time t0 in front of t like this)
 *
 * The step evaluates f and the Jacobian at its new time (fixed grids: the grid point; adaptive: t + dt of the attempt), and the
 * Taylor initialisation differentiates in t as well (u'' = f_u f + f_t, ...).  Such a field runs on the lane and row-team kernels
 * (d(q+1) <= 20, d <= 10); odef_create refuses it above, where the workgroup-per-trajectory kernels would be needed.  Setting
 * has_time with the three-argument f is a compile error.
 *
 * A hipcc child process ($ODEFILTER_HIP_HIPCC, else hipcc on PATH, else /opt/rocm/bin/hipcc) compiles the library's
 * own kernels around it for gfx950 (include_dir = directory holding the csrc headers; NULL: $ODEFILTER_HIP_INCLUDE, else
 * ../csrc next to the loaded library, else the build-time location):
 *   d(q+1) <= 20, d <= 10   one lane per trajectory, and for d(q+1) <= 16 also the 16-lanes-per-trajectory kernels that small
 *                           and sharded ensembles use, chosen by ensemble size exactly as for the compiled-in fields
 *                           (dense output and sampling: d(q+1) <= 12 on lanes, <= 32 on row teams);
 *   above, even d <= 32,    the workgroup-per-trajectory kernels on the matrix cores (filter on fixed grids and adaptive,
 *   d(q+1) <= 176           smoother, dense output, sampling) -- built at odef_create for that order and algorithm as a host +
 *                           device shared object that links against this library (tens of seconds to minutes).
 * Returns 0 and a new rhs id (>= 100) for odef_config.rhs_id; on a compile error returns -1 and odef_last_error(NULL) holds
 * the compiler log (d <= 10: the order-1 lane filter is built at once; above: a probe kernel that evaluates f in double, in
 * forward mode and on Taylor jets).  An odd d above state dimension 20 has no kernel: odef_create says so.  Whatever the
 * compiler rejects comes back as an error with its log. */
int odef_rhs_compile(const char* name, const char* source, int32_t d, int32_t n_params, const char* include_dir,
                     int32_t* rhs_id);

int odef_create(odef_ctx** out, const odef_config* cfg);
void odef_destroy(odef_ctx* ctx);
/* Launch on a caller-owned hipStream_t (e.g. torch's current stream); NULL = the ctx's own. */
int odef_set_stream(odef_ctx* ctx, void* hip_stream);

/* Initial values.  Host layouts are trajectory-major: u0[N][d], p[N][n_params] (or
 * p[n_params] when params_shared) -- i.e. Julia's d x N column-major matrices. */
int odef_set_problem(odef_ctx* ctx, const double* u0, const double* p, double t0);
/* Same from device memory already in the device layout u0[d][N], p[n_params][N]. */
int odef_set_problem_device(odef_ctx* ctx, const double* d_u0, const double* d_p, double t0);
/* Synthetic ensemble generated on the device (the EnsembleProblem prob_func of SURVEY 8d):
 * u0_i[k] = base_u0[k] + scale*(2U-1) for k < n_perturbed, U = (splitmix64(seed +
 * n_perturbed*(first_index+i) + k) >> 11) * 2^-53.  p = shared parameter vector. */
int odef_set_problem_perturbed(odef_ctx* ctx, const double* base_u0, const double* p, double t0,
                               double scale, uint64_t seed, int64_t first_index, int32_t n_perturbed);

/* Fixed-step filter over the host time grid tgrid[0..n_t-1] (n_t-1 steps for every trajectory). */
int odef_solve_fixed(odef_ctx* ctx, const double* tgrid, int64_t n_t);
/* Adaptive filter from t0 to t1.  ONE RECORD PER ATTEMPTED STEP (at most max_steps per trajectory, NSAVED = attempts
 * + 1): an accepted step stores the new state at the new time, a rejected attempt stores the unchanged state again at
 * the unchanged time.  All lanes of a wavefront then write record k in the same instructions (full 512-byte rows);
 * odef_smooth / odef_dense_output / odef_sample treat the repeated record as the reference treats a duplicated save
 * time (src/smoothing.jl:13-16).  A binding that wants the reference's sol.t / sol.u (accepted steps only,
 * src/integrator_utils.jl:33-48) drops records whose T equals the previous T (host.py EnsembleSolution._order). */
int odef_solve_adaptive(odef_ctx* ctx, double t1, double abstol, double reltol, double dt0,
                        const odef_controller* ctrl, int64_t max_steps);
/* Rauch-Tung-Striebel pass over the stored filter states. */
int odef_smooth(odef_ctx* ctx);

/* Dense output / saveat (src/solution.jl:165-210): posterior of every trajectory at the n_q host times tq
 * (smoothed != 0: the smoothed posterior, needs odef_smooth first).  Results in ODEF_F_DENSE_MEAN /
 * ODEF_F_DENSE_COV_TRIL.  Times before t0 give NaN records (the reference throws).  Any state dimension the solver accepts:
 * <= 12 one lane per (trajectory, time), <= 32 one team of 16 / 32 lanes, the workgroup-per-trajectory path (168) on the MFMA smoother's algebra. */
int odef_dense_output(odef_ctx* ctx, const double* tq, int64_t n_q, int smoothed);

/* Posterior sampling on the saved grid (src/solution_sampling.jl:24-62): n_samples joint draws of the whole state
 * path per trajectory, x_N ~ N(mu_N, S_N) and backwards x_i ~ smooth(x_filt[i], delta(x_{i+1})).  Needs
 * ODEF_SAVE_EVERYSTEP (the reference asserts a smoothing solve, :16); odef_smooth itself is not required.
 * The N(0,1) stream is counter-based and reproducible from `seed` (splitmix64 + Box-Muller, see
 * oracle/odefilter_oracle.py sample_normal); noise_scale = 1 gives samples, 0 the chain of conditional means.
 * Result in ODEF_F_SAMPLES; sample(sol, n) of the reference is its rows 0..d-1.  Any state dimension the solver accepts
 * (<= 12 one lane per (trajectory, sample), <= 32 one team of 16 / 32 lanes, the workgroup-per-trajectory path on the MFMA algebra). */
int odef_sample(odef_ctx* ctx, int64_t n_samples, uint64_t seed, double noise_scale);

/* Posterior sampling on a dense grid (dense_sample_states / dense_sample, src/solution_sampling.jl:63-75): the FILTER
 * posterior is interpolated at the n_q host times tq (as odef_dense_output with smoothed = 0; the reference uses
 * range(t0, t_end, length = 1000)) and the backward sampler of odef_sample runs over those states, the diffusion
 * of an interval looked up by time (:41).  Overwrites ODEF_F_DENSE_MEAN / ODEF_F_DENSE_COV_TRIL; result in
 * ODEF_F_SAMPLES as [n_q][D][n_samples][N].  tq must be non-decreasing and >= t0.  Any state dimension the solver accepts. */
int odef_dense_sample(odef_ctx* ctx, const double* tq, int64_t n_q, int64_t n_samples, uint64_t seed, double noise_scale);

int64_t odef_n_save(const odef_ctx* ctx); /* leading dimension of MEAN/COV_TRIL/DIFFUSION/T */
int odef_field_bytes(const odef_ctx* ctx, int field, size_t* bytes);
int odef_get(odef_ctx* ctx, int field, void* host_dst, size_t bytes);
int odef_get_device(odef_ctx* ctx, int field, void** dev_ptr, size_t* bytes);
/* Use a caller-owned device buffer for an output field (before odef_solve_*). */
int odef_bind_device(odef_ctx* ctx, int field, void* dev_ptr, size_t bytes);
int odef_synchronize(odef_ctx* ctx);

/* Device time of the last filter (which=0) / smoother (which=1) / ensemble-summary (which=2) / solution-error (which=3) /
 * data-likelihood (which=4) / event-location (which=5) / ensemble-quantile (which=6) / weighted-summary (which=7) launch, measured with
 * hipEvents on the launch stream; n_launches = kernels launched by that call. */
int odef_kernel_time_ms(odef_ctx* ctx, int which, float* ms, int* n_launches);
/* Name of the kernel that call launched (the dominant one of a multi-kernel pass), as a profiler prints it, e.g.
 * "odef::ek_filter_fixed_kernel<odef::RhsLorenz63, 3, true, true, false>": which kernel serves a configuration depends on
 * the state dimension and the ensemble size (crossovers in csrc/ek_kernels.h), and a benchmark line should name the kernel
 * that ran, not re-derive those thresholds.  NUL-terminated into buf (truncated to n); "" before the first launch. */
int odef_kernel_name(odef_ctx* ctx, int which, char* buf, size_t n);

/* ---- ensemble sharded over the GPUs of one node, single host process -------------------------------
 * Trajectories are independent, so the ensemble is cut into contiguous blocks, one per device; nothing is exchanged
 * while stepping; odef_allgather is the ONE collective (ncclAllGather over xGMI, librccl bound with dlopen at the first
 * call; `ncclCommInitAll`, no MPI, no second process).  A Julia host drives 8 GPUs through these calls alone. */
typedef struct odef_group odef_group;
/* block [first, first + count) of shard `shard` out of n_shards: the first n_traj % n_shards shards are one longer */
int odef_shard_range(int64_t n_traj, int32_t n_shards, int32_t shard, int64_t* first, int64_t* count);
/* Layout of the gathered block (host arithmetic, no device needed): every device ends odef_allgather with
 * [n_devices][state_dim][cnt_max] doubles -- shard k's final means in block k, its `count[k]` columns first, the columns
 * up to cnt_max = the longest shard's count zero-padded (RCCL's all-gather wants equal blocks).  first / count: arrays of
 * n_devices entries (either may be NULL); block_doubles = state_dim * cnt_max.  What a caller that consumes the block on
 * the device (odef_group_get_gathered's dev_ptr) needs to address it. */
int odef_group_layout(int64_t n_traj, int32_t n_devices, int32_t state_dim, int64_t* first, int64_t* count, int64_t* cnt_max,
                      int64_t* block_doubles);
/* ... and the same block with the padding dropped: gathered [n_devices][state_dim][cnt_max] (host memory) ->
 * dst [state_dim][n_traj], trajectory index fastest as everywhere.  odef_group_get_gathered's host path is this function. */
int odef_unpad_gathered(const double* gathered, int32_t n_devices, int32_t state_dim, int64_t n_traj, double* dst);
/* cfg->n_traj is the size of the WHOLE ensemble; cfg->device is ignored; device_ids == NULL: devices 0..n_devices-1 */
int odef_group_create(odef_group** out, const odef_config* cfg, int32_t n_devices, const int32_t* device_ids);
void odef_group_destroy(odef_group* g);
const char* odef_group_last_error(const odef_group* g); /* g may be NULL: last error of odef_group_create */
int32_t odef_group_size(const odef_group* g);
odef_ctx* odef_group_ctx(odef_group* g, int32_t shard);  /* the shard's context (owned by the group): odef_get etc. */
int odef_group_shard(const odef_group* g, int32_t shard, int64_t* first, int64_t* count);
/* u0[N][d], p[N][n_params] (or shared p) of the whole ensemble in host memory; each shard takes its block */
int odef_group_set_problem(odef_group* g, const double* u0, const double* p, double t0);
/* odef_set_problem_perturbed with GLOBAL trajectory numbering: the ensemble does not depend on the number of devices */
int odef_group_set_problem_perturbed(odef_group* g, const double* base_u0, const double* p, double t0, double scale,
                                     uint64_t seed, int32_t n_perturbed);
/* the shards' kernels are launched one after the other and run concurrently; the call returns when all are done */
int odef_group_solve_fixed(odef_group* g, const double* tgrid, int64_t n_t);
int odef_group_solve_adaptive(odef_group* g, double t1, double abstol, double reltol, double dt0,
                              const odef_controller* ctrl, int64_t max_steps);
int odef_group_smooth(odef_group* g);
/* All-gather of the FINAL posterior mean of every trajectory (smoothed == 0: filter, record NSAVED-1; != 0: smoothed):
 * afterwards every device holds [n_shards][D][count_max] doubles (blocks of the shorter shards zero-padded). */
int odef_allgather(odef_group* g, int smoothed);
/* the gathered result as device `shard` holds it: host_dst (may be NULL) receives [D][n_traj] with the padding
 * removed; dev_ptr / dev_bytes (may be NULL) the raw device block */
int odef_group_get_gathered(odef_group* g, int32_t shard, double* host_dst, void** dev_ptr, size_t* dev_bytes);

/* Constants (host side, for tests and host mirrors). A, Q_L: D x D row-major. */
int odef_ibm(int d, int q, double* A, double* Q_L);
int odef_preconditioner(int d, int q, double h, double* P_diag);

/* Step-level entry points on batched Gaussians held in HOST memory (copied to the device,
 * computed by HIP kernels, copied back).  n instances; mu[n][D]; L[n][D][D] row-major
 * square-root factors (Sigma = L L'); A, Q_L: D x D row-major shared by the batch.
 * D <= ODEF_MAX_STEP_DIM. */
#define ODEF_MAX_STEP_DIM 32
int odef_predict(int D, int64_t n, const double* mu, const double* L, const double* A, const double* Q_L,
                 double* mu_out, double* cov_out /* [n][D][D] full symmetric */);
/* measurement Z = N(z, S) with S = H Sigma_pred H' (R = 0, asserted by the reference at src/filtering.jl:81) */
int odef_update(int D, int o, int64_t n, const double* mu_pred, const double* L_pred, const double* H /* [n][o][D] */,
                const double* z /* [n][o] */, double* mu_out, double* cov_out /* [n][D][D] */);
int odef_smooth_step(int D, int64_t n, const double* mu, const double* L, const double* mu_s, const double* L_s,
                     const double* A, const double* Q_L, double* mu_out, double* cov_out);

#ifdef __cplusplus
}
#endif
#endif /* ODEFILTER_H */
