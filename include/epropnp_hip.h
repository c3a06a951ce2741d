/*
 * epropnp_hip.h -- C ABI of libepropnp_hip.so, the MI355X (gfx950) implementation of the EPro-PnP hot path.
 *
 * The reference (tjiiv-cprg/EPro-PnP) has no FFI layer: its boundary is the Python class API of `epropnp/`.
 * Each entry point below replaces a span of that Python code (cited per function, paths relative to the
 * reference checkout); the Python classes in epro-pnp_amd/epropnp/ keep the reference's names/signatures and
 * call these through ctypes (see INTEGRATION.md for the binding a reference maintainer would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 (HBM), owned by the caller; outputs are caller-allocated;
 *   - `stream` is a hipStream_t (passed as void*); the call enqueues work on it and returns without synchronising;
 *   - return value: 0 on success, negative EPROPNP_E* code on error; epropnp_last_error() gives the message
 *     (thread-local).  Nothing is ever computed on the host: without a HIP device the calls fail.
 *   - dof is 6 (pose = [x,y,z, w,i,j,k], unit quaternion) or 4 (pose = [x,y,z, yaw], rotation about Y).
 *   - B objects, N points per object; x3d (B,N,3), x2d (B,N,2), w2d (B,N,2).
 */
#ifndef EPROPNP_HIP_H
#define EPROPNP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EPROPNP_OK 0
#define EPROPNP_EINVAL (-1)   /* bad argument (null pointer, unsupported dof, size limit)        */
#define EPROPNP_ELAUNCH (-2)  /* HIP launch/runtime error                                         */
#define EPROPNP_ENODEV (-3)   /* no HIP device / not a gfx950 code object                         */

#define EPROPNP_ABI_VERSION 7

/* Correspondences + camera + robust-cost parameters of one batch of objects.
 * Mirrors the state of PerspectiveCamera (epropnp/camera.py:35-62) and HuberPnPCost.delta
 * (epropnp/cost_fun.py:25-31,123-126) after the callers' set_param(). */
typedef struct epropnp_problem {
  const float* x3d;      /* (B,N,3) */
  const float* x2d;      /* (B,N,2) */
  const float* w2d;      /* (B,N,2) */
  const float* cam_mats; /* (B,3,3) row-major */
  const float* lb;       /* (B,2) lower bound [x,y] of the projection clamp, or NULL (camera.py:81-93)  */
  const float* ub;       /* (B,2) upper bound, or NULL; the clamp is applied only if both are non-NULL  */
  const float* delta;    /* (B,) Huber threshold per object                                             */
  float z_min;           /* camera.py:16,28                                                             */
  int32_t num_obj;       /* B */
  int32_t num_pts;       /* N */
  int32_t dof;           /* 6 or 4 */
  float huber_eps;       /* HuberPnPCost.eps (cost_fun.py:18-22,29): floor of |r| in the robust rescaling
                            sqrt(min(delta / max(|r|, eps), 1)); <= 0 selects the reference default 1e-10            */
  int32_t* status;       /* optional DEVICE int32[2] (or NULL): kernels OR EPROPNP_ST_* flags into status[0] and
                            atomicMin the first offending object index into status[1] (initialise to {0, INT32_MAX}).
                            Lets a caller reproduce, after a synchronisation of its choosing, the RuntimeError that
                            torch.linalg.solve / torch.inverse raise in the reference (levenberg_marquardt.py:15-19,
                            :178-181) instead of receiving NaN poses silently.  NULL selects the library's default
                            status word (epropnp_async_status below).                                                 */
  const float* delta_stats;  /* optional: the (B,4) `stats` of the epropnp_adaptive_delta call that produced `delta` from THIS
                            w2d (AdaptiveHuberPnPCost.set_param, cost_fun.py:123-126), else NULL.  Then d delta[b] / d w2d[b,n,c]
                            is the same number for every n, c -- stats[b][1] * delta_relative / (2 N) -- and the entry points
                            that return grad_w2d together with grad_delta (epropnp_amis_backward[_split], epropnp_gn_step_backward,
                            epropnp_pose_opt_plus_backward) add grad_delta[b] times it to every element of grad_w2d[b] themselves
                            (the backward kernel's epilogue, or one follow-up launch) instead of leaving three elementwise
                            launches and a (B,N,2) add to the caller's autograd; the caller must then NOT propagate grad_delta to
                            w2d again.  Forward entry points ignore it.                                                    */
  float delta_relative;      /* the relative_delta of that call (used only with delta_stats)                              */
} epropnp_problem;

/* status[0] flags */
#define EPROPNP_ST_LM_NOT_SPD 1        /* a damped normal-equation system had no Cholesky factor (singular / NaN input) */
#define EPROPNP_ST_NONFINITE_POSE 2    /* lm_solve / rslm_solve / gn_step produced a non-finite pose                    */
#define EPROPNP_ST_CHOL_FALLBACK 4     /* a proposal covariance was replaced by its default (cholesky_wrapper,
                                          epropnp.py:16-33: what the reference does silently as well)                  */
#define EPROPNP_ST_NONFINITE_WEIGHT 8  /* an AMIS log-weight is NaN / +inf                                              */
#define EPROPNP_ST_SPLIT_TIMEOUT 16    /* PERFORMANCE event, results unaffected: in a launch that splits an object over several
                                          workgroups (amis_forward at few objects, lm_solve beyond 2048 points) a part did
                                          not see a sibling's partial sums within EPROPNP_SPLIT_TIMEOUT_CYCLES (the
                                          siblings were not all resident: CU mask, partitioned GPU, a foreign kernel holding
                                          CUs) and recomputed them itself from the object's points, to the same bits     */

/* Trust-region parameters of LMSolver.__init__ (epropnp/levenberg_marquardt.py:31-53). */
typedef struct epropnp_lm_params {
  int32_t num_iter;
  int32_t fast_mode;                 /* 1: Gauss-Newton, no trust region, no clip_jac (:136-152) */
  float min_lm_diagonal;
  float max_lm_diagonal;
  float min_relative_decrease;
  float initial_trust_region_radius;
  float max_trust_region_radius;
  float eps;
} epropnp_lm_params;

/* AMIS parameters of EProPnPBase/EProPnP6DoF.__init__ (epropnp/epropnp.py:47-62,273-280). */
typedef struct epropnp_amis_params {
  int32_t mc_samples;     /* S, multiple of num_iter */
  int32_t num_iter;       /* K                        */
  float eps;              /* 1e-5                     */
  int32_t acg_mle_iter;   /* 3     (6-DoF only)       */
  float acg_dispersion;   /* 0.001 (6-DoF only)       */
  uint64_t seed;          /* Philox key when `noise` is NULL */
  uint64_t offset;        /* Philox counter offset (advance by 1 per call for fresh draws) */
  const uint64_t* offset_dev; /* optional DEVICE counter added to `offset` when the kernel runs: lets a captured hipGraph
                                 draw fresh samples on every replay (the caller increments it inside the graph) */
  void* split_scratch;        /* optional DEVICE scratch of `split_scratch_bytes` bytes (or NULL / 0).  With few objects
                                 (one workgroup per object would leave most CUs idle) epropnp_amis_forward deals an object's
                                 point tiles to several workgroups, which exchange partial costs through this buffer; it
                                 takes the split only if the buffer holds epropnp_amis_forward_split_bytes() bytes.  The
                                 library fills it on the stream before the launch; contents are undefined afterwards.     */
  uint64_t split_scratch_bytes;
  uint64_t* advance;          /* optional (NULL: none): `advance_count` consecutive DEVICE uint64 counters that the launch increments
                                 by one when its LAST workgroup retires -- every workgroup has read `offset_dev` long before.  With
                                 `offset_dev` (and epropnp_mc_params.rslm_offset_dev) among them a captured step advances its Philox
                                 counters inside the sampler's own launch: no add kernel per step (round 5; ~2.5 us of a replayed
                                 step, ~8 us of an eager one).  Needs `advance_ticket`.                                          */
  int32_t* advance_ticket;    /* DEVICE int32, zero before the first launch; the library returns it to zero                     */
  int32_t advance_count;
} epropnp_amis_params;

/* Bytes of `split_scratch` with which epropnp_amis_forward would split the objects of this problem over workgroups
 * (0: it would not -- enough objects to fill the device, too few point tiles, or a shape the split does not serve). */
uint64_t epropnp_amis_forward_split_bytes(const epropnp_problem* prob, int32_t mc_samples, int32_t num_iter);

/* Launch plans: WHICH kernel instantiation a call would launch for a problem of these sizes.  Host functions that launch nothing and
 * touch no device memory -- of `prob` only num_obj, num_pts, dof and whether lb / ub / delta_stats are non-NULL are read -- and
 * that are the very functions the launchers decide with, so they cannot drift from what is launched.  The environment
 * (EPROPNP_TUNE, EPROPNP_FWD_SPLIT, EPROPNP_*_PROJ) is read as a launch reads it.  num_cus: plan for a device of that many compute
 * units (0: the current device).  They exist for tests and tuning tools: a test of an instantiation asserts through them that
 * its shape still reaches that instantiation after the heuristics have changed.
 *   epropnp_plan_amis_forward: has_scratch = the caller hands over epropnp_amis_forward_split_bytes() of split_scratch.
 *     out[8] = {waves, point tiles resident per wave (0: the points stream through LDS), G workgroups per object, chunks the tiles
 *               go through the registers in, bf16 projection, sampler state spilled to global scratch, pose tile truncated (a tile
 *               holds less than one iteration's samples), the chunked instantiation is the one launched}
 *   epropnp_plan_amis_backward: what epropnp_amis_backward (num_split 1) / epropnp_amis_backward_split launch.
 *     out[5] = {waves, point tiles per wave and chunk, bf16 projection, grad_w2d rows parked in LDS for the delta fold,
 *               the all-VALU kernel is taken instead (then the first four are 0)}
 *   epropnp_plan_evaluate_cost: out[2] = {waves, points per lane} */
int epropnp_plan_amis_forward(const epropnp_problem* prob, int32_t mc_samples, int32_t num_iter, int32_t has_scratch,
                              int32_t num_cus, int32_t* out);
int epropnp_plan_amis_backward(const epropnp_problem* prob, int32_t mc_samples, int32_t with_pose_init, int32_t num_split,
                               int32_t num_cus, int32_t* out);
int epropnp_plan_evaluate_cost(const epropnp_problem* prob, int32_t num_cus, int32_t* out);

/* Everything EProPnPBase.monte_carlo_forward does between its arguments and its return tuple
 * (epropnp/epropnp.py:87-196): one host call that enqueues, in order,
 *   [pnp_normalize: centre x3d, shift pose_init (common.py:103-124)] -> cost of pose_init (:121-124) ->
 *   [RSLM initialiser, and per object the cheaper of {pose_init, RSLM pose} (levenberg_marquardt.py:115-130)] ->
 *   LM solve with covariance (:132-190) -> AMIS loop (:132-182) -> [pnp_denormalize of pose_opt and the samples]. */
typedef struct epropnp_mc_params {
  epropnp_lm_params lm;          /* the main solve                                                                   */
  epropnp_amis_params amis;
  int32_t normalize;             /* 1: EProPnPBase(normalize=True)                                                   */
  int32_t init_mode;             /* 0: start LM from pose_init; 1: RSLM only (pose_init NULL);
                                    2: force_init_solve=True with pose_init: per object the cheaper of the two      */
  epropnp_lm_params rslm_lm;     /* RSLMSolver's own LM parameters (sub-problems)                                   */
  int32_t rslm_points, rslm_proposals;
  uint64_t rslm_seed, rslm_offset;
  const uint64_t* rslm_offset_dev;
  const int64_t* rslm_inds;      /* injected sub-sample indices (P,B,n) or NULL                                      */
  const float* rslm_rot;         /* injected initial rotations or NULL                                               */
  void* rslm_scratch;            /* optional scratch of epropnp_rslm_solve (see there) or NULL                       */
  uint64_t rslm_scratch_bytes;
  void* lm_scratch;              /* optional split scratch of the main epropnp_lm_solve (see there) or NULL          */
  uint64_t lm_scratch_bytes;
} epropnp_mc_params;

/*   pose_init (B,pose_len) or NULL (init_mode 1); noise as in epropnp_amis_forward
 *   scratch the caller owns (it must outlive the backward): x3d_centered (B,N,3) + offset (B,3) + pose_init_n
 *     (B,pose_len) when normalize, NULL otherwise; start_pose (B,pose_len) + start_cost (B,) when init_mode != 0
 *   -> in the (normalised) solver frame: pose_opt_n (B,pose_len), pose_cov (B,dof,dof), cost (B,) or NULL,
 *      pose_samples_n (S,B,pose_len), logweights (S,B), cost_init (B,) (NULL iff pose_init NULL)
 *   -> in the caller's frame (only when normalize; otherwise pass NULL and use the _n buffers):
 *      pose_opt (B,pose_len), pose_samples (S,B,pose_len).
 * The backward is epropnp_amis_backward on the problem with x3d = x3d_centered and pose_samples_n / pose_init_n. */
int epropnp_monte_carlo_forward(const epropnp_problem* prob, const epropnp_mc_params* par, const float* pose_init,
                                const float* noise, float* x3d_centered, float* offset, float* pose_init_n,
                                float* start_pose, float* start_cost, float* pose_opt_n, float* pose_cov, float* cost,
                                float* pose_samples_n, float* logweights, float* cost_init, float* pose_opt,
                                float* pose_samples, void* stream);

/* Per-object diagnostics of the one-call forward: what a user of the reference can print between its stages -- which LM steps
 * were accepted (levenberg_marquardt.py:227-229), which random-sample proposal won (:346-347), what the fitted proposals were and
 * whether cholesky_wrapper fell back (epropnp.py:16-33), how degenerate the importance weights are.  Every member is optional
 * (NULL: not wanted); all are DEVICE pointers to caller-owned, caller-allocated memory. */
typedef struct epropnp_diag {
  int32_t* lm_accept_mask;  /* (B,)     bit i = step i of the MAIN solve accepted, as epropnp_lm_solve's accept_mask (0 in fast_mode) */
  int32_t* rslm_winner;     /* (B,)     init_mode 1 / 2: index in [0, rslm_proposals) of the proposal whose pose the main solve
                                        started from; -1 where init_mode 2 kept pose_init; not written in init_mode 0            */
  float*   proposals;       /* (B,K,40) as epropnp_amis_forward's `proposals`                                                     */
  float*   weight_stats;    /* (B,K+3)  see epropnp_weight_stats; computed from the call's own logweights                         */
} epropnp_diag;

/* epropnp_monte_carlo_forward with diagnostics.  diag == NULL or all members NULL: exactly the launches of the plain entry.  With
 * any member set every regular output keeps its bits (with and without the rslm / lm / split scratch buffers): lm_accept_mask and
 * proposals are outputs the solver and sampler launches already have, weight_stats is one more launch behind the sampler, and
 * with rslm_winner the initialiser's winner is selected by its own reduce launch (the rule of the selection folded into the LM
 * launch, which is skipped) so that the index of the pose handed on can be reported.  Not for use inside a hipGraph capture. */
int epropnp_monte_carlo_forward_diag(const epropnp_problem* prob, const epropnp_mc_params* par, const float* pose_init,
                                     const float* noise, float* x3d_centered, float* offset, float* pose_init_n,
                                     float* start_pose, float* start_cost, float* pose_opt_n, float* pose_cov, float* cost,
                                     float* pose_samples_n, float* logweights, float* cost_init, float* pose_opt,
                                     float* pose_samples, const epropnp_diag* diag, void* stream);

/* Degeneracy of the importance weights, per object.  logweights (S,B) are the samples of num_iter AMIS iterations of
 * S / num_iter consecutive rows each; with w_j = exp(logw_j - max_j logw_j):
 *   stats[b] = [ess, max_share, lse, mass_0 .. mass_{K-1}]      (B, 3 + num_iter)
 *   ess = (sum w)^2 / sum w^2 (effective sample size, in [1, S]), max_share = max w / sum w, lse = max + log sum w (the number
 *   epropnp_mc_loss_forward keeps), mass_k = share of iteration k's samples in sum w.
 * A column that is all -inf gives ess = max_share = mass_k = 0 and lse = -inf; a column holding a NaN or +inf gives a row of NaNs.
 * Fixed summation order, no atomics: two launches agree to the last bit.  1 <= num_iter <= 64, mc_samples a multiple of it. */
int epropnp_weight_stats(const float* logweights, int32_t mc_samples, int32_t num_obj, int32_t num_iter, float* stats,
                         void* stream);

/* Posterior summary of the weighted pose samples, per object, in one launch: what the consumers of monte_carlo_forward's raw
 * (pose_samples, pose_sample_logweights) otherwise re-derive with chains of elementwise and reduce launches over (S,B,.) temporaries
 * -- the Det head's test-time orientation score (EPro-PnP-Det deform_pnp_head.py:532-537: softmax(dim=0) of the log-weights, norm of
 * pose_samples[..., [0, 2]] - pose_opt[:, [0, 2]], ((-log2 + 2.5) / 4).clamp(0, 1), sum over the samples) and the moments of the
 * distribution.  With w_j = exp(logw_j - max_j logw_j) (one rounding in the exponent's argument), W = sum w_j, t the translation
 * (words 0..2 of a pose), samples of weight 0 skipped (a NaN pose under a -inf log-weight reaches no sum):
 *   summary[b] (16 floats, every word written):
 *    0..2   trans_mean = sum w t / W
 *    3..8   upper triangle (xx, xy, xz, yy, yz, zz) of trans_cov = sum w (t - mean)(t - mean)^T / W (the definition of the
 *           proposals' translation moments, epropnp.py:240-248), accumulated about the object's heaviest sample
 *    9      score_te = sum w clamp((-log2 |t_xz - ref_xz| + 2.5) / 4, 0, 1) / W (deform_pnp_head.py:532-537 with pose_ref =
 *           pose_opt; a deviation of 0 scores 1); NaN when pose_ref is NULL
 *    10     rotation concentration: 4-DoF the mean resultant length |(sum w cos yaw, sum w sin yaw)| / W; 6-DoF the largest
 *           eigenvalue of M = sum w q q^T / W, in [1/4, 1]
 *    11..14 4-DoF: the circular mean atan2(sum w sin yaw, sum w cos yaw) (epropnp.py:251-257), then three zeros; 6-DoF: the unit
 *           eigenvector of M for that eigenvalue (the antipodally symmetric mean: q and -q count alike, as for the angular
 *           central Gaussian proposals of EProPnP6DoF), signed so that its dot with pose_ref's quaternion is >= 0, without pose_ref so that its first
 *           non-zero component is positive
 *    15     reserved, 0
 * pose_samples (S,B,P), P = 4 (dof 4) | 7 (dof 6); logweights (S,B); pose_ref (B,P) or NULL.  A column that holds a NaN or +inf
 * log-weight, or nothing but -inf, gives a row of NaNs.  The eigenvector comes from a fixed number of cyclic Jacobi sweeps; fixed
 * summation order, no atomics: two launches agree to the last bit.  Any mc_samples >= 1.  Capturable into a hipGraph. */
#define EPROPNP_POSTERIOR_WORDS 16
int epropnp_posterior_summary(const float* pose_samples, const float* logweights, const float* pose_ref, int32_t mc_samples,
                              int32_t num_obj, int32_t dof, float* summary, void* stream);

/* Systematic resampling of the weighted pose samples into num_draws equally weighted draws per object, in one launch: with one
 * uniform u_b in [0, 1) per object -- u[b], or with u == NULL the Philox4x32-10 stream of (seed, offset, b) -- draw r is the first
 * sample, in sample order, whose running sum of w exceeds (u_b + r) / num_draws * W.
 *   index (R,B) int32: the sample drawn, non-decreasing in r; every entry is written exactly once; samples of weight 0 are never drawn
 *   poses (R,B,P) or NULL: pose_samples[index[r, b], b], bit for bit
 * Bad and empty columns (as above): index -1, NaN poses.  Deterministic; capturable into a hipGraph. */
int epropnp_posterior_resample(const float* pose_samples, const float* logweights, int32_t mc_samples, int32_t num_obj,
                               int32_t dof, int32_t num_draws, const float* u, uint64_t seed, uint64_t offset, int32_t* index,
                               float* poses, void* stream);

/* Posterior modes: quick-shift clustering of the weighted pose samples, per object -- where the peaks of the pose distribution are,
 * how much probability mass each holds and which samples belong to which (a symmetric object's yaw posterior has two peaks pi
 * apart; the moments of epropnp_posterior_summary describe neither).  Per object b, all in fp32:
 *   weights   w_j = exp(logw_j - max_j logw_j), W = sum w_j.  A sample with w_j == 0 takes no part (a NaN pose may sit there).
 *   distance  D_ij = |t_i - t_j|^2 / h_t^2 + rho_ij / h_r^2 with (h_t, h_r) = bandwidth[b] -- "the scale below which two poses are
 *             the same hypothesis", h_r in radians -- and rho written so that fp32 does not cancel:
 *               4-DoF  rho = 4 sin^2((yaw_i - yaw_j) / 2)
 *               6-DoF  d^2 = min(|q_i - q_j|^2, |q_i + q_j|^2), rho = d^2 (4 - d^2)      (= 4 (1 - (q_i . q_j)^2): q and -q count alike)
 *   density   f_i = sum_j w_j exp(-D_ij / 2) / W over the participating j, j = i included
 *   link      parent(i) = the participating j with (f_j > f_i or (f_j == f_i and j < i)) and D_ij <= link^2 that minimises D_ij,
 *             ties to the lowest j, the comparison on the fp32 densities as written; no such j: i is a root, a mode
 *   label     the root of i's chain; the mass of a mode is sum w_i / W over its tree; modes are ranked by mass, descending, ties to
 *             the lower root index
 * Outputs (every element of every output is written); M = max_modes:
 *   density (S,B) f_i | parent (S,B) (a root is its own parent) | labels (S,B) the root's sample index | num_modes (B,) the number
 *   of roots, which may exceed M | rows m < min(M, num_modes): mode_index (M,B) the root's sample index, mode_mass (M,B),
 *   mode_poses (M,B,P) or NULL = pose_samples[mode_index, b] bit for bit; rows beyond: index -1, mass 0, NaN poses.
 *   Samples that take no part: density NaN, parent and label -1.  A bad column -- a NaN or +inf log-weight, nothing but -inf, a
 *   bandwidth that is not finite and > 0 -- : num_modes 0, index, parent and label -1, mass, density and poses NaN.
 * density, parent and labels are the scratch of the call: three launches on `stream`, no allocation, no host synchronisation; sums
 * in a fixed order, no floating-point atomics: two launches agree to the last bit.  Any mc_samples >= 1 (columns beyond 4096 samples
 * stream through LDS in tiles).  EPROPNP_EINVAL: dof not 4 or 6, mc_samples < 1, max_modes < 1, link not finite or not > 0, a NULL
 * pointer other than mode_poses.  num_obj == 0 launches nothing.  Capturable into a hipGraph. */
int epropnp_posterior_modes(const float* pose_samples, const float* logweights, const float* bandwidth /* (B,2): h_t, h_r */,
                            int32_t mc_samples, int32_t num_obj, int32_t dof, float link, int32_t max_modes,
                            float* density /* (S,B) */, int32_t* parent /* (S,B) */, int32_t* labels /* (S,B) */,
                            int32_t* num_modes /* (B,) */, int32_t* mode_index /* (M,B) */, float* mode_mass /* (M,B) */,
                            float* mode_poses /* (M,B,P) or NULL */, void* stream);

/* Pose-error metrics of the 6-DoF evaluation, on the device: rotation and translation error, ARP-2D, ADD and ADD-S of
 * num_rows_per_obj x num_obj pose rows against num_obj ground-truth poses (EPro-PnP-6DoF lib/utils/eval.py:585-736: re, te, arp_2d,
 * add, adi, calc_all_errs, there a host loop with one scipy cKDTree per symmetric object).  Row (r, b) of pose_est (R,B,P) is scored
 * against pose_gt[b] over the points of model model_id[b] (model 0 with model_id == NULL): model_points (Mtot,3) holds the models
 * back to back, model_range[c] = (first point, number of points) of model c.  Quaternions are normalised first; a 4-DoF pose is
 * (x, y, z, yaw) about the y axis.  Per row, in fp32 (the row's set-up runs in fp64 and is rounded once):
 *    0  rot_deg     rotation angle of R_est^T R_gt in degrees, 2 atan2(|v|, |w|) of the relative quaternion (what
 *                   |logm(R_est^T R_gt)|_F / sqrt 2 is, accurate at small angles); 4-DoF: |wrap(yaw_est - yaw_gt)|
 *    1  trans       |t_est - t_gt|
 *    2  arp_2d      mean_i |proj(K (R_est p_i + t_est)) - proj(K (R_gt p_i + t_gt))| in pixels, proj a plain division by z (no
 *                   z_min clamp), K = cam_mats[b]; NaN with cam_mats == NULL
 *    3  add         mean_i |(R_est p_i + t_est) - (R_gt p_i + t_gt)|, evaluated as |(R_est - R_gt) p_i + (t_est - t_gt)|
 *    4  adi         ADD-S: mean_i min_j |(R_gt p_i + t_gt) - (R_est p_j + t_est)|, evaluated in the estimate's model frame as
 *                   min_j |q_i - p_j| with q_i = R_est^T R_gt p_i + R_est^T (t_gt - t_est); only for objects with symmetric[b] != 0,
 *                   NaN otherwise (and with symmetric == NULL)
 *    5  add_or_adi  adi where symmetric[b] != 0, else add: what calc_all_errs returns
 *    6, 7           reserved, 0
 * half_turn[b] != 0 (the reference's eggbox rule): when the raw rot_deg exceeds 90, rot_deg, trans and arp_2d are taken with
 * R_est diag(-1, -1, 1) (4-DoF: yaw + pi); add and adi keep the raw estimate.  Identical poses give exact zeros.
 * ADD-S needs scratch: epropnp_pose_errors_scratch_bytes(R, B, M) bytes serve models of up to M points (one float per row and tile
 * of EPROPNP_POSE_ERROR_QUERY_TILE points); scratch may be NULL with symmetric == NULL.  What only the device can see gives NaN in
 * words 0..5 of the row concerned and leaves every other row intact: a model_id outside [0, num_models), a model with first < 0 or
 * count < 1, a pose component that is not finite, a zero quaternion; a symmetric row whose model has more points than the scratch
 * serves gets NaN in adi and add_or_adi.  Every word of every row is written.  Two launches on `stream` (one with symmetric ==
 * NULL), no allocation, no host synchronisation, no floating-point atomics, sums in a fixed order: two launches agree to the last
 * bit, whatever EPROPNP_TUNE="nn_parts=<workgroups per row>" deals the tiles to.  EPROPNP_EINVAL: a NULL pose_est, pose_gt,
 * model_points, model_range or errors, a NULL scratch with a symmetric mask, dof not 4 or 6, num_rows_per_obj < 1, num_models < 1,
 * num_obj < 0, scratch_bytes below epropnp_pose_errors_scratch_bytes(R, B, 1).  num_obj == 0 launches nothing and follows no
 * pointer.  Capturable into a hipGraph. */
#define EPROPNP_POSE_ERROR_WORDS 8   /* rot_deg, trans, arp_2d, add, adi, add_or_adi, 0, 0 */
#define EPROPNP_POSE_ERROR_QUERY_TILE 1024   /* model points per ADD-S query tile: one scratch float per row and tile */
#define EPROPNP_POSE_ERROR_CAND_TILE 1024    /* model points per LDS tile of ADD-S candidates */
int epropnp_pose_errors(const float* pose_est /* (R,B,P), R >= 1 */, const float* pose_gt /* (B,P) */,
                        int32_t num_rows_per_obj /* R */, int32_t num_obj, int32_t dof,
                        const float* model_points /* (Mtot,3) */, const int32_t* model_range /* (C,2): first, count */,
                        int32_t num_models, const int32_t* model_id /* (B,) or NULL: model 0 */,
                        const float* cam_mats /* (B,3,3) or NULL */, const uint8_t* symmetric /* (B,) or NULL */,
                        const uint8_t* half_turn /* (B,) or NULL */, void* scratch, size_t scratch_bytes,
                        float* errors /* (R,B,8) */, void* stream);
size_t epropnp_pose_errors_scratch_bytes(int32_t num_rows_per_obj, int32_t num_obj, int32_t max_model_points);

/* Rotated bird's-eye-view boxes: overlap area / IoU and the grouped greedy non-maximum suppression the detection head ends with
 * (EPro-PnP-Det core/bbox_3d/misc.py:300-324 batched_bev_nms and nuscenes3d_dataset.py:395 nms_gpu, there through the CUDA extension
 * ops/iou3d, whose suppression mask is copied to the host and reduced in a C++ loop).
 * A box is five floats (cx, cy, dx, dy, angle); its corners are (cx + u cos a + v sin a, cy - u sin a + v cos a) for u = +-dx/2,
 * v = +-dy/2 -- the yaw convention of the 4-DoF pose with (x, z) as the plane, and the reference's rotate_around_center applied to
 * its (x1, y1, x2, y2, ry) boxes.  A box is valid iff all five numbers are finite and dx >= 0, dy >= 0.
 * One fp32 overlap routine serves every entry: A's corners in B's frame (relative to B's centre, half axes turned by
 * angle_A - angle_B), then | sum over A's edges of the integral of clamp(y, -dy_B/2, dy_B/2) dx over the edge's part inside
 * |x| <= dx_B/2 |, each edge by the trapezoid rule on its three linear pieces.  No collected intersection points, no margins: the
 * result is continuous in the ten inputs.  The angle difference is reduced by the single constant fl(pi/2): identical boxes, a box
 * against itself turned by k fl(pi/2), boxes sharing an edge or a corner, a zero-width box and distant boxes give exactly the area /
 * exactly 0.  iou = overlap / max(area_a + area_b - overlap, 1e-8).
 *
 * epropnp_bev_overlap: out (num_a, num_b), or (num_a,) with aligned != 0 (which needs num_a == num_b: out[i] of boxes_a[i] and
 * boxes_b[i], the bits of the pairwise call's diagonal), holds the overlap area (want_iou == 0) or the IoU.  NaN exactly where either
 * box is invalid; every element is written.  One launch of 64 x 64 tiles (EPROPNP_BEV_TILE), both tiles' boxes staged in LDS in
 * prepared form.  num_a == 0 or num_b == 0 launches nothing and follows no pointer.  EPROPNP_EINVAL: a negative count, aligned with
 * num_a != num_b, a NULL pointer, num_a beyond 65535 tiles.
 *
 * epropnp_bev_nms: greedy suppression in the caller's visiting order.  order (N,) holds box indices, by descending score for the
 * usual use; an entry outside [0, N) is a position without a box: it is skipped and nothing is read out of bounds.  Walking `order`,
 * a valid box that is not yet suppressed is kept, and then suppresses every LATER box of the same group (group[i], all one group
 * with group == NULL) whose IoU with it is > iou_thr -- strictly, as in the reference.  Boxes of different groups never interact (no
 * coordinate is shifted to keep them apart); an invalid box is not kept and suppresses nothing.  Outputs, every element written:
 * keep_index (N,) the kept indices in visiting order, then -1; keep_mask (N,) 1 / 0 by box index; num_keep (1,).
 * Two launches on `stream`, no cross-workgroup waiting, no atomics, no host synchronisation: (1) one wave per 64 x 64 tile of the
 * visiting order, column tile >= row tile, writes one 64-bit word per row and tile into scratch -- pairs of different groups and
 * pairs whose centres are further apart than the sum of the half diagonals are rejected before the overlap arithmetic; (2) one
 * workgroup walks the row tiles with the `removed` bitset in LDS.  Two calls agree to the last bit.  scratch: at least
 * epropnp_bev_nms_scratch_bytes(N) = N * ceil(N / 64) * 8 bytes (the mask; the reduce launch needs nothing beyond it).
 * num_boxes == 0 launches the reduce kernel alone, which writes num_keep[0] = 0 (boxes, order, scratch, keep_index and keep_mask are
 * not followed).  EPROPNP_EINVAL: num_boxes < 0 or above 262144, scratch_bytes below the size query, a NULL num_keep, a NULL boxes /
 * order / scratch / keep_index / keep_mask with num_boxes > 0.  Capturable into a hipGraph. */
#define EPROPNP_BEV_TILE 64   /* boxes per tile edge: one mask word per row and column tile */
int epropnp_bev_overlap(const float* boxes_a /* (num_a,5) */, int32_t num_a, const float* boxes_b /* (num_b,5) */, int32_t num_b,
                        int32_t want_iou, int32_t aligned, float* out /* (num_a,num_b) or (num_a,) */, void* stream);
size_t epropnp_bev_nms_scratch_bytes(int32_t num_boxes);
int epropnp_bev_nms(const float* boxes /* (N,5) */, const int32_t* order /* (N,) */, const int32_t* group /* (N,) or NULL */,
                    int32_t num_boxes, float iou_thr, void* scratch, size_t scratch_bytes, int32_t* keep_index /* (N,) */,
                    uint8_t* keep_mask /* (N,) */, int32_t* num_keep /* (1,) */, void* stream);

/* Box overlaps under the reference's criteria: rotated, 3D and axis-aligned image boxes, pairwise, aligned or per segment -- what
 * EPro-PnP-Det's numba-CUDA files compute (core/bbox_3d/iou_calculators/rotate_iou_kernel.py + bbox3d_iou_calculator.py for the
 * score targets of score_type='iou', core/evaluation/kitti_utils/rotate_iou.py + eval.py: image_box_overlap, d3_box_overlap for
 * calculate_iou_partly).  One pair function around the overlap routine above:
 *   kind EPROPNP_BOX_BEV   five floats (cx, cy, dx, dy, angle): inter = the overlap area, size = dx * dy.
 *   kind EPROPNP_BOX_3D    seven floats [x0, x1, x2, d0, d1, d2, ry]; the BEV box is the two centres and the two sizes that are not
 *        z_axis's, in that order, and ry ([0, 2, 3, 5, 6] for z_axis = 1: the reference's bev_axes).  With z = x[z_axis], h = d[z_axis]:
 *        lo = z - h * z_center, hi = z + h * (1 - z_center);  height rule EPROPNP_BOX_HEIGHT_INTERVAL: iw = max(min(hi_a, hi_b) -
 *        max(lo_a, lo_b), 0);  EPROPNP_BOX_HEIGHT_REFERENCE_TORCH: iw = max(min(hi_a, hi_b) - min(lo_a, lo_b), 0), which is what the
 *        reference's bev_to_box3d_overlaps_aligned_torch computes (bbox3d_iou_calculator.py:151 takes torch.min where the numpy twin at
 *        :90 takes np.maximum) and what its training targets are built with.  inter = area * iw, size = (dx * dy) * h.
 *   kind EPROPNP_BOX_IMAGE four floats (x1, y1, x2, y2): iw = min(x2) - max(x1), ih likewise, inter = iw * ih if both are > 0, else 0;
 *        size = (x2 - x1) * (y2 - y1).
 *   criterion EPROPNP_BOX_CRIT_IOU: inter / max(size_a + size_b - inter, 1e-8);  _A: inter / max(size_a, 1e-8);  _B: inter /
 *        max(size_b, 1e-8), each through min(., 1);  _INTER: the raw area or volume.  The numbers are the reference's (-1, 0, 1, 2).
 *        The 1e-8 floor is that of the IoU above; the reference's aligned functions floor at 1e-6 and its pairwise ones not at all: the
 *        results differ only for boxes of zero size.
 * A box is valid iff all its numbers are finite and its sizes are >= 0 (image: x2 >= x1 and y2 >= y1); the result is NaN exactly
 * where either box is invalid.  Every output element is written.  Products are uncontracted: the three pairings give the same bits
 * for the same pair, and kind BEV with _INTER gives the bits of epropnp_bev_overlap.  z_axis, z_center and height_rule are read for
 * kind 3D only (and validated always).  No atomics, no allocation, no synchronisation; capturable into a hipGraph.
 *
 * epropnp_box_overlap: out (num_a, num_b) in 64 x 64 tiles, or with aligned != 0 (num_a == num_b) out (num_a,), the bits of the
 * pairwise diagonal.  num_a == 0 or num_b == 0 launches nothing and follows no pointer.  EPROPNP_EINVAL: a negative count, aligned
 * with num_a != num_b, an unknown kind / criterion / height rule, z_axis outside 0 .. 2 for kind 3D, a z_center that is not finite, a
 * NULL pointer, num_a beyond 65535 tiles.
 *
 * epropnp_box_overlap_plan: a host function, no device work.  Segment g pairs the next counts_a[g] boxes of boxes_a with the next
 * counts_b[g] boxes of boxes_b; its (counts_a[g], counts_b[g]) block lies row-major in one flat output, block after block.  The table
 * has EPROPNP_BOX_TILE_INTS = 6 int32 per 64 x 64 tile: first row (index into boxes_a), rows in the tile (1 .. 64), first column
 * (index into boxes_b), columns in the tile (1 .. 64), output index of the tile's first element, row stride (= counts_b[g]).  A
 * segment with an empty side has no tiles.  With tiles == NULL only *num_tiles and *num_out are written (either may be NULL): the
 * size query.  EPROPNP_EINVAL: num_segments < 0, NULL counts, a negative count, 2^31 or more boxes on a side or output elements, a
 * table given with tiles_capacity (in tiles) below the tiles needed.
 *
 * epropnp_box_overlap_segmented: one launch, one workgroup per table entry; `tiles` (num_tiles, 6) is DEVICE memory, out has num_out
 * elements.  An entry that points outside [0, num_a) x [0, num_b) or outside out is skipped: nothing is read or written out of
 * bounds.  num_tiles == 0 (or no boxes, or num_out == 0) launches nothing and follows no pointer.  EPROPNP_EINVAL: a negative count,
 * num_out outside 0 .. 2^31 - 1, an unknown kind / criterion / height rule, z_axis, z_center as above, a NULL pointer. */
#define EPROPNP_BOX_BEV 0
#define EPROPNP_BOX_3D 1
#define EPROPNP_BOX_IMAGE 2
#define EPROPNP_BOX_CRIT_IOU (-1)
#define EPROPNP_BOX_CRIT_A 0
#define EPROPNP_BOX_CRIT_B 1
#define EPROPNP_BOX_CRIT_INTER 2
#define EPROPNP_BOX_HEIGHT_INTERVAL 0
#define EPROPNP_BOX_HEIGHT_REFERENCE_TORCH 1
#define EPROPNP_BOX_TILE_INTS 6
int epropnp_box_overlap(const float* boxes_a /* (num_a,5|7|4) */, int32_t num_a, const float* boxes_b /* (num_b,5|7|4) */,
                        int32_t num_b, int32_t kind, int32_t criterion, int32_t z_axis, float z_center, int32_t height_rule,
                        int32_t aligned, float* out /* (num_a,num_b) or (num_a,) */, void* stream);
int epropnp_box_overlap_plan(const int32_t* counts_a /* (G,) host */, const int32_t* counts_b /* (G,) host */, int32_t num_segments,
                             int32_t* tiles /* (tiles_capacity,6) host, or NULL */, int64_t tiles_capacity, int64_t* num_tiles,
                             int64_t* num_out);
int epropnp_box_overlap_segmented(const float* boxes_a, int32_t num_a, const float* boxes_b, int32_t num_b, int32_t kind,
                                  int32_t criterion, int32_t z_axis, float z_center, int32_t height_rule,
                                  const int32_t* tiles /* (num_tiles,6) device */, int32_t num_tiles, float* out /* (num_out,) */,
                                  int64_t num_out, void* stream);

/* KITTI AP evaluation behind the per-image overlap blocks: greedy matching, recall thresholds and PR sums of the reference's
 * core/evaluation/kitti_utils/eval.py for C "cases" (class x difficulty x minimum overlap) in one launch per stage.
 * Layout, all DEVICE memory.  The I images are concatenated: gt_offsets, dt_offsets, dc_offsets (I+1,) int32 into the G ground
 * truths, D detections and Q DontCare boxes, block_offsets (I+1,) int64 into the flat overlaps, whose block i is the row-major
 * (detections of i, ground truths of i) matrix -- what epropnp_box_overlap_segmented writes with the detections as side A.  overlaps
 * is float, or double with overlaps_fp64 != 0; every comparison is made in fp64 on the values as given.  gt_data (G,5): bbox x1 y1
 * x2 y2, alpha.  dt_data (D,6): bbox, alpha, score.  dc_boxes (Q,4).  Per case: ignored_gt (C,G) and ignored_det (C,D) int8 in
 * {-1, 0, 1} (clean_data's flags), min_overlap (C,) double, num_valid_gt (C,) int32.
 * The offsets are memory: an image whose ranges leave [0,G], [0,D], [0,Q] or whose block leaves the overlaps is skipped -- nothing is
 * read or written out of bounds, and such an image's slots of tp_scores / gt_state are the only output elements not written.
 * Integer sums go through integer atomics; the fp64 similarity is added in a fixed order (chunks of consecutive images in image order, then
 * the chunk sums in chunk order): a second call returns the same bits.  No allocation, no synchronisation.
 *
 * epropnp_kitti_match (compute_statistics_jit with compute_fp=False, eval.py:166-284, for every case and image): each ground truth
 * that is not of another class takes, among the detections that are not of another class, not yet taken and overlap it by more than
 * min_overlap, the one with the largest score > -1e7 (lowest index on a tie).  tp_scores (C,G) double: that score where the match is a
 * true positive (neither side has ignore flag 1), -inf elsewhere.  tp_count (C,) int32: the true positives of each case.  gt_state
 * (C,G) int8 or NULL: EPROPNP_KITTI_GT_* per ground truth.  scratch: epropnp_kitti_match_scratch_bytes(num_dt, num_cases) bytes.
 *
 * epropnp_kitti_thresholds (get_thresholds, eval.py:12-30): sorted_scores (C,G) is tp_scores with every row sorted descending;
 * row c's first tp_count[c] entries are scanned with the reference's fp64 expressions ((i + 1) / num_gt, current_recall +=
 * recall_step; recall_step = 1 / 40.0 for the 41 sample points).  thresholds (C,41) double, zeros beyond thr_count (C,) int32.
 *
 * epropnp_kitti_statistics (compute_statistics_jit with compute_fp=True summed by fused_compute_statistics, eval.py:296-343): for
 * every case, image and threshold index below thr_count[c], which is read on the device.  pr (C,41,4) double: tp, fp, fn (exact
 * integers) and the similarity sum of (1 + cos(gt_alpha - dt_alpha)) / 2 over the true positives (0 unless compute_aos); zeros beyond
 * thr_count.  metric 0 takes detections inside DontCare boxes off fp.  tp_scores (C,41,G) or NULL: as epropnp_kitti_match's, per
 * threshold; rows beyond thr_count are not written.  scratch: epropnp_kitti_statistics_scratch_bytes(num_images,
 * num_dt, num_cases, compute_aos) bytes.
 *
 * num_cases == 0 launches nothing and follows no pointer.  EPROPNP_EINVAL: a negative count, more than 65535 cases, a metric outside
 * 0 .. 2, a recall_step that is not positive, a NULL pointer to an array that has elements, scratch below the size query. */
#define EPROPNP_KITTI_SAMPLE_PTS 41
#define EPROPNP_KITTI_GT_SKIPPED (-1)      /* ignore flag -1: not visited */
#define EPROPNP_KITTI_GT_UNMATCHED 0       /* ignore flag 1, no detection */
#define EPROPNP_KITTI_GT_TRUE_POSITIVE 1
#define EPROPNP_KITTI_GT_MISSED 2          /* ignore flag 0, no detection: a false negative */
#define EPROPNP_KITTI_GT_IGNORED_MATCH 3   /* a detection was taken, and either side has ignore flag 1 */
size_t epropnp_kitti_match_scratch_bytes(int32_t num_dt, int32_t num_cases);
int epropnp_kitti_match(const void* overlaps, int32_t overlaps_fp64, int64_t num_overlaps, const int32_t* gt_offsets /* (I+1,) */,
                        const int32_t* dt_offsets /* (I+1,) */, const int64_t* block_offsets /* (I+1,) */, int32_t num_images,
                        const double* dt_data /* (D,6) */, int32_t num_gt, int32_t num_dt, const int8_t* ignored_gt /* (C,G) */,
                        const int8_t* ignored_det /* (C,D) */, const double* min_overlap /* (C,) */, int32_t num_cases, void* scratch,
                        size_t scratch_bytes, double* tp_scores /* (C,G) */, int32_t* tp_count /* (C,) */,
                        int8_t* gt_state /* (C,G) or NULL */, void* stream);
int epropnp_kitti_thresholds(const double* sorted_scores /* (C,G) */, const int32_t* tp_count /* (C,) */,
                             const int32_t* num_valid_gt /* (C,) */, int32_t num_gt, int32_t num_cases, double recall_step,
                             double* thresholds /* (C,41) */, int32_t* thr_count /* (C,) */, void* stream);
size_t epropnp_kitti_statistics_scratch_bytes(int32_t num_images, int32_t num_dt, int32_t num_cases, int32_t compute_aos);
int epropnp_kitti_statistics(const void* overlaps, int32_t overlaps_fp64, int64_t num_overlaps, const int32_t* gt_offsets,
                             const int32_t* dt_offsets, const int32_t* dc_offsets, const int64_t* block_offsets, int32_t num_images,
                             const double* gt_data /* (G,5) */, const double* dt_data /* (D,6) */, const double* dc_boxes /* (Q,4) */,
                             int32_t num_gt, int32_t num_dt, int32_t num_dc, const int8_t* ignored_gt, const int8_t* ignored_det,
                             const double* min_overlap, int32_t num_cases, const double* thresholds /* (C,41) */,
                             const int32_t* thr_count /* (C,) */, int32_t metric, int32_t compute_aos, void* scratch,
                             size_t scratch_bytes, double* pr /* (C,41,4) */, double* tp_scores /* (C,41,G) or NULL */,
                             void* stream);

/* Density pictures of the posterior, the weighted pose samples (S,B,P) + log-weights (S,B).  Both entries are one primitive -- a list
 * of weighted points (canvas, plane, pixel, weight) summed into pixels, then a zero-padded box sum of odd size -- in two launches:
 * one workgroup per object turns its samples into weights and bins; one workgroup per (canvas, 32 x 32 pixel tile) sums the points
 * that fall into tile + halo in LDS, each pixel in sample order, box-sums and writes the outputs.  No floating-point atomics: two
 * calls agree to the last bit.  Every output element is written.  No allocation, no synchronisation; capturable into a hipGraph.
 * Weights, per object b: w_j = exp(logw[j,b] - max_j logw[:,b]) / sum_j exp(..), one rounding in the exponent's argument, as
 * epropnp_posterior_summary.  A bad column holds a NaN / +inf log-weight or nothing but -inf.
 *
 * epropnp_orient_density (EPro-PnP-6DoF lib/utils/draw_orient_density.py:10-73, called at lib/test.py:219-225): dof must be 6.
 * Sample j of object b gives three points, one per plane k: a = column k of the rotation matrix of its quaternion [w,x,y,z], taken
 * as it is (the reference's `axisrot`; not normalised);  px = rint(a_x * (0.4 size) + (size / 2 - 0.5)), py likewise from a_y, round
 * half to even as torch.round;  front hemisphere iff a_z <= 0.  A point off the canvas or with a coordinate that is not finite is
 * dropped (the reference would raise).  front[b,y,x,k] / back[b,y,x,k] = sum of w_j over the points of plane k whose pixel lies in the
 * (window_h, window_w) window about (y, x): the reference's avg_pool2d(..) * kh * kw without intensity_scale.  image[b,y,x,c] =
 * (back_layer * sphere_opacity + circle * (1 - sphere_opacity)) * front_layer with layer_c = prod_k col[k,c] ^ (intensity_scale *
 * density_k), col = eye(3) * saturation + (1 - saturation) / 2, circle = 1 - 0.5 [((x - c) / r)^2 + ((y - c) / r)^2 <= 1],
 * c = size / 2 - 0.5, r = 0.4 size.  pose_opt (num_obj,7) or NULL: its three axes as lines from the centre to their projections,
 * drawn onto the bracket before the multiplication by front_layer -- a pixel whose centre lies within 1.5 px of segment k takes the
 * pure colour of axis k, a later axis over an earlier one (our rule in place of cv2.line(thickness=3, shift=3); OpenCV's rasteriser is
 * not reproduced pixel for pixel).  An object with a bad column: front, back and image are NaN everywhere.
 * bins (S,B,3) int32: py * size + px, + size^2 on the back hemisphere, -1 when dropped; the geometry alone decides it.
 * image, front, back, bins: each may be NULL (not wanted), not all four.  num_obj == 0 launches nothing and follows no pointer.
 * EPROPNP_EINVAL: num_obj < 0 or > 65535, dof != 6, mc_samples < 1, size outside 1 .. 4096, a window that is even or outside 1 .. 9, a
 * NULL pose_samples / logweights / scratch or four NULL outputs with num_obj > 0, scratch_bytes below the size query.
 *
 * epropnp_bev_density (EPro-PnP-Det core/visualizer/image_bev_vis.py:79-95 show_bev, fed by deform_pnp_head.py:554-598 and
 * detectors/epropnp_det.py:118-126): dof 4 or 6, only the translation is read.  Objects are sorted by group: group g owns the objects
 * obj_offsets[g] .. obj_offsets[g+1] - 1 (obj_offsets (num_groups + 1,), clamped into [0, num_obj]; offsets that do not ascend are not
 * detected: such a group is empty).  Sample j of object b adds w_j * obj_weight[b] (1 with obj_weight == NULL) at px = rint(z * scale)
 * + origin_x, py = rint(x * scale) + origin_y -- the reference's proj_mat = [[0, scale], [scale, 0]].  Samples off the grid are
 * dropped; an object with a bad column adds nothing.  density (num_groups, height, width): the zero-padded window x window box sum,
 * i.e. cv2.blur * window^2 except in the outermost window / 2 rows and columns, where cv2.blur reflects at the border.
 * bins (S,B) int32: py * width + px, -1 when dropped.  May be NULL.
 * num_groups == 0: density is not followed; num_obj == 0: every density element is 0 and no sample pointer is followed.
 * EPROPNP_EINVAL: a negative count, num_groups > 65535, dof not 4 or 6, mc_samples < 1, height or width outside 1 .. 4096, a window
 * that is even or outside 1 .. 9, a NULL pose_samples / logweights / scratch with num_obj > 0, a NULL obj_offsets / density with
 * num_groups > 0, scratch_bytes below the size query.
 *
 * scratch: at least epropnp_*_density_scratch_bytes(mc_samples, num_obj) = num_obj * 32 + mc_samples * num_obj * 4 * (1 + K) bytes
 * (K = 3 points per sample for the sphere, 1 for the grid): per-object bounding boxes, the weights and the bins. */
size_t epropnp_orient_density_scratch_bytes(int32_t mc_samples, int32_t num_obj);
int epropnp_orient_density(const float* pose_samples /* (S,B,7) */, const float* logweights /* (S,B) */,
                           const float* pose_opt /* (B,7) or NULL */, int32_t mc_samples, int32_t num_obj, int32_t dof, int32_t size,
                           int32_t window_h, int32_t window_w, float saturation, float sphere_opacity, float intensity_scale,
                           void* scratch, size_t scratch_bytes, float* image /* (B,size,size,3) */, float* front /* (B,size,size,3) */,
                           float* back /* (B,size,size,3) */, int32_t* bins /* (S,B,3) */, void* stream);
size_t epropnp_bev_density_scratch_bytes(int32_t mc_samples, int32_t num_obj);
int epropnp_bev_density(const float* pose_samples /* (S,B,4|7) */, const float* logweights /* (S,B) */,
                        const float* obj_weight /* (B,) or NULL */, const int32_t* obj_offsets /* (G+1,) */, int32_t mc_samples,
                        int32_t num_obj, int32_t num_groups, int32_t dof, int32_t height, int32_t width, float scale, int32_t origin_x,
                        int32_t origin_y, int32_t window, void* scratch, size_t scratch_bytes, float* density /* (G,H,W) */,
                        int32_t* bins /* (S,B) */, void* stream);

/* Centre targets of the detection head's training step: EPro-PnP-Det core/bbox_3d/center_target.py:42-259, VolumeCenter with the box
 * mesh (called first thing by deform_pnp_head.py:776-780), without a mesh rasteriser and without a render.  For the box mesh the
 * rasteriser's near / far depth pair of a pixel is the ray-box slab intersection; the whole target is three launches (a per-object
 * table; per (image, 16 x 16 tile of output cells) partial sums; a reduce over the tiles in tile order in fp64).  No floating-point
 * atomics: two calls agree to the last bit.  Every output element is written.  No allocation, no synchronisation; capturable into a
 * hipGraph.  No input value ever forms an address.
 *
 * Inputs: bboxes_3d (num_obj,7) = [l, h, w, x, y, z, yaw]; objects sorted by image, image g owns obj_offsets[g] .. obj_offsets[g+1] - 1
 * (obj_offsets (num_img + 1,), clamped into [0, num_obj]; offsets that do not ascend are not detected; an object in no image is
 * invalid); cam_intrinsic (num_img,3,3); dense_x2d (num_img,2,h_out,w_out), the original-image pixel coordinates (x, y) of each output
 * cell; dense_mask (num_img,1,h_out,w_out).
 * Render grid: h_rend x w_rend pixels (the reference's pad_shape // render_stride, pad_shape = ceil(max_shape / output_stride) *
 * output_stride).  Render pixel (row r, col c) has its centre at original-image coordinates u = render_stride (c + 0.5) - 0.5,
 * v = render_stride (r + 0.5) - 0.5 (pixel centres at integers); its ray is d = ((u - cx) / fx, (v - cy) / fy, 1), so the ray
 * parameter is camera depth.
 * Box: vertices +-0.5 [l, h, w] rotated about y by yaw ([[c,0,s],[0,1,0],[-s,0,c]]) and translated by [x, y, z]; the slab test in the box
 * frame gives t_near and t_far.  Each of the two that exists and is > z_clip is a fragment of the ray (the rasteriser clips at z_clip
 * and leaves the mesh open).
 * Valid pixel of an object: both fragments exist (t_far > t_near > z_clip) and the number of fragments of the objects of the same
 * image at that pixel with depth < t_far, the object's own near fragment included, is < faces_per_pixel (0: no limit; where 2 x the
 * image's objects <= faces_per_pixel the count cannot bind and is skipped).  thickness = t_far - t_near where valid, else 0.
 * Output cell (i, j) of the object's image: the bilinear sample (zeros outside, align_corners False) of thickness and of the 0 / 1
 * valid map at render coordinates ((x + 0.5) / render_stride - 0.5, (y + 0.5) / render_stride - 0.5), both times the mask value; the four
 * taps are four ray-box tests.  A cell with a coordinate that is not finite contributes nothing.
 * centers_2d (num_obj,2): with p = (j output_stride + output_stride / 2, i output_stride + output_stride / 2) and W = sum t:
 * sum t p / W; (0, 0) where W = 0.
 * bboxes_2d (num_obj,4): get_bbox_2d != 0: over the cells whose resampled valid value is >= 0.5, x1 = min j output_stride, x2 = max j
 * output_stride + output_stride, y alike; [w_out output_stride, h_out output_stride, output_stride, output_stride] without such a
 * cell.  get_bbox_2d == 0: a copy of bboxes_2d_in (num_obj,4), which may be NULL otherwise.
 * valid (num_obj,) bytes: W >= 1e-6 and both box sides >= min_box_size.  A box or intrinsics that are not finite (or a zero focal
 * length): valid = 0, centre (0, 0).
 *
 * epropnp_box_thickness: what the fused pass never stores -- thickness (num_obj,h_rend,w_rend) and valid (num_obj,h_rend,w_rend)
 * bytes per render pixel, through the same device function.
 *
 * scratch: at least epropnp_volume_centers_scratch_bytes(num_obj, h_out, w_out) bytes, 8-byte aligned: 64 bytes per object plus 40
 * bytes per (tile, object); epropnp_box_thickness takes the size with h_out = w_out = 0.
 * num_obj == 0 launches nothing and follows no pointer.
 * EPROPNP_EINVAL: a negative count, num_img > 65535 (epropnp_box_thickness: num_obj > 65535), objects without an image, a size
 * outside 1 .. 4096, a stride < 1, faces_per_pixel < 2 other than 0, a negative z_clip, a NULL pointer with num_obj > 0, scratch_bytes
 * below the size query. */
size_t epropnp_volume_centers_scratch_bytes(int32_t num_obj, int32_t h_out, int32_t w_out);
int epropnp_volume_centers(const float* bboxes_3d /* (B,7) */, const float* bboxes_2d_in /* (B,4) or NULL */,
                           const int32_t* obj_offsets /* (G+1,) */, const float* cam_intrinsic /* (G,3,3) */,
                           const float* dense_x2d /* (G,2,h,w) */, const float* dense_mask /* (G,1,h,w) */, int32_t num_obj,
                           int32_t num_img, int32_t h_out, int32_t w_out, int32_t h_rend, int32_t w_rend, int32_t output_stride,
                           int32_t render_stride, int32_t faces_per_pixel, float z_clip, float min_box_size, int32_t get_bbox_2d,
                           void* scratch, size_t scratch_bytes, float* centers_2d /* (B,2) */, float* bboxes_2d /* (B,4) */,
                           uint8_t* valid /* (B,) */, void* stream);
int epropnp_box_thickness(const float* bboxes_3d /* (B,7) */, const int32_t* obj_offsets /* (G+1,) */,
                          const float* cam_intrinsic /* (G,3,3) */, int32_t num_obj, int32_t num_img, int32_t h_rend, int32_t w_rend,
                          int32_t render_stride, int32_t faces_per_pixel, float z_clip, void* scratch, size_t scratch_bytes,
                          float* thickness /* (B,Hr,Wr) */, uint8_t* valid /* (B,Hr,Wr) */, void* stream);

/* Point targets of the detection head's training step: EPro-PnP-Det models/dense_heads/fcos_emb_head.py:299-438,
 * FCOSEmbHead.get_targets (called by deform_pnp_head.py:808 on the centre targets' output), in one pass over (image, point): a
 * one-word fill and one launch, a workgroup per (tile of 256 points, image) with the image's objects in LDS, 64 at a time.  No
 * scratch, no floating-point atomics (num_fg is built with integer adds), no synchronisation: two calls agree to the last bit; capturable
 * into a hipGraph.  Every output element is written.
 *
 * Inputs: points (num_points,2) = (x, y), shared by all images, level 0 first; gt_bboxes (num_gt,4) = [x1, y1, x2, y2]; centers2d
 * (num_gt,2); gt_labels (num_gt,) int64; objects sorted by image, image i owns img_offsets[i] .. img_offsets[i+1] - 1 (img_offsets
 * (num_img + 1,) on the device, clamped into [0, num_gt]; offsets that do not ascend are not detected).
 * HOST arrays, read during the call: lvl_offsets (num_levels + 1,), the starts of the levels in `points` (0 .. num_points, ascending,
 * num_levels <= 8); per level radius_px = stride x center_sample_radius (> 0), the regress range [regress_lo, regress_hi], and
 * level_strides (int64; NULL unless `strides` is wanted).
 * Definition: point (x, y) of level l in image i; each object j of image i in ascending order, with s = radius_px[l]:
 *   inside:   min(x - (cx - s), y - (cy - s), (cx + s) - x, (cy + s) - y) > 0
 *   in range: regress_lo[l] <= max(x - x1, y - y1, x2 - x, y2 - y) <= regress_hi[l]
 *   d_j = sqrtf(dx dx + dy dy), (dx, dy) = (x - cx, y - cy), each product and the sum rounded on its own (no fused multiply-add, so
 *   that objects mirrored about a point give equal bits), when both hold, else 1e8.
 * The winner is the lowest j with the smallest d_j (strict < while scanning: torch.min's first-minimum rule).  A comparison with a NaN
 * operand is false: an object with a NaN among its six numbers never wins.
 *   labels = gt_labels[winner], or num_classes when the smallest d is 1e8;
 *   centerness_targets = expf(-centerness_alpha (d_min / (1.414f s))), which underflows to 0 for background;
 *   gt_inds = img_offsets[i] + winner; the winner of an all-background row is local index 0, and so is that of an image without
 *   objects (label num_classes, centerness 0): what the reference returns for both;
 *   strides (optional, NULL: not wanted) = level_strides[l] (deform_pnp_head.py:825-827).
 * Outputs, all (num_img num_points,) in the reference's flattened order -- level-major, then image, then the point within the level,
 * i.e. torch.cat of get_targets' per-level lists: element num_img lvl_offsets[l] + i n_l + (p - lvl_offsets[l]), n_l the level's
 * points.  num_fg (1,) int32: the number of elements with label < num_classes.
 * num_points == 0 or num_img == 0: nothing is launched, no pointer is followed and num_fg is not written.
 * EPROPNP_EINVAL: a negative count, num_levels outside 1 .. 8, num_img > 65535, a NaN centerness_alpha, lvl_offsets that do not run
 * from 0 to num_points ascending, a radius_px that is not > 0, a NaN regress range, strides without level_strides, a NULL pointer
 * that would be followed. */
int epropnp_point_targets(const float* points /* (P,2) */, const int32_t* lvl_offsets /* host (L+1,) */,
                          const float* radius_px /* host (L,) */, const float* regress_lo /* host (L,) */,
                          const float* regress_hi /* host (L,) */, const int64_t* level_strides /* host (L,) or NULL */,
                          int32_t num_levels, const float* gt_bboxes /* (G,4) */, const float* centers2d /* (G,2) */,
                          const int64_t* gt_labels /* (G,) */, const int32_t* img_offsets /* (num_img+1,) */, int32_t num_points,
                          int32_t num_gt, int32_t num_img, int32_t num_classes, float centerness_alpha,
                          int64_t* labels /* (num_img P,) */, float* centerness_targets /* (num_img P,) */,
                          int64_t* gt_inds /* (num_img P,) */, int64_t* strides /* (num_img P,) or NULL */, int32_t* num_fg /* (1,) */,
                          void* stream);

/* The object sampler of the same step behind its draws: deform_pnp_head.py:1148-1174 (obj_sampler), one launch of one workgroup.
 * With fg = fg_mask != 0 (bytes), c = centerness_targets, S = sum of c over the foreground, n = its count,
 * u = min(num_uniform, n) / num_obj_samples:
 *   prob_k = c_k fg_k / max(S, eps);  prob_mix_k = fg_k / max(n, 1) u + prob_k (1 - u);
 * per sample i with its drawn point p_i = sample_point_inds[i] (clamped into the points before it forms an address):
 *   sample_gt_inds_i = gt_inds[p_i];  w_i = prob / prob_mix at p_i;
 *   sample_weights_i = w_i / max(sum of w_j over the samples j with the same gt index, eps), divided by max(their mean, eps);
 *   sample_uniform_weights_i = 1 / max(number of samples with the same gt index, 1), divided by max(their mean, eps).
 * max(v, least) keeps a NaN v, as torch's clamp(min=) does (a drawn point outside the foreground gives 0 / 0).  Every sum runs in a
 * fixed order in fp64 -- thread t of 1024 over the points t, t + 1024, ..., then a binary tree; per sample over the samples in
 * ascending order -- so two calls agree to the last bit; samples are grouped by comparing their gt indices: no (num_gt, N) mask and
 * no largest index.  num_fg (1,) int32, optional (NULL: not wanted): n.  No scratch, no allocation, no synchronisation.
 * num_obj_samples == 0 launches nothing and follows no pointer.
 * EPROPNP_EINVAL: a negative count, num_obj_samples > 2048, num_uniform outside 0 .. num_obj_samples, eps that is not > 0, samples
 * without points, a NULL pointer that would be followed. */
int epropnp_obj_sample_weights(const uint8_t* fg_mask /* (T,) */, const float* centerness_targets /* (T,) */,
                               const int64_t* gt_inds /* (T,) */, int64_t num_total_point,
                               const int64_t* sample_point_inds /* (N,) */, int32_t num_obj_samples, int32_t num_uniform, float eps,
                               int64_t* sample_gt_inds /* (N,) */, float* sample_weights /* (N,) */,
                               float* sample_uniform_weights /* (N,) */, int32_t* num_fg /* (1,) or NULL */, void* stream);

int epropnp_abi_version(void);
const char* epropnp_last_error(void);

/* Optional per-stage timing: while enabled, every kernel stage this library launches -- also the ones inside
 * epropnp_monte_carlo_forward -- is bracketed by two HIP events on its launch stream.  epropnp_profile_read synchronises
 * on the recorded events of `stage` ("evaluate_cost", "normal_equations", "lm_solve", "rslm_solve", "amis_forward",
 * "amis_backward", "adaptive_delta", "mc_loss_forward", "mc_loss_backward", "gn_step_forward", "gn_step_backward",
 * "center_points", "shift_poses", "weight_stats", "posterior_summary", "posterior_resample", "posterior_modes", "pose_errors", "bev_overlap", "bev_nms", "box_overlap", "box_overlap_segmented", "orient_density", "bev_density", "kitti_match", "kitti_thresholds", "kitti_statistics", "volume_centers", "box_thickness", "point_targets", "obj_sample_weights") and returns their mean duration and count; bench.py's per-kernel times and roofline
 * figures come from here.  Not for use inside a hipGraph capture. */
int epropnp_profile_enable(int on);
int epropnp_profile_reset(void);
int epropnp_profile_read(const char* stage, float* mean_ms, int32_t* count);

/* The default status word.  With `epropnp_problem.status == NULL` kernels report the events above into a per-device
 * int32[2] in host memory mapped into the device: no cost without an event, and the host notices a failure with a plain
 * load -- no synchronisation.  `epropnp_async_status` returns the flags seen so far on the current device (and the first
 * offending object in flags_and_first[1]), optionally clearing them; `epropnp_async_status_word` returns the word itself
 * for callers that poll it directly (NULL when switched off with EPROPNP_ASYNC_STATUS=0).  The Python layer polls on entry
 * to every call and reports EPROPNP_ST_LM_NOT_SPD / _NONFINITE_POSE -- asynchronously: at the first call after the failing
 * kernel has run, as HIP reports its own faults -- as a RuntimeWarning, or as the RuntimeError of
 * levenberg_marquardt.py:15-19,178-181 with EPROPNP_ASYNC_STATUS=raise (the reference's LU raises only on an exactly zero
 * pivot and otherwise hands NaN poses on, which its losses zero: monte_carlo_pose_loss.py:31). */
int epropnp_async_status(int32_t* flags_and_first, int clear);
int32_t* epropnp_async_status_word(void);

/* Floats per (iteration, sample, object) of an injected-noise buffer for the given dof (8 for 6-DoF:
 * [z0,z1,z2, chi2, g0..g3]; 4 + 3*16 for 4-DoF: [z0,z1,z2, chi2, u | 16x(u1,u2,u3)]). */
int epropnp_noise_stride(int dof);

/* evaluate_pnp(..., out_cost=True) for P poses per object: the cost-only path
 * epropnp/common.py:67-100 -> camera.py:21-30,81-93 (project_b + clamp) -> cost_fun.py:45-61 (Huber).
 *   poses (P,B,pose_len)  ->  cost (P,B) */
int epropnp_evaluate_cost(const epropnp_problem* prob, const float* poses, int32_t num_poses, float* cost,
                          void* stream);

/* Gradients of sum_j a_j cost(pose_j) w.r.t. the camera intrinsics and, for one of the poses, the reduction behind the
 * gradient w.r.t. that pose -- what autograd records in the reference for cost_init = evaluate_pnp(pose=pose_init,
 * out_cost=True) and for the AMIS log-weights w.r.t. camera.cam_mats and pose_init (epropnp/epropnp.py:121-124,139-169 ->
 * common.py:90-99 -> camera.py:21-30,81-93 -> cost_fun.py:8-12,45-61).  With h = K (R X + t), g_h = d cost / d h:
 *   poses (P,B,pose_len), weights (P,B) | NULL (= 1), m_pose in [-1, P)
 *   -> grad_cam (B,3,3) | NULL  = sum_j a_j sum_n g_h (R_j X_n + t_j)^T
 *   -> grad_h_outer (B,3,4) | NULL = a_m sum_n g_h (X_n, Y_n, Z_n, 1)^T for pose m = m_pose (zeros for m_pose = -1):
 *      d/dt_m = K^T M[:,3],  d/dR_m = K^T M[:,:3]  (per object, on the caller's side). */
int epropnp_cost_pose_cam_grad(const epropnp_problem* prob, const float* poses, const float* weights, int32_t num_poses,
                               int32_t m_pose, float* grad_h_outer, float* grad_cam, void* stream);

/* evaluate_pnp(..., out_jacobian, out_residual, out_cost) fused with the normal equations the LM solver forms
 * from them: common.py:67-100 -> camera.py:10-18,81-143 (project_a, Jacobian, clip_jac) -> cost_fun.py:63-84
 * (robust rescaling) -> levenberg_marquardt.py:205-214 (JtJ, Jtr).  The (B,2N,dof) Jacobian is never written.
 *   pose (B,pose_len) -> jtj (B,dof,dof), jtr (B,dof), cost (B,) */
int epropnp_normal_equations(const epropnp_problem* prob, const float* pose, int32_t clip_jac, float* jtj,
                             float* jtr, float* cost, void* stream);

/* LMSolver.solve with a given starting pose (epropnp/levenberg_marquardt.py:132-190, _lm_iter :192-241,
 * pose_add :255-265): the whole iteration runs inside one kernel, points stay in registers.
 *   pose_init (B,pose_len) -> pose_opt (B,pose_len); pose_cov (B,dof,dof) or NULL; cost (B,) or NULL;
 *   accept_mask (B,) int32 or NULL: bit i = step i accepted (diagnostics for the trust-region flip rate). */
int epropnp_lm_solve(const epropnp_problem* prob, const epropnp_lm_params* lm, const float* pose_init, float* pose_opt,
                     float* pose_cov, float* cost, int32_t* accept_mask, void* split_scratch, uint64_t split_scratch_bytes,
                     void* stream);
/* split_scratch: optional DEVICE buffer (or NULL / 0).  With few objects of many points (LineMOD: 32 crops x 4096 dense
 * correspondences on 256 CUs) and epropnp_lm_solve_split_bytes() bytes of scratch, the points of an object are dealt to up to
 * 8 workgroups that exchange their partial normal equations through it after every sweep; the library fills it on the stream
 * before the launch, contents are undefined afterwards.  0: the library would not split this problem. */
uint64_t epropnp_lm_solve_split_bytes(const epropnp_problem* prob, const epropnp_lm_params* lm);

/* The AMIS loop of EProPnPBase.monte_carlo_forward (epropnp/epropnp.py:132-182) including initial_fit,
 * gen_new_distr/gen_old_distr, estimate_params (:199-342), the proposal densities (epropnp/distributions.py,
 * pyro MultivariateStudentT) and the weight algebra (:156-169).
 *   pose_opt (B,pose_len), pose_cov (B,dof,dof) from the solver
 *   noise: NULL (on-device Philox) or (B,K,S/K,epropnp_noise_stride(dof)) injected base draws
 *   -> pose_samples (S,B,pose_len), logweights (S,B)
 *   -> proposals (optional, may be NULL): (B,K,40) fitted proposal parameters, for diagnostics/tests.
 * Arithmetic: fp32.  The pose x point projection of the cost sweep (camera.py:21-30) runs on v_mfma_f32_16x16x32_bf16 with each
 * fp32 operand split into three bf16 pieces that sum to it exactly (8 of the 9 cross products, fp32 accumulation: 1.4e-7
 * relative, the fp32 MFMA's 1.2e-7) wherever the points are register-resident; environment EPROPNP_FWD_PROJ=f32 selects
 * v_mfma_f32_16x16x4_f32 (and EPROPNP_BWD_PROJ=f32 does so for epropnp_amis_backward). */
int epropnp_amis_forward(const epropnp_problem* prob, const epropnp_amis_params* amis, const float* pose_opt,
                         const float* pose_cov, const float* noise, float* pose_samples, float* logweights,
                         float* proposals, void* stream);

/* Backward of  sum_b [ g_init[b]*cost(pose_init[b]) + sum_j g_logw[j,b]*logw[j,b] ]  w.r.t. x3d, x2d, w2d, delta:
 * what autograd replays through evaluate_pnp in the reference, recomputed
 * from the points instead of stored activations.  logw = -cost - const  =>  weight of sample j is -g_logw[j,b].
 * Samples whose TOTAL |weight| is below 2^-24 of the object's total (one fp32 rounding of the sum) are skipped;
 * environment EPROPNP_BWD_DROP=<fraction> changes that budget, 0 evaluates every non-zero sample (exact).
 *   pose_samples (S,B,pose_len), grad_logweights (S,B), pose_init (B,pose_len) or NULL, grad_cost_init (B,) or NULL
 *   -> grad_x3d (B,N,3), grad_x2d (B,N,2), grad_w2d (B,N,2), grad_delta (B,) */
int epropnp_amis_backward(const epropnp_problem* prob, const float* pose_samples, const float* grad_logweights,
                          int32_t mc_samples, const float* pose_init, const float* grad_cost_init,
                          float* grad_x3d, float* grad_x2d, float* grad_w2d, float* grad_delta, void* stream);

/* The same backward for FEW objects (a single CU is busy ~70 us with one object's 512 x 512 point-poses): the point
 * chunks of an object are dealt to `num_split` workgroups.  grad_x3d / grad_x2d / grad_w2d are bit-identical to
 * epropnp_amis_backward; grad_delta comes back as partials
 *   grad_delta_parts (B, num_split)   with   grad_delta[b] = sum_c grad_delta_parts[b, c]
 * for the caller to add in a fixed order (no atomics).  1 <= num_split <= min(16, ceil(num_pts / 64)); needs the
 * LDS-resident pose table (mc_samples <~ 2700), EPROPNP_EINVAL otherwise. */
int epropnp_amis_backward_split(const epropnp_problem* prob, const float* pose_samples, const float* grad_logweights,
                                int32_t mc_samples, const float* pose_init, const float* grad_cost_init, int32_t num_split,
                                float* grad_x3d, float* grad_x2d, float* grad_w2d, float* grad_delta_parts, void* stream);

/* ---- The threshold's gradient from the forward's sample costs ------------------------------------------------------------------
 * grad_delta = sum_pairs a_j max(rho - delta, 0) is the one output of the backward that is a number per object, and its sweep term
 * sum_pairs a_j min(|r|^2, 1) (residuals r in units of delta) is known before the backward starts: with c1 = min(1, 1 / rho),
 *     cost_j / delta^2 = sum_n m (rho - m / 2),  m = min(rho, 1)   =   sum_n c1 |r|^2 - 1/2 sum_n min(|r|^2, 1)
 * (inlier: |r|^2 / 2 on both sides; outlier: rho - 1/2 on both sides), so that
 *     grad_delta / delta = 2 sum_j a_j cost_j / delta^2 - sum_pairs c1 a_j |r|^2,
 * where the last sum is what the sweep accumulates for grad_w2d anyway.  cost_j is the Huber cost the AMIS forward computed for
 * sample j (logw_j = -cost_j - const discards it); the cost of pose_init is the forward's cost_init.  The entries below are the
 * existing ones with that cost array as one more output (forward) / input (backward):
 *   sample_costs (S,B), the layout of logweights; cost_init (B,) as epropnp_monte_carlo_forward returns it (= epropnp_evaluate_cost of
 *   pose_init on the same problem).
 * Forward: sample_costs == NULL is the existing entry, bit for bit; with it every other output keeps its bits.
 * Backward: sample_costs == NULL -- or cost_init == NULL while pose_init and grad_cost_init are given, or mc_samples == 0 -- is the
 * existing entry, bit for bit (the per-pair term).  With the costs grad_x3d, grad_x2d and the sweep's grad_w2d keep their bits;
 * grad_delta (and its share of grad_w2d under epropnp_problem.delta_stats) agrees with the per-pair form within fp32 rounding of
 * the two sums, ~ulp * sum_j |a_j| cost_j / delta, not bit for bit.  The costs must be those of pose_samples on THIS problem (same
 * points, weights, threshold, bounds, z_min); costs of samples that the weight threshold drops are not read and may be anything.
 * A threshold that the kernels carry as 1e-12 (delta <= 1e-12) makes cost_init -- evaluated at the caller's threshold -- unusable:
 * the kernel evaluates the cost of pose_init itself for such objects.  huber_eps does not enter: it smooths the solver's Jacobian,
 * not the Huber value that the sampler and this backward differentiate, so the identity holds for every problem.
 * The all-VALU kernel (EPROPNP_TUNE=bwd_impl=valu, pose table beyond LDS) ignores the costs; EPROPNP_TUNE=bwd_dcost=0 makes every
 * launch ignore them.  The launch plan (epropnp_plan_amis_backward) is the same with and without costs. */
int epropnp_amis_forward_costs(const epropnp_problem* prob, const epropnp_amis_params* amis, const float* pose_opt,
                               const float* pose_cov, const float* noise, float* pose_samples, float* logweights,
                               float* proposals, float* sample_costs, void* stream);
/* epropnp_monte_carlo_forward[_diag] (diag may be NULL) with sample_costs (S,B): the costs of pose_samples_n in the solver frame */
int epropnp_monte_carlo_forward_costs(const epropnp_problem* prob, const epropnp_mc_params* par, const float* pose_init,
                                      const float* noise, float* x3d_centered, float* offset, float* pose_init_n,
                                      float* start_pose, float* start_cost, float* pose_opt_n, float* pose_cov, float* cost,
                                      float* pose_samples_n, float* logweights, float* cost_init, float* pose_opt,
                                      float* pose_samples, const epropnp_diag* diag, float* sample_costs, void* stream);
/* For callers that reach the forward through an interface with a fixed argument list (the package's ctypes nodes): the NEXT call of
 * epropnp_amis_forward / epropnp_monte_carlo_forward / epropnp_monte_carlo_forward_diag on this host thread also writes its samples'
 * costs to sample_costs (S,B), as the _costs entries do, and forgets the request whatever it returns.  NULL withdraws a request. */
int epropnp_request_sample_costs(float* sample_costs);
int epropnp_amis_backward_costs(const epropnp_problem* prob, const float* pose_samples, const float* grad_logweights,
                                int32_t mc_samples, const float* pose_init, const float* grad_cost_init,
                                const float* sample_costs, const float* cost_init, float* grad_x3d, float* grad_x2d,
                                float* grad_w2d, float* grad_delta, void* stream);
int epropnp_amis_backward_split_costs(const epropnp_problem* prob, const float* pose_samples, const float* grad_logweights,
                                      int32_t mc_samples, const float* pose_init, const float* grad_cost_init, int32_t num_split,
                                      const float* sample_costs, const float* cost_init, float* grad_x3d, float* grad_x2d,
                                      float* grad_w2d, float* grad_delta_parts, void* stream);

/* AdaptiveHuberPnPCost.set_param (epropnp/cost_fun.py:123-126):
 *   delta[b] = mean(w2d[b]) * sqrt(sum_xy var_N(x2d[b])) * relative_delta      (unbiased variance)
 * x2d (B,N,2), w2d (B,N,2) -> delta (B,), stats (B,4) = [mean_w, x2d_std, mean_x, mean_y] (kept for the backward,
 * which is three broadcast expressions evaluated by the caller).  The variance is taken about the mean (two passes inside the
 * launch): its accuracy does not depend on where any one point lies.  As in the reference, a NaN or an infinity in x2d, a NaN in w2d
 * and num_pts = 1 (0 / 0) give delta = NaN; identical points give exactly 0. */
int epropnp_adaptive_delta(const float* x2d, const float* w2d, int32_t num_obj, int32_t num_pts, float relative_delta,
                           float* delta, float* stats, void* stream);

/* Monte-Carlo pose loss per object (EPro-PnP-6DoF/lib/models/monte_carlo_pose_loss.py:28-32):
 *   loss[b] = cost_target[b] + logsumexp_j logweights[j,b];  NaN -> 0.   lse (B,) is kept for the backward.
 * logweights (S,B), cost_target (B,) or NULL. */
int epropnp_mc_loss_forward(const float* logweights, const float* cost_target, int32_t mc_samples, int32_t num_obj,
                            float* loss, float* lse, void* stream);
/* grad_logweights[j,b] = grad_loss[b] * exp(logweights[j,b] - lse[b])   (0 where the loss was NaN);
 * grad_cost_target (B,) or NULL: grad_loss[b] (0 where the loss was NaN). */
int epropnp_mc_loss_backward(const float* logweights, const float* lse, const float* loss, const float* grad_loss,
                             int32_t mc_samples, int32_t num_obj, float* grad_logweights, float* grad_cost_target,
                             void* stream);
/* The SCALAR both reference loss modules return, from the per-object losses of epropnp_mc_loss_forward, in one
 * single-workgroup launch (EPro-PnP-Det epropnp_det/models/losses/monte_carlo_pose_loss.py:41-66 incl. mmdet's
 * weight_reduce_loss; EPro-PnP-6DoF lib/models/monte_carlo_pose_loss.py:20-35):
 *   norm_factor[0] <- (1 - momentum) * norm_factor[0] + momentum * norm_factor_in[0]     if norm_factor_in != NULL (training)
 *   out[0] = (sum_b weight[b] * loss[b]) * scale / norm_factor[0],    out[1] = scale / norm_factor[0]  (for the backward)
 * scale = loss_weight / num_obj ('mean'), loss_weight ('sum') or loss_weight / avg_factor.  weight (B,) or NULL (ones),
 * norm_factor (1,) device scalar or NULL (1.0), out (2,).  Fixed summation order: bit-reproducible.
 *   norm_factor_in: `norm_factor_in_count` values `norm_factor_in_stride` floats apart, averaged in index order -- the
 *   world mean of mmdet's reduce_mean read straight out of the receive buffer of the step's one all-gather (count = ranks,
 *   stride = floats per rank; sharding.ObjectExchange); count 1 for a plain scalar. */
int epropnp_mc_loss_reduce(const float* loss, const float* weight, int32_t num_obj, float scale, float momentum,
                           const float* norm_factor_in, int32_t norm_factor_in_count, int64_t norm_factor_in_stride,
                           float* norm_factor, float* out, void* stream);

/* Send buffer of the Det step's one collective (sharding.ObjectExchange), packed by ONE launch:
 *   send[0 .. n_scalars)            = scalars[i]                       (or, with sum_src != NULL, send[0] = sum_scale * sum(sum_src[0 .. sum_floats)),
 *                                                                      a fixed-order sum -- the detection head's norm_factor input,
 *                                                                      deform_pnp_head.py:870 -- and scalars[i] for i >= 1)
 *   send[n_scalars .. + row_floats) = rows                             (this rank's per-object outputs, flattened)
 * scalars may be NULL when n_scalars == 0 or (n_scalars == 1 and sum_src != NULL).
 * sum_row_weight (or NULL): sum_src is a (rows, sum_row_len) array and element [i, c] counts sum_row_weight[i] times -- the head's
 * `(scale * sample_weights[:, None]).sum() / max(2 n, 1)` in one go. */
int epropnp_exchange_pack(const float* rows, uint64_t row_floats, const float* scalars, int32_t n_scalars,
                          const float* sum_src, uint64_t sum_floats, float sum_scale, const float* sum_row_weight,
                          int32_t sum_row_len, float* send, void* stream);
/* Its backward through epropnp_mc_loss_forward: with g_b = grad_out[0] * coef[0] * weight[b] (coef = out + 1 of the forward),
 *   grad_logweights[j,b] = g_b * exp(logweights[j,b] - lse[b]),  grad_cost_target[b] = g_b (or NULL)   (0 where the loss was NaN).
 * grad_out and coef are device scalars: nothing is read back, the node is capturable. */
int epropnp_mc_loss_reduce_backward(const float* logweights, const float* lse, const float* weight, const float* coef,
                                    const float* grad_out, int32_t mc_samples, int32_t num_obj, float* grad_logweights,
                                    float* grad_cost_target, void* stream);

/* LMSolver.gn_step (epropnp/levenberg_marquardt.py:243-253), the differentiable Gauss-Newton step behind
 * `pose_opt_plus`:  step = -(J^T J + eps I)^-1 J^T r  at `pose` (clip_jac on).   pose (B,pose_len) -> step (B,dof). */
int epropnp_gn_step_forward(const epropnp_problem* prob, float eps, const float* pose, float* step, void* stream);
/* Its backward w.r.t. x3d, x2d, w2d, delta (the pose is not differentiated, as in the reference):
 * grad_step (B,dof) -> grad_x3d (B,N,3), grad_x2d (B,N,2), grad_w2d (B,N,2), grad_delta (B,). */
int epropnp_gn_step_backward(const epropnp_problem* prob, float eps, const float* pose, const float* grad_step,
                             float* grad_x3d, float* grad_x2d, float* grad_w2d, float* grad_delta, void* stream);

/* The same step composed with LMSolver.pose_add (levenberg_marquardt.py:70-72,255-265):
 *   pose_plus = pose (+) gn_step(pose)   (B,pose_len)   -- `pose_opt_plus` of LMSolver.forward in one launch,
 * and its backward from grad_pose_plus (B,pose_len) (the adjoint of pose_add is applied inside the kernel). */
int epropnp_pose_opt_plus_forward(const epropnp_problem* prob, float eps, const float* pose, float* pose_plus,
                                  void* stream);
int epropnp_pose_opt_plus_backward(const epropnp_problem* prob, float eps, const float* pose,
                                   const float* grad_pose_plus, float* grad_x3d, float* grad_x2d, float* grad_w2d,
                                   float* grad_delta, void* stream);

/* Sub-sample indices of the RSLM initialiser (epropnp/levenberg_marquardt.py:305-308): for each of the P x B
 * (proposal, object) rows draw n_pts distinct point indices with probability proportional to mean(w2d[b,n,:]),
 * sequentially without replacement (exponential-race keys -log(u)/w, the n_pts smallest win; same law as
 * torch.multinomial(replacement=False)).   w2d (B,N,2) -> inds (P,B,n_pts) int64, Philox(seed, offset). */
int epropnp_rslm_draw(const float* w2d, int32_t num_obj, int32_t num_pts, int32_t num_proposals, int32_t n_pts,
                      uint64_t seed, uint64_t offset, int64_t* inds, void* stream);

/* pnp_normalize (epropnp/common.py:103-124): offset[b] = mean_n x3d[b,n,:], x3d_centered = x3d - offset.
 * x3d (B,N,3) -> offset (B,3), x3d_centered (B,N,3). */
int epropnp_center_points(const float* x3d, int32_t num_obj, int32_t num_pts, float* offset, float* x3d_centered,
                          void* stream);
/* The pose half of pnp_normalize / pnp_denormalize (epropnp/common.py:118-136):
 * out[j,b] = pose[j,b] with translation += sign * R(pose[j,b]) offset[b]   (sign +1 normalise, -1 denormalise).
 * pose (P,B,pose_len), offset (B,3) -> out (P,B,pose_len); out may alias pose. */
int epropnp_shift_poses(const float* pose, const float* offset, int32_t num_poses, int32_t num_obj, int32_t dof,
                        float sign, float* out, void* stream);

/* Correspondence pre-processing of the reference's training loops, fused (the callers' side of the layer):
 *   x3d = noc * dim                                            EPro-PnP-6DoF/lib/train.py:141, Det deform_pnp_head.py:873
 *   mode 0: w2d = softmax_N(logits) * scale                    Det deform_pnp_head.py:418-423,874
 *   mode 1: w2d = exp(logits - mean_N(logits) - log N) * scale EPro-PnP-6DoF/lib/train.py:163-166
 * noc (B,N,3), dim (B,3) (both NULL with x3d NULL: weights only), logits (B,N,2), scale (B,2) or NULL
 * -> x3d (B,N,3), w2d (B,N,2), stats (B,4) kept for the backward: [0:2] the maximum (softmax) or the mean (mean_exp) of the logits
 * per channel; [2:4] the sum of exponentials (softmax).  For mean_exp [2:4] holds N and is no normaliser: log N sits inside the
 * exponent, and the backward does not read it. */
#define EPROPNP_W2D_SOFTMAX 0
#define EPROPNP_W2D_MEAN_EXP 1
int epropnp_prepare_forward(const float* noc, const float* dim, const float* logits, const float* scale,
                            int32_t num_obj, int32_t num_pts, int32_t mode, float* x3d, float* w2d, float* stats,
                            void* stream);
/* grad_x3d (B,N,3) or NULL, grad_w2d (B,N,2) -> grad_noc (B,N,3), grad_dim (B,3), grad_logits (B,N,2),
 * grad_scale (B,2) (grad_noc / grad_dim / grad_scale may be NULL). */
int epropnp_prepare_backward(const float* noc, const float* dim, const float* logits, const float* scale,
                             const float* stats, const float* grad_x3d, const float* grad_w2d, int32_t num_obj,
                             int32_t num_pts, int32_t mode, float* grad_noc, float* grad_dim, float* grad_logits,
                             float* grad_scale, void* stream);

/* The same pre-processing reading the network's DENSE maps (EPro-PnP-6DoF/lib/train.py:141-166): the maps are gathered
 * at `inds` (pixel index row * width + col; the reference draws them with np.random.choice, :157-162:
 * `x.flatten(2).transpose(-1, -2)[batch_inds, sample_inds]`) without materialising the transposed maps, and the pixel
 * grid of the sampled pixels is generated in place of the meshgrid of :147-152:
 *   x2d[b,n] = (box[b,0] + col * box[b,2], box[b,1] + row * box[b,2])     box = [wh_begin_x, wh_begin_y, wh_unit]
 * noc_map (B,3,H,W), dim (B,3) (both NULL with x3d NULL), logit_map (B,2,H,W), scale (B,2) or NULL, box (B,3) (NULL with
 * x2d NULL), inds (B,N) int64 -> x3d (B,N,3), x2d (B,N,2), w2d (B,N,2), stats (B,4). */
int epropnp_prepare_dense_forward(const float* noc_map, const float* dim, const float* logit_map, const float* scale,
                                  const float* box, const int64_t* inds, int32_t num_obj, int32_t num_pts, int32_t height,
                                  int32_t width, int32_t mode, float* x3d, float* x2d, float* w2d, float* stats,
                                  void* stream);
/* grad_x3d (B,N,3) or NULL, grad_w2d (B,N,2) -> grad_noc_map (B,3,H,W), grad_logit_map (B,2,H,W) (zero-filled here, then
 * scattered at `inds`; repeated indices accumulate), grad_dim (B,3), grad_scale (B,2) or NULL. */
int epropnp_prepare_dense_backward(const float* noc_map, const float* dim, const float* logit_map, const float* scale,
                                   const int64_t* inds, const float* stats, const float* grad_x3d, const float* grad_w2d,
                                   int32_t num_obj, int32_t num_pts, int32_t height, int32_t width, int32_t mode,
                                   float* grad_noc_map, float* grad_dim, float* grad_logit_map, float* grad_scale,
                                   void* stream);

/* The deformable attention sampler of the detection head, fused (EPro-PnP-Det epropnp_det/ops/deformable_attention_sampler.py:77-137,
 * called from deform_pnp_head.py:447-451).  Per object b, head j, point p, with image i = obj_img_ind[b]:
 *   px = x / stride - 0.5, py = y / stride - 0.5           :84-93: the normalise / un-normalise round trip, align_corners=False
 *   k, v, x2d : bilinear, border padding (px, py clamped to the map)        :96-121     head j reads channels j*D .. j*D+D-1
 *   mask      : bilinear, zero padding (no clamp)                             :122-128
 *   a_samples = q . k / sqrt(D)                                               :131
 *   attn      = sum_p v_p softmax_P(a)_p mask_p                               :132-137   (what the reference feeds to out_proj)
 * query (B,H,D), key / value (NI, H*D, h, w) read through the element strides (stride_n, stride_c, stride_h, stride_w) -- contiguous
 * NCHW or channels-last without a copy; channels-last is the fast layout (one corner of one head is D contiguous floats) --,
 * dense_x2d (NI,2,h,w) and dense_mask (NI,1,h,w) contiguous, sampling_location (B,H,P,2) input-image pixels [x, y], obj_img_ind (B,)
 * int64, `stride` the map's stride
 *   -> attn (B,H*D), v_samples (B,H,P,D) POINT-major (the reference's (B,H,D,P) is its transposed view), a_samples (B,H,P),
 *      mask_samples (B,H,P), x2d_samples (B,H,P,2) point-major, stats (B,H,2) = {max_p a, sum_p exp(a - max)} kept for the backward.
 * Memory safety is part of the semantics -- no input value forms an out-of-range address: corner indices are clamped as integers
 * after the conversion; a NaN location samples the border-mode maps at coordinate 0 and a huge one at the clamped coordinate, both
 * give mask_samples = 0 and a zero location gradient along that axis; obj_img_ind is clamped to [0, NI - 1] on the device (a host check would
 * synchronise).  One launch, no allocation, no synchronisation; capturable into a hipGraph.  num_obj == 0 launches nothing.
 * EPROPNP_EINVAL: num_points or head_dim outside 1 .. 64, num_heads / num_img / height / width / stride < 1, a stride below 1 or
 * strides that reach outside NI * H*D * h * w elements, a NULL pointer. */
int epropnp_deform_sample_forward(const float* query, const float* key, const float* value, const float* dense_x2d,
                                  const float* dense_mask, const float* sampling_location, const int64_t* obj_img_ind,
                                  int32_t num_obj, int32_t num_img, int32_t num_heads, int32_t num_points, int32_t head_dim,
                                  int32_t height, int32_t width, int32_t stride, int64_t stride_n, int64_t stride_c,
                                  int64_t stride_h, int64_t stride_w, float* attn, float* v_samples, float* a_samples,
                                  float* mask_samples, float* x2d_samples, float* stats, void* stream);
/* Its backward.  Cotangents in the forward's layouts, NULL = absent: grad_attn (B,H*D), grad_v_samples (B,H,P,D), grad_a_samples
 * (B,H,P), grad_mask_samples (B,H,P), grad_x2d_samples (B,H,P,2).  Gradients, NULL = not wanted: grad_query (B,H,D), grad_location
 * (B,H,P,2) -- through k, v, x2d and the mask; zero along an axis on which the coordinate is clamped, as grid_sample's -- both
 * summed in a fixed order; grad_key / grad_value: NI * H*D * h * w floats each with the maps' strides, zero-filled here and then
 * scattered into with float atomics (their last bits depend on the arrival order).  dense_x2d, dense_mask get no gradient. */
int epropnp_deform_sample_backward(const float* query, const float* key, const float* value, const float* dense_x2d,
                                   const float* dense_mask, const float* sampling_location, const int64_t* obj_img_ind,
                                   const float* stats, const float* grad_attn, const float* grad_v_samples,
                                   const float* grad_a_samples, const float* grad_mask_samples, const float* grad_x2d_samples,
                                   int32_t num_obj, int32_t num_img, int32_t num_heads, int32_t num_points, int32_t head_dim,
                                   int32_t height, int32_t width, int32_t stride, int64_t stride_n, int64_t stride_c,
                                   int64_t stride_h, int64_t stride_w, float* grad_query, float* grad_key, float* grad_value,
                                   float* grad_location, void* stream);

/* The cross-RoI logsumexp of the detection head's auxiliary losses, fused (EPro-PnP-Det epropnp_det/ops/inter_roi_ops.py:19-81, called
 * from deform_pnp_head.py:985 through logsoftmax_across_rois and from mvd_gaussian_mixture_nll_loss.py:50).  roi_inputs (n,c,rh,rw),
 * rois (n,5) = [image id, x1, y1, x2, y2], id = round(rois[:,0]).  RoI j is a neighbour of i when j != i, id_j == id_i >= 0 and
 * min(x2_i, x2_j) - max(x1_i, x1_j) > 0, the same in y (strict, in fp32: touching, empty and NaN boxes never pair)      :9-16, :31-43
 *   X = x1_i + (px + 0.5) / rw * (x2_i - x1_i)                      the image position of cell (py, px) of RoI i; Y alike
 *   gx = 2 (X - x1_j) / (x2_j - x1_j) - 1, valid = -1 < gx, gy < 1  :51-66, :71  (the overlap box of affine_mat cancels)
 *   s_j = bilinear sample of roi_inputs[j, c] at u = clamp(((gx + 1) rw - 1) / 2, 0, rw - 1), v alike (border, align_corners=False)  :68
 *   out[i,c,py,px] = log(exp(roi_inputs[i,c,py,px]) + sum over the neighbours j with valid: exp(s_j))                    :73-80
 * computed in fp64 between the loads and the one rounding of out, with a running maximum (any magnitude of the inputs); a RoI
 * without neighbours gets its input bits back.  Image ids and box corners only enter comparisons and the coordinate arithmetic: no
 * value read from a tensor forms an address unchecked.  One launch, no allocation, no synchronisation; capturable into a hipGraph.
 * num_rois == 0 or channels == 0 launches nothing.  EPROPNP_EINVAL: roi_height or roi_width < 1, roi_height * roi_width > 4096,
 * num_rois * channels > 2^31 - 1, a NULL pointer. */
int epropnp_roi_logsumexp_forward(const float* roi_inputs, const float* rois, int32_t num_rois, int32_t channels, int32_t roi_height,
                                  int32_t roi_width, float* out, void* stream);
/* Its backward w.r.t. roi_inputs (rois gets no gradient): `out` as the forward wrote it, grad_out (n,c,rh,rw) -> grad_inputs (n,c,rh,rw),
 *   grad_inputs_j(q) = grad_out_j(q) exp(x_j(q) - out_j(q)) + sum over the i that have j as a neighbour, over their cells p with valid:
 *                      grad_out_i(p) exp(s_j(p) - out_i(p)) wy(py, qy) wx(px, qx),   wx = max(0, 1 - |u(px) - qx|), wy alike.
 * One launch, no float atomic, every summation order fixed: two launches give the same bits. */
int epropnp_roi_logsumexp_backward(const float* roi_inputs, const float* rois, const float* out, const float* grad_out, int32_t num_rois,
                                   int32_t channels, int32_t roi_height, int32_t roi_width, float* grad_inputs, void* stream);

/* RoIAlign with average pooling, the op behind the detection head's extract_rois (EPro-PnP-Det deform_pnp_head.py:719-741, three
 * mmcv.ops.roi_align calls through roi_align_wrapper :1187-1196), for ONE map (map1 = out1 = NULL) or TWO maps of identical shape and
 * strides that share the per-RoI sampling tables (key and value).  map (NI,C,h,w) and out (num_rois,C,out_h,out_w) are read / written
 * through explicit element strides (n, c, h, w): contiguous NCHW or channels-last without a copy (map_stride_c == 1 selects the
 * channels-last kernels).  rois (num_rois,5) = [image id, x1, y1, x2, y2].  With o = 0.5 if aligned else 0:
 *   xs = x1 scale - o, xe = x2 scale - o, rw = xe - xs (clamped to >= 1 only when not aligned), bw = rw / out_w; ys, rh, bh alike
 *   gw = sampling_ratio if sampling_ratio > 0 else ceil(bw); gh alike; count = max(gh gw, 1)
 *   out[r,c,i,j] = 1/count sum_{iy < gh, ix < gw} bilinear(map[n,c], y = ys + i bh + (iy + .5) bh / gh, x = xs + j bw + (ix + .5) bw / gw)
 *   a sample with y < -1, y > h, x < -1 or x > w is 0; any other has y, x clamped to [0, h - 1], [0, w - 1]
 * so a RoI of zero or negative size on the adaptive grid (sampling_ratio = 0) has no samples and gives zeros.  The sum is evaluated
 * in its separable form out = Wy map Wx^T in fp64 and rounded once; every order is fixed (two launches give the same bits, and two
 * maps give the bits of two one-map calls).  A RoI whose image id is not in [0, NI) (the id is truncated, as the reference's), whose
 * corners are not finite or whose grid exceeds 2^30 samples per cell and axis gives zeros and no gradient: no input value forms an
 * address unchecked.  One launch, no allocation, no synchronisation; capturable into a hipGraph.  num_rois == 0 launches nothing.
 * EPROPNP_EINVAL: num_img / channels / height / width / out_height / out_width < 1, num_rois < 0, sampling_ratio outside 0 .. 32768,
 * a non-finite spatial_scale, a stride below 1 or strides whose largest offset reaches outside num_img * channels * height * width
 * (num_rois * channels * out_height * out_width) elements, a NULL pointer, map1 without out1 or the reverse. */
int epropnp_roi_align_forward(const float* map0, const float* map1, const float* rois, int32_t num_rois, int32_t num_img,
                              int32_t channels, int32_t height, int32_t width, int32_t out_height, int32_t out_width,
                              float spatial_scale, int32_t sampling_ratio, int32_t aligned, int64_t map_stride_n, int64_t map_stride_c,
                              int64_t map_stride_h, int64_t map_stride_w, int64_t out_stride_n, int64_t out_stride_c,
                              int64_t out_stride_h, int64_t out_stride_w, float* out0, float* out1, void* stream);
/* Its backward w.r.t. the maps (rois gets no gradient): grad_out (num_rois,C,out_h,out_w) with the out strides -> grad_map (NI,C,h,w)
 * with the map strides, grad_map = sum_r Wy_r^T grad_out_r Wx_r, gathered by destination: every element of grad_map0 (and grad_map1)
 * is written exactly once with a plain store, zeros included -- the buffers need no zero fill, there is no float atomic, and the RoIs
 * are summed in ascending order: two launches give the same bits.  num_rois == 0 writes zeros.  Errors as the forward's, and
 * num_img * ceil(channels / 64) > 65535. */
int epropnp_roi_align_backward(const float* grad_out0, const float* grad_out1, const float* rois, int32_t num_rois, int32_t num_img,
                               int32_t channels, int32_t height, int32_t width, int32_t out_height, int32_t out_width,
                               float spatial_scale, int32_t sampling_ratio, int32_t aligned, int64_t map_stride_n, int64_t map_stride_c,
                               int64_t map_stride_h, int64_t map_stride_w, int64_t out_stride_n, int64_t out_stride_c,
                               int64_t out_stride_h, int64_t out_stride_w, float* grad_map0, float* grad_map1, void* stream);

/* Backward of epropnp_shift_poses w.r.t. the pose (the offset is a constant, pnp_normalize detaches it):
 * grad_out (P,B,pose_len) -> grad_pose (P,B,pose_len). */
int epropnp_shift_poses_backward(const float* pose, const float* offset, const float* grad_out, int32_t num_poses,
                                 int32_t num_obj, int32_t dof, float sign, float* grad_pose, void* stream);

/* RSLMSolver.solve (epropnp/levenberg_marquardt.py:283-353) in one launch: center_based_init, weighted sub-sampling
 * of `num_points` (<= 16) correspondences per proposal, random initial rotations, `num_proposals` LM/GN solves per
 * object on the sub-samples (parameters `lm`, as LMSolver.solve), full-set cost of every proposal, argmin.
 *   inds: NULL (drawn on the device, same stream as epropnp_rslm_draw) or (P,B,num_points) int64 injected indices
 *   rot:  NULL (drawn on the device) or (P,B,1) yaw / (P,B,4) unit quaternions, injected
 *   offset_dev: optional device counter added to `offset` at run time (hipGraph replay), or NULL
 *   scratch: optional DEVICE buffer of scratch_bytes bytes (or NULL / 0): with epropnp_rslm_solve_scratch_bytes() bytes the
 *            proposals of an object are dealt to 2 or 4 workgroups (finer load balance: 600 objects x 64 proposals 66 ->
 *            51 us) whose candidates meet there; contents undefined afterwards.  Results do not depend on it.
 *   -> pose (B,pose_len) best proposal, cost (B,) its full-set Huber cost (may be NULL).   num_pts in [2, 512]. */
int epropnp_rslm_solve(const epropnp_problem* prob, const epropnp_lm_params* lm, int32_t num_proposals,
                       int32_t num_points, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                       const int64_t* inds, const float* rot, float* pose, float* cost, void* scratch,
                       uint64_t scratch_bytes, void* stream);
uint64_t epropnp_rslm_solve_scratch_bytes(const epropnp_problem* prob, int32_t num_proposals);
/* The same solve, reporting which proposal won: winner (B,) int32 (or NULL) = index in [0, num_proposals) of the proposal whose pose
 * is returned (ties: as the solve breaks them).  Pose and cost are bit-identical to epropnp_rslm_solve, with and without scratch. */
int epropnp_rslm_solve_diag(const epropnp_problem* prob, const epropnp_lm_params* lm, int32_t num_proposals,
                            int32_t num_points, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                            const int64_t* inds, const float* rot, float* pose, float* cost, void* scratch,
                            uint64_t scratch_bytes, int32_t* winner, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPROPNP_HIP_H */
