// pnp_host.h -- host-side plumbing shared by the launchers: argument checks, error reporting, workgroup
// shape selection.  No torch types anywhere: the library is a plain C ABI over device pointers.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/epropnp_hip.h"
#include "pnp_sweep.h"

namespace pnp {

char* last_error_buffer();   // thread-local, defined in c_api.hip
int32_t* default_status_word();   // per-device host-mapped int32[2] the kernels report into when the caller gives none (c_api.hip)

inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(last_error_buffer(), 512, fmt, ap);
  va_end(ap);
  return code;
}

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EPROPNP_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
  return EPROPNP_OK;
}

inline int check_problem(const epropnp_problem* p) {
  if (p == nullptr) return fail(EPROPNP_EINVAL, "problem is NULL");
  if (p->dof != 4 && p->dof != 6) return fail(EPROPNP_EINVAL, "dof must be 4 or 6, got %d", p->dof);
  if (p->num_obj < 0 || p->num_pts < 0) return fail(EPROPNP_EINVAL, "negative sizes");
  if (p->num_obj > 0 && p->num_pts > 0 &&
      (!p->x3d || !p->x2d || !p->w2d || !p->cam_mats || !p->delta))
    return fail(EPROPNP_EINVAL, "NULL device pointer in problem");
  if (!(p->z_min >= 0.f)) return fail(EPROPNP_EINVAL, "z_min must be >= 0 (a depth clamp), got %g", (double)p->z_min);
  return EPROPNP_OK;
}

// what the launch-plan queries read of a problem: sizes and dof (the device pointers may all be NULL)
inline int check_plan_problem(const epropnp_problem* p) {
  if (p == nullptr) return fail(EPROPNP_EINVAL, "problem is NULL");
  if (p->dof != 4 && p->dof != 6) return fail(EPROPNP_EINVAL, "dof must be 4 or 6, got %d", p->dof);
  if (p->num_obj <= 0 || p->num_pts <= 0) return fail(EPROPNP_EINVAL, "launch plan: num_obj and num_pts must be positive");
  return EPROPNP_OK;
}

inline Problem to_device_problem(const epropnp_problem* p) {
  Problem d;
  d.x3d = p->x3d; d.x2d = p->x2d; d.w2d = p->w2d; d.cam = p->cam_mats;
  d.lb = p->lb; d.ub = p->ub; d.delta = p->delta;
  d.z_min = p->z_min; d.B = p->num_obj; d.N = p->num_pts;
  d.huber_eps = (p->huber_eps > 0.f) ? p->huber_eps : 1e-10f;
  d.inv_huber_eps = 1.0f / d.huber_eps;
  d.status = p->status ? p->status : default_status_word();
  d.delta_stats = p->delta_stats; d.delta_relative = p->delta_relative;
  return d;
}

inline bool has_bounds(const epropnp_problem* p) { return p->lb != nullptr && p->ub != nullptr; }

constexpr int kMaxResidentPoints = 64 * 16 * 8;   // 16 waves x 64 lanes x 8 points per lane

// Pick waves-per-object and points-per-lane for kernels that keep the object's points in registers.
// Few objects -> more waves per object (fill the 1024 SIMDs); many objects -> fewer, fatter waves.
inline Shape choose_shape(int B, int N, int max_ppl = 8, int want_waves_total = 4096) {
  Shape s;
  int wmin = 1;
  while (64 * wmin * max_ppl < N && wmin < 16) wmin *= 2;
  // 16-wave (1024-thread) groups are limited to 128 VGPRs per lane and spill: only used when N demands it
  int wmax = 1;
  while (64 * wmax < N && wmax < 8) wmax *= 2;
  if (wmax < wmin) wmax = wmin;
  int w = wmin;
  while (w < wmax && (long)B * w < want_waves_total) w *= 2;
  s.waves = w;
  int ppl = 1;
  while (64 * w * ppl < N) ppl *= 2;
  s.ppl = ppl;
  return s;
}

// a (waves, points-per-lane) override from a tuning variable is taken only if it is one the kernels are instantiated for
// and covers the object: anything else is ignored (a typo must not change results)
inline bool valid_shape_override(int waves, int ppl, int N) {
  const bool w_ok = waves == 1 || waves == 2 || waves == 4 || waves == 8 || waves == 16;
  const bool p_ok = ppl == 1 || ppl == 2 || ppl == 4 || ppl == 8;
  return w_ok && p_ok && 64L * waves * ppl >= N;
}

inline bool parse_ints(const char* v, int* out, int n) {
  if (!v || !*v) return false;
  for (int i = 0; i < n; ++i) {
    char* end = nullptr;
    out[i] = (int)strtol(v, &end, 10);
    if (end == v) return false;
    v = (*end == ',') ? end + 1 : end;
  }
  return true;
}

// A user-facing knob EPROPNP_<NAME>="a[,b]" (INTEGRATION.md lists them all: *_PROJ, BWD_DROP, *_SPLIT, ASYNC_STATUS, NO_TORCH_EXT,
// DELTA_FOLD, LOSS_FUSED, SPLIT_TIMEOUT_CYCLES).
inline bool env_ints(const char* name, int* out, int n) { return parse_ints(getenv(name), out, n); }

// Everything else that used to be an environment variable of its own -- launch-shape overrides, implementation selectors,
// phase ablation: what tools/tune.py and the shape tests need, not what a user does -- is ONE string:
//     EPROPNP_TUNE="lm_shape=1,8;bwd_impl=valu;rslm_composite"
// `tune_value(key)` returns the text behind "key=" ("" for a bare key), or nullptr when the key is absent.
inline const char* tune_value(const char* key) {
  static thread_local char buf[64];
  const char* s = getenv("EPROPNP_TUNE");
  if (!s) return nullptr;
  const size_t kl = strlen(key);
  while (*s) {
    const char* end = strchr(s, ';');
    const size_t len = end ? (size_t)(end - s) : strlen(s);
    if (len >= kl && strncmp(s, key, kl) == 0 && (len == kl || s[kl] == '=')) {
      const size_t vl = (len == kl) ? 0 : len - kl - 1;
      if (vl >= sizeof(buf)) return nullptr;
      memcpy(buf, s + kl + (len == kl ? 0 : 1), vl);
      buf[vl] = 0;
      return buf;
    }
    if (!end) break;
    s = end + 1;
  }
  return nullptr;
}
inline bool tune_ints(const char* key, int* out, int n) { return parse_ints(tune_value(key), out, n); }
inline bool tune_flag(const char* key) { return tune_value(key) != nullptr; }

// The cost sweep (evaluate_cost): choose_shape with its defaults, or EPROPNP_TUNE="ev_shape=<waves>,<ppl>" -- the rule of ne_shape /
// lm_shape, ignored when invalid -- with which a few objects reach the fat-lane instantiations that thousands of objects take.
// Shared by the launcher and by epropnp_plan_evaluate_cost.
inline Shape cost_sweep_shape(int B, int N) {
  Shape s = choose_shape(B, N);
  int ov[2];
  if (tune_ints("ev_shape", ov, 2) && valid_shape_override(ov[0], ov[1], N)) { s.waves = ov[0]; s.ppl = ov[1]; }
  return s;
}

// EPROPNP_TUNE="bwd_impl=valu": epropnp_amis_backward takes the all-VALU kernel (amis_kernels.hip) whatever the shape
inline bool backward_valu_forced() {
  const char* impl = tune_value("bwd_impl");
  return impl && impl[0] == 'v';
}

// Compute units of the current device (hipDeviceAttributeMultiprocessorCount, cached): what the workgroup-split variants
// size their grids against -- a partitioned (CPX) MI355X or another part reports its own count; the CPU emulation of the
// tests is a "device" with ONE compute unit (it runs one workgroup at a time), which switches the splits off by default.
// (The launch-plan queries -- epropnp_plan_*, c_api.hip -- can ask for the plan of another CU count: PlanCuScope.)
inline int& plan_cu_override() {
  static thread_local int cus = 0;
  return cus;
}
struct PlanCuScope {
  int prev;
  explicit PlanCuScope(int cus) : prev(plan_cu_override()) { if (cus > 0) plan_cu_override() = cus; }
  ~PlanCuScope() { plan_cu_override() = prev; }
};
inline int device_cu_count() {
  if (plan_cu_override() > 0) return plan_cu_override();
  static int cached[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int n = __atomic_load_n(&cached[dev], __ATOMIC_RELAXED);
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    __atomic_store_n(&cached[dev], n, __ATOMIC_RELAXED);
  }
  return n;
}

// How long (shader cycles) a part of a split kernel waits for a sibling's exchange words before it recomputes them itself
// (wave_ops.h: xwg_poll).  Default 2^18 (~0.1 ms: siblings normally arrive within ~2 us); EPROPNP_SPLIT_TIMEOUT_CYCLES
// overrides, 0 = never wait (every part recomputes whatever is not there yet: the tests' way of forcing that path).
inline unsigned split_timeout_cycles() {
  int ov[1];
  if (env_ints("EPROPNP_SPLIT_TIMEOUT_CYCLES", ov, 1) && ov[0] >= 0) return (unsigned)ov[0];
  return 1u << 18;
}

// kernels with more than 64 KiB of dynamic LDS have to be told so once
inline void allow_dynamic_lds(const void* kern, size_t bytes) {
  if (bytes > 64 * 1024) (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// Fraction of an object's total |weight| that the backward may leave out (see mass_drop_threshold, amis_common.h).
// Default 2^-24; EPROPNP_BWD_DROP=<float> overrides it, 0 = exact (every non-zero sample is evaluated).
inline float backward_drop_eps() {
  const char* v = getenv("EPROPNP_BWD_DROP");
  if (v && *v) {
    char* end = nullptr;
    const float f = strtof(v, &end);
    if (end != v && f >= 0.f && f < 1.f) return f;
  }
  return 5.9604644775390625e-08f;
}

// Optional per-stage timing (epropnp_profile_*, include/epropnp_hip.h): HIP events on the launch stream around each
// kernel stage, recorded inside the library so that stages launched from epropnp_monte_carlo_forward are visible too.
bool profile_begin(const char* stage, hipStream_t st);     // false (and no work) unless profiling is enabled
void profile_end(hipStream_t st);
struct StageScope {
  hipStream_t st;
  bool on;
  StageScope(const char* stage, hipStream_t s) : st(s), on(profile_begin(stage, s)) {}
  ~StageScope() { if (on) profile_end(st); }
};

// launchers (one per .hip translation unit)
int launch_monte_carlo_forward(const epropnp_problem* prob, const epropnp_mc_params* par, const float* pose_init,
                               const float* noise, float* x3d_centered, float* offset, float* pose_init_n,
                               float* start_pose, float* start_cost, float* pose_opt_n, float* pose_cov, float* cost,
                               float* pose_samples_n, float* logweights, float* cost_init, float* pose_opt,
                               float* pose_samples, hipStream_t st, const epropnp_diag* diag = nullptr,
                               float* sample_costs = nullptr);
unsigned long long amis_forward_split_bytes(const epropnp_problem* prob, int mc_samples, int num_iter);
// launch plans as int records (include/epropnp_hip.h: epropnp_plan_*): host only, nothing is launched
int plan_amis_forward_record(const epropnp_problem* prob, int S, int K, unsigned long long scratch_bytes, int32_t* out);
int plan_amis_backward_record(const epropnp_problem* prob, int mc_samples, int with_init, int nsplit, int32_t* out);
int launch_evaluate_cost(const epropnp_problem* prob, const float* poses, int num_poses, float* cost, hipStream_t st);
int launch_cost_pose_cam_grad(const epropnp_problem* prob, const float* poses, const float* weights, int num_poses,
                              int m_pose, float* out_m, float* out_gk, hipStream_t st);
int launch_normal_equations(const epropnp_problem* prob, const float* pose, int clip_jac, float* jtj, float* jtr,
                            float* cost, hipStream_t st);
int launch_amis_backward_mfma(const epropnp_problem* prob, const float* pose_samples, const float* grad_logweights,
                              int mc_samples, const float* pose_init, const float* grad_cost_init, float* grad_x3d,
                              float* grad_x2d, float* grad_w2d, float* grad_delta, int nsplit, hipStream_t st,
                              const float* sample_costs = nullptr, const float* cost_init = nullptr);
int launch_rslm_solve(const epropnp_problem* prob, const epropnp_lm_params* lm, int P, int n_pts, unsigned long long seed,
                      unsigned long long offset, const unsigned long long* offset_dev, const long long* inds, const float* rot,
                      float* pose_out, float* cost_out, void* scratch, unsigned long long scratch_bytes,
                      hipStream_t st, const float* rival_pose = nullptr, const float* rival_cost = nullptr,
                      bool* rival_taken = nullptr, int* deferred_parts = nullptr, int32_t* winner = nullptr);
unsigned long long rslm_scratch_bytes(const epropnp_problem* prob, int num_proposals);
int launch_shift_poses_pair(const float* pose_a, float* out_a, int Pa, const float* pose_b, float* out_b, int Pb,
                            const float* offset, int B, int dof, float sign, hipStream_t st);
int launch_center_points(const float* x3d, int B, int N, float* offset, float* out, hipStream_t st);
int launch_center_cost(const epropnp_problem* prob, const float* pose, float* offset, float* x3d_centered, float* pose_n,
                       float* cost, hipStream_t st);
int launch_center_points_shift(const float* x3d, int B, int N, float* offset, float* out, const float* pose, float* pose_out,
                               int dof, hipStream_t st);
int launch_shift_poses(const float* pose, const float* offset, int P, int B, int dof, float sign, float* out,
                       hipStream_t st);
int launch_prepare_forward(const float* noc, const float* dim, const float* logits, const float* scale, int B, int N,
                           int mode, float* x3d, float* w2d, float* stats, hipStream_t st);
int launch_prepare_backward(const float* noc, const float* dim, const float* logits, const float* scale, const float* stats,
                            const float* gx3d, const float* gw2d, int B, int N, int mode, float* gnoc, float* gdim,
                            float* glogits, float* gscale, hipStream_t st);
int launch_prepare_dense_forward(const float* noc_map, const float* dim, const float* logit_map, const float* scale,
                                 const float* box, const long long* inds, int B, int N, int H, int W, int mode, float* x3d,
                                 float* x2d, float* w2d, float* stats, hipStream_t st);
int launch_prepare_dense_backward(const float* noc_map, const float* dim, const float* logit_map, const float* scale,
                                  const long long* inds, const float* stats, const float* gx3d, const float* gw2d, int B,
                                  int N, int H, int W, int mode, float* gnoc_map, float* gdim, float* glogit_map,
                                  float* gscale, hipStream_t st);
int launch_shift_poses_backward(const float* pose, const float* offset, const float* gout, int P, int B, int dof, float sign,
                                float* gpose, hipStream_t st);
int launch_gn_step_forward(const epropnp_problem* prob, float eps, const float* pose, float* step, float* pose_plus,
                           hipStream_t st);
int launch_gn_step_backward(const epropnp_problem* prob, float eps, const float* pose, const float* grad_step,
                            const float* grad_pose_plus, float* grad_x3d, float* grad_x2d, float* grad_w2d, float* grad_delta, hipStream_t st);
int launch_rslm_draw(const float* w2d, int B, int N, int P, int n_pts, unsigned long long seed, unsigned long long offset,
                     long long* inds, hipStream_t st);
int launch_adaptive_delta(const float* x2d, const float* w2d, int B, int N, float rel, float* delta, float* stats,
                          hipStream_t st);
int launch_mc_loss_forward(const float* logw, const float* ct, int S, int B, float* loss, float* lse, hipStream_t st);
int launch_weight_stats(const float* logw, int S, int B, int K, float* stats, hipStream_t st);
// posterior_kernels.hip: moments / systematic resampling of the weighted pose samples (epropnp_posterior_summary / _resample)
int launch_posterior_summary(const float* pose, const float* logw, const float* ref, int S, int B, int dof, float* out,
                             hipStream_t st);
int launch_posterior_resample(const float* pose, const float* logw, int S, int B, int dof, int R, const float* u,
                              unsigned long long seed, unsigned long long offset, int32_t* index, float* poses, hipStream_t st);
// quick-shift modes of the weighted pose samples (epropnp_posterior_modes): two pair launches and a label launch
int launch_posterior_modes(const float* pose, const float* logw, const float* bandwidth, int S, int B, int dof, float link,
                           int max_modes, float* density, int32_t* parent, int32_t* labels, int32_t* num_modes,
                           int32_t* mode_index, float* mode_mass, float* mode_poses, hipStream_t st);
// metrics_kernels.hip: pose-error metrics of R x B pose rows against B ground-truth poses (epropnp_pose_errors): the ADD-S
// nearest-neighbour launch when a symmetric mask is given, then the streaming launch that writes every row
int launch_pose_errors(const float* pose_est, const float* pose_gt, int R, int B, int dof, const float* points,
                       const int32_t* range, int C, const int32_t* model_id, const float* cam, const uint8_t* symmetric,
                       const uint8_t* half_turn, void* scratch, size_t scratch_bytes, float* errors, hipStream_t st);
size_t pose_errors_scratch_bytes(int R, int B, int max_model_points);
// boxes_kernels.hip: rotated BEV boxes (epropnp_bev_overlap, epropnp_bev_nms): pairwise / aligned overlap or IoU in one launch; the
// grouped greedy suppression in two (the 64 x 64 mask tiles of the visiting order, then the one-workgroup reduce)
int launch_bev_overlap(const float* boxes_a, int M, const float* boxes_b, int N, int want_iou, int aligned, float* out,
                       hipStream_t st);
int launch_bev_nms(const float* boxes, const int32_t* order, const int32_t* group, int N, float thr, void* scratch,
                   size_t scratch_bytes, int32_t* keep_index, uint8_t* keep_mask, int32_t* num_keep, hipStream_t st);
size_t bev_nms_scratch_bytes(int N);
// rotated / 3D / image box overlaps under the four criteria (epropnp_box_overlap, _plan, _segmented): one launch each; the plan is a
// host function that turns per-segment counts into the segmented launch's tile table
int launch_box_overlap(const float* boxes_a, int M, const float* boxes_b, int N, int kind, int crit, int z_axis, float z_center,
                       int rule, int aligned, float* out, hipStream_t st);
int box_overlap_plan(const int32_t* counts_a, const int32_t* counts_b, int G, int32_t* tiles, long long capacity, long long* num_tiles,
                     long long* num_out);
int launch_box_overlap_segmented(const float* boxes_a, int M, const float* boxes_b, int N, int kind, int crit, int z_axis,
                                 float z_center, int rule, const int32_t* tiles, int num_tiles, float* out, long long num_out,
                                 hipStream_t st);
// kitti_eval_kernels.hip: the KITTI AP evaluation behind the overlap blocks (epropnp_kitti_match, _thresholds, _statistics): a count
// fill and one launch for the matching pass, one launch for the thresholds, a count fill and two launches (per image, then the
// fixed-order reduce) for the PR sums -- the same number whatever the images and cases
int launch_kitti_match(const void* overlaps, int ov64, long long num_ov, const int32_t* gt_off, const int32_t* dt_off,
                       const long long* blk_off, int I, const double* dt_data, int G, int D, const int8_t* ign_gt, const int8_t* ign_dt,
                       const double* min_ov, int C, void* scratch, size_t scratch_bytes, double* tp_scores, int32_t* tp_count,
                       int8_t* gt_state, hipStream_t st);
int launch_kitti_thresholds(const double* sorted, const int32_t* tp_count, const int32_t* num_valid_gt, int G, int C, double recall_step,
                            double* thresholds, int32_t* thr_count, hipStream_t st);
int launch_kitti_statistics(const void* overlaps, int ov64, long long num_ov, const int32_t* gt_off, const int32_t* dt_off,
                            const int32_t* dc_off, const long long* blk_off, int I, const double* gt_data, const double* dt_data,
                            const double* dc_boxes, int G, int D, int Q, const int8_t* ign_gt, const int8_t* ign_dt, const double* min_ov,
                            int C, const double* thresholds, const int32_t* thr_count, int metric, int compute_aos, void* scratch,
                            size_t scratch_bytes, double* pr, double* tp_scores, hipStream_t st);
size_t kitti_match_scratch_bytes(int D, int C);
size_t kitti_statistics_scratch_bytes(int I, int D, int C, int compute_aos);
// density_kernels.hip: density pictures of the weighted pose samples (epropnp_orient_density, epropnp_bev_density): one launch that
// turns samples into weighted bins, one that sums them per 32 x 32 tile in LDS, box-filters and writes the picture
int launch_orient_density(const float* pose, const float* logw, const float* pose_opt, int S, int B, int dof, int size, int kh,
                          int kw, float saturation, float opacity, float intensity, void* scratch, size_t scratch_bytes,
                          float* image, float* front, float* back, int32_t* bins, hipStream_t st);
int launch_bev_density(const float* pose, const float* logw, const float* obj_weight, const int32_t* offsets, int S, int B, int G,
                       int dof, int H, int W, float scale, int ox, int oy, int window, void* scratch, size_t scratch_bytes,
                       float* density, int32_t* bins, hipStream_t st);
size_t orient_density_scratch_bytes(int S, int B);
size_t bev_density_scratch_bytes(int S, int B);
// center_target_kernels.hip: the training step's centre targets (epropnp_volume_centers: the per-object table, the per-tile partials,
// the fixed-order fp64 reduce -- three launches) and the render the fused pass never stores (epropnp_box_thickness: table + one launch)
int launch_volume_centers(const float* boxes3d, const float* boxes2d_in, const int32_t* offsets, const float* cam, const float* x2d,
                          const float* mask, int B, int G, int h, int w, int Hr, int Wr, int os, int rs, int K, float zc,
                          float min_box, int want_box, void* scratch, size_t scratch_bytes, float* centers, float* boxes2d,
                          uint8_t* valid, hipStream_t st);
int launch_box_thickness(const float* boxes3d, const int32_t* offsets, const float* cam, int B, int G, int Hr, int Wr, int rs, int K,
                         float zc, void* scratch, size_t scratch_bytes, float* thick, uint8_t* valid, hipStream_t st);
size_t volume_centers_scratch_bytes(int B, int h, int w);
// point_target_kernels.hip: the training step's point targets (epropnp_point_targets: a one-word fill and one launch, a workgroup per
// (tile of points, image) with the image's objects in LDS) and the sampler's weights behind its draws (epropnp_obj_sample_weights:
// one launch of one workgroup, every sum in a fixed order).  lvl_off .. level_strides are HOST arrays
int launch_point_targets(const float* points, const int32_t* lvl_off, const float* radius_px, const float* regress_lo,
                         const float* regress_hi, const long long* level_strides, int L, const float* gt_bboxes, const float* centers2d,
                         const long long* gt_labels, const int32_t* img_off, int P, int G, int num_img, int num_classes, float alpha,
                         long long* labels, float* centerness, long long* gt_inds, long long* strides, int32_t* num_fg,
                         hipStream_t st);
int launch_obj_sample_weights(const uint8_t* fg_mask, const float* centerness, const long long* gt_inds, long long T,
                              const long long* sample_point_inds, int N, int num_uniform, float eps, long long* sample_gt_inds,
                              float* sample_weights, float* sample_uniform_weights, int32_t* num_fg, hipStream_t st);
// deform_kernels.hip: the detection head's deformable attention sampler (epropnp_deform_sample_forward / _backward): one launch each,
// one wave per (object, head); the backward zero-fills the map gradients it is given and scatters into them with float atomics
int launch_deform_forward(const float* query, const float* key, const float* value, const float* x2d, const float* mask,
                          const float* loc, const long long* img, int B, int NI, int H, int P, int D, int h, int w, int stride,
                          long long sN, long long sC, long long sH, long long sW, float* attn, float* v_out, float* a_out,
                          float* m_out, float* x_out, float* stats, hipStream_t st);
int launch_deform_backward(const float* query, const float* key, const float* value, const float* x2d, const float* mask,
                           const float* loc, const long long* img, const float* stats, const float* g_attn, const float* g_v,
                           const float* g_a, const float* g_m, const float* g_x, int B, int NI, int H, int P, int D, int h, int w,
                           int stride, long long sN, long long sC, long long sH, long long sW, float* dq, float* dkey,
                           float* dvalue, float* dloc, hipStream_t st);
// roi_kernels.hip: the cross-RoI logsumexp of the detection head's auxiliary losses (epropnp_roi_logsumexp_forward / _backward): one
// launch each, a workgroup per (RoI, channel); no atomics, every summation order fixed
int launch_roi_logsumexp_forward(const float* x, const float* rois, int n, int c, int rh, int rw, float* out, hipStream_t st);
int launch_roi_logsumexp_backward(const float* x, const float* rois, const float* out, const float* gout, int n, int c, int rh, int rw,
                                  float* gx, hipStream_t st);
// roi_align_kernels.hip: RoIAlign ('avg') of one or two maps of identical geometry (epropnp_roi_align_forward / _backward): one launch
// each; the backward gathers by destination and writes every element of the gradient maps once -- no zero fill, no atomics
int launch_roi_align_forward(const float* map0, const float* map1, const float* rois, int bn, int NI, int C, int h, int w, int ph, int pw,
                             float scale, int sampling, int aligned, long long sN, long long sC, long long sH, long long sW,
                             long long oN, long long oC, long long oH, long long oW, float* out0, float* out1, hipStream_t st);
int launch_roi_align_backward(const float* gout0, const float* gout1, const float* rois, int bn, int NI, int C, int h, int w, int ph,
                              int pw, float scale, int sampling, int aligned, long long sN, long long sC, long long sH, long long sW,
                              long long oN, long long oC, long long oH, long long oW, float* gmap0, float* gmap1, hipStream_t st);
// grad_w2d += grad_delta * d delta / d w2d for a threshold from AdaptiveHuberPnPCost (epropnp_problem.delta_stats); no-op without
int launch_delta_path(const epropnp_problem* prob, const float* gdelta, int nparts, float* gw2d, hipStream_t st);
// stream-ordered fill as a kernel (never hipMemsetAsync: eval_kernels.hip, fill_u32_kernel)
int launch_fill_u32(void* p, unsigned v, size_t words, hipStream_t st);
// The exchange scratch of the split LM solve and of the split AMIS forward start out as 0xffffffff words ("not yet written").  The
// one-call forward fills BOTH with one launch when the caller hands them over as one contiguous block (mc_forward.hip) and marks
// the range here; a launcher whose scratch lies inside the marked range skips its own fill.  Thread-local, valid for the duration
// of that one host call.
struct PrefilledRange { const char* lo; const char* hi; };
PrefilledRange& prefilled_exchange_range();      // mc_forward.hip
inline bool exchange_prefilled(const void* p, size_t bytes) {
  const PrefilledRange& r = prefilled_exchange_range();
  return r.lo != nullptr && (const char*)p >= r.lo && (const char*)p + bytes <= r.hi;
}
int launch_mc_loss_reduce(const float* loss, const float* weight, int B, float scale, float momentum, const float* nf_in,
                          int nf_count, long long nf_stride, float* nf, float* out, hipStream_t st);
int launch_exchange_pack(const float* rows, size_t row_floats, const float* scalars, int n_scal, const float* sum_src,
                         size_t sum_floats, float sum_scale, const float* row_w, int row_len, float* send, hipStream_t st);
int launch_mc_loss_reduce_backward(const float* logw, const float* lse, const float* weight, const float* coef,
                                   const float* gout, int S, int B, float* glogw, float* gct, hipStream_t st);
int launch_mc_loss_backward(const float* logw, const float* lse, const float* loss, const float* g, int S, int B,
                            float* glogw, float* gct, hipStream_t st);
struct StartSelect;      // lm_core.h
int launch_lm_solve(const epropnp_problem* prob, const epropnp_lm_params* lm, const float* pose_init, float* pose_opt,
                    float* pose_cov, float* cost, int32_t* accept_mask, void* split_scratch,
                    unsigned long long split_scratch_bytes, hipStream_t st, const StartSelect* select = nullptr);
unsigned long long lm_split_bytes(const epropnp_problem* prob, const epropnp_lm_params* lm);
// (one-call forward on a pnp_normalize'd problem: the AMIS launch also writes pose_opt and the samples in the caller's frame --
//  AmisParams.dn_* -- instead of a shift_poses_pair launch behind it)
struct DenormOut { const float* offset; float* samples; float* pose_opt; };
int launch_amis_forward(const epropnp_problem* prob, const epropnp_amis_params* amis, const float* pose_opt,
                        const float* pose_cov, const float* noise, float* pose_samples, float* logweights,
                        float* proposals, hipStream_t st, const DenormOut* dn = nullptr, float* sample_costs = nullptr);
int launch_amis_backward_split(const epropnp_problem* prob, const float* pose_samples, const float* grad_logweights,
                               int mc_samples, const float* pose_init, const float* grad_cost_init, int nsplit,
                               float* grad_x3d, float* grad_x2d, float* grad_w2d, float* grad_delta_parts, hipStream_t st,
                               const float* sample_costs = nullptr, const float* cost_init = nullptr);
int launch_amis_backward(const epropnp_problem* prob, const float* pose_samples, const float* grad_logweights,
                         int mc_samples, const float* pose_init, const float* grad_cost_init, float* grad_x3d,
                         float* grad_x2d, float* grad_w2d, float* grad_delta, hipStream_t st,
                         const float* sample_costs = nullptr, const float* cost_init = nullptr);

}  // namespace pnp
