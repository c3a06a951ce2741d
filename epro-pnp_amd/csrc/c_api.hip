// c_api.hip -- extern "C" surface of libepropnp_hip.so (declared in include/epropnp_hip.h).
#include <string.h>

#include <mutex>
#include <vector>

#include "pnp_host.h"

namespace pnp {
int tuning_phase_cycles(unsigned long long* out, int reset);          // amis_forward_mfma.hip / rslm_kernel.hip (tuning.h)
int tuning_rslm_phase_cycles(unsigned long long* out, int reset);
int tuning_bwd_phase_cycles(unsigned long long* out, int reset);
char* last_error_buffer() {
  static thread_local char buf[512] = {0};
  return buf;
}

// ---- per-stage HIP-event timing ------------------------------------------------------------------------------------
namespace {
struct StageRec { const char* stage; hipEvent_t e0, e1; bool closed; };
std::mutex g_prof_mu;
bool g_prof_on = false;
std::vector<StageRec> g_prof;          // records in use
std::vector<hipEvent_t> g_pool;        // events created ahead of time: no hipEventCreate inside a timed region
constexpr size_t kMaxStageRecs = 1 << 15;
void fill_pool(size_t want) {
  while (g_pool.size() < want) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) break;
    g_pool.push_back(e);
  }
}
void drop_records() {
  for (auto& r : g_prof) { g_pool.push_back(r.e0); g_pool.push_back(r.e1); }
  g_prof.clear();
}
}  // namespace
bool profile_begin(const char* stage, hipStream_t st) {
  if (!g_prof_on) return false;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (g_prof.size() >= kMaxStageRecs) return false;
  if (g_pool.size() < 2) fill_pool(64);
  if (g_pool.size() < 2) return false;
  StageRec r{stage, g_pool[g_pool.size() - 1], g_pool[g_pool.size() - 2], false};
  g_pool.resize(g_pool.size() - 2);
  (void)hipEventRecord(r.e0, st);
  g_prof.push_back(r);
  return true;
}
void profile_end(hipStream_t st) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (size_t i = g_prof.size(); i-- > 0;)
    if (!g_prof[i].closed) { (void)hipEventRecord(g_prof[i].e1, st); g_prof[i].closed = true; break; }
}
}  // namespace pnp

namespace pnp {
// The default status word: when a caller passes no `epropnp_problem.status`, kernels report numerical events (a singular
// damped system, a non-finite pose: what torch.linalg.solve / torch.inverse raise on in the reference,
// levenberg_marquardt.py:15-19,178-181) into a per-device int32[2] in HOST memory mapped into the device.  It costs nothing
// on the normal path (no event -> no memory operation) and lets the host side notice a failure with a plain load -- no
// synchronisation, no copy: the Python layer polls it on entry to every call and raises what the reference would have
// raised, one call late at most (`epropnp_async_status`).  EPROPNP_ASYNC_STATUS=0 switches it off.
static int32_t* g_status_words[64] = {nullptr};
static int g_status_mode = -1;

int32_t* default_status_word() {
  if (g_status_mode < 0) {
    const char* e = getenv("EPROPNP_ASYNC_STATUS");
    g_status_mode = (e != nullptr && e[0] == '0') ? 0 : 1;
  }
  if (g_status_mode == 0) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  int32_t* w = __atomic_load_n(&g_status_words[dev], __ATOMIC_ACQUIRE);
  if (w != nullptr) return w;
  // may be the first call of a process that is already capturing a graph: a host allocation is not a stream operation,
  // relax the thread's capture mode around it
  hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
  (void)hipThreadExchangeStreamCaptureMode(&mode);
  void* mem = nullptr;
  const hipError_t rc = hipHostMalloc(&mem, 2 * sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent);
  (void)hipThreadExchangeStreamCaptureMode(&mode);
  if (rc != hipSuccess) { (void)hipGetLastError(); g_status_mode = 0; return nullptr; }
  w = (int32_t*)mem;
  w[0] = 0;
  w[1] = INT32_MAX;
  int32_t* expected = nullptr;
  if (!__atomic_compare_exchange_n(&g_status_words[dev], &expected, w, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) {
    (void)hipHostFree(w);
    w = expected;
  }
  return w;
}
}  // namespace pnp

namespace pnp {
// epropnp_request_sample_costs: where the next forward entry of this host thread stores its samples' costs; taken (and forgotten)
// by that call whatever it returns
static thread_local float* g_requested_costs = nullptr;
static float* take_requested_costs() {
  float* p = g_requested_costs;
  g_requested_costs = nullptr;
  return p;
}
}  // namespace pnp

extern "C" {

int epropnp_request_sample_costs(float* sample_costs) {
  pnp::g_requested_costs = sample_costs;
  return EPROPNP_OK;
}

int32_t* epropnp_async_status_word(void) { return pnp::default_status_word(); }

int epropnp_async_status(int32_t* flags_and_first, int clear) {
  int32_t* w = pnp::default_status_word();
  const int32_t f = w ? __atomic_load_n(&w[0], __ATOMIC_RELAXED) : 0;
  const int32_t o = w ? __atomic_load_n(&w[1], __ATOMIC_RELAXED) : INT32_MAX;
  if (flags_and_first) { flags_and_first[0] = f; flags_and_first[1] = o; }
  if (w && clear) { __atomic_store_n(&w[0], 0, __ATOMIC_RELAXED); __atomic_store_n(&w[1], INT32_MAX, __ATOMIC_RELAXED); }
  return f;
}

int epropnp_abi_version(void) { return EPROPNP_ABI_VERSION; }

const char* epropnp_last_error(void) { return pnp::last_error_buffer(); }

uint64_t epropnp_amis_forward_split_bytes(const epropnp_problem* prob, int32_t mc_samples, int32_t num_iter) {
  return pnp::amis_forward_split_bytes(prob, mc_samples, num_iter);
}

// ---- launch plans: what the launchers would decide, from the same host functions; nothing is launched ----
static int plan_args_ok(const epropnp_problem* prob, const int32_t* out, const char* what) {
  if (int rc = pnp::check_plan_problem(prob)) return rc;
  if (out == nullptr) return pnp::fail(EPROPNP_EINVAL, "%s: out is NULL", what);
  return EPROPNP_OK;
}

int epropnp_plan_amis_forward(const epropnp_problem* prob, int32_t mc_samples, int32_t num_iter, int32_t has_scratch,
                              int32_t num_cus, int32_t* out) {
  if (int rc = plan_args_ok(prob, out, "plan_amis_forward")) return rc;
  if (num_iter <= 0 || mc_samples <= 0 || mc_samples % num_iter != 0)
    return pnp::fail(EPROPNP_EINVAL, "plan_amis_forward: mc_samples (%d) must be a positive multiple of num_iter (%d)", mc_samples, num_iter);
  pnp::PlanCuScope cus(num_cus);
  return pnp::plan_amis_forward_record(prob, mc_samples, num_iter, has_scratch ? ~0ull : 0ull, out);
}

int epropnp_plan_amis_backward(const epropnp_problem* prob, int32_t mc_samples, int32_t with_pose_init, int32_t num_split,
                               int32_t num_cus, int32_t* out) {
  if (int rc = plan_args_ok(prob, out, "plan_amis_backward")) return rc;
  if (mc_samples < 0 || num_split < 1 || num_split > 16)
    return pnp::fail(EPROPNP_EINVAL, "plan_amis_backward: mc_samples %d / num_split %d out of range", mc_samples, num_split);
  pnp::PlanCuScope cus(num_cus);
  return pnp::plan_amis_backward_record(prob, mc_samples, with_pose_init, num_split, out);
}

int epropnp_plan_evaluate_cost(const epropnp_problem* prob, int32_t num_cus, int32_t* out) {
  if (int rc = plan_args_ok(prob, out, "plan_evaluate_cost")) return rc;
  if (prob->num_pts > pnp::kMaxResidentPoints)
    return pnp::fail(EPROPNP_EINVAL, "plan_evaluate_cost: num_pts %d exceeds the register-resident limit %d", prob->num_pts,
                     pnp::kMaxResidentPoints);
  pnp::PlanCuScope cus(num_cus);
  const pnp::Shape s = pnp::cost_sweep_shape(prob->num_obj, prob->num_pts);
  out[0] = s.waves; out[1] = s.ppl;
  return EPROPNP_OK;
}

int epropnp_noise_stride(int dof) { return dof == 6 ? 8 : (dof == 4 ? 4 + 3 * 16 : -1); }

int epropnp_monte_carlo_forward(const epropnp_problem* prob, const epropnp_mc_params* par, const float* pose_init,
                                const float* noise, float* x3d_centered, float* offset, float* pose_init_n,
                                float* start_pose, float* start_cost, float* pose_opt_n, float* pose_cov, float* cost,
                                float* pose_samples_n, float* logweights, float* cost_init, float* pose_opt,
                                float* pose_samples, void* stream) {
  return pnp::launch_monte_carlo_forward(prob, par, pose_init, noise, x3d_centered, offset, pose_init_n, start_pose,
                                         start_cost, pose_opt_n, pose_cov, cost, pose_samples_n, logweights, cost_init,
                                         pose_opt, pose_samples, (hipStream_t)stream, nullptr, pnp::take_requested_costs());
}

int epropnp_monte_carlo_forward_diag(const epropnp_problem* prob, const epropnp_mc_params* par, const float* pose_init,
                                     const float* noise, float* x3d_centered, float* offset, float* pose_init_n,
                                     float* start_pose, float* start_cost, float* pose_opt_n, float* pose_cov, float* cost,
                                     float* pose_samples_n, float* logweights, float* cost_init, float* pose_opt,
                                     float* pose_samples, const epropnp_diag* diag, void* stream) {
  return pnp::launch_monte_carlo_forward(prob, par, pose_init, noise, x3d_centered, offset, pose_init_n, start_pose,
                                         start_cost, pose_opt_n, pose_cov, cost, pose_samples_n, logweights, cost_init,
                                         pose_opt, pose_samples, (hipStream_t)stream, diag, pnp::take_requested_costs());
}

int epropnp_weight_stats(const float* logweights, int32_t mc_samples, int32_t num_obj, int32_t num_iter, float* stats,
                         void* stream) {
  pnp::StageScope prof_("weight_stats", (hipStream_t)stream);
  return pnp::launch_weight_stats(logweights, mc_samples, num_obj, num_iter, stats, (hipStream_t)stream);
}

int epropnp_posterior_summary(const float* pose_samples, const float* logweights, const float* pose_ref, int32_t mc_samples,
                              int32_t num_obj, int32_t dof, float* summary, void* stream) {
  pnp::StageScope prof_("posterior_summary", (hipStream_t)stream);
  return pnp::launch_posterior_summary(pose_samples, logweights, pose_ref, mc_samples, num_obj, dof, summary, (hipStream_t)stream);
}

int epropnp_posterior_resample(const float* pose_samples, const float* logweights, int32_t mc_samples, int32_t num_obj,
                               int32_t dof, int32_t num_draws, const float* u, uint64_t seed, uint64_t offset, int32_t* index,
                               float* poses, void* stream) {
  pnp::StageScope prof_("posterior_resample", (hipStream_t)stream);
  return pnp::launch_posterior_resample(pose_samples, logweights, mc_samples, num_obj, dof, num_draws, u, seed, offset, index, poses,
                                        (hipStream_t)stream);
}

int epropnp_posterior_modes(const float* pose_samples, const float* logweights, const float* bandwidth, int32_t mc_samples,
                            int32_t num_obj, int32_t dof, float link, int32_t max_modes, float* density, int32_t* parent,
                            int32_t* labels, int32_t* num_modes, int32_t* mode_index, float* mode_mass, float* mode_poses,
                            void* stream) {
  pnp::StageScope prof_("posterior_modes", (hipStream_t)stream);
  return pnp::launch_posterior_modes(pose_samples, logweights, bandwidth, mc_samples, num_obj, dof, link, max_modes, density, parent,
                                     labels, num_modes, mode_index, mode_mass, mode_poses, (hipStream_t)stream);
}

int epropnp_pose_errors(const float* pose_est, const float* pose_gt, int32_t num_rows_per_obj, int32_t num_obj, int32_t dof,
                        const float* model_points, const int32_t* model_range, int32_t num_models, const int32_t* model_id,
                        const float* cam_mats, const uint8_t* symmetric, const uint8_t* half_turn, void* scratch,
                        size_t scratch_bytes, float* errors, void* stream) {
  pnp::StageScope prof_("pose_errors", (hipStream_t)stream);
  return pnp::launch_pose_errors(pose_est, pose_gt, num_rows_per_obj, num_obj, dof, model_points, model_range, num_models, model_id,
                                 cam_mats, symmetric, half_turn, scratch, scratch_bytes, errors, (hipStream_t)stream);
}

size_t epropnp_pose_errors_scratch_bytes(int32_t num_rows_per_obj, int32_t num_obj, int32_t max_model_points) {
  return pnp::pose_errors_scratch_bytes(num_rows_per_obj, num_obj, max_model_points);
}

int epropnp_bev_overlap(const float* boxes_a, int32_t num_a, const float* boxes_b, int32_t num_b, int32_t want_iou, int32_t aligned,
                        float* out, void* stream) {
  pnp::StageScope prof_("bev_overlap", (hipStream_t)stream);
  return pnp::launch_bev_overlap(boxes_a, num_a, boxes_b, num_b, want_iou, aligned, out, (hipStream_t)stream);
}

size_t epropnp_bev_nms_scratch_bytes(int32_t num_boxes) { return pnp::bev_nms_scratch_bytes(num_boxes); }

int epropnp_bev_nms(const float* boxes, const int32_t* order, const int32_t* group, int32_t num_boxes, float iou_thr, void* scratch,
                    size_t scratch_bytes, int32_t* keep_index, uint8_t* keep_mask, int32_t* num_keep, void* stream) {
  pnp::StageScope prof_("bev_nms", (hipStream_t)stream);
  return pnp::launch_bev_nms(boxes, order, group, num_boxes, iou_thr, scratch, scratch_bytes, keep_index, keep_mask, num_keep,
                             (hipStream_t)stream);
}

int epropnp_box_overlap(const float* boxes_a, int32_t num_a, const float* boxes_b, int32_t num_b, int32_t kind, int32_t criterion,
                        int32_t z_axis, float z_center, int32_t height_rule, int32_t aligned, float* out, void* stream) {
  pnp::StageScope prof_("box_overlap", (hipStream_t)stream);
  return pnp::launch_box_overlap(boxes_a, num_a, boxes_b, num_b, kind, criterion, z_axis, z_center, height_rule, aligned, out,
                                 (hipStream_t)stream);
}

int epropnp_box_overlap_plan(const int32_t* counts_a, const int32_t* counts_b, int32_t num_segments, int32_t* tiles,
                             int64_t tiles_capacity, int64_t* num_tiles, int64_t* num_out) {
  long long nt = 0, no = 0;
  const int rc = pnp::box_overlap_plan(counts_a, counts_b, num_segments, tiles, tiles_capacity, &nt, &no);
  if (rc == EPROPNP_OK && num_tiles) *num_tiles = nt;
  if (rc == EPROPNP_OK && num_out) *num_out = no;
  return rc;
}

int epropnp_box_overlap_segmented(const float* boxes_a, int32_t num_a, const float* boxes_b, int32_t num_b, int32_t kind,
                                  int32_t criterion, int32_t z_axis, float z_center, int32_t height_rule, const int32_t* tiles,
                                  int32_t num_tiles, float* out, int64_t num_out, void* stream) {
  pnp::StageScope prof_("box_overlap_segmented", (hipStream_t)stream);
  return pnp::launch_box_overlap_segmented(boxes_a, num_a, boxes_b, num_b, kind, criterion, z_axis, z_center, height_rule, tiles,
                                           num_tiles, out, num_out, (hipStream_t)stream);
}

size_t epropnp_kitti_match_scratch_bytes(int32_t num_dt, int32_t num_cases) { return pnp::kitti_match_scratch_bytes(num_dt, num_cases); }

// eval.py:166-284 with compute_fp=False, every case and image
int epropnp_kitti_match(const void* overlaps, int32_t overlaps_fp64, int64_t num_overlaps, const int32_t* gt_offsets,
                        const int32_t* dt_offsets, const int64_t* block_offsets, int32_t num_images, const double* dt_data,
                        int32_t num_gt, int32_t num_dt, const int8_t* ignored_gt, const int8_t* ignored_det, const double* min_overlap,
                        int32_t num_cases, void* scratch, size_t scratch_bytes, double* tp_scores, int32_t* tp_count, int8_t* gt_state,
                        void* stream) {
  pnp::StageScope prof_("kitti_match", (hipStream_t)stream);
  return pnp::launch_kitti_match(overlaps, overlaps_fp64, (long long)num_overlaps, gt_offsets, dt_offsets, (const long long*)block_offsets,
                                 num_images, dt_data, num_gt, num_dt, ignored_gt, ignored_det, min_overlap, num_cases, scratch,
                                 scratch_bytes, tp_scores, tp_count, gt_state, (hipStream_t)stream);
}

// eval.py:12-30, every case
int epropnp_kitti_thresholds(const double* sorted_scores, const int32_t* tp_count, const int32_t* num_valid_gt, int32_t num_gt,
                             int32_t num_cases, double recall_step, double* thresholds, int32_t* thr_count, void* stream) {
  pnp::StageScope prof_("kitti_thresholds", (hipStream_t)stream);
  return pnp::launch_kitti_thresholds(sorted_scores, tp_count, num_valid_gt, num_gt, num_cases, recall_step, thresholds, thr_count,
                                      (hipStream_t)stream);
}

size_t epropnp_kitti_statistics_scratch_bytes(int32_t num_images, int32_t num_dt, int32_t num_cases, int32_t compute_aos) {
  return pnp::kitti_statistics_scratch_bytes(num_images, num_dt, num_cases, compute_aos);
}

// eval.py:166-284 with compute_fp=True under every threshold, summed over the images as eval.py:296-343 does
int epropnp_kitti_statistics(const void* overlaps, int32_t overlaps_fp64, int64_t num_overlaps, const int32_t* gt_offsets,
                             const int32_t* dt_offsets, const int32_t* dc_offsets, const int64_t* block_offsets, int32_t num_images,
                             const double* gt_data, const double* dt_data, const double* dc_boxes, int32_t num_gt, int32_t num_dt,
                             int32_t num_dc, const int8_t* ignored_gt, const int8_t* ignored_det, const double* min_overlap,
                             int32_t num_cases, const double* thresholds, const int32_t* thr_count, int32_t metric, int32_t compute_aos,
                             void* scratch, size_t scratch_bytes, double* pr, double* tp_scores, void* stream) {
  pnp::StageScope prof_("kitti_statistics", (hipStream_t)stream);
  return pnp::launch_kitti_statistics(overlaps, overlaps_fp64, (long long)num_overlaps, gt_offsets, dt_offsets, dc_offsets,
                                      (const long long*)block_offsets, num_images, gt_data, dt_data, dc_boxes, num_gt, num_dt, num_dc,
                                      ignored_gt, ignored_det, min_overlap, num_cases, thresholds, thr_count, metric, compute_aos, scratch,
                                      scratch_bytes, pr, tp_scores, (hipStream_t)stream);
}

size_t epropnp_orient_density_scratch_bytes(int32_t mc_samples, int32_t num_obj) {
  return pnp::orient_density_scratch_bytes(mc_samples, num_obj);
}

int epropnp_orient_density(const float* pose_samples, const float* logweights, const float* pose_opt, int32_t mc_samples,
                           int32_t num_obj, int32_t dof, int32_t size, int32_t window_h, int32_t window_w, float saturation,
                           float sphere_opacity, float intensity_scale, void* scratch, size_t scratch_bytes, float* image,
                           float* front, float* back, int32_t* bins, void* stream) {
  pnp::StageScope prof_("orient_density", (hipStream_t)stream);
  return pnp::launch_orient_density(pose_samples, logweights, pose_opt, mc_samples, num_obj, dof, size, window_h, window_w, saturation,
                                    sphere_opacity, intensity_scale, scratch, scratch_bytes, image, front, back, bins,
                                    (hipStream_t)stream);
}

size_t epropnp_bev_density_scratch_bytes(int32_t mc_samples, int32_t num_obj) {
  return pnp::bev_density_scratch_bytes(mc_samples, num_obj);
}

int epropnp_bev_density(const float* pose_samples, const float* logweights, const float* obj_weight, const int32_t* obj_offsets,
                        int32_t mc_samples, int32_t num_obj, int32_t num_groups, int32_t dof, int32_t height, int32_t width,
                        float scale, int32_t origin_x, int32_t origin_y, int32_t window, void* scratch, size_t scratch_bytes,
                        float* density, int32_t* bins, void* stream) {
  pnp::StageScope prof_("bev_density", (hipStream_t)stream);
  return pnp::launch_bev_density(pose_samples, logweights, obj_weight, obj_offsets, mc_samples, num_obj, num_groups, dof, height,
                                 width, scale, origin_x, origin_y, window, scratch, scratch_bytes, density, bins, (hipStream_t)stream);
}

size_t epropnp_volume_centers_scratch_bytes(int32_t num_obj, int32_t h_out, int32_t w_out) {
  return pnp::volume_centers_scratch_bytes(num_obj, h_out, w_out);
}

// center_target.py:42-259 (VolumeCenter.get_centers_2d + post_proc, box mesh) without a render
int epropnp_volume_centers(const float* bboxes_3d, const float* bboxes_2d_in, const int32_t* obj_offsets, const float* cam_intrinsic,
                           const float* dense_x2d, const float* dense_mask, int32_t num_obj, int32_t num_img, int32_t h_out,
                           int32_t w_out, int32_t h_rend, int32_t w_rend, int32_t output_stride, int32_t render_stride,
                           int32_t faces_per_pixel, float z_clip, float min_box_size, int32_t get_bbox_2d, void* scratch,
                           size_t scratch_bytes, float* centers_2d, float* bboxes_2d, uint8_t* valid, void* stream) {
  pnp::StageScope prof_("volume_centers", (hipStream_t)stream);
  return pnp::launch_volume_centers(bboxes_3d, bboxes_2d_in, obj_offsets, cam_intrinsic, dense_x2d, dense_mask, num_obj, num_img, h_out,
                                    w_out, h_rend, w_rend, output_stride, render_stride, faces_per_pixel, z_clip, min_box_size,
                                    get_bbox_2d, scratch, scratch_bytes, centers_2d, bboxes_2d, valid, (hipStream_t)stream);
}

int epropnp_box_thickness(const float* bboxes_3d, const int32_t* obj_offsets, const float* cam_intrinsic, int32_t num_obj,
                          int32_t num_img, int32_t h_rend, int32_t w_rend, int32_t render_stride, int32_t faces_per_pixel, float z_clip,
                          void* scratch, size_t scratch_bytes, float* thickness, uint8_t* valid, void* stream) {
  pnp::StageScope prof_("box_thickness", (hipStream_t)stream);
  return pnp::launch_box_thickness(bboxes_3d, obj_offsets, cam_intrinsic, num_obj, num_img, h_rend, w_rend, render_stride,
                                   faces_per_pixel, z_clip, scratch, scratch_bytes, thickness, valid, (hipStream_t)stream);
}

// fcos_emb_head.py:299-438 (FCOSEmbHead.get_targets) in one pass over (image, point), outputs in the flattened level-major order
int epropnp_point_targets(const float* points, const int32_t* lvl_offsets, const float* radius_px, const float* regress_lo,
                          const float* regress_hi, const int64_t* level_strides, int32_t num_levels, const float* gt_bboxes,
                          const float* centers2d, const int64_t* gt_labels, const int32_t* img_offsets, int32_t num_points,
                          int32_t num_gt, int32_t num_img, int32_t num_classes, float centerness_alpha, int64_t* labels,
                          float* centerness_targets, int64_t* gt_inds, int64_t* strides, int32_t* num_fg, void* stream) {
  pnp::StageScope prof_("point_targets", (hipStream_t)stream);
  return pnp::launch_point_targets(points, lvl_offsets, radius_px, regress_lo, regress_hi, (const long long*)level_strides, num_levels,
                                   gt_bboxes, centers2d, (const long long*)gt_labels, img_offsets, num_points, num_gt, num_img,
                                   num_classes, centerness_alpha, (long long*)labels, centerness_targets, (long long*)gt_inds,
                                   (long long*)strides, num_fg, (hipStream_t)stream);
}

// deform_pnp_head.py:1148-1174 (obj_sampler behind its draws)
int epropnp_obj_sample_weights(const uint8_t* fg_mask, const float* centerness_targets, const int64_t* gt_inds,
                               int64_t num_total_point, const int64_t* sample_point_inds, int32_t num_obj_samples,
                               int32_t num_uniform, float eps, int64_t* sample_gt_inds, float* sample_weights,
                               float* sample_uniform_weights, int32_t* num_fg, void* stream) {
  pnp::StageScope prof_("obj_sample_weights", (hipStream_t)stream);
  return pnp::launch_obj_sample_weights(fg_mask, centerness_targets, (const long long*)gt_inds, (long long)num_total_point,
                                        (const long long*)sample_point_inds, num_obj_samples, num_uniform, eps,
                                        (long long*)sample_gt_inds, sample_weights, sample_uniform_weights, num_fg,
                                        (hipStream_t)stream);
}

int epropnp_deform_sample_forward(const float* query, const float* key, const float* value, const float* dense_x2d,
                                  const float* dense_mask, const float* sampling_location, const int64_t* obj_img_ind,
                                  int32_t num_obj, int32_t num_img, int32_t num_heads, int32_t num_points, int32_t head_dim,
                                  int32_t height, int32_t width, int32_t stride, int64_t stride_n, int64_t stride_c,
                                  int64_t stride_h, int64_t stride_w, float* attn, float* v_samples, float* a_samples,
                                  float* mask_samples, float* x2d_samples, float* stats, void* stream) {
  pnp::StageScope prof_("deform_sample_forward", (hipStream_t)stream);
  return pnp::launch_deform_forward(query, key, value, dense_x2d, dense_mask, sampling_location, (const long long*)obj_img_ind, num_obj,
                                    num_img, num_heads, num_points, head_dim, height, width, stride, stride_n, stride_c, stride_h,
                                    stride_w, attn, v_samples, a_samples, mask_samples, x2d_samples, stats, (hipStream_t)stream);
}

int epropnp_deform_sample_backward(const float* query, const float* key, const float* value, const float* dense_x2d,
                                   const float* dense_mask, const float* sampling_location, const int64_t* obj_img_ind,
                                   const float* stats, const float* grad_attn, const float* grad_v_samples,
                                   const float* grad_a_samples, const float* grad_mask_samples, const float* grad_x2d_samples,
                                   int32_t num_obj, int32_t num_img, int32_t num_heads, int32_t num_points, int32_t head_dim,
                                   int32_t height, int32_t width, int32_t stride, int64_t stride_n, int64_t stride_c,
                                   int64_t stride_h, int64_t stride_w, float* grad_query, float* grad_key, float* grad_value,
                                   float* grad_location, void* stream) {
  pnp::StageScope prof_("deform_sample_backward", (hipStream_t)stream);
  return pnp::launch_deform_backward(query, key, value, dense_x2d, dense_mask, sampling_location, (const long long*)obj_img_ind, stats,
                                     grad_attn, grad_v_samples, grad_a_samples, grad_mask_samples, grad_x2d_samples, num_obj, num_img,
                                     num_heads, num_points, head_dim, height, width, stride, stride_n, stride_c, stride_h, stride_w,
                                     grad_query, grad_key, grad_value, grad_location, (hipStream_t)stream);
}

int epropnp_roi_logsumexp_forward(const float* roi_inputs, const float* rois, int32_t num_rois, int32_t channels, int32_t roi_height,
                                  int32_t roi_width, float* out, void* stream) {
  pnp::StageScope prof_("roi_logsumexp_forward", (hipStream_t)stream);
  return pnp::launch_roi_logsumexp_forward(roi_inputs, rois, num_rois, channels, roi_height, roi_width, out, (hipStream_t)stream);
}

int epropnp_roi_logsumexp_backward(const float* roi_inputs, const float* rois, const float* out, const float* grad_out, int32_t num_rois,
                                   int32_t channels, int32_t roi_height, int32_t roi_width, float* grad_inputs, void* stream) {
  pnp::StageScope prof_("roi_logsumexp_backward", (hipStream_t)stream);
  return pnp::launch_roi_logsumexp_backward(roi_inputs, rois, out, grad_out, num_rois, channels, roi_height, roi_width, grad_inputs,
                                            (hipStream_t)stream);
}

int epropnp_roi_align_forward(const float* map0, const float* map1, const float* rois, int32_t num_rois, int32_t num_img,
                              int32_t channels, int32_t height, int32_t width, int32_t out_height, int32_t out_width,
                              float spatial_scale, int32_t sampling_ratio, int32_t aligned, int64_t map_stride_n, int64_t map_stride_c,
                              int64_t map_stride_h, int64_t map_stride_w, int64_t out_stride_n, int64_t out_stride_c,
                              int64_t out_stride_h, int64_t out_stride_w, float* out0, float* out1, void* stream) {
  pnp::StageScope prof_("roi_align_forward", (hipStream_t)stream);
  return pnp::launch_roi_align_forward(map0, map1, rois, num_rois, num_img, channels, height, width, out_height, out_width, spatial_scale,
                                       sampling_ratio, aligned, map_stride_n, map_stride_c, map_stride_h, map_stride_w, out_stride_n,
                                       out_stride_c, out_stride_h, out_stride_w, out0, out1, (hipStream_t)stream);
}

int epropnp_roi_align_backward(const float* grad_out0, const float* grad_out1, const float* rois, int32_t num_rois, int32_t num_img,
                               int32_t channels, int32_t height, int32_t width, int32_t out_height, int32_t out_width,
                               float spatial_scale, int32_t sampling_ratio, int32_t aligned, int64_t map_stride_n, int64_t map_stride_c,
                               int64_t map_stride_h, int64_t map_stride_w, int64_t out_stride_n, int64_t out_stride_c,
                               int64_t out_stride_h, int64_t out_stride_w, float* grad_map0, float* grad_map1, void* stream) {
  pnp::StageScope prof_("roi_align_backward", (hipStream_t)stream);
  return pnp::launch_roi_align_backward(grad_out0, grad_out1, rois, num_rois, num_img, channels, height, width, out_height, out_width,
                                        spatial_scale, sampling_ratio, aligned, map_stride_n, map_stride_c, map_stride_h, map_stride_w,
                                        out_stride_n, out_stride_c, out_stride_h, out_stride_w, grad_map0, grad_map1, (hipStream_t)stream);
}

int epropnp_evaluate_cost(const epropnp_problem* prob, const float* poses, int32_t num_poses, float* cost, void* stream) {
  pnp::StageScope prof_("evaluate_cost", (hipStream_t)stream);
  return pnp::launch_evaluate_cost(prob, poses, num_poses, cost, (hipStream_t)stream);
}

int epropnp_cost_pose_cam_grad(const epropnp_problem* prob, const float* poses, const float* weights, int32_t num_poses,
                               int32_t m_pose, float* grad_h_outer, float* grad_cam, void* stream) {
  pnp::StageScope prof_("cost_pose_cam_grad", (hipStream_t)stream);
  return pnp::launch_cost_pose_cam_grad(prob, poses, weights, num_poses, m_pose, grad_h_outer, grad_cam, (hipStream_t)stream);
}

int epropnp_normal_equations(const epropnp_problem* prob, const float* pose, int32_t clip_jac, float* jtj, float* jtr,
                             float* cost, void* stream) {
  pnp::StageScope prof_("normal_equations", (hipStream_t)stream);
  return pnp::launch_normal_equations(prob, pose, clip_jac, jtj, jtr, cost, (hipStream_t)stream);
}

int epropnp_lm_solve(const epropnp_problem* prob, const epropnp_lm_params* lm, const float* pose_init, float* pose_opt,
                     float* pose_cov, float* cost, int32_t* accept_mask, void* split_scratch, uint64_t split_scratch_bytes,
                     void* stream) {
  pnp::StageScope prof_("lm_solve", (hipStream_t)stream);
  return pnp::launch_lm_solve(prob, lm, pose_init, pose_opt, pose_cov, cost, accept_mask, split_scratch, split_scratch_bytes,
                              (hipStream_t)stream);
}

uint64_t epropnp_lm_solve_split_bytes(const epropnp_problem* prob, const epropnp_lm_params* lm) {
  return pnp::lm_split_bytes(prob, lm);
}

int epropnp_amis_forward(const epropnp_problem* prob, const epropnp_amis_params* amis, const float* pose_opt,
                         const float* pose_cov, const float* noise, float* pose_samples, float* logweights,
                         float* proposals, void* stream) {
  pnp::StageScope prof_("amis_forward", (hipStream_t)stream);
  return pnp::launch_amis_forward(prob, amis, pose_opt, pose_cov, noise, pose_samples, logweights, proposals,
                                  (hipStream_t)stream, nullptr, pnp::take_requested_costs());
}

int epropnp_amis_backward(const epropnp_problem* prob, const float* pose_samples, const float* grad_logweights,
                          int32_t mc_samples, const float* pose_init, const float* grad_cost_init, float* grad_x3d,
                          float* grad_x2d, float* grad_w2d, float* grad_delta, void* stream) {
  pnp::StageScope prof_("amis_backward", (hipStream_t)stream);
  return pnp::launch_amis_backward(prob, pose_samples, grad_logweights, mc_samples, pose_init, grad_cost_init, grad_x3d,
                                   grad_x2d, grad_w2d, grad_delta, (hipStream_t)stream);
}

int epropnp_amis_backward_split(const epropnp_problem* prob, const float* pose_samples, const float* grad_logweights,
                                int32_t mc_samples, const float* pose_init, const float* grad_cost_init, int32_t num_split,
                                float* grad_x3d, float* grad_x2d, float* grad_w2d, float* grad_delta_parts, void* stream) {
  pnp::StageScope prof_("amis_backward", (hipStream_t)stream);
  return pnp::launch_amis_backward_split(prob, pose_samples, grad_logweights, mc_samples, pose_init, grad_cost_init,
                                         num_split, grad_x3d, grad_x2d, grad_w2d, grad_delta_parts, (hipStream_t)stream);
}

int epropnp_amis_forward_costs(const epropnp_problem* prob, const epropnp_amis_params* amis, const float* pose_opt,
                               const float* pose_cov, const float* noise, float* pose_samples, float* logweights,
                               float* proposals, float* sample_costs, void* stream) {
  (void)pnp::take_requested_costs();      // (an explicit output: a pending request is dropped, not carried to a later call)
  pnp::StageScope prof_("amis_forward", (hipStream_t)stream);
  return pnp::launch_amis_forward(prob, amis, pose_opt, pose_cov, noise, pose_samples, logweights, proposals,
                                  (hipStream_t)stream, nullptr, sample_costs);
}

int epropnp_monte_carlo_forward_costs(const epropnp_problem* prob, const epropnp_mc_params* par, const float* pose_init,
                                      const float* noise, float* x3d_centered, float* offset, float* pose_init_n,
                                      float* start_pose, float* start_cost, float* pose_opt_n, float* pose_cov, float* cost,
                                      float* pose_samples_n, float* logweights, float* cost_init, float* pose_opt,
                                      float* pose_samples, const epropnp_diag* diag, float* sample_costs, void* stream) {
  (void)pnp::take_requested_costs();
  return pnp::launch_monte_carlo_forward(prob, par, pose_init, noise, x3d_centered, offset, pose_init_n, start_pose,
                                         start_cost, pose_opt_n, pose_cov, cost, pose_samples_n, logweights, cost_init,
                                         pose_opt, pose_samples, (hipStream_t)stream, diag, sample_costs);
}

int epropnp_amis_backward_costs(const epropnp_problem* prob, const float* pose_samples, const float* grad_logweights,
                                int32_t mc_samples, const float* pose_init, const float* grad_cost_init,
                                const float* sample_costs, const float* cost_init, float* grad_x3d, float* grad_x2d,
                                float* grad_w2d, float* grad_delta, void* stream) {
  pnp::StageScope prof_("amis_backward", (hipStream_t)stream);
  return pnp::launch_amis_backward(prob, pose_samples, grad_logweights, mc_samples, pose_init, grad_cost_init, grad_x3d,
                                   grad_x2d, grad_w2d, grad_delta, (hipStream_t)stream, sample_costs, cost_init);
}

int epropnp_amis_backward_split_costs(const epropnp_problem* prob, const float* pose_samples, const float* grad_logweights,
                                      int32_t mc_samples, const float* pose_init, const float* grad_cost_init, int32_t num_split,
                                      const float* sample_costs, const float* cost_init, float* grad_x3d, float* grad_x2d,
                                      float* grad_w2d, float* grad_delta_parts, void* stream) {
  pnp::StageScope prof_("amis_backward", (hipStream_t)stream);
  return pnp::launch_amis_backward_split(prob, pose_samples, grad_logweights, mc_samples, pose_init, grad_cost_init,
                                         num_split, grad_x3d, grad_x2d, grad_w2d, grad_delta_parts, (hipStream_t)stream,
                                         sample_costs, cost_init);
}

int epropnp_adaptive_delta(const float* x2d, const float* w2d, int32_t num_obj, int32_t num_pts, float relative_delta,
                           float* delta, float* stats, void* stream) {
  pnp::StageScope prof_("adaptive_delta", (hipStream_t)stream);
  return pnp::launch_adaptive_delta(x2d, w2d, num_obj, num_pts, relative_delta, delta, stats, (hipStream_t)stream);
}

int epropnp_mc_loss_forward(const float* logweights, const float* cost_target, int32_t mc_samples, int32_t num_obj,
                            float* loss, float* lse, void* stream) {
  pnp::StageScope prof_("mc_loss_forward", (hipStream_t)stream);
  return pnp::launch_mc_loss_forward(logweights, cost_target, mc_samples, num_obj, loss, lse, (hipStream_t)stream);
}

int epropnp_mc_loss_backward(const float* logweights, const float* lse, const float* loss, const float* grad_loss,
                             int32_t mc_samples, int32_t num_obj, float* grad_logweights, float* grad_cost_target,
                             void* stream) {
  pnp::StageScope prof_("mc_loss_backward", (hipStream_t)stream);
  return pnp::launch_mc_loss_backward(logweights, lse, loss, grad_loss, mc_samples, num_obj, grad_logweights,
                                      grad_cost_target, (hipStream_t)stream);
}

int epropnp_mc_loss_reduce(const float* loss, const float* weight, int32_t num_obj, float scale, float momentum,
                           const float* norm_factor_in, int32_t norm_factor_in_count, int64_t norm_factor_in_stride,
                           float* norm_factor, float* out, void* stream) {
  pnp::StageScope prof_("mc_loss_reduce", (hipStream_t)stream);
  return pnp::launch_mc_loss_reduce(loss, weight, num_obj, scale, momentum, norm_factor_in, norm_factor_in_count,
                                    (long long)norm_factor_in_stride, norm_factor, out, (hipStream_t)stream);
}

int epropnp_exchange_pack(const float* rows, uint64_t row_floats, const float* scalars, int32_t n_scalars,
                          const float* sum_src, uint64_t sum_floats, float sum_scale, const float* sum_row_weight,
                          int32_t sum_row_len, float* send, void* stream) {
  return pnp::launch_exchange_pack(rows, (size_t)row_floats, scalars, n_scalars, sum_src, (size_t)sum_floats, sum_scale,
                                   sum_row_weight, sum_row_len, send, (hipStream_t)stream);
}

int epropnp_mc_loss_reduce_backward(const float* logweights, const float* lse, const float* weight, const float* coef,
                                    const float* grad_out, int32_t mc_samples, int32_t num_obj, float* grad_logweights,
                                    float* grad_cost_target, void* stream) {
  pnp::StageScope prof_("mc_loss_backward", (hipStream_t)stream);
  return pnp::launch_mc_loss_reduce_backward(logweights, lse, weight, coef, grad_out, mc_samples, num_obj, grad_logweights,
                                             grad_cost_target, (hipStream_t)stream);
}

int epropnp_rslm_draw(const float* w2d, int32_t num_obj, int32_t num_pts, int32_t num_proposals, int32_t n_pts,
                      uint64_t seed, uint64_t offset, int64_t* inds, void* stream) {
  return pnp::launch_rslm_draw(w2d, num_obj, num_pts, num_proposals, n_pts, seed, offset, (long long*)inds,
                               (hipStream_t)stream);
}

int epropnp_gn_step_forward(const epropnp_problem* prob, float eps, const float* pose, float* step, void* stream) {
  pnp::StageScope prof_("gn_step_forward", (hipStream_t)stream);
  return pnp::launch_gn_step_forward(prob, eps, pose, step, nullptr, (hipStream_t)stream);
}

int epropnp_gn_step_backward(const epropnp_problem* prob, float eps, const float* pose, const float* grad_step,
                             float* grad_x3d, float* grad_x2d, float* grad_w2d, float* grad_delta, void* stream) {
  pnp::StageScope prof_("gn_step_backward", (hipStream_t)stream);
  return pnp::launch_gn_step_backward(prob, eps, pose, grad_step, nullptr, grad_x3d, grad_x2d, grad_w2d, grad_delta,
                                      (hipStream_t)stream);
}

int epropnp_shift_poses_backward(const float* pose, const float* offset, const float* grad_out, int32_t num_poses,
                                 int32_t num_obj, int32_t dof, float sign, float* grad_pose, void* stream) {
  return pnp::launch_shift_poses_backward(pose, offset, grad_out, num_poses, num_obj, dof, sign, grad_pose,
                                          (hipStream_t)stream);
}

int epropnp_pose_opt_plus_forward(const epropnp_problem* prob, float eps, const float* pose, float* pose_plus,
                                  void* stream) {
  pnp::StageScope prof_("gn_step_forward", (hipStream_t)stream);
  return pnp::launch_gn_step_forward(prob, eps, pose, nullptr, pose_plus, (hipStream_t)stream);
}

int epropnp_pose_opt_plus_backward(const epropnp_problem* prob, float eps, const float* pose, const float* grad_pose_plus,
                                   float* grad_x3d, float* grad_x2d, float* grad_w2d, float* grad_delta, void* stream) {
  pnp::StageScope prof_("gn_step_backward", (hipStream_t)stream);
  return pnp::launch_gn_step_backward(prob, eps, pose, nullptr, grad_pose_plus, grad_x3d, grad_x2d, grad_w2d, grad_delta,
                                      (hipStream_t)stream);
}

int epropnp_rslm_solve(const epropnp_problem* prob, const epropnp_lm_params* lm, int32_t num_proposals,
                       int32_t num_points, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                       const int64_t* inds, const float* rot, float* pose, float* cost, void* scratch,
                       uint64_t scratch_bytes, void* stream) {
  pnp::StageScope prof_("rslm_solve", (hipStream_t)stream);
  return pnp::launch_rslm_solve(prob, lm, num_proposals, num_points, seed, offset, (const unsigned long long*)offset_dev,
                                (const long long*)inds, rot, pose, cost, scratch, scratch_bytes, (hipStream_t)stream);
}

int epropnp_rslm_solve_diag(const epropnp_problem* prob, const epropnp_lm_params* lm, int32_t num_proposals,
                            int32_t num_points, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                            const int64_t* inds, const float* rot, float* pose, float* cost, void* scratch,
                            uint64_t scratch_bytes, int32_t* winner, void* stream) {
  pnp::StageScope prof_("rslm_solve", (hipStream_t)stream);
  return pnp::launch_rslm_solve(prob, lm, num_proposals, num_points, seed, offset, (const unsigned long long*)offset_dev,
                                (const long long*)inds, rot, pose, cost, scratch, scratch_bytes, (hipStream_t)stream, nullptr,
                                nullptr, nullptr, nullptr, winner);
}

uint64_t epropnp_rslm_solve_scratch_bytes(const epropnp_problem* prob, int32_t num_proposals) {
  return pnp::rslm_scratch_bytes(prob, num_proposals);
}

int epropnp_center_points(const float* x3d, int32_t num_obj, int32_t num_pts, float* offset, float* x3d_centered,
                          void* stream) {
  pnp::StageScope prof_("center_points", (hipStream_t)stream);
  return pnp::launch_center_points(x3d, num_obj, num_pts, offset, x3d_centered, (hipStream_t)stream);
}

int epropnp_shift_poses(const float* pose, const float* offset, int32_t num_poses, int32_t num_obj, int32_t dof,
                        float sign, float* out, void* stream) {
  pnp::StageScope prof_("shift_poses", (hipStream_t)stream);
  return pnp::launch_shift_poses(pose, offset, num_poses, num_obj, dof, sign, out, (hipStream_t)stream);
}

int epropnp_prepare_forward(const float* noc, const float* dim, const float* logits, const float* scale,
                            int32_t num_obj, int32_t num_pts, int32_t mode, float* x3d, float* w2d, float* stats,
                            void* stream) {
  return pnp::launch_prepare_forward(noc, dim, logits, scale, num_obj, num_pts, mode, x3d, w2d, stats, (hipStream_t)stream);
}

int epropnp_prepare_backward(const float* noc, const float* dim, const float* logits, const float* scale,
                             const float* stats, const float* grad_x3d, const float* grad_w2d, int32_t num_obj,
                             int32_t num_pts, int32_t mode, float* grad_noc, float* grad_dim, float* grad_logits,
                             float* grad_scale, void* stream) {
  return pnp::launch_prepare_backward(noc, dim, logits, scale, stats, grad_x3d, grad_w2d, num_obj, num_pts, mode, grad_noc,
                                      grad_dim, grad_logits, grad_scale, (hipStream_t)stream);
}

int epropnp_prepare_dense_forward(const float* noc_map, const float* dim, const float* logit_map, const float* scale,
                                  const float* box, const int64_t* inds, int32_t num_obj, int32_t num_pts, int32_t height,
                                  int32_t width, int32_t mode, float* x3d, float* x2d, float* w2d, float* stats,
                                  void* stream) {
  return pnp::launch_prepare_dense_forward(noc_map, dim, logit_map, scale, box, (const long long*)inds, num_obj, num_pts,
                                           height, width, mode, x3d, x2d, w2d, stats, (hipStream_t)stream);
}

int epropnp_prepare_dense_backward(const float* noc_map, const float* dim, const float* logit_map, const float* scale,
                                   const int64_t* inds, const float* stats, const float* grad_x3d, const float* grad_w2d,
                                   int32_t num_obj, int32_t num_pts, int32_t height, int32_t width, int32_t mode,
                                   float* grad_noc_map, float* grad_dim, float* grad_logit_map, float* grad_scale,
                                   void* stream) {
  return pnp::launch_prepare_dense_backward(noc_map, dim, logit_map, scale, (const long long*)inds, stats, grad_x3d, grad_w2d,
                                            num_obj, num_pts, height, width, mode, grad_noc_map, grad_dim, grad_logit_map,
                                            grad_scale, (hipStream_t)stream);
}

int epropnp_profile_enable(int on) {
  std::lock_guard<std::mutex> lk(pnp::g_prof_mu);
  if (on) pnp::fill_pool(8192);        // 4096 stage launches before anything is created inside a timed region
  pnp::g_prof_on = on != 0;
  return EPROPNP_OK;
}

int epropnp_profile_reset(void) {
  std::lock_guard<std::mutex> lk(pnp::g_prof_mu);
  pnp::drop_records();
  return EPROPNP_OK;
}

int epropnp_profile_read(const char* stage, float* mean_ms, int32_t* count) {
  if (!stage || !mean_ms || !count) return pnp::fail(EPROPNP_EINVAL, "profile_read: NULL argument");
  *mean_ms = 0.f;
  *count = 0;
  std::lock_guard<std::mutex> lk(pnp::g_prof_mu);
  double sum = 0.0;
  for (auto& r : pnp::g_prof) {
    if (!r.closed || strcmp(r.stage, stage) != 0) continue;
    if (hipEventSynchronize(r.e1) != hipSuccess) return pnp::fail(EPROPNP_ELAUNCH, "profile_read: event synchronise failed");
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) continue;
    sum += ms;
    ++*count;
  }
  if (*count > 0) *mean_ms = (float)(sum / *count);
  return EPROPNP_OK;
}

// Not part of the ABI (tools/tune.py): per-phase shader-clock totals of amis_forward_mfma_kernel / rslm_solve_kernel in a tuning
// build (build.py -D PNP_TUNING); -1 in the product build, whose kernels carry no counters.
int epropnp_tuning_phase_cycles(unsigned long long* out, int reset) { return pnp::tuning_phase_cycles(out, reset); }
int epropnp_tuning_rslm_cycles(unsigned long long* out, int reset) { return pnp::tuning_rslm_phase_cycles(out, reset); }
int epropnp_tuning_bwd_cycles(unsigned long long* out, int reset) { return pnp::tuning_bwd_phase_cycles(out, reset); }

}  // extern "C"
