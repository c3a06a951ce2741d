// kitti_eval_kernels.hip -- the KITTI AP evaluation behind the per-image overlap blocks (epropnp_kitti_match, epropnp_kitti_thresholds,
// epropnp_kitti_statistics): greedy matching, recall thresholds and the PR sums of the reference's
// core/evaluation/kitti_utils/eval.py (compute_statistics_jit :166-284, get_thresholds :12-30, fused_compute_statistics :296-343).
//
// Lane mapping.  One (case, image, threshold) is a SERIAL job: the ground truths are visited in order and every match changes which
// detections the next one may take.  What is parallel is the job axis, and jobs of one image read the same overlaps, scores and boxes.
// So a wave owns one image and its LANES are jobs: 64 cases in the matching pass, the (up to 41) thresholds of one case in the
// statistics pass.  Loop counters and addresses are wave-uniform -- a load serves every lane -- and a lane runs the reference's
// decision sequence itself, with no cross-lane step at all: ties resolve as in the sequential loops by construction, and the
// arithmetic is fp64 throughout (overlaps widened, never min_overlap rounded).  At KITTI's sizes (<= 24 ground truths, <= 50
// detections) a lane per detection would fill under half a wave and pay a 64-lane keyed reduction per ground truth and threshold;
// a lane per threshold fills 41 of 64 lanes and pays nothing.
//
// The detection loop is a keyed argmax in both passes (lowest index on ties, since only a strictly better key replaces the best):
//   pass 1   key = score, among detections that are not of another class, not assigned, overlap > min_overlap;
//   pass 2   key = overlap among those with ignore flag 0 (scores below the threshold are out); if there is none, the FIRST candidate
//            with ignore flag 1.  The sequential loop lets a flag-0 candidate replace a flag-1 one unconditionally and a flag-1 one
//            never replace anything, which is this rule.
//
// Which detections are assigned is one bit per (lane, detection): a 64-bit register per lane while the image has at most 64
// detections, else two int32 words per detection in the caller's scratch (bit = lane), read and written with agent-scope atomics
// (a lane owns its bit, the word is shared).  No cap on either count beyond int32.
//
// Sums.  tp / fp / fn are integers and go through integer atomics (order-independent).  The similarity is fp64: every (case, image)
// writes its 41 partials, and one workgroup per case adds them in a fixed order (sixteen chunks of consecutive images, each in image
// order, then the chunk sums in chunk order) -- no float atomic, two calls give the same bits.
//
// The offsets live on the device and are memory: an image whose ranges leave the arrays (or whose block leaves the overlaps) is
// skipped as a whole, nothing is read or written out of bounds.
#include <math.h>

#include "pnp_host.h"
#include "pnp_math.h"
#include "wave_ops.h"

namespace pnp {
namespace {

constexpr int kKittiPts = EPROPNP_KITTI_SAMPLE_PTS;      // 41 recall positions
constexpr int kKittiThreads = 64;                        // one wave: lanes are jobs
constexpr double kNoDetection = -10000000.0;             // the reference's NO_DETECTION: a score <= -1e7 never matches in pass 1

// one image's slice of the concatenated arrays
struct KittiImage {
  const void* ov;          // (nd, ng) row-major block
  const double* gt;        // (ng, 5) bbox, alpha
  const double* dt;        // (nd, 6) bbox, alpha, score
  const double* dc;        // (nc, 4) DontCare boxes
  int ng, nd, nc;
  int gt0, dt0;            // offsets into the (C, G) / (C, D) arrays
  bool ok;
};

PNP_FN bool range_ok(int lo, int hi, int n) { return lo >= 0 && hi >= lo && hi <= n; }

PNP_FN KittiImage kitti_image(int img, const void* overlaps, int ov64, long long num_ov, const int32_t* gt_off, const int32_t* dt_off,
                              const int32_t* dc_off, const long long* blk_off, const double* gt_data, const double* dt_data,
                              const double* dc_boxes, int G, int D, int Q) {
  KittiImage v;
  const int g0 = gt_off[img], g1 = gt_off[img + 1], d0 = dt_off[img], d1 = dt_off[img + 1];
  const int q0 = dc_off ? dc_off[img] : 0, q1 = dc_off ? dc_off[img + 1] : 0;
  const long long b0 = blk_off[img];
  v.ok = range_ok(g0, g1, G) && range_ok(d0, d1, D) && range_ok(q0, q1, Q) && b0 >= 0 && b0 <= num_ov &&
         (long long)(g1 - g0) * (long long)(d1 - d0) <= num_ov - b0;
  v.ng = v.ok ? g1 - g0 : 0;
  v.nd = v.ok ? d1 - d0 : 0;
  v.nc = v.ok ? q1 - q0 : 0;
  v.gt0 = g0;
  v.dt0 = d0;
  v.ov = v.ok ? (ov64 ? (const void*)((const double*)overlaps + b0) : (const void*)((const float*)overlaps + b0)) : nullptr;
  v.gt = v.ok && gt_data ? gt_data + (size_t)g0 * 5 : nullptr;
  v.dt = v.ok ? dt_data + (size_t)d0 * 6 : nullptr;
  v.dc = v.ok && dc_boxes ? dc_boxes + (size_t)q0 * 4 : nullptr;
  return v;
}

template <bool OV64>
PNP_FN double overlap_at(const KittiImage& v, int j, int i) {
  const size_t at = (size_t)j * (size_t)v.ng + (size_t)i;
  if (OV64) return ((const double*)v.ov)[at];
  return (double)((const float*)v.ov)[at];
}

// "detection j is assigned", per lane
struct RegFlags {
  unsigned long long m;
  PNP_FN bool test(int j) const { return (m >> j) & 1ull; }
  PNP_FN void set(int j) { m |= 1ull << j; }
};
struct MemFlags {
  int* words;      // (nd, 2) of this (row, image)
  int half, bit;
  PNP_FN bool test(int j) const {
    return (__hip_atomic_load(words + 2 * (size_t)j + half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) != 0;
  }
  PNP_FN void set(int j) {
    atomicOr(words + 2 * (size_t)j + half, bit);
    __threadfence();
  }
};

struct KittiCounts {
  int tp, fp, fn;
  double similarity;
};

// One job: the reference's compute_statistics_jit on one image.  FP = false: pass 1.  FP = true: pass 2 under `thresh`.  tp_scores /
// gt_state, when given, get one entry per ground truth.
template <bool FP, bool OV64, class Flags>
PNP_FN KittiCounts kitti_job(const KittiImage& v, const int8_t* ign_gt, const int8_t* ign_dt, double min_ov, double thresh, int metric,
                             Flags& assigned, double* tp_scores, int8_t* gt_state) {
#pragma clang fp contract(off)
  KittiCounts r{0, 0, 0, 0.0};
  for (int i = 0; i < v.ng; ++i) {
    const int ig = ign_gt[i];
    int det = -1, state = EPROPNP_KITTI_GT_SKIPPED;
    if (ig != -1) {
      double best = FP ? 0.0 : kNoDetection;      // pass 2: the reference's max_overlap starts at 0
      bool det_ignored = false;
      for (int j = 0; j < v.nd; ++j) {
        const int id = ign_dt[j];
        if (id == -1 || assigned.test(j)) continue;
        const double score = v.dt[(size_t)j * 6 + 5];
        if (FP && score < thresh) continue;
        const double ov = overlap_at<OV64>(v, j, i);
        if (!(ov > min_ov)) continue;
        if (!FP) {
          if (score > best) { best = score; det = j; }
        } else if (id == 0) {
          if (ov > best || det_ignored) { best = ov; det = j; det_ignored = false; }
        } else if (id == 1 && det < 0) {
          det = j;
          det_ignored = true;
        }
      }
      if (det < 0) {
        state = EPROPNP_KITTI_GT_UNMATCHED;
        if (ig == 0) { r.fn += 1; state = EPROPNP_KITTI_GT_MISSED; }
      } else if (ig == 1 || ign_dt[det] == 1) {
        assigned.set(det);
        state = EPROPNP_KITTI_GT_IGNORED_MATCH;
        det = -1;
      } else {
        assigned.set(det);
        state = EPROPNP_KITTI_GT_TRUE_POSITIVE;
        r.tp += 1;
        if (FP) r.similarity += (1.0 + cos(v.gt[(size_t)i * 5 + 4] - v.dt[(size_t)det * 6 + 4])) / 2.0;
      }
    }
    {
      if (tp_scores) tp_scores[i] = state == EPROPNP_KITTI_GT_TRUE_POSITIVE ? v.dt[(size_t)det * 6 + 5] : -INFINITY;
      if (gt_state) gt_state[i] = (int8_t)state;
    }
  }
  if (FP) {
    // false positives: unassigned, of this class and tall enough, not below the threshold -- and, for image boxes, not mostly inside a
    // DontCare box (intersection over the DETECTION's area, fp64 from the fp64 rows)
    for (int j = 0; j < v.nd; ++j) {
      if (ign_dt[j] != 0 || assigned.test(j)) continue;
      const double* d = v.dt + (size_t)j * 6;
      if (d[5] < thresh) continue;
      bool stuff = false;
      if (metric == 0) {
        for (int k = 0; k < v.nc && !stuff; ++k) {
          const double* q = v.dc + (size_t)k * 4;
          double ov = 0.0;
          const double iw = fmin(d[2], q[2]) - fmax(d[0], q[0]);
          if (iw > 0.0) {
            const double ih = fmin(d[3], q[3]) - fmax(d[1], q[1]);
            if (ih > 0.0) ov = iw * ih / ((d[2] - d[0]) * (d[3] - d[1]));
          }
          stuff = ov > min_ov;
        }
      }
      if (!stuff) r.fp += 1;
    }
  }
  return r;
}

// the scratch words of one (row, image), zeroed by the wave that owns them before any lane sets a bit
PNP_FN int* flag_words(int* scratch, int row, int D, const KittiImage& v) {
  int* w = scratch + ((size_t)row * (size_t)D + (size_t)v.dt0) * 2;
  for (int j = lane_id(); j < 2 * v.nd; j += kWave) __hip_atomic_store(w + j, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __threadfence();
  __builtin_amdgcn_wave_barrier();
  return w;
}

// ---- pass 1: grid (images, ceil(C / 64)), lane = case ------------------------------------------------------------------------------
template <bool OV64>
__global__ __launch_bounds__(kKittiThreads) void kitti_match_kernel(const void* __restrict__ overlaps, long long num_ov,
                                                                    const int32_t* __restrict__ gt_off, const int32_t* __restrict__ dt_off,
                                                                    const long long* __restrict__ blk_off, const double* __restrict__ dt_data,
                                                                    int G, int D, const int8_t* __restrict__ ign_gt,
                                                                    const int8_t* __restrict__ ign_dt, const double* __restrict__ min_ov,
                                                                    int C, int* __restrict__ flags, double* __restrict__ tp_scores,
                                                                    int32_t* __restrict__ tp_count, int8_t* __restrict__ gt_state) {
  const int img = (int)blockIdx.x, lane = lane_id(), c = (int)blockIdx.y * kWave + lane;
  const KittiImage v = kitti_image(img, overlaps, OV64, num_ov, gt_off, dt_off, nullptr, blk_off, nullptr, dt_data, nullptr, G, D, 0);
  if (!v.ok || v.ng == 0) return;
  const bool wide = v.nd > 64;      // wave-uniform
  int* words = wide ? flag_words(flags, (int)blockIdx.y, D, v) : nullptr;
  if (c >= C) return;
  const int8_t* ig = ign_gt + (size_t)c * G + v.gt0;
  const int8_t* id = ign_dt + (size_t)c * D + v.dt0;
  double* out = tp_scores + (size_t)c * G + v.gt0;
  int8_t* st = gt_state ? gt_state + (size_t)c * G + v.gt0 : nullptr;
  KittiCounts r;
  if (wide) {
    MemFlags f{words, lane >> 5, (int)(1u << (lane & 31))};
    r = kitti_job<false, OV64>(v, ig, id, min_ov[c], 0.0, 0, f, out, st);
  } else {
    RegFlags f{0ull};
    r = kitti_job<false, OV64>(v, ig, id, min_ov[c], 0.0, 0, f, out, st);
  }
  if (r.tp > 0) atomicAdd(tp_count + c, r.tp);
}

// ---- get_thresholds: one lane per case ---------------------------------------------------------------------------------------------
// The reference scans the descending scores and skips score i while (r_recall - current_recall) < (current_recall - l_recall), with
// l_recall = (i + 1) / num_gt, r_recall = (i + 2) / num_gt (= l_recall for the last score, which is never skipped).  Under correctly
// rounded fp64 the left side does not decrease with i and the right side does not increase, so the first score that is kept is found
// by bisection; the expressions are the reference's, evaluated as written.
__global__ __launch_bounds__(kKittiThreads) void kitti_thresholds_kernel(const double* __restrict__ sorted, const int32_t* __restrict__ tp_count,
                                                                         const int32_t* __restrict__ num_valid_gt, int G, int C,
                                                                         double recall_step, double* __restrict__ thresholds,
                                                                         int32_t* __restrict__ thr_count) {
#pragma clang fp contract(off)
  const int c = (int)blockIdx.x * kKittiThreads + (int)threadIdx.x;
  if (c >= C) return;
  const double* s = sorted + (size_t)c * G;
  double* out = thresholds + (size_t)c * kKittiPts;
  int n = tp_count[c];
  n = n < 0 ? 0 : (n > G ? G : n);
  const double num_gt = (double)num_valid_gt[c];
  double current_recall = 0.0;
  int k = 0, i = 0;
  while (i < n && k < kKittiPts) {
    int lo = i, hi = n - 1;
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;      // mid < n - 1
      const double l_recall = (double)(mid + 1) / num_gt, r_recall = (double)(mid + 2) / num_gt;
      if ((r_recall - current_recall) < (current_recall - l_recall)) lo = mid + 1; else hi = mid;
    }
    out[k++] = s[lo];
    current_recall += recall_step;
    i = lo + 1;
  }
  thr_count[c] = k;
  for (; k < kKittiPts; ++k) out[k] = 0.0;
}

// ---- pass 2: grid (images, C), lane = threshold ------------------------------------------------------------------------------------
template <bool OV64>
__global__ __launch_bounds__(kKittiThreads) void kitti_statistics_kernel(
    const void* __restrict__ overlaps, long long num_ov, const int32_t* __restrict__ gt_off, const int32_t* __restrict__ dt_off,
    const int32_t* __restrict__ dc_off, const long long* __restrict__ blk_off, int I, const double* __restrict__ gt_data,
    const double* __restrict__ dt_data, const double* __restrict__ dc_boxes, int G, int D, int Q, const int8_t* __restrict__ ign_gt,
    const int8_t* __restrict__ ign_dt, const double* __restrict__ min_ov, const double* __restrict__ thresholds,
    const int32_t* __restrict__ thr_count, int metric, int* __restrict__ flags, int32_t* __restrict__ counts,
    double* __restrict__ sim_part, double* __restrict__ tp_scores) {
  const int img = (int)blockIdx.x, c = (int)blockIdx.y, t = lane_id();
  const KittiImage v = kitti_image(img, overlaps, OV64, num_ov, gt_off, dt_off, dc_off, blk_off, gt_data, dt_data, dc_boxes, G, D, Q);
  int n = thr_count[c];
  n = n < 0 ? 0 : (n > kKittiPts ? kKittiPts : n);
  const bool wide = v.nd > 64;
  int* words = wide ? flag_words(flags, c, D, v) : nullptr;
  if (t >= n) return;
  KittiCounts r{0, 0, 0, 0.0};
  if (v.ok) {
    const int8_t* ig = ign_gt + (size_t)c * G + v.gt0;
    const int8_t* id = ign_dt + (size_t)c * D + v.dt0;
    const double thresh = thresholds[(size_t)c * kKittiPts + t];
    double* out = tp_scores ? tp_scores + ((size_t)c * kKittiPts + t) * (size_t)G + v.gt0 : nullptr;
    if (wide) {
      MemFlags f{words, t >> 5, (int)(1u << (t & 31))};
      r = kitti_job<true, OV64>(v, ig, id, min_ov[c], thresh, metric, f, out, nullptr);
    } else {
      RegFlags f{0ull};
      r = kitti_job<true, OV64>(v, ig, id, min_ov[c], thresh, metric, f, out, nullptr);
    }
  }
  int32_t* cnt = counts + ((size_t)c * kKittiPts + t) * 3;
  if (r.tp) atomicAdd(cnt + 0, r.tp);
  if (r.fp) atomicAdd(cnt + 1, r.fp);
  if (r.fn) atomicAdd(cnt + 2, r.fn);
  if (sim_part) sim_part[((size_t)c * (size_t)I + (size_t)img) * kKittiPts + t] = r.similarity;
}

// pr (C, 41, 4): the integer sums as fp64 and the similarity partials added in a fixed order -- wave w adds the images of the w-th
// of kReduceWaves equal chunks in image order (lane = threshold), lane t of wave 0 then adds the chunk sums in chunk order; zeros
// beyond the case's threshold count
constexpr int kReduceWaves = 16;
__global__ __launch_bounds__(kReduceWaves * kWave) void kitti_pr_reduce_kernel(const int32_t* __restrict__ counts,
                                                                              const double* __restrict__ sim_part,
                                                                              const int32_t* __restrict__ thr_count, int I,
                                                                              double* __restrict__ pr) {
  __shared__ double chunk_sum[kReduceWaves][kWave];
  const int c = (int)blockIdx.x, t = lane_id(), w = wave_id();
  int n = thr_count[c];
  n = n < 0 ? 0 : (n > kKittiPts ? kKittiPts : n);
  double sim = 0.0;
  if (sim_part && t < n) {
    const int per = (I + kReduceWaves - 1) / kReduceWaves, lo = w * per, hi = lo + per < I ? lo + per : I;
    const double* p = sim_part + (size_t)c * (size_t)I * kKittiPts + t;
#pragma unroll 8
    for (int img = lo; img < hi; ++img) sim += p[(size_t)img * kKittiPts];
  }
  chunk_sum[w][t] = sim;
  __syncthreads();
  if (w != 0 || t >= kKittiPts) return;
  double* out = pr + ((size_t)c * kKittiPts + t) * 4;
  if (t >= n) {
    out[0] = out[1] = out[2] = out[3] = 0.0;
    return;
  }
  sim = chunk_sum[0][t];
  for (int k = 1; k < kReduceWaves; ++k) sim += chunk_sum[k][t];
  const int32_t* cnt = counts + ((size_t)c * kKittiPts + t) * 3;
  out[0] = (double)cnt[0];
  out[1] = (double)cnt[1];
  out[2] = (double)cnt[2];
  out[3] = sim;
}

size_t round8(size_t n) { return (n + 7) & ~(size_t)7; }
size_t flag_bytes(long long rows, int D) { return round8((size_t)rows * (size_t)D * 2 * sizeof(int32_t)); }
size_t sim_bytes(int I, int C) { return (size_t)C * (size_t)I * kKittiPts * sizeof(double); }
size_t count_bytes(int C) { return round8((size_t)C * kKittiPts * 3 * sizeof(int32_t)); }

int kitti_check_common(const char* who, int I, int G, int D, int C) {
  if (I < 0 || G < 0 || D < 0 || C < 0)
    return fail(EPROPNP_EINVAL, "%s: counts must be >= 0, got %d images, %d ground truths, %d detections, %d cases", who, I, G, D, C);
  if (C > 65535) return fail(EPROPNP_EINVAL, "%s: %d cases are more than the 65535 of one launch", who, C);
  return EPROPNP_OK;
}

}  // namespace

size_t kitti_match_scratch_bytes(int D, int C) {
  if (D <= 0 || C <= 0) return 0;
  return flag_bytes(((long long)C + kWave - 1) / kWave, D);
}

size_t kitti_statistics_scratch_bytes(int I, int D, int C, int compute_aos) {
  if (C <= 0) return 0;
  return (compute_aos && I > 0 ? sim_bytes(I, C) : 0) + count_bytes(C) + (D > 0 ? flag_bytes(C, D) : 0);
}

int launch_kitti_match(const void* overlaps, int ov64, long long num_ov, const int32_t* gt_off, const int32_t* dt_off,
                       const long long* blk_off, int I, const double* dt_data, int G, int D, const int8_t* ign_gt, const int8_t* ign_dt,
                       const double* min_ov, int C, void* scratch, size_t scratch_bytes, double* tp_scores, int32_t* tp_count,
                       int8_t* gt_state, hipStream_t st) {
  const char* who = "epropnp_kitti_match";
  if (int rc = kitti_check_common(who, I, G, D, C)) return rc;
  if (num_ov < 0) return fail(EPROPNP_EINVAL, "%s: num_overlaps must be >= 0, got %lld", who, num_ov);
  if (C == 0) return EPROPNP_OK;
  if (!tp_count) return fail(EPROPNP_EINVAL, "%s: tp_count is NULL", who);
  const bool work = I > 0 && G > 0;      // else there is nothing to match and tp_scores has no element
  if (work) {
    if (!gt_off || !dt_off || !blk_off || !ign_gt || !min_ov || !tp_scores) return fail(EPROPNP_EINVAL, "%s: NULL pointer", who);
    if (D > 0 && (!dt_data || !ign_dt)) return fail(EPROPNP_EINVAL, "%s: NULL detections", who);
    if (num_ov > 0 && !overlaps) return fail(EPROPNP_EINVAL, "%s: overlaps is NULL", who);
    const size_t need = kitti_match_scratch_bytes(D, C);
    if (need > 0 && (!scratch || scratch_bytes < need))
      return fail(EPROPNP_EINVAL, "%s: scratch of %zu bytes, %zu are needed", who, scratch ? scratch_bytes : (size_t)0, need);
  }
  if (int rc = launch_fill_u32(tp_count, 0u, (size_t)C, st)) return rc;
  if (!work) return EPROPNP_OK;
  const dim3 grid((unsigned)I, (unsigned)((C + kWave - 1) / kWave)), block(kKittiThreads);
  if (ov64) {
    PNP_LAUNCH(kitti_match_kernel<true>, grid, block, 0, st, overlaps, num_ov, gt_off, dt_off, blk_off, dt_data, G, D, ign_gt, ign_dt,
               min_ov, C, (int*)scratch, tp_scores, tp_count, gt_state);
  } else {
    PNP_LAUNCH(kitti_match_kernel<false>, grid, block, 0, st, overlaps, num_ov, gt_off, dt_off, blk_off, dt_data, G, D, ign_gt, ign_dt,
               min_ov, C, (int*)scratch, tp_scores, tp_count, gt_state);
  }
  return check_launch("kitti_match_kernel");
}

int launch_kitti_thresholds(const double* sorted, const int32_t* tp_count, const int32_t* num_valid_gt, int G, int C, double recall_step,
                            double* thresholds, int32_t* thr_count, hipStream_t st) {
  const char* who = "epropnp_kitti_thresholds";
  if (G < 0 || C < 0) return fail(EPROPNP_EINVAL, "%s: counts must be >= 0, got %d ground truths, %d cases", who, G, C);
  if (!(recall_step > 0.0)) return fail(EPROPNP_EINVAL, "%s: recall_step must be positive", who);
  if (C == 0) return EPROPNP_OK;
  if (!tp_count || !num_valid_gt || !thresholds || !thr_count || (G > 0 && !sorted)) return fail(EPROPNP_EINVAL, "%s: NULL pointer", who);
  const dim3 grid((unsigned)((C + kKittiThreads - 1) / kKittiThreads)), block(kKittiThreads);
  PNP_LAUNCH(kitti_thresholds_kernel, grid, block, 0, st, sorted, tp_count, num_valid_gt, G, C, recall_step, thresholds, thr_count);
  return check_launch("kitti_thresholds_kernel");
}

int launch_kitti_statistics(const void* overlaps, int ov64, long long num_ov, const int32_t* gt_off, const int32_t* dt_off,
                            const int32_t* dc_off, const long long* blk_off, int I, const double* gt_data, const double* dt_data,
                            const double* dc_boxes, int G, int D, int Q, const int8_t* ign_gt, const int8_t* ign_dt, const double* min_ov,
                            int C, const double* thresholds, const int32_t* thr_count, int metric, int compute_aos, void* scratch,
                            size_t scratch_bytes, double* pr, double* tp_scores, hipStream_t st) {
  const char* who = "epropnp_kitti_statistics";
  if (int rc = kitti_check_common(who, I, G, D, C)) return rc;
  if (Q < 0) return fail(EPROPNP_EINVAL, "%s: num_dc must be >= 0, got %d", who, Q);
  if (num_ov < 0) return fail(EPROPNP_EINVAL, "%s: num_overlaps must be >= 0, got %lld", who, num_ov);
  if (metric < 0 || metric > 2) return fail(EPROPNP_EINVAL, "%s: metric must be 0, 1 or 2, got %d", who, metric);
  if (C == 0) return EPROPNP_OK;
  if (!thresholds || !thr_count || !pr || !min_ov) return fail(EPROPNP_EINVAL, "%s: NULL pointer", who);
  if (I > 0 && (!gt_off || !dt_off || !dc_off || !blk_off)) return fail(EPROPNP_EINVAL, "%s: NULL offsets", who);
  if (G > 0 && (!gt_data || !ign_gt)) return fail(EPROPNP_EINVAL, "%s: NULL ground truths", who);
  if (D > 0 && (!dt_data || !ign_dt)) return fail(EPROPNP_EINVAL, "%s: NULL detections", who);
  if (Q > 0 && !dc_boxes) return fail(EPROPNP_EINVAL, "%s: dc_boxes is NULL", who);
  if (num_ov > 0 && !overlaps) return fail(EPROPNP_EINVAL, "%s: overlaps is NULL", who);
  const size_t need = kitti_statistics_scratch_bytes(I, D, C, compute_aos);
  if (!scratch || scratch_bytes < need)
    return fail(EPROPNP_EINVAL, "%s: scratch of %zu bytes, %zu are needed", who, scratch ? scratch_bytes : (size_t)0, need);
  const bool aos = compute_aos && I > 0;
  double* sim_part = aos ? (double*)scratch : nullptr;
  int32_t* counts = (int32_t*)((char*)scratch + (aos ? sim_bytes(I, C) : 0));
  int* flags = (int*)((char*)counts + count_bytes(C));
  if (int rc = launch_fill_u32(counts, 0u, (size_t)C * kKittiPts * 3, st)) return rc;
  if (I > 0) {
    const dim3 grid((unsigned)I, (unsigned)C), block(kKittiThreads);
    if (ov64) {
      PNP_LAUNCH(kitti_statistics_kernel<true>, grid, block, 0, st, overlaps, num_ov, gt_off, dt_off, dc_off, blk_off, I, gt_data, dt_data,
                 dc_boxes, G, D, Q, ign_gt, ign_dt, min_ov, thresholds, thr_count, metric, flags, counts, sim_part, tp_scores);
    } else {
      PNP_LAUNCH(kitti_statistics_kernel<false>, grid, block, 0, st, overlaps, num_ov, gt_off, dt_off, dc_off, blk_off, I, gt_data, dt_data,
                 dc_boxes, G, D, Q, ign_gt, ign_dt, min_ov, thresholds, thr_count, metric, flags, counts, sim_part, tp_scores);
    }
    if (int rc = check_launch("kitti_statistics_kernel")) return rc;
  }
  PNP_LAUNCH(kitti_pr_reduce_kernel, dim3((unsigned)C), dim3(kReduceWaves * kWave), 0, st, counts, sim_part, thr_count, I, pr);
  return check_launch("kitti_pr_reduce_kernel");
}

}  // namespace pnp
