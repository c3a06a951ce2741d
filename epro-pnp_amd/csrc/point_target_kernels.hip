// point_target_kernels.hip -- the two steps of the detection head's training step between the centre targets and the PnP layer
// (include/epropnp_hip.h: epropnp_point_targets, epropnp_obj_sample_weights): EPro-PnP-Det models/dense_heads/fcos_emb_head.py:299-438
// (FCOSEmbHead.get_targets / _get_target_single) and deform_pnp_head.py:1148-1174 (obj_sampler after its draws).
//
//   point_target_kernel : one workgroup per (tile of kPtThreads points, image); a lane owns one point.  The image's objects (centre
//       and box, 6 floats) are staged in LDS kPtChunk at a time; every lane scans the chunk, all lanes reading the same LDS word (a
//       broadcast).  A lane finds its level by comparing its point index with the at most 8 level starts, which travel by value, so a
//       tile may straddle a level boundary.  The distance's square root is taken only where a lane passed both tests.  The point's
//       three (four) targets are written in the reference's flattened order (level, image, point), contiguous within a level.  The
//       foreground count is built with integer adds only: an LDS counter per workgroup, then one integer atomic per workgroup into
//       a word a one-word fill launch zeroed before.
//   obj_sample_weights_kernel : ONE workgroup of 1024 threads.  Thread t adds centerness x fg of the points t, t + 1024, ... in fp64
//       and counts the foreground; a binary tree in LDS adds the threads in a fixed order.  Then a thread owns a sample: the
//       gt index and the probability weight of its drawn point go to LDS, every sample scans all samples in ascending order (again a
//       broadcast) for the sum and the count of those with its gt index -- no (num_gt, N) mask and no largest index --, and two more
//       trees give the means the two weight vectors are divided by.
//
// No floating-point atomics and every order fixed: two launches agree to the last bit.  A drawn point index is clamped into the
// points before it forms an address; nothing else read from memory does.  Every output element is written; no allocation, no
// synchronisation, no scratch.
#include "pnp_host.h"
#include "tuning.h"

namespace pnp {

constexpr int kPtThreads = PNP_PT_THREADS, kPtChunk = PNP_PT_CHUNK, kPtMaxLvl = 8, kPtObj = 6;
constexpr float kPtInf = 1e8f;
constexpr int kOsThreads = 1024, kOsMaxN = 2048, kOsPer = kOsMaxN / kOsThreads, kOsAhead = 16;
static_assert(kPtThreads % 64 == 0 && kPtThreads <= 1024 && kPtChunk >= 1, "whole waves; a chunk holds an object");

struct PtArgs {
  const float* points; const float* boxes; const float* centers; const long long* gt_labels; const int32_t* img_off;
  long long* labels; float* centerness; long long* gt_inds; long long* strides; int32_t* num_fg;
  int P, G, num_img, L, num_classes;
  float alpha;
  int lvl_off[kPtMaxLvl + 1];                    // entries beyond L repeat P
  float radius[kPtMaxLvl], lo[kPtMaxLvl], hi[kPtMaxLvl];
  long long stride_val[kPtMaxLvl];
};

__global__ __launch_bounds__(kPtThreads) void point_target_kernel(PtArgs a) {
  __shared__ float obj[kPtChunk * kPtObj];       // per object: cx, cy, x1, y1, x2, y2
  __shared__ int fg_count;
  const int tid = (int)threadIdx.x, img = (int)blockIdx.y;
  if (tid == 0) fg_count = 0;
  __syncthreads();
  const int p = (int)blockIdx.x * kPtThreads + tid;
  const bool live = p < a.P;
  // ---- this lane's level: the last one that starts at or before the point ----
  int l_off = a.lvl_off[0], l_end = a.lvl_off[1];
  float s = a.radius[0], lo = a.lo[0], hi = a.hi[0];
  long long sv = a.stride_val[0];
#pragma unroll
  for (int k = 1; k < kPtMaxLvl; ++k) {
    const bool at = k < a.L && p >= a.lvl_off[k];
    l_off = at ? a.lvl_off[k] : l_off;
    l_end = at ? a.lvl_off[k + 1] : l_end;
    s = at ? a.radius[k] : s;
    lo = at ? a.lo[k] : lo;
    hi = at ? a.hi[k] : hi;
    sv = at ? a.stride_val[k] : sv;
  }
  const float x = live ? a.points[(size_t)p * 2] : 0.f, y = live ? a.points[(size_t)p * 2 + 1] : 0.f;
  const int o0 = max(0, min(a.img_off[img], a.G)), o1 = max(o0, min(a.img_off[img + 1], a.G));
  float best = kPtInf;
  int win = 0;
  for (int oc = o0; oc < o1; oc += kPtChunk) {
    const int nc = min(kPtChunk, o1 - oc);
    __syncthreads();                             // the chunk before has been scanned
    for (int k = tid; k < nc; k += kPtThreads) {
      const float* b = a.boxes + (size_t)(oc + k) * 4;
      const float* c = a.centers + (size_t)(oc + k) * 2;
      float v[kPtObj] = {c[0], c[1], b[0], b[1], b[2], b[3]};
      bool nan = false;
#pragma unroll
      for (int q = 0; q < kPtObj; ++q) nan = nan || v[q] != v[q];
      if (nan) { v[0] = NAN; v[1] = NAN; }       // every comparison below is then false: the object never wins
#pragma unroll
      for (int q = 0; q < kPtObj; ++q) obj[k * kPtObj + q] = v[q];
    }
    __syncthreads();
    for (int o = 0; o < nc; ++o) {
      const float* r = obj + o * kPtObj;
      const float cx = r[0], cy = r[1];
      const float in_min = fminf(fminf(x - (cx - s), y - (cy - s)), fminf((cx + s) - x, (cy + s) - y));
      const float reg_max = fmaxf(fmaxf(x - r[2], y - r[3]), fmaxf(r[4] - x, r[5] - y));
      if (in_min > 0.f && reg_max >= lo && reg_max <= hi) {
        const float dx = x - cx, dy = y - cy;
        const float d = sqrtf(add_unfused(mul_unfused(dx, dx), mul_unfused(dy, dy)));
        if (d < best) {                          // strict: the lowest index among equal distances
          best = d;
          win = oc + o - o0;
        }
      }
    }
  }
  bool fg = false;
  if (live) {
    const long long at = (long long)a.num_img * l_off + (long long)img * (l_end - l_off) + (p - l_off);
    long long label = a.num_classes;
    float cen = 0.f;
    if (o1 > o0) {
      if (best != kPtInf) label = a.gt_labels[o0 + win];
      const float rel = best / mul_unfused(1.414f, s);
      cen = expf(mul_unfused(-a.alpha, rel));
    }
    a.labels[at] = label;
    a.centerness[at] = cen;
    a.gt_inds[at] = (long long)(o0 + win);
    if (a.strides) a.strides[at] = sv;
    fg = label < (long long)a.num_classes;
  }
  if (fg) atomicAdd(&fg_count, 1);               // integer adds only: LDS first, one add to memory per workgroup
  __syncthreads();
  if (tid == 0 && fg_count > 0) atomicAdd(a.num_fg, fg_count);
}

int launch_point_targets(const float* points, const int32_t* lvl_off, const float* radius_px, const float* regress_lo,
                         const float* regress_hi, const long long* level_strides, int L, const float* gt_bboxes, const float* centers2d,
                         const long long* gt_labels, const int32_t* img_off, int P, int G, int num_img, int num_classes, float alpha,
                         long long* labels, float* centerness, long long* gt_inds, long long* strides, int32_t* num_fg,
                         hipStream_t st) {
  const char* who = "epropnp_point_targets";
  if (P < 0 || G < 0 || num_img < 0) return fail(EPROPNP_EINVAL, "%s: num_points, num_gt and num_img must be >= 0, got %d, %d and %d", who, P, G, num_img);
  if (L < 1 || L > kPtMaxLvl) return fail(EPROPNP_EINVAL, "%s: num_levels must be 1 .. %d, got %d", who, kPtMaxLvl, L);
  if (num_img > 65535) return fail(EPROPNP_EINVAL, "%s: num_img = %d is more than the 65535 of one call", who, num_img);
  if (num_classes < 0) return fail(EPROPNP_EINVAL, "%s: num_classes must be >= 0, got %d", who, num_classes);
  if (!(alpha == alpha)) return fail(EPROPNP_EINVAL, "%s: centerness_alpha is NaN", who);
  if (P == 0 || num_img == 0) return EPROPNP_OK;           // no output element exists; no pointer is followed, num_fg is not written
  if (!lvl_off || !radius_px || !regress_lo || !regress_hi)
    return fail(EPROPNP_EINVAL, "%s: lvl_offsets, radius_px, regress_lo and regress_hi are host arrays and may not be NULL", who);
  if (lvl_off[0] != 0 || lvl_off[L] != P) return fail(EPROPNP_EINVAL, "%s: lvl_offsets must run from 0 to num_points = %d, got %d .. %d", who, P, lvl_off[0], lvl_off[L]);
  for (int k = 0; k < L; ++k) {
    if (lvl_off[k + 1] < lvl_off[k]) return fail(EPROPNP_EINVAL, "%s: lvl_offsets must ascend, got %d after %d", who, lvl_off[k + 1], lvl_off[k]);
    if (!(radius_px[k] > 0.f)) return fail(EPROPNP_EINVAL, "%s: radius_px[%d] must be > 0, got %g", who, k, (double)radius_px[k]);
    if (regress_lo[k] != regress_lo[k] || regress_hi[k] != regress_hi[k]) return fail(EPROPNP_EINVAL, "%s: regress range %d is NaN", who, k);
  }
  if (strides && !level_strides) return fail(EPROPNP_EINVAL, "%s: strides are wanted but level_strides is NULL", who);
  if (!points || !img_off || !labels || !centerness || !gt_inds || !num_fg) return fail(EPROPNP_EINVAL, "%s: NULL pointer", who);
  if (G > 0 && (!gt_bboxes || !centers2d || !gt_labels)) return fail(EPROPNP_EINVAL, "%s: NULL ground-truth pointer with num_gt = %d", who, G);
  const int rc = launch_fill_u32(num_fg, 0u, 1, st);
  if (rc != EPROPNP_OK) return rc;
  PtArgs a{};
  a.points = points; a.boxes = gt_bboxes; a.centers = centers2d; a.gt_labels = gt_labels; a.img_off = img_off;
  a.labels = labels; a.centerness = centerness; a.gt_inds = gt_inds; a.strides = strides; a.num_fg = num_fg;
  a.P = P; a.G = G; a.num_img = num_img; a.L = L; a.num_classes = num_classes; a.alpha = alpha;
  for (int k = 0; k <= kPtMaxLvl; ++k) a.lvl_off[k] = k <= L ? lvl_off[k] : P;
  for (int k = 0; k < kPtMaxLvl; ++k) {
    const int q = k < L ? k : L - 1;
    a.radius[k] = radius_px[q]; a.lo[k] = regress_lo[q]; a.hi[k] = regress_hi[q];
    a.stride_val[k] = level_strides ? level_strides[q] : 0;
  }
  PNP_LAUNCH(point_target_kernel, dim3((unsigned)((P + kPtThreads - 1) / kPtThreads), (unsigned)num_img), dim3(kPtThreads), 0, st, a);
  return check_launch("point_target_kernel");
}

// ---- obj_sampler after its draws ---------------------------------------------------------------------------------------------------
struct OsArgs {
  const uint8_t* fg; const float* cen; const long long* gt; const long long* draws;
  long long* sample_gt; float* weights; float* uniform_weights; int32_t* num_fg;
  long long T;
  int N, num_uniform;
  float eps;
};

// the sum of one double per thread in a fixed binary tree; every thread receives it (`red` holds kOsThreads doubles)
PNP_FN double os_tree_sum(double v, double* red, int tid) {
  __syncthreads();                               // `red` is free again
  red[tid] = v;
  for (int h = kOsThreads / 2; h > 0; h >>= 1) {
    __syncthreads();
    if (tid < h) red[tid] += red[tid + h];
  }
  __syncthreads();
  return red[0];
}

PNP_FN double os_floor(double v, double least) { return v < least ? least : v; }      // clamp(min=): a NaN stays a NaN

__global__ __launch_bounds__(kOsThreads) void obj_sample_weights_kernel(OsArgs a) {
  __shared__ double red[kOsThreads];
  __shared__ double s_w[kOsMaxN];
  __shared__ long long s_gt[kOsMaxN];
  const int tid = (int)threadIdx.x;
  // ---- sum of centerness over the foreground and its count, thread t over t, t + 1024, ... ----
  double acc = 0.0, cnt = 0.0;                   // (counts below 2^53 are exact in fp64)
  // kOsAhead independent loads of each array are issued before the first add (one workgroup has to hide the memory latency by
  // itself); the adds keep their order
  long long k = tid;
  for (; k + (long long)(kOsAhead - 1) * kOsThreads < a.T; k += (long long)kOsAhead * kOsThreads) {
    uint8_t f[kOsAhead];
    float c[kOsAhead];
#pragma unroll
    for (int u = 0; u < kOsAhead; ++u) {
      f[u] = a.fg[k + (long long)u * kOsThreads];
      c[u] = a.cen[k + (long long)u * kOsThreads];
    }
#pragma unroll
    for (int u = 0; u < kOsAhead; ++u) {
      acc += f[u] != 0 ? (double)c[u] : 0.0;
      cnt += f[u] != 0 ? 1.0 : 0.0;
    }
  }
  for (; k < a.T; k += kOsThreads) {
    const uint8_t f = a.fg[k];
    const float c = a.cen[k];
    acc += f != 0 ? (double)c : 0.0;
    cnt += f != 0 ? 1.0 : 0.0;
  }
  const double total = os_tree_sum(acc, red, tid), count = os_tree_sum(cnt, red, tid);
  if (tid == 0 && a.num_fg) *a.num_fg = (int32_t)fmin(count, 2147483647.0);
  const double denom = os_floor(total, (double)a.eps);
  const double nu = fmin((double)a.num_uniform, count), ratio = nu / (double)a.N;
  const double uni = 1.0 / os_floor(count, 1.0);
  // ---- the drawn points: gt index and prob / prob_mix ----
  double w[kOsPer];
  long long g[kOsPer];
#pragma unroll
  for (int q = 0; q < kOsPer; ++q) {
    const int i = tid + q * kOsThreads;
    w[q] = 0.0;
    g[q] = 0;
    if (i < a.N) {
      long long at = a.draws[i];
      at = at < 0 ? 0 : (at >= a.T ? a.T - 1 : at);
      const bool f = a.fg[at] != 0;
      const double prob = (f ? (double)a.cen[at] : 0.0) / denom;
      const double mix = (f ? uni : 0.0) * ratio + prob * (1.0 - ratio);
      w[q] = prob / mix;
      g[q] = a.gt[at];
      s_w[i] = w[q];
      s_gt[i] = g[q];
      a.sample_gt[i] = g[q];
    }
  }
  __syncthreads();
  // ---- per sample: sum and count over the samples of its object, in ascending order ----
  double sw[kOsPer], uw[kOsPer], part_s = 0.0, part_u = 0.0;
#pragma unroll
  for (int q = 0; q < kOsPer; ++q) {
    const int i = tid + q * kOsThreads;
    sw[q] = 0.0;
    uw[q] = 0.0;
    if (i < a.N) {
      double sum = 0.0;
      int same = 0;
      for (int j = 0; j < a.N; ++j) {
        const bool eq = s_gt[j] == g[q];
        sum += eq ? s_w[j] : 0.0;
        same += eq ? 1 : 0;
      }
      sw[q] = w[q] * (1.0 / os_floor(sum, (double)a.eps));
      uw[q] = 1.0 / (double)max(same, 1);
      part_s += sw[q];
      part_u += uw[q];
    }
  }
  const double mean_s = os_tree_sum(part_s, red, tid) / (double)a.N, mean_u = os_tree_sum(part_u, red, tid) / (double)a.N;
  const double div_s = os_floor(mean_s, (double)a.eps), div_u = os_floor(mean_u, (double)a.eps);
#pragma unroll
  for (int q = 0; q < kOsPer; ++q) {
    const int i = tid + q * kOsThreads;
    if (i < a.N) {
      a.weights[i] = (float)(sw[q] / div_s);
      a.uniform_weights[i] = (float)(uw[q] / div_u);
    }
  }
}

int launch_obj_sample_weights(const uint8_t* fg_mask, const float* centerness, const long long* gt_inds, long long T,
                              const long long* sample_point_inds, int N, int num_uniform, float eps, long long* sample_gt_inds,
                              float* sample_weights, float* sample_uniform_weights, int32_t* num_fg, hipStream_t st) {
  const char* who = "epropnp_obj_sample_weights";
  if (T < 0 || N < 0) return fail(EPROPNP_EINVAL, "%s: num_total_point and num_obj_samples must be >= 0, got %lld and %d", who, T, N);
  if (N > kOsMaxN) return fail(EPROPNP_EINVAL, "%s: num_obj_samples = %d is more than the %d of one call", who, N, kOsMaxN);
  if (num_uniform < 0 || num_uniform > N) return fail(EPROPNP_EINVAL, "%s: num_uniform must be 0 .. num_obj_samples = %d, got %d", who, N, num_uniform);
  if (!(eps > 0.f)) return fail(EPROPNP_EINVAL, "%s: eps must be > 0, got %g", who, (double)eps);
  if (N == 0) return EPROPNP_OK;
  if (T == 0) return fail(EPROPNP_EINVAL, "%s: %d samples but num_total_point = 0", who, N);
  if (!fg_mask || !centerness || !gt_inds || !sample_point_inds || !sample_gt_inds || !sample_weights || !sample_uniform_weights)
    return fail(EPROPNP_EINVAL, "%s: NULL pointer", who);
  OsArgs a{};
  a.fg = fg_mask; a.cen = centerness; a.gt = gt_inds; a.draws = sample_point_inds;
  a.sample_gt = sample_gt_inds; a.weights = sample_weights; a.uniform_weights = sample_uniform_weights; a.num_fg = num_fg;
  a.T = T; a.N = N; a.num_uniform = num_uniform; a.eps = eps;
  PNP_LAUNCH(obj_sample_weights_kernel, dim3(1), dim3(kOsThreads), 0, st, a);
  return check_launch("obj_sample_weights_kernel");
}

}  // namespace pnp
