// posterior_kernels.hip -- device-side consumers of the layer's product, the weighted pose samples (S,B,P) + log-weights (S,B):
//
//   posterior_summary_kernel  : per object the weighted moments of the samples -- mean and covariance of the translation, the
//       orientation score of the Det head (EPro-PnP-Det deform_pnp_head.py:532-537: softmax of the log-weights, norm of the xz
//       deviation from pose_opt, ((-log2 + 2.5) / 4).clamp(0, 1), sum over the samples: ~8 ATen launches over (S,B) temporaries),
//       mean orientation and its concentration.  include/epropnp_hip.h: epropnp_posterior_summary.
//   posterior_resample_kernel : systematic resampling of the samples into equally weighted draws.  epropnp_posterior_resample.
//   posterior_modes_*_kernel  : quick-shift modes of the samples (further down, with their own decomposition).  epropnp_posterior_modes.
//
// The first two keep the decomposition of the loss kernels (eval_kernels.hip: mc_loss_forward_kernel, weight_stats_kernel): a 512-thread
// block owns 16 adjacent objects, so that a sample row of the block is 64 contiguous bytes of log-weights and 16 * P contiguous
// floats of poses (256 B / 448 B), and splits the S rows over 32 row groups that meet in LDS.  Two passes over the column as in
// weight_stats_kernel and for its reason: w = exp(logw - max) with ONE rounding in the exponent's argument; the second pass finds
// the block's log-weights in L2 (S * 64 B) and streams the poses, which are read once.  No atomics, every sum in a fixed order:
// two launches agree to the last bit.  LDS use does not depend on S.
#include <type_traits>

#include "pnp_host.h"

namespace pnp {

constexpr int kPostCols = 16, kPostRows = 32, kPostCP = kPostCols + 1;
constexpr int kJacobiSweeps = 8;      // cyclic Jacobi on a 4x4: off-diagonal mass falls quadratically, fp32 is reached in 4 - 5

// Maximum of rows lo, lo + step, .. < hi of column b (batches of 8 independent loads) and the first row that holds it; a NaN or
// +inf poisons the column.
PNP_FN void column_max(const float* __restrict__ logw, int B, int b, int lo, int hi, int step, float& m, int& jm, bool& bad) {
  for (int j0 = lo; j0 < hi; j0 += step * 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int j = j0 + k * step;
      v[k] = (j < hi) ? logw[(size_t)j * B + b] : -INFINITY;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      bad = bad || (v[k] != v[k]) || (v[k] == INFINITY);
      if (v[k] > m) { m = v[k]; jm = j0 + k * step; }
    }
  }
}

// The 32 row groups' maxima of column c meet in red[32][17] / arg[32][17]: the column's maximum and the lowest row that holds it.
PNP_FN void block_column_max(float* red, int* arg, int rg, int c, float m, int jm, float& M, int& jM, bool& bad) {
  red[rg * kPostCP + c] = bad ? NAN : m;
  arg[rg * kPostCP + c] = jm;
  __syncthreads();
  M = -INFINITY;
  jM = 0x7fffffff;
  for (int k = 0; k < kPostRows; ++k) {
    const float mk = red[k * kPostCP + c];
    const int jk = arg[k * kPostCP + c];
    bad = bad || (mk != mk);
    if (mk > M || (mk == M && jk < jM)) { M = mk; jM = jk; }
  }
  __syncthreads();
}

// w_j = exp(logw_j - M): the largest weight is exactly 1, exp(-inf) = 0 (a -inf sample, the padding of a batch of loads)
PNP_FN float post_weight(float v, float M) { return (v == M) ? 1.0f : expf(v - M); }

PNP_FN float clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }      // (a NaN stays a NaN, as torch's clamp keeps it)

// Accumulators of one thread / one object:
//   [0] sum w | [1..3] sum w d | [4..9] sum w d d^T (xx xy xz yy yz zz), d = t - pivot | [10] sum w score_te
//   4-DoF: [11] sum w cos yaw, [12] sum w sin yaw        6-DoF: [11..20] sum w q q^T (upper triangle, row-major)
template <int DOF>
struct PostAcc {
  static constexpr int N = 11 + (DOF == 6 ? 10 : 2);
};

template <int DOF>
PNP_FN void post_accumulate(float w, const float (&p)[PoseLen<DOF>::value], const float (&piv)[3], bool has_ref, float rx, float rz,
                            float (&acc)[PostAcc<DOF>::N]) {
  const float dx = p[0] - piv[0], dy = p[1] - piv[1], dz = p[2] - piv[2];
  const float wx = w * dx, wy = w * dy, wz = w * dz;
  acc[0] += w;
  acc[1] += wx; acc[2] += wy; acc[3] += wz;
  acc[4] = fmaf(wx, dx, acc[4]); acc[5] = fmaf(wx, dy, acc[5]); acc[6] = fmaf(wx, dz, acc[6]);
  acc[7] = fmaf(wy, dy, acc[7]); acc[8] = fmaf(wy, dz, acc[8]); acc[9] = fmaf(wz, dz, acc[9]);
  if (has_ref) {
    const float ex = p[0] - rx, ez = p[2] - rz;
    // a deviation of 0: -log2(0) = +inf, which the clamp turns into 1 (deform_pnp_head.py:534-536 does the same)
    acc[10] = fmaf(w, clamp01((2.5f - log2f(sqrtf(ex * ex + ez * ez))) * 0.25f), acc[10]);
  }
  if (DOF == 6) {
    // q and -q give the same bits: every term is a product of two components
    int idx = 11;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float wq = w * p[3 + i];
#pragma unroll
      for (int j = i; j < 4; ++j) {
        acc[idx] = fmaf(wq, p[3 + j], acc[idx]);
        ++idx;
      }
    }
  } else {
    acc[11] = fmaf(w, cosf(p[3]), acc[11]);
    acc[12] = fmaf(w, sinf(p[3]), acc[12]);
  }
}

// Eigen-decomposition of a symmetric 4x4 by cyclic Jacobi: kJacobiSweeps sweeps of the six rotations whatever the data, so that the
// result is a fixed sequence of operations.  On return the diagonal of a holds the eigenvalues, the columns of v the eigenvectors.
PNP_FN void jacobi4(float (&a)[4][4], float (&v)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) v[i][j] = (i == j) ? 1.f : 0.f;
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const float apq = a[p][q];
        const float theta = (a[q][q] - a[p][p]) / (2.0f * apq);
        float t = 1.0f / (fabsf(theta) + sqrtf(fmaf(theta, theta, 1.0f)));      // (|theta| = inf: t = 0, the pair is diagonal already)
        t = (theta < 0.f) ? -t : t;
        t = (apq == 0.f) ? 0.f : t;                                              // (0 / 0 above)
        const float cs = 1.0f / sqrtf(fmaf(t, t, 1.0f)), sn = t * cs;
        a[p][p] -= t * apq;
        a[q][q] += t * apq;
        a[p][q] = a[q][p] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k != p && k != q) {
            const float akp = a[k][p], akq = a[k][q];
            a[k][p] = a[p][k] = cs * akp - sn * akq;
            a[k][q] = a[q][k] = sn * akp + cs * akq;
          }
          const float vkp = v[k][p], vkq = v[k][q];
          v[k][p] = cs * vkp - sn * vkq;
          v[k][q] = sn * vkp + cs * vkq;
        }
      }
    }
  }
}

// LDS: part[NA][32][17] per-(accumulator, row group) sums | red / arg[32][17] row-group maxima | tot[NA][16]   (6-DoF: 50 KiB)
template <int DOF>
__global__ __launch_bounds__(512) void posterior_summary_kernel(const float* __restrict__ pose, const float* __restrict__ logw,
                                                                 const float* __restrict__ ref, int S, int B,
                                                                 float* __restrict__ out) {
  constexpr int P = PoseLen<DOF>::value, NA = PostAcc<DOF>::N, UNR = (DOF == 6) ? 4 : 8;
  __shared__ float part[NA * kPostRows * kPostCP];
  __shared__ float red[kPostRows * kPostCP];
  __shared__ int arg[kPostRows * kPostCP];
  __shared__ float tot[NA * kPostCols];
  const int c = (int)(threadIdx.x % kPostCols), rg = (int)(threadIdx.x / kPostCols);
  const int b = (int)blockIdx.x * kPostCols + c;
  const bool live = b < B;
  // ---- pass 1: column maximum, and the first sample that holds it (weight 1: the pivot of the translation moments) ----
  float m = -INFINITY, M;
  int jm = 0x7fffffff, jM;
  bool bad = false;
  if (live) column_max(logw, B, b, rg, S, kPostRows, m, jm, bad);
  block_column_max(red, arg, rg, c, m, jm, M, jM, bad);
  const bool skip = !live || bad || M == -INFINITY;
  // ---- pass 2: this row group's share of every sum; a sample of weight 0 is skipped, not multiplied (its pose may be a NaN) ----
  float acc[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) acc[a] = 0.f;
  float piv[3] = {0.f, 0.f, 0.f};
  const bool has_ref = ref != nullptr;
  if (!skip) {
    const float* pm = pose + ((size_t)jM * B + b) * P;
    piv[0] = pm[0]; piv[1] = pm[1]; piv[2] = pm[2];
    const float rx = has_ref ? ref[(size_t)b * P + 0] : 0.f, rz = has_ref ? ref[(size_t)b * P + 2] : 0.f;
    for (int j0 = rg; j0 < S; j0 += kPostRows * UNR) {
      float v[UNR], p[UNR][P];
#pragma unroll
      for (int k = 0; k < UNR; ++k) {
        const int j = j0 + k * kPostRows;
        const bool in = j < S;
        v[k] = in ? logw[(size_t)j * B + b] : -INFINITY;
        const float* pj = pose + ((size_t)(in ? j : 0) * B + b) * P;
#pragma unroll
        for (int i = 0; i < P; ++i) p[k][i] = pj[i];
      }
#pragma unroll
      for (int k = 0; k < UNR; ++k) {
        const float w = post_weight(v[k], M);
        if (w != 0.f) post_accumulate<DOF>(w, p[k], piv, has_ref, rx, rz, acc);
      }
    }
  }
#pragma unroll
  for (int a = 0; a < NA; ++a) part[(a * kPostRows + rg) * kPostCP + c] = acc[a];
  __syncthreads();
  // ---- the 32 row groups of (accumulator, column), ascending ----
  for (int idx = (int)threadIdx.x; idx < NA * kPostCols; idx += 512) {
    const int a = idx / kPostCols, cc = idx % kPostCols;
    float t = 0.f;
    for (int k = 0; k < kPostRows; ++k) t += part[(a * kPostRows + k) * kPostCP + cc];
    tot[idx] = t;
  }
  __syncthreads();
  // ---- one lane per object ----
  if (rg != 0 || !live) return;
  float* row = out + (size_t)b * EPROPNP_POSTERIOR_WORDS;
  if (skip) {
#pragma unroll
    for (int i = 0; i < EPROPNP_POSTERIOR_WORDS; ++i) row[i] = NAN;
    return;
  }
  float s[NA];
  const float inv = 1.0f / tot[c];
#pragma unroll
  for (int a = 1; a < NA; ++a) s[a] = tot[a * kPostCols + c] * inv;
  row[0] = piv[0] + s[1]; row[1] = piv[1] + s[2]; row[2] = piv[2] + s[3];
  row[3] = s[4] - s[1] * s[1]; row[4] = s[5] - s[1] * s[2]; row[5] = s[6] - s[1] * s[3];
  row[6] = s[7] - s[2] * s[2]; row[7] = s[8] - s[2] * s[3]; row[8] = s[9] - s[3] * s[3];
  row[9] = has_ref ? s[10] : NAN;
  if (DOF == 6) {
    float a[4][4], v[4][4];
    int idx = 11;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = i; j < 4; ++j) {
        a[i][j] = a[j][i] = s[idx];
        ++idx;
      }
    jacobi4(a, v);
    float lam = a[0][0], q[4] = {v[0][0], v[1][0], v[2][0], v[3][0]};
#pragma unroll
    for (int i = 1; i < 4; ++i) {
      const bool up = a[i][i] > lam;
      lam = up ? a[i][i] : lam;
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] = up ? v[k][i] : q[k];
    }
    const float nrm = 1.0f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    // the sign: towards pose_ref's quaternion, else the first non-zero component positive
    float sg;
    if (has_ref) {
      const float* rq = ref + (size_t)b * P + 3;
      sg = q[0] * rq[0] + q[1] * rq[1] + q[2] * rq[2] + q[3] * rq[3];
    } else {
      sg = q[0] != 0.f ? q[0] : (q[1] != 0.f ? q[1] : (q[2] != 0.f ? q[2] : q[3]));
    }
    const float f = (sg < 0.f) ? -nrm : nrm;
    row[10] = lam;
#pragma unroll
    for (int k = 0; k < 4; ++k) row[11 + k] = q[k] * f;
  } else {
    row[10] = sqrtf(s[11] * s[11] + s[12] * s[12]);
    row[11] = atan2f(s[12], s[11]);
    row[12] = 0.f; row[13] = 0.f; row[14] = 0.f;
  }
  row[15] = 0.f;
}

// Systematic resampling: draw r of object b is the first sample, in sample order, whose running sum of w exceeds (u_b + r) / R * W.
// Each row group owns a CONTIGUOUS chunk of ceil(S / 32) rows; the chunk totals go through LDS, every thread forms the running sum
// of the totals in the same ascending order (its own prefix, the next group's, the total W), then walks its chunk.
// The draws of a sample are [n(c_before), n(c_after)) with ONE monotone fp32 function of the running sum c,
//     n(c) = clamp(ceil(fma(c, R / W, -u)), 0, R)         (the number of thresholds below c),
// and a bound is computed once and shared by both neighbours: inside a chunk the walk carries it from sample to sample; between
// chunks it is n(prefix of the next group), which the last non-zero-weight sample of the chunk takes as its upper bound whatever
// its own running sum says (the walk's sum and the prefix round differently), and which the walk's own bounds are clamped to; the
// last chunk that holds any weight closes at R ((u + R - 1) / R can round to 1).  So the ranges tile [0, R): every index[r, b] is
// written exactly once.  Zero-weight samples own no range.  Bad and empty columns: index -1, NaN poses.
// The gather runs after the block has met, over all 32 row groups: draw r of the column by row group r % 32.
__global__ __launch_bounds__(512) void posterior_resample_kernel(const float* __restrict__ pose, const float* __restrict__ logw,
                                                                  const float* __restrict__ u, unsigned long long seed,
                                                                  unsigned long long offset, int S, int B, int P, int R,
                                                                  int* index, float* __restrict__ out) {
  __shared__ float red[kPostRows * kPostCP];
  __shared__ int arg[kPostRows * kPostCP];
  __shared__ float tots[kPostRows * kPostCP];
  const int c = (int)(threadIdx.x % kPostCols), rg = (int)(threadIdx.x / kPostCols);
  const int b = (int)blockIdx.x * kPostCols + c;
  const bool live = b < B;
  const int chunk = (S + kPostRows - 1) / kPostRows;
  const int lo = min(rg * chunk, S), hi = min(lo + chunk, S);
  float m = -INFINITY, M;
  int jm = 0x7fffffff, jM;
  bool bad = false;
  if (live) column_max(logw, B, b, lo, hi, 1, m, jm, bad);
  block_column_max(red, arg, rg, c, m, jm, M, jM, bad);
  const bool skip = !live || bad || M == -INFINITY;
  // ---- the chunk's total ----
  float acc = 0.f;
  if (!skip)
    for (int j = lo; j < hi; ++j) acc += post_weight(logw[(size_t)j * B + b], M);
  tots[rg * kPostCP + c] = acc;
  __syncthreads();
  if (!skip) {
    // ---- exclusive scan of the chunk totals, in ONE order for every thread of the column ----
    float run = 0.f, pre = 0.f, post = 0.f;
    int last = 0;
    for (int k = 0; k < kPostRows; ++k) {
      const float t = tots[k * kPostCP + c];
      if (k == rg) pre = run;
      run += t;
      if (k == rg) post = run;
      if (t > 0.f) last = k;
    }
    float uu;
    if (u != nullptr) {
      uu = u[b];
    } else {
      const Philox4 r = philox4x32_10((uint32_t)b, 0u, (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed,
                                      (uint32_t)(seed >> 32) ^ 0x2545f491u);
      uu = (float)(r.v[0] >> 8) * (1.0f / 16777216.0f);
    }
    uu = fminf(fmaxf(uu, 0.f), 1.0f - 1.0f / 16777216.0f);      // [0, 1) whatever was passed (a NaN: 0): n(0) = 0
    const float scale = (float)R / run;
    auto count_below = [=](float cs) {
      const float x = ceilf(fmaf(cs, scale, -uu));
      return (x >= (float)R) ? R : ((x > 0.f) ? (int)x : 0);
    };
    const int end = (rg >= last) ? R : count_below(post);
    int lo_r = (rg > last) ? R : count_below(pre);
    float cs = pre;
    int pj = -1;
    for (int j = lo; j <= hi; ++j) {
      const float w = (j < hi) ? post_weight(logw[(size_t)j * B + b], M) : 1.0f;      // (j == hi: closes the chunk's last sample)
      if (w != 0.f) {
        if (pj >= 0) {
          const int hi_r = (j < hi) ? min(count_below(cs), end) : end;
          for (int r = lo_r; r < hi_r; ++r) index[(size_t)r * B + b] = pj;
          lo_r = hi_r;
        }
        pj = j;
        cs += w;
      }
    }
  }
  __syncthreads();      // the column's index entries were written by its 32 row groups: visible to the block from here
  if (!live) return;
  for (int r = rg; r < R; r += kPostRows) {
    int j = -1;
    if (skip) index[(size_t)r * B + b] = -1;
    else if (out != nullptr) j = index[(size_t)r * B + b];
    if (j >= S) j = -1;      // (cannot happen: every entry was written above; an address is never formed from anything else)
    if (out != nullptr) {
      float* dst = out + ((size_t)r * B + b) * P;
      const float* src = pose + ((size_t)(j < 0 ? 0 : j) * B + b) * P;
      for (int i = 0; i < P; ++i) dst[i] = (j < 0) ? NAN : src[i];
    }
  }
}

// ---- posterior modes: quick-shift clustering of the weighted samples (include/epropnp_hip.h: epropnp_posterior_modes) -------------
// Three launches on the caller's stream, the caller's density / parent / labels between them:
//   posterior_modes_pair_kernel<.., false> : density f_i = sum_j w_j exp(-D_ij / 2) / W
//   posterior_modes_pair_kernel<.., true>  : parent_i = the nearest j of higher density within `link`
//   posterior_modes_label_kernel           : labels by pointer jumping on parent, masses, the heaviest max_modes modes
// The pair kernels are the S^2 work.  A workgroup of up to 256 threads owns (object, part): it finds the column's maximum and W (every part
// of an object in the same order: the same bits), stages the column -- poses, weights, in the link pass the densities -- into LDS in
// tiles of up to kModeTile samples (one tile, staged once, up to that many samples; beyond it the tiles stream from global memory
// once per chunk of i), and keeps IPL samples i per lane in registers while j runs over broadcast LDS reads.  Few objects: the
// chunks of i are dealt to `nsplit` workgroups per object, neighbours in the XCD-aware object order.  The exponent works in exp2
// with -1/2 log2 e folded into 1 / h^2; D is compared in the same scaled units (E = 1/2 log2 e D) in both passes.
// A sample of weight 0 is staged as a zero pose with weight 0 / density -inf: it adds nothing and is nobody's parent, without a
// branch in the pair loop.
constexpr int kModeThreads = 256, kModeTile = 4096, kModeSumBlock = 32;
constexpr double kHalfLog2e = 0.72134752044448170368;

// The column's maximum M, W = sum_j exp(logw_j - M) in a fixed order (thread-strided partial sums, then the threads ascending), and
// whether the column is bad (a NaN / +inf log-weight, nothing but -inf).  red: blockDim.x floats of LDS; two barriers.
PNP_FN void modes_column_stats(const float* __restrict__ logw, int S, int B, int b, float* red, float& M, float& W, bool& bad) {
  const int tid = (int)threadIdx.x, T = (int)blockDim.x;
  float m = -INFINITY;
  bool poison = false;
  for (int j = tid; j < S; j += T) {
    const float v = logw[(size_t)j * B + b];
    poison = poison || (v != v) || (v == INFINITY);
    m = (v > m) ? v : m;
  }
  red[tid] = poison ? NAN : m;
  __syncthreads();
  M = -INFINITY;
  bad = false;
  for (int k = 0; k < T; ++k) {
    const float v = red[k];
    bad = bad || (v != v);
    M = (v > M) ? v : M;
  }
  bad = bad || M == -INFINITY;
  __syncthreads();
  float acc = 0.f;
  if (!bad)
    for (int j = tid; j < S; j += T) acc += post_weight(logw[(size_t)j * B + b], M);
  red[tid] = acc;
  __syncthreads();
  W = 0.f;
  for (int k = 0; k < T; ++k) W += red[k];
}

// 1/2 log2 e / h^2 of the object's two bandwidths; false for a bandwidth that is not finite and > 0 (or so small that the factor
// is not finite)
PNP_FN bool modes_scales(const float* __restrict__ bw, int b, float& kt, float& kr) {
  const float ht = bw[2 * (size_t)b], hr = bw[2 * (size_t)b + 1];
  kt = (float)(kHalfLog2e / ((double)ht * (double)ht));
  kr = (float)(kHalfLog2e / ((double)hr * (double)hr));
  return ht > 0.f && ht < INFINITY && hr > 0.f && hr < INFINITY && kt < INFINITY && kr < INFINITY;
}

// E_ij = 1/2 log2 e D_ij; pj: the staged record (pose, weight) of j
template <int DOF>
PNP_FN float modes_pair_energy(const float (&pi)[PoseLen<DOF>::value], const float* pj, float kt, float kr) {
  const float dx = pi[0] - pj[0], dy = pi[1] - pj[1], dz = pi[2] - pj[2];
  const float dt2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
  float rho;
  if constexpr (DOF == 6) {
    float dm = 0.f, dp = 0.f;
#pragma unroll
    for (int k = 3; k < 7; ++k) {
      const float a = pi[k] - pj[k], c = pi[k] + pj[k];
      dm = fmaf(a, a, dm);
      dp = fmaf(c, c, dp);
    }
    const float d2 = fminf(dm, dp);
    rho = d2 * (4.0f - d2);
  } else {
    const float s = sinf(0.5f * (pi[3] - pj[3]));
    rho = 4.0f * s * s;
  }
  return fmaf(kr, rho, kt * dt2);
}

template <int DOF, int IPL, bool LINK>
__global__ __launch_bounds__(kModeThreads) void posterior_modes_pair_kernel(const float* __restrict__ pose,
                                                                            const float* __restrict__ logw,
                                                                            const float* __restrict__ bw, int S, int B, int nsplit,
                                                                            int tile, float link_e, float* density, int* parent) {
  constexpr int P = PoseLen<DOF>::value, R = (DOF == 6) ? 8 : 5;
  PNP_DYN_SMEM(float, rec);                    // rec[tile][R]: pose, weight | dens[tile] (link pass)
  float* dens = rec + (size_t)tile * R;
  __shared__ float red[kModeThreads];
  const int v = object_of_block(B * nsplit);
  if (v >= B * nsplit) return;
  const int b = v / nsplit, part = v - b * nsplit, tid = (int)threadIdx.x, T = (int)blockDim.x, CH = T * IPL;
  float M, W, kt, kr;
  bool bad;
  modes_column_stats(logw, S, B, b, red, M, W, bad);
  bad = !modes_scales(bw, b, kt, kr) || bad;
  const int nch = (S + CH - 1) / CH, ntile = (S + tile - 1) / tile;
  for (int c = part; c < nch; c += nsplit) {
    float pi[IPL][P], wi[IPL], fi[IPL], acc[IPL], run[IPL], best_e[IPL];
    int best[IPL];
#pragma unroll
    for (int k = 0; k < IPL; ++k) {
      const int i = c * CH + k * T + tid;
      const size_t at = (size_t)(i < S ? i : S - 1) * B + b;
      wi[k] = (i < S && !bad) ? post_weight(logw[at], M) : 0.f;
#pragma unroll
      for (int e = 0; e < P; ++e) pi[k][e] = (wi[k] != 0.f) ? pose[at * P + e] : 0.f;
      fi[k] = (LINK && wi[k] != 0.f) ? density[at] : 0.f;
      acc[k] = 0.f;
      run[k] = 0.f;
      best_e[k] = INFINITY;
      best[k] = -1;
    }
    for (int t = 0; t < ntile && !bad; ++t) {
      const int j0 = t * tile, nj = min(tile, S - j0);
      if (ntile > 1 || c == part) {
        __syncthreads();                       // the previous tile has been read by every lane
        for (int jj = tid; jj < nj; jj += T) {
          const size_t at = (size_t)(j0 + jj) * B + b;
          const float w = post_weight(logw[at], M);
#pragma unroll
          for (int e = 0; e < P; ++e) rec[(size_t)jj * R + e] = (w != 0.f) ? pose[at * P + e] : 0.f;
          rec[(size_t)jj * R + P] = w;
          if (LINK) dens[jj] = (w != 0.f) ? density[at] : -INFINITY;
        }
        __syncthreads();
      }
#pragma unroll 4
      for (int jj = 0; jj < nj; ++jj) {
        const float* pj = rec + (size_t)jj * R;
        float rj[R];
        if constexpr (DOF == 6) {
          const float4 lo = *reinterpret_cast<const float4*>(pj), hi = *reinterpret_cast<const float4*>(pj + 4);
          rj[0] = lo.x; rj[1] = lo.y; rj[2] = lo.z; rj[3] = lo.w;
          rj[R - 4] = hi.x; rj[R - 3] = hi.y; rj[R - 2] = hi.z; rj[R - 1] = hi.w;
        } else {
#pragma unroll
          for (int e = 0; e < R; ++e) rj[e] = pj[e];
        }
        const float fj = LINK ? dens[jj] : 0.f;
#pragma unroll
        for (int k = 0; k < IPL; ++k) {
          const float E = modes_pair_energy<DOF>(pi[k], rj, kt, kr);
          if (LINK) {
            // ascending j and a strict `<`: ties in D go to the lowest j
            const int i = c * CH + k * T + tid, j = j0 + jj;
            const bool up = (fj > fi[k]) || (fj == fi[k] && j < i);
            if (up && E <= link_e && E < best_e[k]) { best_e[k] = E; best[k] = j; }
          } else {
            run[k] = fmaf(rj[P], __builtin_amdgcn_exp2f(-E), run[k]);
          }
        }
        // the sum runs in blocks of kModeSumBlock consecutive j (of the column, not of the tile): the rounding error grows with
        // kModeSumBlock + S / kModeSumBlock additions instead of S, in the same order whatever the tiles are
        if (!LINK && ((j0 + jj) & (kModeSumBlock - 1)) == kModeSumBlock - 1) {
#pragma unroll
          for (int k = 0; k < IPL; ++k) { acc[k] += run[k]; run[k] = 0.f; }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < IPL; ++k) acc[k] += run[k];
#pragma unroll
    for (int k = 0; k < IPL; ++k) {
      const int i = c * CH + k * T + tid;
      if (i >= S) continue;
      const bool in = wi[k] != 0.f;
      if (LINK) parent[(size_t)i * B + b] = in ? (best[k] < 0 ? i : best[k]) : -1;
      else density[(size_t)i * B + b] = in ? acc[k] / W : NAN;
    }
  }
}

// Labels, masses and the selection of one object.  LDS: the column's labels and weights live in LDS (up to kModeLabelCap samples);
// otherwise everything lives in the caller's arrays (any S):
//   labels <- parent, then ceil(log2 S) rounds of labels[i] = labels[labels[i]] in place (a value read while another lane replaces it
//   is an ancestor either way, and after that many rounds every chain has collapsed: the result does not depend on the interleaving);
//   the lane that owns a root sums the weights of its tree in sample order and parks the mass in the root's parent word (a root is
//   its own parent: the word is restored at the end); a root's rank is the number of roots that are heavier, or as heavy with a
//   lower index.
constexpr int kModeLabelCap = 16384;

template <bool LDS>
__global__ __launch_bounds__(kModeThreads) void posterior_modes_label_kernel(const float* __restrict__ pose,
                                                                             const float* __restrict__ logw,
                                                                             const float* __restrict__ bw, int S, int B, int P,
                                                                             int MM, int* parent, int* labels, int* num_modes,
                                                                             int* mode_index, float* mode_mass, float* mode_poses) {
  PNP_DYN_SMEM(int, col);                      // LDS: labels[S] | weights[S]
  __shared__ float red[kModeThreads];
  __shared__ int count;
  const int b = object_of_block(B);
  if (b >= B) return;
  const int tid = (int)threadIdx.x, T = (int)blockDim.x;
  float M, W, kt, kr;
  bool bad;
  modes_column_stats(logw, S, B, b, red, M, W, bad);
  bad = !modes_scales(bw, b, kt, kr) || bad;
  auto blank_rows = [&](int from, float mass) {
    for (int m = from + tid; m < MM; m += T) {
      mode_index[(size_t)m * B + b] = -1;
      mode_mass[(size_t)m * B + b] = mass;
      if (mode_poses != nullptr)
        for (int e = 0; e < P; ++e) mode_poses[((size_t)m * B + b) * P + e] = NAN;
    }
  };
  if (bad) {
    for (int i = tid; i < S; i += T) labels[(size_t)i * B + b] = -1;
    blank_rows(0, NAN);
    if (tid == 0) num_modes[b] = 0;
    return;
  }
  volatile int* lab = LDS ? col : labels + b;
  const size_t ls = LDS ? 1 : (size_t)B;
  volatile int* par = parent + b;
  const float* wl = reinterpret_cast<const float*>(col + S);
  auto weight = [&](int j) { return LDS ? wl[j] : post_weight(logw[(size_t)j * B + b], M); };
  if (tid == 0) count = 0;
  for (int i = tid; i < S; i += T) {
    lab[i * ls] = par[(size_t)i * B];
    if (LDS) reinterpret_cast<float*>(col + S)[i] = post_weight(logw[(size_t)i * B + b], M);
  }
  for (int span = 1; span < S; span *= 2) {
    __threadfence();
    __syncthreads();
    for (int i = tid; i < S; i += T) {
      const int l = lab[i * ls];
      if (l >= 0 && l < S) lab[i * ls] = lab[l * ls];
    }
  }
  __threadfence();
  __syncthreads();
  // ---- masses: a root's lane, its tree in sample order ----
  int roots = 0;
  for (int i = tid; i < S; i += T) {
    if (lab[i * ls] != i) continue;
    float sum = 0.f;
    for (int j = 0; j < S; ++j)
      if (lab[j * ls] == i) sum += weight(j);
    par[(size_t)i * B] = __float_as_int(sum / W);
    ++roots;
  }
  if (roots != 0) atomicAdd(&count, roots);
  __threadfence();
  __syncthreads();
  const int nm = count, shown = min(nm, MM);
  // ---- ranks: heavier first, then the lower root index ----
  for (int i = tid; i < S; i += T) {
    if (lab[i * ls] != i) continue;
    const float mass = __int_as_float(par[(size_t)i * B]);
    int rank = 0;
    for (int j = 0; j < S && rank < MM; ++j) {
      if (j == i || lab[j * ls] != j) continue;
      const float mj = __int_as_float(par[(size_t)j * B]);
      rank += (mj > mass || (mj == mass && j < i)) ? 1 : 0;
    }
    if (rank < MM) {
      mode_index[(size_t)rank * B + b] = i;
      mode_mass[(size_t)rank * B + b] = mass;
      if (mode_poses != nullptr)
        for (int e = 0; e < P; ++e) mode_poses[((size_t)rank * B + b) * P + e] = pose[((size_t)i * B + b) * P + e];
    }
  }
  blank_rows(shown, 0.f);
  if (tid == 0) num_modes[b] = nm;
  __syncthreads();                             // every rank has been formed: the roots' parent words go back
  for (int i = tid; i < S; i += T) {
    const int l = lab[i * ls];
    if (l == i) par[(size_t)i * B] = i;
    if (LDS) labels[(size_t)i * B + b] = l;
  }
}

// (IPL, nsplit) of the pair kernels: two samples per lane halve the LDS traffic per pair; with few objects one sample per lane and
// the chunks of i dealt to several workgroups per object fill the device instead.  EPROPNP_TUNE="modes_plan=<ipl>,<nsplit>" and
// "modes_tile=<samples>" override (the shape tests: the split and the streamed tiles at small sizes); an invalid value is ignored.
static void modes_plan(int S, int B, int& ipl, int& nsplit, int& tile, int& threads) {
  const long want = 2L * device_cu_count();
  ipl = ((long)B * ((S + 2 * kModeThreads - 1) / (2 * kModeThreads)) >= want) ? 2 : 1;
  int ov[2];
  const bool forced = tune_ints("modes_plan", ov, 2) && (ov[0] == 1 || ov[0] == 2) && ov[1] >= 1;
  if (forced) ipl = ov[0];
  threads = 64 * ((S + 64 * ipl - 1) / (64 * ipl));      // a short column: no more waves than it has samples for
  threads = threads > kModeThreads ? kModeThreads : threads;
  const int nch = (S + threads * ipl - 1) / (threads * ipl);
  long ns = forced ? ov[1] : (want + B - 1) / B;
  nsplit = (int)(ns < 1 ? 1 : (ns > nch ? nch : ns));
  tile = S < kModeTile ? S : kModeTile;
  if (tune_ints("modes_tile", ov, 1) && ov[0] >= 1 && ov[0] <= kModeTile) tile = ov[0] < S ? ov[0] : S;
}

int launch_posterior_modes(const float* pose, const float* logw, const float* bw, int S, int B, int dof, float link, int MM,
                           float* density, int32_t* parent, int32_t* labels, int32_t* num_modes, int32_t* mode_index,
                           float* mode_mass, float* mode_poses, hipStream_t st) {
  if (B == 0) return EPROPNP_OK;
  if (B < 0) return fail(EPROPNP_EINVAL, "epropnp_posterior_modes: num_obj must be >= 0, got %d", B);
  if (!pose || !logw || !bw || !density || !parent || !labels || !num_modes || !mode_index || !mode_mass)
    return fail(EPROPNP_EINVAL, "epropnp_posterior_modes: NULL pointer");
  if (dof != 4 && dof != 6) return fail(EPROPNP_EINVAL, "epropnp_posterior_modes: dof must be 4 or 6, got %d", dof);
  if (S < 1) return fail(EPROPNP_EINVAL, "epropnp_posterior_modes: mc_samples must be >= 1, got %d", S);
  if (MM < 1) return fail(EPROPNP_EINVAL, "epropnp_posterior_modes: max_modes must be >= 1, got %d", MM);
  if (!(link > 0.f && link < INFINITY))
    return fail(EPROPNP_EINVAL, "epropnp_posterior_modes: link must be finite and > 0, got %g", (double)link);
  int ipl, nsplit, tile, threads;
  modes_plan(S, B, ipl, nsplit, tile, threads);
  if ((long)B * nsplit > 0x7fffff00L) return fail(EPROPNP_EINVAL, "epropnp_posterior_modes: num_obj (%d) is too large", B);
  const float link_e = (float)(kHalfLog2e * (double)link * (double)link);
  const dim3 grid(padded_object_grid(B * nsplit)), block(threads);
  const size_t rec = (size_t)tile * (dof == 6 ? 8 : 5) * sizeof(float);
  auto pair = [&](auto DOF, auto IPL, auto LINK) {
    auto kern = posterior_modes_pair_kernel<decltype(DOF)::value, decltype(IPL)::value, decltype(LINK)::value>;
    const size_t smem = rec + (decltype(LINK)::value ? (size_t)tile * sizeof(float) : 0);
    allow_dynamic_lds((const void*)kern, smem);
    PNP_LAUNCH(kern, grid, block, smem, st, pose, logw, bw, S, B, nsplit, tile, link_e, density, (int*)parent);
  };
  auto both = [&](auto DOF, auto IPL) {
    pair(DOF, IPL, std::false_type());
    pair(DOF, IPL, std::true_type());
  };
  typedef std::integral_constant<int, 1> One;
  typedef std::integral_constant<int, 2> Two;
  if (dof == 6) { if (ipl == 2) both(std::integral_constant<int, 6>(), Two()); else both(std::integral_constant<int, 6>(), One()); }
  else { if (ipl == 2) both(std::integral_constant<int, 4>(), Two()); else both(std::integral_constant<int, 4>(), One()); }
  int rc = check_launch("posterior_modes_pair_kernel");
  if (rc != EPROPNP_OK) return rc;
  // (EPROPNP_TUNE="modes_label_global": the any-S variant at a size that fits LDS, for the shape tests)
  if (S <= kModeLabelCap && !tune_flag("modes_label_global")) {
    const size_t smem = (size_t)S * (sizeof(int) + sizeof(float));
    allow_dynamic_lds((const void*)posterior_modes_label_kernel<true>, smem);
    PNP_LAUNCH(posterior_modes_label_kernel<true>, dim3(padded_object_grid(B)), block, smem, st, pose, logw, bw, S, B,
               dof == 6 ? 7 : 4, MM, (int*)parent, (int*)labels, (int*)num_modes, (int*)mode_index, mode_mass, mode_poses);
  } else {
    PNP_LAUNCH(posterior_modes_label_kernel<false>, dim3(padded_object_grid(B)), block, 0, st, pose, logw, bw, S, B,
               dof == 6 ? 7 : 4, MM, (int*)parent, (int*)labels, (int*)num_modes, (int*)mode_index, mode_mass, mode_poses);
  }
  return check_launch("posterior_modes_label_kernel");
}

int launch_posterior_summary(const float* pose, const float* logw, const float* ref, int S, int B, int dof, float* out,
                             hipStream_t st) {
  if (B == 0) return EPROPNP_OK;
  if (B < 0) return fail(EPROPNP_EINVAL, "epropnp_posterior_summary: num_obj must be >= 0, got %d", B);
  if (!pose || !logw || !out) return fail(EPROPNP_EINVAL, "epropnp_posterior_summary: NULL pointer");
  if (dof != 4 && dof != 6) return fail(EPROPNP_EINVAL, "epropnp_posterior_summary: dof must be 4 or 6, got %d", dof);
  if (S < 1) return fail(EPROPNP_EINVAL, "epropnp_posterior_summary: mc_samples must be >= 1, got %d", S);
  const dim3 grid((B + kPostCols - 1) / kPostCols);
  if (dof == 6) PNP_LAUNCH(posterior_summary_kernel<6>, grid, dim3(512), 0, st, pose, logw, ref, S, B, out);
  else PNP_LAUNCH(posterior_summary_kernel<4>, grid, dim3(512), 0, st, pose, logw, ref, S, B, out);
  return check_launch("posterior_summary_kernel");
}

int launch_posterior_resample(const float* pose, const float* logw, int S, int B, int dof, int R, const float* u,
                              unsigned long long seed, unsigned long long offset, int32_t* index, float* poses, hipStream_t st) {
  if (B == 0) return EPROPNP_OK;
  if (B < 0) return fail(EPROPNP_EINVAL, "epropnp_posterior_resample: num_obj must be >= 0, got %d", B);
  if (!pose || !logw || !index) return fail(EPROPNP_EINVAL, "epropnp_posterior_resample: NULL pointer");
  if (dof != 4 && dof != 6) return fail(EPROPNP_EINVAL, "epropnp_posterior_resample: dof must be 4 or 6, got %d", dof);
  if (S < 1) return fail(EPROPNP_EINVAL, "epropnp_posterior_resample: mc_samples must be >= 1, got %d", S);
  if (R < 1) return fail(EPROPNP_EINVAL, "epropnp_posterior_resample: num_draws must be >= 1, got %d", R);
  PNP_LAUNCH(posterior_resample_kernel, dim3((B + kPostCols - 1) / kPostCols), dim3(512), 0, st, pose, logw, u, seed, offset, S, B,
             dof == 6 ? 7 : 4, R, (int*)index, poses);
  return check_launch("posterior_resample_kernel");
}

}  // namespace pnp
