// metrics_kernels.hip -- pose-error metrics of the 6-DoF evaluation on the device (include/epropnp_hip.h: epropnp_pose_errors):
// rotation and translation error, ARP-2D, ADD and ADD-S of R x B pose rows against B ground-truth poses, over packed object models
// (EPro-PnP-6DoF lib/utils/eval.py:585-736 -- re / te / arp_2d / add / adi / calc_all_errs -- which run per object on the host,
// ADD-S through one scipy cKDTree per pose).
//
//   pose_errors_nn_kernel     : ADD-S of the rows whose object is flagged symmetric (the others leave at once).  Evaluated in the
//       ESTIMATE's model frame: q_i = R_est^T R_gt p_i + R_est^T (t_gt - t_est), then min_j |q_i - p_j| -- the distances of
//       min_j |(R_gt p_i + t_gt) - (R_est p_j + t_est)|, with the RAW model points as candidates: the same for every pose of a
//       model, staged into LDS as they are, no transformed copy of the model per pose anywhere.  A workgroup owns (row, part) and
//       takes the row's query tiles part, part + parts, ..: kNnQpl queries per lane in registers, the model streaming through LDS
//       in tiles of kNnCandTile points padded to float4; every lane reads the same candidate (one broadcast 128-bit LDS read per
//       kNnQpl pairs).  The squared distance is the direct form (qx - px)^2 + ..: a good pose has d^2 ~ 1e-6 against |p|^2 ~ 1e-2,
//       and |q|^2 + |p|^2 - 2 q.p (the form a matrix instruction could evaluate) keeps half the mantissa of it -- no MFMA here.
//       Each query tile leaves sum sqrt(min d^2), reduced in a fixed order, in the caller's scratch.
//   pose_errors_stream_kernel : one workgroup per row, launched behind the first: rot_deg, trans, one strided pass over the model for
//       ADD and ARP-2D (fixed-order reductions), and the finishing step of ADD-S -- the row's tile sums added in tile order, so that
//       the bits do not depend on how the tiles were dealt out.  Writes all eight words of the row.
//
// The row set-up (metric_row_setup) runs once per workgroup, on one lane, in fp64: normalised quaternions, the relative rotation
// from the relative quaternion, and every DIFFERENCE the metrics are made of -- R_est - R_gt, t_est - t_gt, R_rel - I -- formed
// there and rounded to fp32 once.  ADD is |(R_est - R_gt) p + (t_est - t_gt)| and the ADD-S query is p + ((R_rel - I) p + t_rel):
// neither loses the 1e-7 * depth that transforming the points by both poses and subtracting would (at the Det head's 50 m more
// than a good pose's whole ADD), and identical poses give exact zeros.  No atomics, no allocation, no synchronisation.
#include "pnp_host.h"

namespace pnp {

constexpr int kMetThreads = 256, kNnQpl = 4;
constexpr int kNnQueryTile = EPROPNP_POSE_ERROR_QUERY_TILE, kNnCandTile = EPROPNP_POSE_ERROR_CAND_TILE;
static_assert(kNnQueryTile == kMetThreads * kNnQpl, "a query tile is kNnQpl queries per lane");
static_assert(kNnCandTile % 8 == 0, "the last candidate tile is padded to the unroll of the pair loop");
constexpr double kRadToDeg = 57.295779513082320877, kPi = 3.14159265358979323846;

// What a row's workgroup needs of its two poses, its model and its camera (LDS, written by lane 0).
struct MetricRow {
  int ok;             // poses finite, model_id inside [0, C), count >= 1: otherwise the row's metrics are NaN
  int sym, first, count, has_cam;
  float rot_deg, trans;
  float dR[9], dt[3];                          // R_est - R_gt, t_est - t_gt                      (ADD)
  float KdR[9], Kdt[3], KRg[9], Ktg[3];        // K (R_est' - R_gt), K (t_est - t_gt), K R_gt, K t_gt  (ARP-2D; R_est' half-turned or not)
  float dQ[9], tq[3];                          // R_est^T R_gt - I, R_est^T (t_gt - t_est)        (ADD-S)
};

PNP_FN void quat_to_rot_f64(const double (&q)[4], double (&R)[9]) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// r = conj(e) g: the quaternion of R_est^T R_gt.  e == g gives a vector part of exactly 0 -- as long as every product is rounded on
// its own: contracted, e0 g1 - g0 e1 is fma(e0, g1, -round(g0 e1)), the rounding error of a product instead of 0.
PNP_FN void quat_relative(const double (&e)[4], const double (&g)[4], double (&r)[4]) {
#pragma clang fp contract(off)
  r[0] = e[0] * g[0] + e[1] * g[1] + e[2] * g[2] + e[3] * g[3];
  r[1] = e[0] * g[1] - g[0] * e[1] - (e[2] * g[3] - e[3] * g[2]);
  r[2] = e[0] * g[2] - g[0] * e[2] - (e[3] * g[1] - e[1] * g[3]);
  r[3] = e[0] * g[3] - g[0] * e[3] - (e[1] * g[2] - e[2] * g[1]);
}

// rotation angle of a unit quaternion in degrees, q and -q alike: 2 atan2(|v|, |w|) (no acos of a trace near 3)
PNP_FN double quat_angle_deg(const double (&r)[4]) {
  return 2.0 * atan2(sqrt(r[1] * r[1] + r[2] * r[2] + r[3] * r[3]), fabs(r[0])) * kRadToDeg;
}

PNP_FN double wrap_pi(double a) { return a - 2.0 * kPi * rint(a / (2.0 * kPi)); }

PNP_FN void mat3_mul_f64(const double (&A)[9], const double (&B)[9], float (&C)[9]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) C[3 * r + c] = (float)(A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c]);
}

template <int DOF>
PNP_FN void metric_row_setup(const float* __restrict__ pe, const float* __restrict__ pg, const int32_t* __restrict__ range, int C,
                             const int32_t* __restrict__ model_id, const float* __restrict__ cam,
                             const uint8_t* __restrict__ symmetric, const uint8_t* __restrict__ half_turn, int b, MetricRow& s) {
  constexpr int P = PoseLen<DOF>::value;
  const int mid = model_id ? model_id[b] : 0;
  bool ok = mid >= 0 && mid < C;
  const int first = ok ? range[2 * mid] : 0, count = ok ? range[2 * mid + 1] : 0;
  ok = ok && first >= 0 && count >= 1;
  double chk = 0.0;                            // a NaN as soon as one component of either pose is not finite
#pragma unroll
  for (int i = 0; i < P; ++i) chk += 0.0 * (double)pe[i] + 0.0 * (double)pg[i];
  const double te[3] = {pe[0], pe[1], pe[2]}, tg[3] = {pg[0], pg[1], pg[2]};
  const double dtd[3] = {te[0] - tg[0], te[1] - tg[1], te[2] - tg[2]};
  double Re[9], Ra[9], Rg[9], dQ[9], deg;      // Ra: the estimate ARP-2D sees (half-turned or not)
  const bool flip_on = half_turn != nullptr && half_turn[b] != 0;
  if (DOF == 6) {
    double e[4], g[4], r[4];
    const double ne = sqrt((double)pe[3] * pe[3] + (double)pe[4] * pe[4] + (double)pe[5] * pe[5] + (double)pe[6] * pe[6]);
    const double ng = sqrt((double)pg[3] * pg[3] + (double)pg[4] * pg[4] + (double)pg[5] * pg[5] + (double)pg[6] * pg[6]);
    ok = ok && ne > 0.0 && ng > 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { e[i] = (double)pe[3 + i] / ne; g[i] = (double)pg[3 + i] / ng; }
    quat_relative(e, g, r);
    deg = quat_angle_deg(r);
    quat_to_rot_f64(e, Re);
    quat_to_rot_f64(g, Rg);
    // R(r) - I: every entry a product with the vector part, exactly 0 for identical poses
    dQ[0] = -2.0 * (r[2] * r[2] + r[3] * r[3]); dQ[1] = 2.0 * (r[1] * r[2] - r[0] * r[3]);  dQ[2] = 2.0 * (r[1] * r[3] + r[0] * r[2]);
    dQ[3] = 2.0 * (r[1] * r[2] + r[0] * r[3]);  dQ[4] = -2.0 * (r[1] * r[1] + r[3] * r[3]); dQ[5] = 2.0 * (r[2] * r[3] - r[0] * r[1]);
    dQ[6] = 2.0 * (r[1] * r[3] - r[0] * r[2]);  dQ[7] = 2.0 * (r[2] * r[3] + r[0] * r[1]);  dQ[8] = -2.0 * (r[1] * r[1] + r[2] * r[2]);
    if (flip_on && deg > 90.0) {
      // R_est diag(-1, -1, 1) = R(e (0, 0, 0, 1))
      const double f[4] = {-e[3], e[2], -e[1], e[0]};
      quat_relative(f, g, r);
      deg = quat_angle_deg(r);
      quat_to_rot_f64(f, Ra);
    } else {
#pragma unroll
      for (int i = 0; i < 9; ++i) Ra[i] = Re[i];
    }
  } else {
    const double ye = pe[3], yg = pg[3];
    double d = wrap_pi(ye - yg);
    deg = fabs(d) * kRadToDeg;
    const double ce = cos(ye), se = sin(ye), cg = cos(yg), sg = sin(yg);
    const double Re_[9] = {ce, 0.0, se, 0.0, 1.0, 0.0, -se, 0.0, ce}, Rg_[9] = {cg, 0.0, sg, 0.0, 1.0, 0.0, -sg, 0.0, cg};
#pragma unroll
    for (int i = 0; i < 9; ++i) { Re[i] = Re_[i]; Ra[i] = Re_[i]; Rg[i] = Rg_[i]; dQ[i] = 0.0; }
    // R_est^T R_gt = Ry(yg - ye); cos - 1 without the cancellation
    const double h = sin(0.5 * (yg - ye)), sd = sin(yg - ye);
    dQ[0] = -2.0 * h * h; dQ[2] = sd; dQ[6] = -sd; dQ[8] = -2.0 * h * h;
    if (flip_on && deg > 90.0) {
      d = wrap_pi(ye + kPi - yg);
      deg = fabs(d) * kRadToDeg;
      Ra[0] = -ce; Ra[2] = -se; Ra[6] = se; Ra[8] = -ce;      // yaw + pi
    }
  }
  ok = ok && chk == 0.0;
  s.ok = ok ? 1 : 0;
  s.sym = (symmetric != nullptr && symmetric[b] != 0) ? 1 : 0;
  s.first = first;
  s.count = count;
  s.has_cam = cam != nullptr ? 1 : 0;
  s.rot_deg = (float)deg;
  s.trans = (float)sqrt(dtd[0] * dtd[0] + dtd[1] * dtd[1] + dtd[2] * dtd[2]);
#pragma unroll
  for (int i = 0; i < 9; ++i) { s.dR[i] = (float)(Re[i] - Rg[i]); s.dQ[i] = (float)dQ[i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    s.dt[i] = (float)dtd[i];
    s.tq[i] = (float)-(Re[i] * dtd[0] + Re[3 + i] * dtd[1] + Re[6 + i] * dtd[2]);      // R_est^T (t_gt - t_est)
  }
  if (cam != nullptr) {
    double K[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) K[i] = cam[(size_t)b * 9 + i];
    double dRa[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) dRa[i] = Ra[i] - Rg[i];
    mat3_mul_f64(K, dRa, s.KdR);
    mat3_mul_f64(K, Rg, s.KRg);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      s.Kdt[i] = (float)(K[3 * i] * dtd[0] + K[3 * i + 1] * dtd[1] + K[3 * i + 2] * dtd[2]);
      s.Ktg[i] = (float)(K[3 * i] * tg[0] + K[3 * i + 1] * tg[1] + K[3 * i + 2] * tg[2]);
    }
  }
}

PNP_FN float dot3(const float* m, float x, float y, float z, float t) { return fmaf(m[2], z, fmaf(m[1], y, fmaf(m[0], x, t))); }

// Sum of the workgroup's values in a fixed order (a tree over the lanes); valid on lane 0.  red: kMetThreads floats.
PNP_FN float block_sum(float* red, float v) {
  const int tid = (int)threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = kMetThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

template <int DOF>
__global__ __launch_bounds__(kMetThreads) void pose_errors_nn_kernel(const float* __restrict__ pose_est,
                                                                     const float* __restrict__ pose_gt, int B,
                                                                     const float* __restrict__ points,
                                                                     const int32_t* __restrict__ range, int C,
                                                                     const int32_t* __restrict__ model_id,
                                                                     const uint8_t* __restrict__ symmetric, int nparts,
                                                                     int tiles_cap, float* __restrict__ scratch) {
  constexpr int P = PoseLen<DOF>::value;
  __shared__ MetricRow s;
  __shared__ float4 cand[kNnCandTile];
  __shared__ float red[kMetThreads];
  const int row = (int)(blockIdx.x / (unsigned)nparts), part = (int)(blockIdx.x % (unsigned)nparts), b = row % B;
  const int tid = (int)threadIdx.x;
  if (symmetric[b] == 0) return;
  if (tid == 0)
    metric_row_setup<DOF>(pose_est + (size_t)row * P, pose_gt + (size_t)b * P, range, C, model_id, nullptr, symmetric, nullptr, b, s);
  __syncthreads();
  const int M = s.count, ntile = (M + kNnQueryTile - 1) / kNnQueryTile;
  if (!s.ok || ntile > tiles_cap) return;      // the stream kernel writes the row's NaN
  const float* pts = points + (size_t)s.first * 3;
  for (int t = part; t < ntile; t += nparts) {
    float qx[kNnQpl], qy[kNnQpl], qz[kNnQpl], best[kNnQpl];
#pragma unroll
    for (int k = 0; k < kNnQpl; ++k) {
      const int i = t * kNnQueryTile + k * kMetThreads + tid;
      const float* p = pts + (size_t)(i < M ? i : M - 1) * 3;
      const float x = p[0], y = p[1], z = p[2];
      qx[k] = x + dot3(s.dQ + 0, x, y, z, s.tq[0]);
      qy[k] = y + dot3(s.dQ + 3, x, y, z, s.tq[1]);
      qz[k] = z + dot3(s.dQ + 6, x, y, z, s.tq[2]);
      best[k] = INFINITY;
    }
    for (int c0 = 0; c0 < M; c0 += kNnCandTile) {
      const int nj = min(kNnCandTile, M - c0), njp = (nj + 7) & ~7;
      __syncthreads();                         // the previous tile has been read by every lane
      for (int jj = tid; jj < njp; jj += kMetThreads) {
        // the padding of the last tile: an infinite distance, never the minimum
        const float* p = pts + (size_t)(c0 + (jj < nj ? jj : 0)) * 3;
        cand[jj] = (jj < nj) ? make_float4(p[0], p[1], p[2], 0.f) : make_float4(INFINITY, INFINITY, INFINITY, 0.f);
      }
      __syncthreads();
#pragma unroll 8
      for (int jj = 0; jj < njp; ++jj) {
        const float4 c = cand[jj];
#pragma unroll
        for (int k = 0; k < kNnQpl; ++k) {
          const float dx = qx[k] - c.x, dy = qy[k] - c.y, dz = qz[k] - c.z;
          best[k] = fminf(best[k], fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
        }
      }
    }
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < kNnQpl; ++k) sum += (t * kNnQueryTile + k * kMetThreads + tid < M) ? sqrtf(best[k]) : 0.f;
    sum = block_sum(red, sum);
    if (tid == 0) scratch[(size_t)row * tiles_cap + t] = sum;
  }
}

template <int DOF>
__global__ __launch_bounds__(kMetThreads) void pose_errors_stream_kernel(const float* __restrict__ pose_est,
                                                                         const float* __restrict__ pose_gt, int B,
                                                                         const float* __restrict__ points,
                                                                         const int32_t* __restrict__ range, int C,
                                                                         const int32_t* __restrict__ model_id,
                                                                         const float* __restrict__ cam,
                                                                         const uint8_t* __restrict__ symmetric,
                                                                         const uint8_t* __restrict__ half_turn, int tiles_cap,
                                                                         const float* __restrict__ scratch,
                                                                         float* __restrict__ errors) {
  constexpr int P = PoseLen<DOF>::value;
  __shared__ MetricRow s;
  __shared__ float red[kMetThreads];
  const int row = (int)blockIdx.x, b = row % B, tid = (int)threadIdx.x;
  if (tid == 0)
    metric_row_setup<DOF>(pose_est + (size_t)row * P, pose_gt + (size_t)b * P, range, C, model_id, cam, symmetric, half_turn, b, s);
  __syncthreads();
  float* out = errors + (size_t)row * EPROPNP_POSE_ERROR_WORDS;
  if (!s.ok) {
    if (tid < EPROPNP_POSE_ERROR_WORDS) out[tid] = (tid < 6) ? NAN : 0.f;
    return;
  }
  const int M = s.count;
  const float* pts = points + (size_t)s.first * 3;
  float acc_add = 0.f, acc_arp = 0.f;
  for (int i = tid; i < M; i += kMetThreads) {
    const float x = pts[(size_t)i * 3], y = pts[(size_t)i * 3 + 1], z = pts[(size_t)i * 3 + 2];
    const float ax = dot3(s.dR + 0, x, y, z, s.dt[0]), ay = dot3(s.dR + 3, x, y, z, s.dt[1]), az = dot3(s.dR + 6, x, y, z, s.dt[2]);
    acc_add += sqrtf(fmaf(az, az, fmaf(ay, ay, ax * ax)));
    if (s.has_cam) {
      // u_e / z_e - u_g / z_g = ((u_e - u_g) - (u_g / z_g) (z_e - z_g)) / z_e with the differences from K (R_est - R_gt), K (t_est -
      // t_gt): two pixel coordinates of ~1e3 are never subtracted
      const float zg = dot3(s.KRg + 6, x, y, z, s.Ktg[2]), dz = dot3(s.KdR + 6, x, y, z, s.Kdt[2]);
      const float ze = zg + dz;
      const float du = (dot3(s.KdR + 0, x, y, z, s.Kdt[0]) - dot3(s.KRg + 0, x, y, z, s.Ktg[0]) / zg * dz) / ze;
      const float dv = (dot3(s.KdR + 3, x, y, z, s.Kdt[1]) - dot3(s.KRg + 3, x, y, z, s.Ktg[1]) / zg * dz) / ze;
      acc_arp += sqrtf(fmaf(dv, dv, du * du));
    }
  }
  const float sum_add = block_sum(red, acc_add);
  __syncthreads();                             // lane 0 has read the first sum
  const float sum_arp = block_sum(red, acc_arp);
  if (tid != 0) return;
  const float add = sum_add / (float)M;
  float adi = NAN;
  const int ntile = (M + kNnQueryTile - 1) / kNnQueryTile;
  if (s.sym && ntile <= tiles_cap) {
    // the finishing step of ADD-S: the row's query tiles in tile order, whichever workgroups formed them
    float sum = 0.f;
    for (int t = 0; t < ntile; ++t) sum += scratch[(size_t)row * tiles_cap + t];
    adi = sum / (float)M;
  }
  out[0] = s.rot_deg;
  out[1] = s.trans;
  out[2] = s.has_cam ? sum_arp / (float)M : NAN;
  out[3] = add;
  out[4] = adi;
  out[5] = s.sym ? adi : add;
  out[6] = 0.f;
  out[7] = 0.f;
}

static size_t nn_tiles(int max_model_points) {
  const int m = max_model_points < 1 ? 1 : max_model_points;
  return ((size_t)m + kNnQueryTile - 1) / kNnQueryTile;
}

size_t pose_errors_scratch_bytes(int R, int B, int max_model_points) {
  if (R < 1 || B < 1) return 0;
  return (size_t)R * (size_t)B * nn_tiles(max_model_points) * sizeof(float);
}

int launch_pose_errors(const float* pose_est, const float* pose_gt, int R, int B, int dof, const float* points,
                       const int32_t* range, int C, const int32_t* model_id, const float* cam, const uint8_t* symmetric,
                       const uint8_t* half_turn, void* scratch, size_t scratch_bytes, float* errors, hipStream_t st) {
  if (B == 0) return EPROPNP_OK;
  if (B < 0) return fail(EPROPNP_EINVAL, "epropnp_pose_errors: num_obj must be >= 0, got %d", B);
  if (!pose_est || !pose_gt || !points || !range || !errors) return fail(EPROPNP_EINVAL, "epropnp_pose_errors: NULL pointer");
  if (dof != 4 && dof != 6) return fail(EPROPNP_EINVAL, "epropnp_pose_errors: dof must be 4 or 6, got %d", dof);
  if (R < 1) return fail(EPROPNP_EINVAL, "epropnp_pose_errors: num_rows_per_obj must be >= 1, got %d", R);
  if (C < 1) return fail(EPROPNP_EINVAL, "epropnp_pose_errors: num_models must be >= 1, got %d", C);
  const long rows = (long)R * B;
  if (rows > 0x7fffff00L) return fail(EPROPNP_EINVAL, "epropnp_pose_errors: %ld pose rows are too many for one launch", rows);
  long cap = 0;
  if (symmetric != nullptr) {
    if (!scratch) return fail(EPROPNP_EINVAL, "epropnp_pose_errors: NULL scratch with a symmetric mask");
    if (scratch_bytes < pose_errors_scratch_bytes(R, B, 1))
      return fail(EPROPNP_EINVAL, "epropnp_pose_errors: scratch of %zu bytes is smaller than epropnp_pose_errors_scratch_bytes (%zu for one tile per row)",
                  scratch_bytes, pose_errors_scratch_bytes(R, B, 1));
    cap = (long)(scratch_bytes / sizeof(float) / (size_t)rows);
    cap = cap > (1 << 20) ? (1 << 20) : cap;
    // few rows: a row's query tiles are dealt to several workgroups (EPROPNP_TUNE="nn_parts=<n>" overrides; the bits do not
    // depend on it).  Which rows are symmetric only the device knows: the rule counts every row.
    long parts = (4L * device_cu_count() + rows - 1) / rows;
    int ov[1];
    if (tune_ints("nn_parts", ov, 1) && ov[0] >= 1) parts = ov[0];
    parts = parts < 1 ? 1 : (parts > cap ? cap : parts);
    if (rows * parts > 0x7fffff00L) parts = 1;
    const dim3 grid((unsigned)(rows * parts)), block(kMetThreads);
    if (dof == 6)
      PNP_LAUNCH(pose_errors_nn_kernel<6>, grid, block, 0, st, pose_est, pose_gt, B, points, range, C, model_id, symmetric, (int)parts,
                 (int)cap, (float*)scratch);
    else
      PNP_LAUNCH(pose_errors_nn_kernel<4>, grid, block, 0, st, pose_est, pose_gt, B, points, range, C, model_id, symmetric, (int)parts,
                 (int)cap, (float*)scratch);
    const int rc = check_launch("pose_errors_nn_kernel");
    if (rc != EPROPNP_OK) return rc;
  }
  const dim3 grid((unsigned)rows), block(kMetThreads);
  if (dof == 6)
    PNP_LAUNCH(pose_errors_stream_kernel<6>, grid, block, 0, st, pose_est, pose_gt, B, points, range, C, model_id, cam, symmetric,
               half_turn, (int)cap, (const float*)scratch, errors);
  else
    PNP_LAUNCH(pose_errors_stream_kernel<4>, grid, block, 0, st, pose_est, pose_gt, B, points, range, C, model_id, cam, symmetric,
               half_turn, (int)cap, (const float*)scratch, errors);
  return check_launch("pose_errors_stream_kernel");
}

}  // namespace pnp
