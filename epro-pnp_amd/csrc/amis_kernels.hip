// amis_kernels.hip -- the all-VALU gradient (backward) of the AMIS Monte-Carlo pose sampler for gfx950, the Huber threshold's
// follow-up launch (delta_path_kernel) and the backward launchers.  The default backward is the matrix-core variant
// (amis_backward_mfma.hip); the kernel in this file is selected with EPROPNP_TUNE="bwd_impl=valu" and takes over where the MFMA
// backward's LDS pose table does not fit (> ~2700 samples).  The forward has one implementation, kernel and launcher, in
// amis_forward_mfma.hip.
//
// Backward replaces autograd's replay of the forward's cost sweep: gradients of
//   sum_j g_logw[j] * (-cost(pose_j)) + g_init * cost(pose_init)
// w.r.t. x3d, x2d, w2d, delta are RECOMPUTED from the points (lane = point, loop over poses; no atomics,
// nothing saved by the forward except the pose samples themselves).
#include "dispatch.h"
#include "amis_common.h"

namespace pnp {

template <int DOF, int PPL, bool BOUNDS, int MAXW>
__global__ __launch_bounds__(MAXW * 64, (MAXW == 4 ? (PPL >= 8 ? 2 : (PPL == 4 ? 3 : 4)) : 1)) void amis_backward_kernel(Problem p, const float* __restrict__ pose_samples,
                                                                    const float* __restrict__ g_logw, int S,
                                                                    const float* __restrict__ pose_init,
                                                                    const float* __restrict__ g_init,
                                                                    float* __restrict__ gx3d, float* __restrict__ gx2d,
                                                                    float* __restrict__ gw2d, float* __restrict__ gdelta,
                                                                    float drop_eps) {
  constexpr int PL = PoseLen<DOF>::value;
  // pose tiles: 64 poses x {K R (9) | K t (3) | weight | pad} as 4 float4 rows, double buffered
  __shared__ __attribute__((aligned(16))) float tab[2][64][16];
  __shared__ float red[16];
  __shared__ __attribute__((aligned(8))) float hist[kDropHistFloats];
  const int b = object_of_block(p.B);
  if (b >= p.B) return;
  const int T = (int)blockDim.x, tid = (int)threadIdx.x;

  float Kc[9], delta;
  Bounds bd;
  load_camera<BOUNDS>(p, b, Kc, bd, delta);
  const float zmin_v = to_vgpr(p.z_min), delta_v = to_vgpr(delta);
  Point pts[PPL];
  float gX[PPL], gY[PPL], gZ[PPL], gu[PPL], gv[PPL], gwu[PPL], gwv[PPL];
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    pts[k] = load_point(p, b, tid + k * T);
    gX[k] = gY[k] = gZ[k] = gu[k] = gv[k] = gwu[k] = gwv[k] = 0.f;
  }
  float gd = 0.f;

  const bool with_init = (pose_init != nullptr) && (g_init != nullptr);
  const int P = S + (with_init ? 1 : 0);      // pose index S = pose_init
  const int ntile = (P + 63) >> 6;
  // wave-uniform, hence a scalar load: fetched under a uniform branch, not inside a per-lane conditional (scalar loads
  // ignore EXEC; a NULL g_init would fault there even when no lane takes the arm)
  const float g_init_b = with_init ? g_init[b] : 0.f;

  // Samples whose total |weight| is below drop_eps of the object's total are skipped (mass_drop_threshold,
  // amis_common.h): at the default 2^-24 that is under the fp32 rounding of the S-term sums; ~17 % of the AMIS samples
  // after softmax normalisation (the Student-t tails).  drop_eps = 0: exact.
  float amax = 0.f;
  for (int m = tid; m < S; m += T) amax = fmaxf(amax, fabsf(g_logw[(size_t)m * p.B + b]));
  amax = block_max(amax, red);
  const float askip = mass_drop_threshold([&](int m) { return fabsf(g_logw[(size_t)m * p.B + b]); }, S, amax, drop_eps, hist);

  // lanes 0..63 of the workgroup fetch one pose each of tile t (global loads issued early, consumed late)
  float nps[PL], naw = 0.f;
  auto fetch = [&](int t) {
    if (tid < 64) {
      const int m = min(t * 64 + tid, P - 1);
      const float* src = (m < S) ? pose_samples + ((size_t)m * p.B + b) * PL : pose_init + (size_t)b * PL;
#pragma unroll
      for (int i = 0; i < PL; ++i) nps[i] = src[i];
      naw = (m < S) ? -g_logw[(size_t)m * p.B + b] : g_init_b;      // logw = -cost - const
      if (m < S && fabsf(naw) <= askip) naw = 0.f;
    }
  };
  auto publish = [&](int buf) {
    if (tid < 64) {
      float R[9], KR[9], Kt[3];
      pose_to_rot<DOF>(nps, R);
      compose_kr_kt(Kc, R, nps, KR, Kt);
      float4* row = reinterpret_cast<float4*>(&tab[buf][tid][0]);
      row[0] = make_float4(KR[0], KR[1], KR[2], KR[3]);
      row[1] = make_float4(KR[4], KR[5], KR[6], KR[7]);
      row[2] = make_float4(KR[8], Kt[0], Kt[1], Kt[2]);
      row[3] = make_float4(naw, 0.f, 0.f, 0.f);
    }
  };

  if (ntile > 0) {
    fetch(0);
    publish(0);
  }
  __syncthreads();
  for (int t = 0; t < ntile; ++t) {
    const bool more = (t + 1 < ntile);
    if (more) fetch(t + 1);
    const int cnt = min(64, P - t * 64);
    const int buf = t & 1;
    const float4* row0 = reinterpret_cast<const float4*>(&tab[buf][0][0]);   // uniform address: LDS broadcast
    float4 n0 = row0[0], n1 = row0[1], n2 = row0[2], n3 = row0[3];
    for (int j = 0; j < cnt; ++j) {
      const float4 r0 = n0, r1 = n1, r2 = n2, r3 = n3;
      {   // fetch the next pose row now; it is consumed one trip later
        const float4* rn = reinterpret_cast<const float4*>(&tab[buf][min(j + 1, cnt - 1)][0]);
        n0 = rn[0]; n1 = rn[1]; n2 = rn[2]; n3 = rn[3];
      }
      const float a = r3.x;
      if (uniform_is_zero(a)) continue;       // exact zero weight (wave-uniform)
      const float kr[9] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x};
      const float kt[3] = {r2.y, r2.z, r2.w};
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        const Point& q = pts[k];
        const float hx = fmaf(kr[0], q.X, fmaf(kr[1], q.Y, fmaf(kr[2], q.Z, kt[0])));
        const float hy = fmaf(kr[3], q.X, fmaf(kr[4], q.Y, fmaf(kr[5], q.Z, kt[1])));
        const float hz = fmaf(kr[6], q.X, fmaf(kr[7], q.Y, fmaf(kr[8], q.Z, kt[2])));
        const float rz = fast_rcp(fmaxf(hz, zmin_v));
        const float ppx = hx * rz, ppy = hy * rz;          // un-clamped projection
        float px = ppx, py = ppy;
        if (BOUNDS) {
          px = clamp_lu(px, bd.lbx, bd.ubx);
          py = clamp_lu(py, bd.lby, bd.uby);
        }
        const float dx = px - q.u, dy = py - q.v;
        const float rx = dx * q.wu, ry = dy * q.wv;
        const float s2 = fmaf(rx, rx, ry * ry);
        const float rs = fast_rsqrt(fmaxf(s2, 1e-30f));
        const float rho = s2 * rs;
        const float mm = fminf(rho, delta_v);
        const float coef = a * mm * rs;                      // a * min(1, delta / rho)
        gd = fmaf(a, rho - mm, gd);                          // d huber / d delta = max(rho - delta, 0)
        const float crx = coef * rx, cry = coef * ry;
        gwu[k] = fmaf(crx, dx, gwu[k]);
        gwv[k] = fmaf(cry, dy, gwv[k]);
        float gpx = crx * q.wu, gpy = cry * q.wv;
        gu[k] += gpx;                                        // d/du = -g_p ; sign applied at the end
        gv[k] += gpy;
        if (BOUNDS) {                                        // clamp passes no gradient where it is active
          gpx = (ppx < bd.lbx || ppx > bd.ubx) ? 0.f : gpx;
          gpy = (ppy < bd.lby || ppy > bd.uby) ? 0.f : gpy;
        }
        const float ghx = gpx * rz, ghy = gpy * rz;
        float ghz = -(gpx * ppx + gpy * ppy) * rz;
        ghz = (hz >= zmin_v) ? ghz : 0.f;
        gX[k] = fmaf(kr[0], ghx, fmaf(kr[3], ghy, fmaf(kr[6], ghz, gX[k])));
        gY[k] = fmaf(kr[1], ghx, fmaf(kr[4], ghy, fmaf(kr[7], ghz, gY[k])));
        gZ[k] = fmaf(kr[2], ghx, fmaf(kr[5], ghy, fmaf(kr[8], ghz, gZ[k])));
      }
    }
    if (more) publish((t + 1) & 1);
    __syncthreads();
  }

#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    const int n = tid + k * T;
    if (n < p.N) {
      const size_t i = (size_t)b * p.N + n;
      gx3d[i * 3] = gX[k]; gx3d[i * 3 + 1] = gY[k]; gx3d[i * 3 + 2] = gZ[k];
      *reinterpret_cast<float2*>(gx2d + i * 2) = make_float2(-gu[k], -gv[k]);
      *reinterpret_cast<float2*>(gw2d + i * 2) = make_float2(gwu[k], gwv[k]);
    }
  }
  float one[1] = {gd};
  block_sum<1>(one, red);
  if (tid == 0) gdelta[b] = one[0];
}

// ================================================================================================================
// launchers
// ================================================================================================================
// grad_w2d[b, :, :] += (sum over parts of grad_delta[b, part]) * d delta[b] / d w2d  for a Huber threshold that came from
// AdaptiveHuberPnPCost on this w2d (epropnp_problem.delta_stats): the follow-up launch for the backward variants whose kernel
// does not know the object's whole grad_delta at its end (object split over workgroups; the all-VALU kernel).
// (grid: B x ceil(2N / kDeltaPathSpan) workgroups -- one workgroup per object took 10 us for 32 x 4096 points, a launch of 32
// workgroups on a 256-CU device)
constexpr int kDeltaPathSpan = 1024;
__global__ __launch_bounds__(256) void delta_path_kernel(Problem p, const float* __restrict__ gdelta, int nparts,
                                                          float* __restrict__ gw2d, int spans) {
  const int b = (int)blockIdx.x / spans, sp = (int)blockIdx.x - b * spans;
  float g = 0.f;
  for (int q = 0; q < nparts; ++q) g += gdelta[(size_t)b * nparts + q];
  const float add = (g * p.delta_stats[(size_t)b * 4 + 1]) * (p.delta_relative / (2.0f * (float)p.N));
  float* row = gw2d + (size_t)b * p.N * 2;
  const int end = min(2 * p.N, (sp + 1) * kDeltaPathSpan);
  for (int i = sp * kDeltaPathSpan + (int)threadIdx.x; i < end; i += (int)blockDim.x) row[i] += add;
}

int launch_delta_path(const epropnp_problem* prob, const float* gdelta, int nparts, float* gw2d, hipStream_t st) {
  if (prob->delta_stats == nullptr) return EPROPNP_OK;
  const Problem d = to_device_problem(prob);
  const int spans = (2 * d.N + kDeltaPathSpan - 1) / kDeltaPathSpan;
  PNP_LAUNCH(delta_path_kernel, dim3((unsigned)(d.B * spans)), dim3(256), 0, st, d, gdelta, nparts, gw2d, spans);
  return check_launch("delta_path_kernel");
}

// Few objects: one object's S x N point-poses keep a single CU busy for ~70 us at 512 x 512 whatever the wave count, so
// the point chunks of an object are dealt to `nsplit` workgroups (each builds the pose table for itself).  The per-point
// gradients are disjoint and bit-identical to the unsplit kernel; grad_delta comes back as (B, nsplit) partials for the
// caller to add in a fixed order (no atomics: results stay reproducible).
int launch_amis_backward_split(const epropnp_problem* prob, const float* pose_samples, const float* grad_logweights,
                               int mc_samples, const float* pose_init, const float* grad_cost_init, int nsplit,
                               float* grad_x3d, float* grad_x2d, float* grad_w2d, float* grad_delta_parts, hipStream_t st,
                               const float* sample_costs, const float* cost_init) {
  if (int rc = check_problem(prob)) return rc;
  if (prob->num_obj == 0 || prob->num_pts == 0) return EPROPNP_OK;
  if (mc_samples < 0) return fail(EPROPNP_EINVAL, "amis_backward_split: negative mc_samples");
  if ((mc_samples > 0 && (!pose_samples || !grad_logweights)) || !grad_x3d || !grad_x2d || !grad_w2d || !grad_delta_parts)
    return fail(EPROPNP_EINVAL, "amis_backward_split: NULL pointer");
  if (nsplit < 1 || nsplit > 16 || (long long)nsplit * 64 > (long long)((prob->num_pts + 63) / 64) * 64)
    return fail(EPROPNP_EINVAL, "amis_backward_split: nsplit %d not in [1, min(16, ceil(num_pts / 64))]", nsplit);
  const int rc = launch_amis_backward_mfma(prob, pose_samples, grad_logweights, mc_samples, pose_init, grad_cost_init,
                                           grad_x3d, grad_x2d, grad_w2d, grad_delta_parts, nsplit, st, sample_costs, cost_init);
  if (rc == 1) return fail(EPROPNP_EINVAL, "amis_backward_split: mc_samples %d does not fit the LDS pose table", mc_samples);
  if (rc != 0) return rc;
  return nsplit > 1 ? launch_delta_path(prob, grad_delta_parts, nsplit, grad_w2d, st) : EPROPNP_OK;      // (1 part: the kernel's epilogue)
}

int launch_amis_backward(const epropnp_problem* prob, const float* pose_samples, const float* grad_logweights,
                         int mc_samples, const float* pose_init, const float* grad_cost_init, float* grad_x3d,
                         float* grad_x2d, float* grad_w2d, float* grad_delta, hipStream_t st, const float* sample_costs,
                         const float* cost_init) {
  if (int rc = check_problem(prob)) return rc;
  if (prob->num_obj == 0 || prob->num_pts == 0) return EPROPNP_OK;
  if (mc_samples < 0) return fail(EPROPNP_EINVAL, "amis_backward: negative mc_samples");
  if ((mc_samples > 0 && (!pose_samples || !grad_logweights)) || !grad_x3d || !grad_x2d || !grad_w2d || !grad_delta)
    return fail(EPROPNP_EINVAL, "amis_backward: NULL pointer");
  {   // projection on the matrix cores (amis_backward_mfma.hip) unless its LDS pose table does not fit;
      // EPROPNP_TUNE="bwd_impl=valu" forces this file's all-VALU kernel
    if (!backward_valu_forced()) {
      const int rc = launch_amis_backward_mfma(prob, pose_samples, grad_logweights, mc_samples, pose_init, grad_cost_init,
                                               grad_x3d, grad_x2d, grad_w2d, grad_delta, 1, st, sample_costs, cost_init);
      if (rc <= 0) return rc;     // 1 = shape not supported there (pose table larger than LDS)
    }
  }
  if (prob->num_pts > kMaxResidentPoints)
    return fail(EPROPNP_EINVAL, "amis_backward: num_pts %d exceeds the register-resident limit %d", prob->num_pts,
                kMaxResidentPoints);
  const Problem d = to_device_problem(prob);
  // measured on MI355X (profiles/): fewest waves per object wins (per-pose overhead amortised over 8 points/lane)
  Shape s = choose_shape(d.B, d.N, /*max_ppl=*/8, /*want_waves_total=*/4096);
  int ov[2];
  if (tune_ints("bwd_shape", ov, 2) && valid_shape_override(ov[0], ov[1], d.N)) { s.waves = ov[0]; s.ppl = ov[1]; }
  const dim3 grid(padded_object_grid(d.B)), block(64 * s.waves);
  dispatch_shape(prob->dof, s.ppl, has_bounds(prob), s.waves, [&](auto DOF, auto PPL, auto BND, auto MAXW) -> int {
    PNP_LAUNCH((amis_backward_kernel<decltype(DOF)::value, decltype(PPL)::value, decltype(BND)::value, decltype(MAXW)::value>),
               grid, block, 0, st, d, pose_samples, grad_logweights, mc_samples, pose_init, grad_cost_init, grad_x3d,
               grad_x2d, grad_w2d, grad_delta, backward_drop_eps());
    return 0;
  });
  if (int rc = check_launch("amis_backward_kernel")) return rc;
  return launch_delta_path(prob, grad_delta, 1, grad_w2d, st);
}

}  // namespace pnp
