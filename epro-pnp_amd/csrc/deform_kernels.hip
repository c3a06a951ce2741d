// deform_kernels.hip -- the deformable attention sampler of the detection head, forward and backward in one launch each
// (include/epropnp_hip.h: epropnp_deform_sample_forward, epropnp_deform_sample_backward).
//
//   EPro-PnP-Det epropnp_det/ops/deformable_attention_sampler.py:77-137 -- per object b, head j and point p: the key map, the value
//   map, the dense 2-D coordinate map (bilinear, border padding) and its validity mask (bilinear, zero padding) are sampled at a
//   learned location of image obj_img_ind[b]; a = q . k / sqrt(D); attn = sum_p v_p softmax_P(a)_p mask_p.  The reference does it as
//   four grid_sample calls on permuted 5-D views, a softmax and two batched matmuls.
//
// One WAVE per (object, head); a workgroup holds 1, 2 or 4 of them (whatever keeps its LDS under 64 KiB) and they never meet.
//   A  lane = point     : map coordinates px = x / stride - 0.5, the four corner offsets and the two fractions -> LDS table; the mask
//                         and x2d samples (scalar channels: four corners each, read by the lane itself)
//   B  lane = (point sub-index, channel): a point's corner is D contiguous floats of a channels-last map, so with D = 32 one
//                         wave-instruction reads two 128-B segments; the k and v samples -> LDS (row stride D | 1)
//   C  lane = point     : a_p = (q . k_p) / sqrt(D) (a serial sum over d from LDS), the softmax (the maximum by wave_max, the
//                         exponentials summed from LDS in point order), W_p = softmax_p mask_p
//   D  lane = channel   : attn_d = sum_p v_pd W_p, in point order
// The backward repeats A-C from the inputs (same code, same bits) and the saved maximum per (object, head), then
//   D' lane = channel   : dq_d = sum_p da_p k_pd / sqrt(D), in point order
//   E  lane = (point sub-index, channel): reads the corners again (L2), adds w_c dk_pd / w_c dv_pd into the zero-filled map
//                         gradients with float atomics -- the same two 128-B segments per wave-instruction as the reads; corners of
//                         weight exactly 0 are skipped -- and parks dk . dk/dpx + dv . dv/dpx per channel in LDS
//   F  lane = point     : sums those over d in channel order, adds the x2d and mask paths, gates the border-mode part by the clamp and
//                         writes dlocation.
// dquery and dlocation are sums in a fixed order (two launches agree to the bit); dkey / dvalue depend on the atomics' arrival order.
//
// Arithmetic: the kernels move bytes (gathers, atomics), their arithmetic is a few operations per loaded float -- so everything
// between a load and a store is fp64, samples stay fp64 in LDS, and each output is rounded to fp32 once.  An output that is the
// correctly rounded exact value is at least as close to it as ANY fp32 evaluation, the reference's included, on every input; the
// tests hold the kernels to that (tests/test_deform.py: the cap).  The float atomics of dkey / dvalue add in fp32.
//
// Memory safety: no input VALUE forms an address.  Corner indices are clamped as integers after the float -> int conversion of an
// already clamped coordinate (a NaN coordinate compares false and becomes 0), obj_img_ind is clamped to [0, NI - 1] here, and the
// launcher checks that the largest offset the four strides can form lies inside NI * E * h * w elements.
#include "pnp_host.h"

namespace pnp {

constexpr int kDeformMaxP = 64, kDeformMaxD = 64;
// LDS per point: 4 corner offsets (int32), then five doubles: fx, fy, da | e, W, spare use per phase
constexpr int kDeformTab = 14;
constexpr int kDeformHead = kDeformMaxP * kDeformTab + 2 * kDeformMaxD;      // words: the table, then q and the attn cotangent
static_assert(kDeformHead % 2 == 0 && kDeformTab % 2 == 0, "the doubles behind the head and inside a row are 8-byte aligned");

struct DeformArgs {
  const float *query, *key, *value, *x2d, *mask, *loc;
  const long long* img;
  long long sN, sC, sH, sW;
  int B, NI, H, P, D, h, w;
  float stride;
};

// what a lane keeps of ITS point (phase A) for the phases that have the point on the lane again
struct DeformPoint {
  double m, mdx, mdy;          // mask sample and its derivative w.r.t. the map coordinates (zero padding: no clamp)
  double xdx[2], xdy[2];       // derivative of the x2d sample (border padding: gated by gx, gy)
  double gx, gy;               // 1 where the coordinate is strictly inside (0, n - 1), else 0 (clamped, NaN)
};

PNP_FN int deform_row_stride(int D) { return D | 1; }
PNP_FN int* deform_offsets(float* tab, int p) { return reinterpret_cast<int*>(tab + p * kDeformTab); }
PNP_FN double* deform_row(float* tab, int p) { return reinterpret_cast<double*>(tab + p * kDeformTab + 4); }      // fx, fy, da|e, W, -

// clamp to [0, n - 1] as grid_sample's border padding does; NaN -> 0.  `gate` = 1 only strictly inside.
PNP_FN double deform_clamp(double c, int n, double& gate) {
  const double hi = (double)(n - 1);
  gate = (c > 0.0 && c < hi) ? 1.0 : 0.0;
  return (c > 0.0) ? fmin(c, hi) : 0.0;
}

PNP_FN double deform_lerp4(double v00, double v01, double v10, double v11, double fx, double fy) {
  const double ex = 1.0 - fx, ey = 1.0 - fy;
  return (ex * ey * v00 + fx * ey * v01) + (ex * fy * v10 + fx * fy * v11);
}
PNP_FN double deform_ddx(double v00, double v01, double v10, double v11, double fy) { return (1.0 - fy) * (v01 - v00) + fy * (v11 - v10); }
PNP_FN double deform_ddy(double v00, double v01, double v10, double v11, double fx) { return (1.0 - fx) * (v10 - v00) + fx * (v11 - v01); }

// phase A for one point: fills the point's table row, returns the mask / x2d samples and their derivatives
PNP_FN void deform_point(const DeformArgs& A, int img, float x, float y, float* tab, int p, DeformPoint& pt, double& xs0, double& xs1) {
  const double px = (double)x / (double)A.stride - 0.5, py = (double)y / (double)A.stride - 0.5;
  const double cx = deform_clamp(px, A.w, pt.gx), cy = deform_clamp(py, A.h, pt.gy);
  int x0 = (int)floor(cx), y0 = (int)floor(cy);
  x0 = min(max(x0, 0), A.w - 1);
  y0 = min(max(y0, 0), A.h - 1);
  const int x1 = min(x0 + 1, A.w - 1), y1 = min(y0 + 1, A.h - 1);
  const double fx = cx - (double)x0, fy = cy - (double)y0;
  int* o = deform_offsets(tab, p);
  // element offsets inside one image and one channel of the key / value maps; the launcher bounds them by 2^31
  o[0] = (int)(y0 * A.sH + x0 * A.sW);
  o[1] = (int)(y0 * A.sH + x1 * A.sW);
  o[2] = (int)(y1 * A.sH + x0 * A.sW);
  o[3] = (int)(y1 * A.sH + x1 * A.sW);
  double* row = deform_row(tab, p);
  row[0] = fx;
  row[1] = fy;
  const size_t plane = (size_t)A.h * A.w;
  const int i00 = y0 * A.w + x0, i01 = y0 * A.w + x1, i10 = y1 * A.w + x0, i11 = y1 * A.w + x1;
  const float* xm = A.x2d + (size_t)img * 2 * plane;
  {
    const double a00 = xm[i00], a01 = xm[i01], a10 = xm[i10], a11 = xm[i11];
    xs0 = deform_lerp4(a00, a01, a10, a11, fx, fy);
    pt.xdx[0] = deform_ddx(a00, a01, a10, a11, fy);
    pt.xdy[0] = deform_ddy(a00, a01, a10, a11, fx);
    const double b00 = xm[plane + i00], b01 = xm[plane + i01], b10 = xm[plane + i10], b11 = xm[plane + i11];
    xs1 = deform_lerp4(b00, b01, b10, b11, fx, fy);
    pt.xdx[1] = deform_ddx(b00, b01, b10, b11, fy);
    pt.xdy[1] = deform_ddy(b00, b01, b10, b11, fx);
  }
  // the mask: zero padding, the unclamped coordinate.  Outside (-1, n) every corner is off the map (and a NaN or huge coordinate
  // ends here): sample 0, derivative 0.
  pt.m = 0.0; pt.mdx = 0.0; pt.mdy = 0.0;
  if (px > -1.0 && px < (double)A.w && py > -1.0 && py < (double)A.h) {
    const double flx = floor(px), fly = floor(py);
    const int mx0 = (int)flx, my0 = (int)fly;                     // in [-1, n - 1]
    const double gx = px - flx, gy = py - fly;
    const bool xl = mx0 >= 0, xr = mx0 + 1 <= A.w - 1, yt = my0 >= 0, yb = my0 + 1 <= A.h - 1;
    const int ax = max(mx0, 0), bx = min(mx0 + 1, A.w - 1), ay = max(my0, 0), by = min(my0 + 1, A.h - 1);
    const float* mm = A.mask + (size_t)img * plane;
    const double m00 = (xl && yt) ? mm[ay * A.w + ax] : 0.f, m01 = (xr && yt) ? mm[ay * A.w + bx] : 0.f;
    const double m10 = (xl && yb) ? mm[by * A.w + ax] : 0.f, m11 = (xr && yb) ? mm[by * A.w + bx] : 0.f;
    pt.m = deform_lerp4(m00, m01, m10, m11, gx, gy);
    pt.mdx = deform_ddx(m00, m01, m10, m11, gy);
    pt.mdy = deform_ddy(m00, m01, m10, m11, gx);
  }
}

PNP_FN size_t deform_wave_words(int P, int D) { return (size_t)kDeformHead + 4 * (size_t)P * deform_row_stride(D); }

// the (object, head) of this wave, or false for the padded tail; `lds` = the wave's slice of the dynamic LDS
PNP_FN bool deform_wave(const DeformArgs& A, float* smem, int& bh, float*& lds) {
  const int nw = (int)(blockDim.x >> 6), wv = wave_id();
  const long long pair = (long long)blockIdx.x * nw + wv;
  if (pair >= (long long)A.B * A.H) return false;
  bh = (int)pair;
  lds = smem + (size_t)wv * deform_wave_words(A.P, A.D);
  return true;
}

PNP_FN int deform_image(const DeformArgs& A, int b) {
  const long long i = A.img[b];
  return (int)(i < 0 ? 0 : (i > (long long)A.NI - 1 ? (long long)A.NI - 1 : i));
}

// phase B: the k and v samples of every (point, channel) -> ks / vs (and the caller's v_samples, point-major, when given)
PNP_FN void deform_gather(const DeformArgs& A, float* tab, size_t base, int lane, double* ks, double* vs, float* vout) {
  const int DS = deform_row_stride(A.D);
  int lp = 1;
  while (lp < A.D) lp <<= 1;                      // lanes per point: D = 32 -> two points per wave-instruction
  const int sub = lane / lp, d = lane & (lp - 1), pp = 64 / lp;
  const float* kb = A.key + base + (size_t)d * A.sC;
  const float* vb = A.value + base + (size_t)d * A.sC;
  for (int p0 = 0; p0 < A.P; p0 += pp) {
    const int p = p0 + sub;
    if (p < A.P && d < A.D) {
      const int* o = deform_offsets(tab, p);
      const double* row = deform_row(tab, p);
      const int o0 = o[0], o1 = o[1], o2 = o[2], o3 = o[3];
      const double fx = row[0], fy = row[1];
      const float k0 = kb[o0], k1 = kb[o1], k2 = kb[o2], k3 = kb[o3];
      const float v0 = vb[o0], v1 = vb[o1], v2 = vb[o2], v3 = vb[o3];
      const double v = deform_lerp4(v0, v1, v2, v3, fx, fy);
      ks[p * DS + d] = deform_lerp4(k0, k1, k2, k3, fx, fy);
      vs[p * DS + d] = v;
      if (vout != nullptr) vout[(size_t)p * A.D + d] = (float)v;
    }
  }
}

// phase C up to the softmax, lane = point (every lane of the wave calls it): the score a and the normalised weight s; the lanes'
// exponentials meet in the table (row[2]) and every lane adds them up in point order.  `mx_in`: the forward's maximum or NULL.
PNP_FN void deform_softmax(const DeformArgs& A, float* tab, const float* qs, const double* ks, int lane, const float* mx_in, double& a,
                           double& s, float& mx, double& sum) {
  const int DS = deform_row_stride(A.D);
  a = 0.0;
  if (lane < A.P) {
    double acc = 0.0;
    for (int d = 0; d < A.D; ++d) acc += (double)qs[d] * ks[lane * DS + d];
    a = acc / sqrt((double)A.D);
  }
  mx = (mx_in != nullptr) ? *mx_in : wave_max(lane < A.P ? (float)a : -INFINITY);
  const double e = (lane < A.P) ? exp(a - (double)mx) : 0.0;
  if (lane < A.P) deform_row(tab, lane)[2] = e;
  wave_lds_fence();
  sum = 0.0;
  for (int p = 0; p < A.P; ++p) sum += deform_row(tab, p)[2];
  s = e / sum;
  wave_lds_fence();                               // row[2] is written again by the caller
}

__global__ __launch_bounds__(256) void deform_forward_kernel(DeformArgs A, float* __restrict__ attn, float* __restrict__ v_out,
                                                              float* __restrict__ a_out, float* __restrict__ m_out,
                                                              float* __restrict__ x_out, float* __restrict__ stats) {
  PNP_DYN_SMEM(float, smem);
  int bh;
  float* lds;
  if (!deform_wave(A, smem, bh, lds)) return;
  const int lane = lane_id(), b = bh / A.H, hd = bh - b * A.H, DS = deform_row_stride(A.D);
  const int img = deform_image(A, b);
  float* tab = lds;
  float* qs = lds + kDeformMaxP * kDeformTab;
  double* ks = reinterpret_cast<double*>(lds + kDeformHead);
  double* vs = ks + A.P * DS;
  DeformPoint pt;
  pt.m = 0.0;
  if (lane < A.P) {
    const size_t o = (size_t)bh * A.P + lane;
    double xs0, xs1;
    deform_point(A, img, A.loc[2 * o], A.loc[2 * o + 1], tab, lane, pt, xs0, xs1);
    m_out[o] = (float)pt.m;
    x_out[2 * o] = (float)xs0;
    x_out[2 * o + 1] = (float)xs1;
  }
  if (lane < A.D) qs[lane] = A.query[(size_t)bh * A.D + lane];
  wave_lds_fence();
  const size_t base = (size_t)img * A.sN + (size_t)hd * A.D * A.sC;
  deform_gather(A, tab, base, lane, ks, vs, v_out + (size_t)bh * A.P * A.D);
  wave_lds_fence();
  double a, s, sum;
  float mx;
  deform_softmax(A, tab, qs, ks, lane, nullptr, a, s, mx, sum);
  if (lane < A.P) {
    a_out[(size_t)bh * A.P + lane] = (float)a;
    deform_row(tab, lane)[3] = s * pt.m;
  }
  if (lane == 0) { stats[(size_t)bh * 2] = mx; stats[(size_t)bh * 2 + 1] = (float)sum; }
  wave_lds_fence();
  if (lane < A.D) {
    double acc = 0.0;
    for (int p = 0; p < A.P; ++p) acc += vs[p * DS + lane] * deform_row(tab, p)[3];
    attn[(size_t)bh * A.D + lane] = (float)acc;
  }
}

// g_attn (B,E), g_v (B,H,P,D), g_a (B,H,P), g_m (B,H,P), g_x (B,H,P,2): any of them NULL = zero.
// dq (B,H,D), dloc (B,H,P,2), dkey / dvalue (the maps' strides, zero-filled by the launcher): any of them NULL = not wanted.
__global__ __launch_bounds__(256) void deform_backward_kernel(DeformArgs A, const float* __restrict__ stats,
                                                               const float* __restrict__ g_attn, const float* __restrict__ g_v,
                                                               const float* __restrict__ g_a, const float* __restrict__ g_m,
                                                               const float* __restrict__ g_x, float* __restrict__ dq,
                                                               float* dkey, float* dvalue, float* __restrict__ dloc) {
  PNP_DYN_SMEM(float, smem);
  int bh;
  float* lds;
  if (!deform_wave(A, smem, bh, lds)) return;
  const int lane = lane_id(), b = bh / A.H, hd = bh - b * A.H, DS = deform_row_stride(A.D);
  const int img = deform_image(A, b);
  float* tab = lds;
  float* qs = lds + kDeformMaxP * kDeformTab;
  float* gs = qs + kDeformMaxD;
  double* ks = reinterpret_cast<double*>(lds + kDeformHead);
  double* vs = ks + A.P * DS;
  const double c = 1.0 / sqrt((double)A.D);
  DeformPoint pt;
  pt.m = pt.mdx = pt.mdy = pt.gx = pt.gy = 0.0;
  pt.xdx[0] = pt.xdx[1] = pt.xdy[0] = pt.xdy[1] = 0.0;
  const size_t po = (size_t)bh * A.P + lane;      // this lane's point (lane < P)
  if (lane < A.P) {
    double xs0, xs1;
    deform_point(A, img, A.loc[2 * po], A.loc[2 * po + 1], tab, lane, pt, xs0, xs1);
  }
  if (lane < A.D) {
    qs[lane] = A.query[(size_t)bh * A.D + lane];
    gs[lane] = g_attn ? g_attn[(size_t)bh * A.D + lane] : 0.f;
  }
  wave_lds_fence();
  const size_t base = (size_t)img * A.sN + (size_t)hd * A.D * A.sC;
  deform_gather(A, tab, base, lane, ks, vs, nullptr);
  wave_lds_fence();
  // C: per point the score and the softmax as the forward formed them, then the cotangents of the score and of the mask sample
  double a, s, sum;
  float mx;
  deform_softmax(A, tab, qs, ks, lane, stats + (size_t)bh * 2, a, s, mx, sum);
  double t = 0.0;                                   // dL/dW_p = sum_d g_attn_d v_pd
  if (lane < A.P)
    for (int d = 0; d < A.D; ++d) t += (double)gs[d] * vs[lane * DS + d];
  if (lane < A.P) deform_row(tab, lane)[2] = (t * pt.m) * s;
  wave_lds_fence();
  double dot = 0.0;
  for (int p = 0; p < A.P; ++p) dot += deform_row(tab, p)[2];
  wave_lds_fence();
  double dm = 0.0;
  if (lane < A.P) {
    dm = (g_m ? (double)g_m[po] : 0.0) + t * s;
    deform_row(tab, lane)[2] = (g_a ? (double)g_a[po] : 0.0) + s * (t * pt.m - dot);      // da
    deform_row(tab, lane)[3] = s * pt.m;                                                  // W
  }
  wave_lds_fence();
  if (dq != nullptr && lane < A.D) {
    double acc = 0.0;
    for (int p = 0; p < A.P; ++p) acc += deform_row(tab, p)[2] * ks[p * DS + lane];
    dq[(size_t)bh * A.D + lane] = (float)(acc * c);
  }
  if (dkey == nullptr && dvalue == nullptr && dloc == nullptr) return;
  wave_lds_fence();                                  // D' has read ks; E overwrites it
  {
    int lp = 1;
    while (lp < A.D) lp <<= 1;
    const int sub = lane / lp, d = lane & (lp - 1), pp = 64 / lp;
    const size_t off = base + (size_t)d * A.sC;
    const float* kb = A.key + off;
    const float* vb = A.value + off;
    const double qd = (d < A.D) ? qs[d] : 0.f, gd = (d < A.D) ? gs[d] : 0.f;
    for (int p0 = 0; p0 < A.P; p0 += pp) {
      const int p = p0 + sub;
      if (p < A.P && d < A.D) {
        const int* op = deform_offsets(tab, p);
        const double* row = deform_row(tab, p);
        const int o[4] = {op[0], op[1], op[2], op[3]};
        const double fx = row[0], fy = row[1];
        const double dk = c * row[2] * qd;
        const double dv = (g_v ? (double)g_v[((size_t)bh * A.P + p) * A.D + d] : 0.0) + gd * row[3];
        const double ex = 1.0 - fx, ey = 1.0 - fy;
        const double w[4] = {ex * ey, fx * ey, ex * fy, fx * fy};
        if (dkey != nullptr) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (w[i] != 0.0) atomicAdd(dkey + off + o[i], (float)(w[i] * dk));
        }
        if (dvalue != nullptr) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (w[i] != 0.0) atomicAdd(dvalue + off + o[i], (float)(w[i] * dv));
        }
        if (dloc != nullptr) {
          const double k00 = kb[o[0]], k01 = kb[o[1]], k10 = kb[o[2]], k11 = kb[o[3]];
          const double v00 = vb[o[0]], v01 = vb[o[1]], v10 = vb[o[2]], v11 = vb[o[3]];
          ks[p * DS + d] = dk * deform_ddx(k00, k01, k10, k11, fy) + dv * deform_ddx(v00, v01, v10, v11, fy);
          vs[p * DS + d] = dk * deform_ddy(k00, k01, k10, k11, fx) + dv * deform_ddy(v00, v01, v10, v11, fx);
        }
      }
    }
  }
  if (dloc == nullptr) return;
  wave_lds_fence();
  if (lane < A.P) {
    double sx = 0.0, sy = 0.0;
    for (int d = 0; d < A.D; ++d) { sx += ks[lane * DS + d]; sy += vs[lane * DS + d]; }
    if (g_x != nullptr) {
      const double g0 = g_x[2 * po], g1 = g_x[2 * po + 1];
      sx += g0 * pt.xdx[0] + g1 * pt.xdx[1];
      sy += g0 * pt.xdy[0] + g1 * pt.xdy[1];
    }
    // border padding: no gradient along an axis on which the coordinate is clamped (or NaN); the mask's path is not clamped
    dloc[2 * po] = (float)((pt.gx * sx + dm * pt.mdx) / (double)A.stride);
    dloc[2 * po + 1] = (float)((pt.gy * sy + dm * pt.mdy) / (double)A.stride);
  }
}

static int deform_check(const char* what, const float* query, const float* key, const float* value, const float* x2d, const float* mask,
                        const float* loc, const long long* img, int B, int NI, int H, int P, int D, int h, int w, int stride,
                        long long sN, long long sC, long long sH, long long sW) {
  if (B < 0 || NI < 1 || H < 1 || h < 1 || w < 1 || stride < 1)
    return fail(EPROPNP_EINVAL, "%s: num_obj >= 0, num_img, num_heads, height, width, stride >= 1 required", what);
  if (P < 1 || P > kDeformMaxP) return fail(EPROPNP_EINVAL, "%s: num_points %d outside 1 .. %d", what, P, kDeformMaxP);
  if (D < 1 || D > kDeformMaxD) return fail(EPROPNP_EINVAL, "%s: head_dim %d outside 1 .. %d", what, D, kDeformMaxD);
  const double elems = (double)NI * H * D * h * w;
  if (sN < 1 || sC < 1 || sH < 1 || sW < 1 || elems > 9.0e18 ||
      (double)(NI - 1) * sN + ((double)H * D - 1) * sC + (double)(h - 1) * sH + (double)(w - 1) * sW >= elems)
    return fail(EPROPNP_EINVAL, "%s: the key / value strides reach outside num_img * embed * height * width elements", what);
  if ((h - 1) * sH + (w - 1) * sW > 0x7fffffffLL || (long long)h * w > 0x7fffffffLL)
    return fail(EPROPNP_EINVAL, "%s: one channel of one image spans more than 2^31 elements", what);
  if ((long long)B * H > 0x7fffffffLL) return fail(EPROPNP_EINVAL, "%s: num_obj * num_heads exceeds 2^31 - 1", what);
  if (B > 0 && (!query || !key || !value || !x2d || !mask || !loc || !img)) return fail(EPROPNP_EINVAL, "%s: NULL input", what);
  return EPROPNP_OK;
}

// waves per workgroup: as many of 4, 2, 1 as keep the dynamic LDS at or under 64 KiB; one wave at the limits needs 69 KiB
static int deform_waves(int P, int D, size_t& bytes) {
  const size_t per = sizeof(float) * ((size_t)kDeformHead + 4 * (size_t)P * (D | 1));
  int nw = 4;
  while (nw > 1 && per * nw > 64 * 1024) nw >>= 1;
  bytes = per * nw;
  return nw;
}

int launch_deform_forward(const float* query, const float* key, const float* value, const float* x2d, const float* mask,
                          const float* loc, const long long* img, int B, int NI, int H, int P, int D, int h, int w, int stride,
                          long long sN, long long sC, long long sH, long long sW, float* attn, float* v_out, float* a_out,
                          float* m_out, float* x_out, float* stats, hipStream_t st) {
  if (int rc = deform_check("deform_sample_forward", query, key, value, x2d, mask, loc, img, B, NI, H, P, D, h, w, stride, sN, sC, sH, sW))
    return rc;
  if (B == 0) return EPROPNP_OK;
  if (!attn || !v_out || !a_out || !m_out || !x_out || !stats) return fail(EPROPNP_EINVAL, "deform_sample_forward: NULL output");
  const DeformArgs A = {query, key, value, x2d, mask, loc, img, sN, sC, sH, sW, B, NI, H, P, D, h, w, (float)stride};
  size_t bytes;
  const int nw = deform_waves(P, D, bytes);
  const unsigned grid = (unsigned)(((long long)B * H + nw - 1) / nw);
  allow_dynamic_lds((const void*)deform_forward_kernel, bytes);
  PNP_LAUNCH(deform_forward_kernel, dim3(grid), dim3(64 * nw), bytes, st, A, attn, v_out, a_out, m_out, x_out, stats);
  return check_launch("deform_forward_kernel");
}

int launch_deform_backward(const float* query, const float* key, const float* value, const float* x2d, const float* mask,
                           const float* loc, const long long* img, const float* stats, const float* g_attn, const float* g_v,
                           const float* g_a, const float* g_m, const float* g_x, int B, int NI, int H, int P, int D, int h, int w,
                           int stride, long long sN, long long sC, long long sH, long long sW, float* dq, float* dkey,
                           float* dvalue, float* dloc, hipStream_t st) {
  if (int rc = deform_check("deform_sample_backward", query, key, value, x2d, mask, loc, img, B, NI, H, P, D, h, w, stride, sN, sC, sH, sW))
    return rc;
  const size_t words = (size_t)NI * H * D * h * w;
  if (dkey != nullptr && launch_fill_u32(dkey, 0u, words, st) != EPROPNP_OK) return fail(EPROPNP_ELAUNCH, "deform_sample_backward: zero fill");
  if (dvalue != nullptr && launch_fill_u32(dvalue, 0u, words, st) != EPROPNP_OK) return fail(EPROPNP_ELAUNCH, "deform_sample_backward: zero fill");
  if (B == 0 || (!dq && !dkey && !dvalue && !dloc)) return EPROPNP_OK;
  if (!stats) return fail(EPROPNP_EINVAL, "deform_sample_backward: NULL stats");
  const DeformArgs A = {query, key, value, x2d, mask, loc, img, sN, sC, sH, sW, B, NI, H, P, D, h, w, (float)stride};
  size_t bytes;
  const int nw = deform_waves(P, D, bytes);
  const unsigned grid = (unsigned)(((long long)B * H + nw - 1) / nw);
  allow_dynamic_lds((const void*)deform_backward_kernel, bytes);
  PNP_LAUNCH(deform_backward_kernel, dim3(grid), dim3(64 * nw), bytes, st, A, stats, g_attn, g_v, g_a, g_m, g_x, dq, dkey, dvalue, dloc);
  return check_launch("deform_backward_kernel");
}

}  // namespace pnp
