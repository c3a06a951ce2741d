// roi_kernels.hip -- the cross-RoI logsumexp of the detection head's auxiliary losses, forward and backward in one launch each
// (include/epropnp_hip.h: epropnp_roi_logsumexp_forward, epropnp_roi_logsumexp_backward).
//
//   EPro-PnP-Det epropnp_det/ops/inter_roi_ops.py:19-81 -- every RoI i carries a (c, rh, rw) map over its box.  RoI j of the same
//   image whose box overlaps i's is a NEIGHBOUR: its map is resampled (bilinear, border padding, align_corners=False) at the image
//   positions of i's cell centres, and out_i = log(exp(x_i) + sum over the neighbours whose box covers the position of exp(s_j)).
//   The reference is a Python loop over images and RoIs around affine_grid, grid_sample, masked_fill and logsumexp.
//
// Forward: one workgroup per (RoI i, channel).  256 candidates j at a time are tested in parallel, one per thread, and the hits meet
// as a 256-bit mask in LDS (no list, no prefix sum, no cap on the number of neighbours); the workgroup then walks the set bits in
// ascending j.  The map from i's cells into j's map is separable, so per neighbour the clamped sample coordinate and the validity
// are formed once per column and once per row (fp64) and every cell reads its two table entries.  Each thread keeps a running
// (maximum, sum) per output cell, so the magnitude of the inputs does not matter; a cell nobody else covers returns its input bits.
// Backward: one workgroup per (RECEIVER RoI j, channel), x[j, ch] in LDS.  For every sender i that has j as a neighbour, in ascending i:
// G(p) = valid(p) gout_i(p) exp(s_j(p) - out_i(p)) over i's cells p into an LDS tile (s_j re-sampled from the LDS copy), then the
// thread that owns cell q of j adds sum_py wy(py, qy) sum_px wx(px, qx) G(py, px) over the contiguous ranges of cells whose clamped
// coordinate lies within one pixel of q (the coordinate is monotonic in the cell index; found once per pair and axis) -- along x into
// a second LDS tile first, then along y, so a small box inside a large one costs rw + rh terms per cell, not rw * rh.  No float
// atomic and every order fixed: two launches agree to the bit.  Cells are handled 4 per thread at a time, so registers do not grow
// with rh * rw; a map of more than 1024 cells repeats the walk over the RoIs per 1024 cells.
//
// Arithmetic: fp64 between the loads and the one rounding of each output, as in deform_kernels.hip -- the kernels gather and
// exponentiate, a few operations per loaded float --, so an output is at least as close to the exact value as any fp32 evaluation.
// Memory safety: no value read from a tensor forms an address unchecked.  Image ids and box corners only enter comparisons and the
// coordinate arithmetic; a sample coordinate is clamped as a double (NaN -> 0) and its corner indices again as integers.
#include "pnp_host.h"

namespace pnp {

// a workgroup is 256 threads, or one wave where the map has no more cells than a wave handles at once; kRoiPer cells per thread and pass
constexpr int kRoiThreads = 256, kRoiPer = 4, kRoiRound = 256;
constexpr int kRoiMaxCells = 64 * 64;

struct RoiBox {
  float id, x1, y1, x2, y2;
};

PNP_FN RoiBox roi_box(const float* __restrict__ rois, int i) {
  const float* r = rois + (size_t)i * 5;
  return RoiBox{rintf(r[0]), r[1], r[2], r[3], r[4]};       // torch.round: half to even
}

// inter_roi_ops.py:9-16, :31-39 -- same image (never a negative id) and a strictly positive overlap, in fp32 as the reference forms
// it.  Comparisons only; the extents are tested too, so that a NaN corner (which fminf / fmaxf would drop) never pairs.
PNP_FN bool roi_neighbours(const RoiBox& a, const RoiBox& b) {
  if (!(a.id == b.id && a.id >= 0.f)) return false;
  const float ow = fminf(a.x2, b.x2) - fmaxf(a.x1, b.x1), oh = fminf(a.y2, b.y2) - fmaxf(a.y1, b.y1);
  return ow > 0.f && oh > 0.f && a.x2 - a.x1 > 0.f && a.y2 - a.y1 > 0.f && b.x2 - b.x1 > 0.f && b.y2 - b.y1 > 0.f;
}

// cell p of the r cells along one axis of the box [a1, a2], seen from the box [b1, b2] (b2 > b1): the sample coordinate in b's map,
// clamped to [0, r - 1] (NaN -> 0), and whether the cell centre lies strictly inside b.  The forward and the backward must agree on
// the validity bit for bit, so nothing here is contracted.
PNP_FN bool roi_axis(double a1, double a2, double b1, double b2, int r, int p, double& u) {
#pragma clang fp contract(off)
  const double X = a1 + ((double)p + 0.5) / (double)r * (a2 - a1);
  const double g = 2.0 * (X - b1) / (b2 - b1) - 1.0;
  const double raw = ((g + 1.0) * (double)r - 1.0) / 2.0;
  u = (raw > 0.0) ? fmin(raw, (double)(r - 1)) : 0.0;
  return g > -1.0 && g < 1.0;
}

// tu / tv: the column table (rw entries), then the row table (rh entries)
PNP_FN void roi_tables(const RoiBox& from, const RoiBox& into, int rh, int rw, double* tu, int* tv) {
  for (int k = (int)threadIdx.x; k < rw + rh; k += (int)blockDim.x) {
    double u;
    const bool ok = (k < rw) ? roi_axis(from.x1, from.x2, into.x1, into.x2, rw, k, u)
                             : roi_axis(from.y1, from.y2, into.y1, into.y2, rh, k - rw, u);
    tu[k] = u;
    tv[k] = ok ? 1 : 0;
  }
}

// bilinear sample of one (rh, rw) map at the clamped coordinate (v, u)
PNP_FN double roi_sample(const float* map, int rh, int rw, double v, double u) {
  int u0 = min(max((int)u, 0), rw - 1), v0 = min(max((int)v, 0), rh - 1);
  const int u1 = min(u0 + 1, rw - 1), v1 = min(v0 + 1, rh - 1);
  const double fu = u - (double)u0, fv = v - (double)v0, eu = 1.0 - fu, ev = 1.0 - fv;
  const double a00 = map[v0 * rw + u0], a01 = map[v0 * rw + u1], a10 = map[v1 * rw + u0], a11 = map[v1 * rw + u1];
  return (eu * ev * a00 + fu * ev * a01) + (eu * fv * a10 + fu * fv * a11);
}

// the neighbours of `me` (RoI `self`) among j0 .. j0 + kRoiRound - 1 as 8 words of 32 bits; ends on a barrier
PNP_FN void roi_mask(const float* __restrict__ rois, const RoiBox& me, int self, int j0, int n, int* mask) {
  const int t = (int)threadIdx.x;
  if (t < 8) mask[t] = 0;
  __syncthreads();
  for (int k = t; k < kRoiRound; k += (int)blockDim.x) {
    const int j = j0 + k;
    if (j < n && j != self && roi_neighbours(me, roi_box(rois, j))) atomicOr(&mask[k >> 5], (int)(1u << (k & 31)));
  }
  __syncthreads();
}

__global__ __launch_bounds__(kRoiThreads) void roi_lse_forward_kernel(const float* __restrict__ x, const float* __restrict__ rois, int n,
                                                                      int c, int rh, int rw, float* __restrict__ out) {
  PNP_DYN_SMEM(double, smem);
  __shared__ int mask[8];
  double* tu = smem;
  int* tv = reinterpret_cast<int*>(tu + rw + rh);
  const int t = (int)threadIdx.x, nt = (int)blockDim.x, cells = rh * rw;
  const int i = (int)(blockIdx.x / (unsigned)c), ch = (int)(blockIdx.x - (unsigned)i * (unsigned)c);
  const RoiBox me = roi_box(rois, i);
  const size_t plane = ((size_t)i * c + ch) * cells;
  for (int base = 0; base < cells; base += nt * kRoiPer) {
    double mx[kRoiPer], sum[kRoiPer];
    int px[kRoiPer], py[kRoiPer];
#pragma unroll
    for (int e = 0; e < kRoiPer; ++e) {
      const int p = base + e * nt + t;
      py[e] = p / rw;
      px[e] = p - py[e] * rw;
      mx[e] = (p < cells) ? (double)x[plane + p] : 0.0;
      sum[e] = 1.0;
    }
    for (int j0 = 0; j0 < n; j0 += kRoiRound) {
      roi_mask(rois, me, i, j0, n, mask);
      for (int w = 0; w < 8; ++w) {
        unsigned bits = (unsigned)__builtin_amdgcn_readfirstlane(mask[w]);
        while (bits != 0u) {
          const int j = j0 + w * 32 + __builtin_ctz(bits);
          bits &= bits - 1u;
          roi_tables(me, roi_box(rois, j), rh, rw, tu, tv);
          __syncthreads();
          const float* map = x + ((size_t)j * c + ch) * cells;
#pragma unroll
          for (int e = 0; e < kRoiPer; ++e) {
            if (base + e * nt + t < cells && tv[px[e]] != 0 && tv[rw + py[e]] != 0) {
              const double s = roi_sample(map, rh, rw, tu[rw + py[e]], tu[px[e]]);
              if (s > mx[e]) {
                sum[e] = sum[e] * exp(mx[e] - s) + 1.0;
                mx[e] = s;
              } else if (s == mx[e]) {                // also two -inf or two +inf
                sum[e] += 1.0;
              } else {
                sum[e] += exp(s - mx[e]);
              }
            }
          }
          __syncthreads();
        }
      }
    }
#pragma unroll
    for (int e = 0; e < kRoiPer; ++e) {
      const int p = base + e * nt + t;
      if (p < cells) out[plane + p] = (float)(mx[e] + log(sum[e]));      // sum = 1: the input's bits
    }
  }
}

__global__ __launch_bounds__(kRoiThreads) void roi_lse_backward_kernel(const float* __restrict__ x, const float* __restrict__ rois,
                                                                       const float* __restrict__ out, const float* __restrict__ gout,
                                                                       int n, int c, int rh, int rw, float* __restrict__ gx) {
  PNP_DYN_SMEM(double, smem);
  __shared__ int mask[8];
  const int t = (int)threadIdx.x, nt = (int)blockDim.x, cells = rh * rw, axes = rw + rh;
  double* G = smem;
  double* R = G + cells;
  double* tu = R + cells;
  float* xs = reinterpret_cast<float*>(tu + axes);
  int* tv = reinterpret_cast<int*>(xs + cells);
  int* lo = tv + axes;
  int* hi = lo + axes;
  const int j = (int)(blockIdx.x / (unsigned)c), ch = (int)(blockIdx.x - (unsigned)j * (unsigned)c);
  const RoiBox me = roi_box(rois, j);
  const size_t plane = ((size_t)j * c + ch) * cells;
  for (int p = t; p < cells; p += nt) xs[p] = x[plane + p];
  for (int base = 0; base < cells; base += nt * kRoiPer) {
    double acc[kRoiPer];
    int qx[kRoiPer], qy[kRoiPer];
#pragma unroll
    for (int e = 0; e < kRoiPer; ++e) {
      const int q = base + e * nt + t;
      qy[e] = q / rw;
      qx[e] = q - qy[e] * rw;
      acc[e] = 0.0;
      if (q < cells) {                                // the self term g exp(x - out)
        const double xv = x[plane + q], o = out[plane + q], g = gout[plane + q];
        acc[e] = (xv == o) ? g : g * exp(xv - o);
      }
    }
    for (int i0 = 0; i0 < n; i0 += kRoiRound) {
      roi_mask(rois, me, j, i0, n, mask);             // (also orders the writes of xs before its first read)
      for (int w = 0; w < 8; ++w) {
        unsigned bits = (unsigned)__builtin_amdgcn_readfirstlane(mask[w]);
        while (bits != 0u) {
          const int i = i0 + w * 32 + __builtin_ctz(bits);
          bits &= bits - 1u;
          roi_tables(roi_box(rois, i), me, rh, rw, tu, tv);
          __syncthreads();
          // per cell q of an axis of j: the cells of i whose coordinate lies within one pixel of it
          for (int k = t; k < axes; k += nt) {
            const int first = (k < rw) ? 0 : rw, count = (k < rw) ? rw : rh;
            const double q = (double)(k - first);
            int l = count, h = -1;
            for (int p = 0; p < count; ++p)
              if (fabs(tu[first + p] - q) < 1.0) {
                l = min(l, p);
                h = p;
              }
            lo[k] = l;
            hi[k] = h;
          }
          const size_t src = ((size_t)i * c + ch) * cells;
          for (int p = t; p < cells; p += nt) {
            const int py = p / rw, px = p - py * rw;
            double g = 0.0;
            if (tv[px] != 0 && tv[rw + py] != 0) {
              const double s = roi_sample(xs, rh, rw, tu[rw + py], tu[px]), o = out[src + p];
              g = gout[src + p];
              if (s != o) g *= exp(s - o);
            }
            G[p] = g;
          }
          __syncthreads();
          // the weights are separable: along x per row of i first, R(py, qx) = sum_px wx(px, qx) G(py, px), ...
          for (int p = t; p < cells; p += nt) {
            const int py = p / rw, cq = p - py * rw;
            const double cx = (double)cq;
            double row = 0.0;
            for (int px = lo[cq]; px <= hi[cq]; ++px) row += fmax(0.0, 1.0 - fabs(tu[px] - cx)) * G[py * rw + px];
            R[p] = row;
          }
          __syncthreads();
          // ... then along y per cell of j
#pragma unroll
          for (int e = 0; e < kRoiPer; ++e) {
            if (base + e * nt + t < cells) {
              const double cy = (double)qy[e];
              double total = 0.0;
              for (int py = lo[rw + qy[e]]; py <= hi[rw + qy[e]]; ++py) total += fmax(0.0, 1.0 - fabs(tu[rw + py] - cy)) * R[py * rw + qx[e]];
              acc[e] += total;
            }
          }
          __syncthreads();
        }
      }
    }
#pragma unroll
    for (int e = 0; e < kRoiPer; ++e) {
      const int q = base + e * nt + t;
      if (q < cells) gx[plane + q] = (float)acc[e];
    }
  }
}

static unsigned roi_threads(int rh, int rw) { return (rh * rw <= 64 * kRoiPer) ? 64u : (unsigned)kRoiThreads; }

static int roi_check(const char* what, const void* x, const void* rois, int n, int c, int rh, int rw) {
  if (n < 0 || c < 0 || rh < 1 || rw < 1) return fail(EPROPNP_EINVAL, "%s: num_rois, channels >= 0 and roi_height, roi_width >= 1 required", what);
  if ((long long)rh * rw > kRoiMaxCells) return fail(EPROPNP_EINVAL, "%s: roi_height * roi_width = %lld exceeds %d", what, (long long)rh * rw, kRoiMaxCells);
  if ((long long)n * c > 0x7fffffffLL) return fail(EPROPNP_EINVAL, "%s: num_rois * channels exceeds 2^31 - 1", what);
  if ((long long)n * c > 0 && (!x || !rois)) return fail(EPROPNP_EINVAL, "%s: NULL input", what);
  return EPROPNP_OK;
}

int launch_roi_logsumexp_forward(const float* x, const float* rois, int n, int c, int rh, int rw, float* out, hipStream_t st) {
  if (int rc = roi_check("roi_logsumexp_forward", x, rois, n, c, rh, rw)) return rc;
  if ((long long)n * c == 0) return EPROPNP_OK;
  if (!out) return fail(EPROPNP_EINVAL, "roi_logsumexp_forward: NULL output");
  const size_t bytes = (size_t)(rw + rh) * (sizeof(double) + sizeof(int));
  allow_dynamic_lds((const void*)roi_lse_forward_kernel, bytes);
  PNP_LAUNCH(roi_lse_forward_kernel, dim3((unsigned)(n * c)), dim3(roi_threads(rh, rw)), bytes, st, x, rois, n, c, rh, rw, out);
  return check_launch("roi_lse_forward_kernel");
}

int launch_roi_logsumexp_backward(const float* x, const float* rois, const float* out, const float* gout, int n, int c, int rh, int rw,
                                  float* gx, hipStream_t st) {
  if (int rc = roi_check("roi_logsumexp_backward", x, rois, n, c, rh, rw)) return rc;
  if ((long long)n * c == 0) return EPROPNP_OK;
  if (!out || !gout || !gx) return fail(EPROPNP_EINVAL, "roi_logsumexp_backward: NULL output, cotangent or gradient");
  const size_t cells = (size_t)rh * rw, axes = (size_t)rw + rh;
  const size_t bytes = cells * (2 * sizeof(double) + sizeof(float)) + axes * (sizeof(double) + 3 * sizeof(int));
  allow_dynamic_lds((const void*)roi_lse_backward_kernel, bytes);
  PNP_LAUNCH(roi_lse_backward_kernel, dim3((unsigned)(n * c)), dim3(roi_threads(rh, rw)), bytes, st, x, rois, out, gout, n, c, rh, rw, gx);
  return check_launch("roi_lse_backward_kernel");
}

}  // namespace pnp
