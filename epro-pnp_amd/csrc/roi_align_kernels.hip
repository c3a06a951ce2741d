// roi_align_kernels.hip -- RoIAlign (average pooling) of the detection head's auxiliary branch, forward and backward in one launch
// each, for one or two maps of identical geometry (include/epropnp_hip.h: epropnp_roi_align_forward, epropnp_roi_align_backward).
//
//   EPro-PnP-Det deform_pnp_head.py:719-741 (extract_rois) -- three mmcv roi_align calls, 28 x 28 cells, sampling_ratio = 0, 'avg',
//   aligned = True, on img_dense_x2d, key and value.  Cell (i, j) of RoI r is the mean of gh x gw bilinear samples of the map on a
//   regular grid inside the cell; a sample further than one pixel outside the map counts as 0, any other is clamped to the map.
//
// Average pooling over a regular grid is a SEPARABLE linear map: per RoI and channel out = Wy . map . Wx^T, where row i of Wy
// (ph x h) holds, for every map row Y, 1/gh times the sum over the cell's valid samples y of max(0, 1 - |clamp(y) - Y|) -- the two
// bilinear weights of every sample, merged per map row -- and Wx (pw x w) alike.  "Valid" is separable too: a sample is dropped when
// its y OR its x is out of range, which is the product of the two per-axis indicators.  A row of Wy is non-zero on a span of about
// bin size + 2 map rows.  `ra_weight` is that merged weight, formed in fp64 from the few samples that can reach the map row; the
// forward and the backward both take their tables from it, so the backward is the exact adjoint of the forward's weights.
//
// Forward: one workgroup per (RoI, cell row i, block of 32 cell columns).  The span of row i and the spans of the 32 columns go to
// LDS as merged weights (at most 64 entries per cell at a time: a longer span -- a bin of more than 62 map pixels -- is walked in
// chunks of 64 x 64, the later chunks adding to the cell in the same thread), then the threads walk (channel, cell) pairs and read
// every map element under a cell once, instead of 4 gh gw times.  Channels-last maps: a lane owns a channel, so one wave-instruction
// reads 256 contiguous bytes of a pixel; NCHW maps: a lane owns a cell along pw.  Two maps share the tables.
// Backward: dmap = sum_r Wy^T . dout_r . Wx, GATHERED by destination.  A workgroup owns an 8 x 8 pixel tile of one image's gradient
// map and 64 channels; it tests all RoIs, one per thread and 256 at a time (a bit mask in LDS), for its image and for a footprint that reaches
// the tile, walks the hits in ascending order, builds the weights of the tile's 8 rows and 8 columns against the RoI's cells (32 x 32 cells at a time)
// in LDS, finds per row / column the range of cells with a non-zero weight, and adds the RoI's contribution to the 16 elements each
// thread keeps in registers.  Every element of the gradient map is written exactly once with a plain store, zeros included: no
// zero-fill pass, no float atomic, every order fixed -- two launches return the same bits, forward and backward.
//
// Arithmetic: fp64 between the loads and the one rounding of each output, as in deform_kernels.hip and roi_kernels.hip (the kernels
// move bytes; fp64 FMAs are not what they wait for), so an output is the correctly rounded value of the separable form.
// Memory safety: no input VALUE forms an address unchecked.  The image id is compared against [0, NI) before it is used; a box with a
// non-finite corner or a grid of more than 2^30 samples per cell and axis is dropped whole (zeros, no gradient); every map index comes
// from a coordinate clamped to [0, size - 1] as a double first, and the launcher checks that the largest offset the strides can form
// lies inside the buffers.
#include "pnp_host.h"

namespace pnp {

constexpr int kRaThreads = 256;
constexpr int kRaCells = 32;                   // forward: cell columns per workgroup; backward: cells per axis and table round
constexpr int kRaSpan = 64, kRaRow = kRaSpan + 1;      // forward: weights per cell and chunk; the odd row stride spreads the LDS banks
constexpr int kRaTile = 8, kRaChan = 64, kRaAcc = kRaTile * kRaTile * kRaChan / kRaThreads;      // backward: tile, channels, registers
constexpr int kRaCol = kRaCells + 1;
constexpr int kRaMaxSampling = 1 << 15;
constexpr double kRaMaxGrid = 1073741824.0;    // 2^30 samples per cell and axis

struct RaArgs {
  const float* rois;
  long long sN, sC, sH, sW, oN, oC, oH, oW;    // element strides of the maps (and their gradients), of the outputs (and their cotangents)
  int bn, NI, C, h, w, ph, pw, sampling, aligned, nmaps;
  float scale;
};

// one axis of a RoI: sample s of cell c lies at start + c bin + (s + .5) bin / g; g = 0: no samples
struct RaAxis {
  double start, bin;
  int g;
};

struct RaBox {
  int n;                                       // image, -1: the RoI is dropped
  RaAxis y, x;
};

PNP_FN bool ra_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }      // false for NaN and +-inf

PNP_FN RaAxis ra_axis(float c1, float c2, int cells, const RaArgs& A, bool& ok) {
  const double o = A.aligned ? 0.5 : 0.0;
  const double s = (double)c1 * (double)A.scale - o, e = (double)c2 * (double)A.scale - o;
  double len = e - s;
  if (!A.aligned) len = fmax(len, 1.0);
  RaAxis a;
  a.start = s;
  a.bin = len / (double)cells;
  const double g = (A.sampling > 0) ? (double)A.sampling : ceil(a.bin);
  if (!(g <= kRaMaxGrid)) ok = false;
  a.g = (g >= 1.0 && g <= kRaMaxGrid) ? (int)g : 0;
  return a;
}

PNP_FN RaBox ra_box(const RaArgs& A, int r) {
  const float* q = A.rois + (size_t)r * 5;
  const float id = q[0], x1 = q[1], y1 = q[2], x2 = q[3], y2 = q[4];
  RaBox b;
  bool ok = id > -1.f && id < (float)A.NI && ra_finite(x1) && ra_finite(y1) && ra_finite(x2) && ra_finite(y2) && ra_finite(A.scale);
  b.y = ra_axis(y1, y2, A.ph, A, ok);
  b.x = ra_axis(x1, x2, A.pw, A, ok);
  b.n = ok ? min(max((int)id, 0), A.NI - 1) : -1;          // the conversion truncates, as the reference's
  return b;
}

PNP_FN double ra_coord(const RaAxis& a, int cell, int s) {
#pragma clang fp contract(off)
  return a.start + (double)cell * a.bin + ((double)s + 0.5) * a.bin / (double)a.g;
}

// the map indices that samples s0 of cell c0 .. s1 of cell c1 can touch: [lo, lo + n), n = 0 when all of them are out of range
PNP_FN void ra_reach(const RaAxis& a, int c0, int c1, int size, int& lo, int& n) {
  lo = 0;
  n = 0;
  if (a.g < 1) return;
  const double p = ra_coord(a, c0, 0), q = ra_coord(a, c1, a.g - 1);
  const double mn = fmin(p, q), mx = fmax(p, q), top = (double)(size - 1);
  if (!(mx >= -1.0 && mn <= (double)size)) return;
  lo = min(max((int)fmin(fmax(mn, 0.0), top), 0), size - 1);
  const int hi = min(max((int)fmin(fmax(mx, 0.0), top), 0) + 1, size - 1);
  n = hi - lo + 1;
}

// Row `cell` of Wy (or Wx) at map index X: 1/g times the sum over the cell's samples of valid(u) max(0, 1 - |clamp(u) - X|).  Only the
// samples within one pixel of X can contribute (a sample in [-1, 0) is clamped to 0, one in (size - 1, size] to size - 1: both still
// within one pixel of the index that receives them), so the sum runs over those, with a margin, in ascending s.
PNP_FN double ra_weight(const RaAxis& a, int cell, int X, int size) {
#pragma clang fp contract(off)
  if (a.g < 1) return 0.0;
  int s0 = 0, s1 = a.g - 1;
  const double step = a.bin / (double)a.g;
  if (step > 0.0 && a.g > 4) {
    const double base = a.start + (double)cell * a.bin, last = (double)(a.g - 1);
    const double lo = floor(((double)X - 1.0 - base) / step - 0.5) - 1.0, hi = ceil(((double)X + 1.0 - base) / step - 0.5) + 1.0;
    s0 = (int)fmin(fmax(lo, 0.0), last + 1.0);
    s1 = (int)fmin(fmax(hi, -1.0), last);
  }
  const double top = (double)(size - 1), at = (double)X;
  double acc = 0.0;
  for (int s = s0; s <= s1; ++s) {
    const double u = ra_coord(a, cell, s);
    if (!(u >= -1.0 && u <= (double)size)) continue;
    acc += fmax(0.0, 1.0 - fabs(fmin(fmax(u, 0.0), top) - at));
  }
  return acc / (double)a.g;
}

template <bool CL>
__global__ __launch_bounds__(kRaThreads) void roi_align_forward_kernel(RaArgs A, const float* __restrict__ map0,
                                                                       const float* __restrict__ map1, float* __restrict__ out0,
                                                                       float* __restrict__ out1) {
  __shared__ double wx[kRaCells * kRaRow];
  __shared__ double wy[kRaSpan];
  __shared__ int xlo[kRaCells], xn[kRaCells];
  const int t = (int)threadIdx.x;
  const int r = (int)(blockIdx.x / (unsigned)A.ph), i = (int)(blockIdx.x - (unsigned)r * (unsigned)A.ph);
  const int j0 = (int)blockIdx.y * kRaCells, nj = min(kRaCells, A.pw - j0);
  const RaBox B = ra_box(A, r);
  int ylo = 0, yn = 0;
  if (B.n >= 0) ra_reach(B.y, i, i, A.h, ylo, yn);
  if (t < nj) {
    int lo = 0, n = 0;
    if (B.n >= 0) ra_reach(B.x, j0 + t, j0 + t, A.w, lo, n);
    xlo[t] = lo;
    xn[t] = n;
  }
  __syncthreads();
  int xmax = 0;
  for (int k = 0; k < nj; ++k) xmax = max(xmax, xn[k]);
  const bool two = A.nmaps > 1;
  const int items = A.C * nj, sH = (int)A.sH, sW = (int)A.sW;      // offsets inside one plane fit 32 bits (launcher)
  if (yn == 0 || xmax == 0) {                  // nothing of row i lies on the map (or the RoI is dropped): zeros
    for (int item = t; item < items; item += kRaThreads) {
      const int c = CL ? item % A.C : item / nj, j = CL ? item / A.C : item % nj;
      const long long o = (long long)r * A.oN + (long long)c * A.oC + (long long)i * A.oH + (long long)(j0 + j) * A.oW;
      out0[o] = 0.f;
      if (A.nmaps > 1) out1[o] = 0.f;
    }
    return;
  }
  for (int qy = 0; qy < yn; qy += kRaSpan)
    for (int qx = 0; qx < xmax; qx += kRaSpan) {
      __syncthreads();                         // the previous chunk's tables are read no more
      const int ny = min(kRaSpan, yn - qy);
      for (int k = t; k < kRaSpan; k += kRaThreads) wy[k] = (k < ny) ? ra_weight(B.y, i, ylo + qy + k, A.h) : 0.0;
      for (int e = t; e < nj * kRaSpan; e += kRaThreads) {      // entries behind a span are 0: the loops below run in steps of 2 and 4
        const int j = e / kRaSpan, k = e - j * kRaSpan;
        wx[j * kRaRow + k] = (qx + k < xn[j]) ? ra_weight(B.x, j0 + j, xlo[j] + qx + k, A.w) : 0.0;
      }
      __syncthreads();
      const bool first = qy == 0 && qx == 0;
      for (int item = t; item < items; item += kRaThreads) {
        const int c = CL ? item % A.C : item / nj, j = CL ? item / A.C : item % nj;
        const int nx = min(kRaSpan, xn[j] - qx);
        const double* wj = wx + j * kRaRow;
        const long long src = (long long)B.n * A.sN + (long long)c * A.sC + (long long)(ylo + qy) * A.sH + (long long)(xlo[j] + qx) * A.sW;
        const long long o = (long long)r * A.oN + (long long)c * A.oC + (long long)i * A.oH + (long long)(j0 + j) * A.oW;
        if (nx <= 0) {                         // this cell's span ended in an earlier chunk
          if (first) {
            out0[o] = 0.f;
            if (two) out1[o] = 0.f;
          }
          continue;
        }
        // Two rows x four columns x two maps per trip: 16 independent loads in flight instead of one (the loop waits for memory
        // latency, not for arithmetic).  An index behind the span is clamped to its last element and meets a weight of 0; the sums
        // keep their order: columns ascending inside a row, rows ascending.
        const float* p0 = map0 + src;
        const float* p1 = two ? map1 + src : p0;
        double acc0 = 0.0, acc1 = 0.0;
        for (int ky = 0; ky < ny; ky += 2) {
          const int r0 = ky * sH, r1 = min(ky + 1, ny - 1) * sH;
          double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
          for (int kx = 0; kx < nx; kx += 4) {
            float u[4], v[4], g[4], q[4];
#pragma unroll
            for (int z = 0; z < 4; ++z) {
              const int c = min(kx + z, nx - 1) * sW;
              u[z] = p0[r0 + c];
              v[z] = p0[r1 + c];
              g[z] = two ? p1[r0 + c] : 0.f;
              q[z] = two ? p1[r1 + c] : 0.f;
            }
#pragma unroll
            for (int z = 0; z < 4; ++z) {
              const double wz = wj[kx + z];
              a0 += wz * (double)u[z];
              a1 += wz * (double)v[z];
              b0 += wz * (double)g[z];
              b1 += wz * (double)q[z];
            }
          }
          const double w0 = wy[ky], w1 = wy[ky + 1];
          acc0 += w0 * a0;
          acc0 += w1 * a1;
          acc1 += w0 * b0;
          acc1 += w1 * b1;
        }
        out0[o] = first ? (float)acc0 : (float)((double)out0[o] + acc0);
        if (two) out1[o] = first ? (float)acc1 : (float)((double)out1[o] + acc1);
      }
    }
}

template <bool CL>
__global__ __launch_bounds__(kRaThreads) void roi_align_backward_kernel(RaArgs A, const float* __restrict__ gout0,
                                                                        const float* __restrict__ gout1, float* __restrict__ gmap0,
                                                                        float* __restrict__ gmap1) {
  __shared__ double wt[2 * kRaTile * kRaCol];              // the tile's 8 rows against 32 cell rows, then its 8 columns against 32 cell columns
  __shared__ int rng[4 * kRaTile];                         // per tile row: first, last cell row with a weight; per tile column alike
  __shared__ int hits[kRaThreads / 32];
  const int t = (int)threadIdx.x, lane = t & 63, wv = t >> 6;
  const int cblocks = (A.C + kRaChan - 1) / kRaChan, tiles_x = (A.w + kRaTile - 1) / kRaTile;
  const int n = (int)(blockIdx.y / (unsigned)cblocks), cb = (int)(blockIdx.y - (unsigned)n * (unsigned)cblocks);
  const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
  const bool two = A.nmaps > 1;
  const int Y0 = ty * kRaTile, X0 = tx * kRaTile, oH = (int)A.oH, oW = (int)A.oW;      // offsets inside one plane fit 32 bits (launcher)
  // element e of this thread: channels-last -- the lane is the channel, the wave takes 16 of the 64 pixels; NCHW -- the lane is the pixel
  const int c_first = cb * kRaChan + (CL ? lane : wv * kRaAcc), p_first = CL ? wv * kRaAcc : lane;
  double acc[2][kRaAcc];
#pragma unroll
  for (int e = 0; e < kRaAcc; ++e) acc[0][e] = acc[1][e] = 0.0;
  for (int r0 = 0; r0 < A.bn; r0 += kRaThreads) {
    // the RoIs of this image whose footprint reaches the tile, 256 candidates at a time, one per thread: a 256-bit mask in LDS
    __syncthreads();
    if (t < kRaThreads / 32) hits[t] = 0;
    __syncthreads();
    if (r0 + t < A.bn) {
      const RaBox Q = ra_box(A, r0 + t);
      if (Q.n == n) {
        int lo, cnt, lo2, cnt2;
        ra_reach(Q.y, 0, A.ph - 1, A.h, lo, cnt);
        ra_reach(Q.x, 0, A.pw - 1, A.w, lo2, cnt2);
        if (cnt > 0 && lo <= Y0 + kRaTile - 1 && lo + cnt - 1 >= Y0 && cnt2 > 0 && lo2 <= X0 + kRaTile - 1 && lo2 + cnt2 - 1 >= X0)
          atomicOr(&hits[t >> 5], (int)(1u << (t & 31)));
      }
    }
    __syncthreads();
    for (int word = 0; word < kRaThreads / 32; ++word) {
    unsigned bits = (unsigned)__builtin_amdgcn_readfirstlane(hits[word]);
    while (bits != 0u) {                         // ascending RoI index: the order of the sum
    const int r = r0 + word * 32 + __builtin_ctz(bits);
    bits &= bits - 1u;
    const RaBox B = ra_box(A, r);
    for (int ib = 0; ib < A.ph; ib += kRaCells)
      for (int jb = 0; jb < A.pw; jb += kRaCells) {
        __syncthreads();                       // the previous round's tables are read no more
        for (int e = t; e < 2 * kRaTile * kRaCells; e += kRaThreads) {
          const int ax = e / (kRaTile * kRaCells), k = e - ax * (kRaTile * kRaCells), row = k / kRaCells, cell = k - row * kRaCells;
          double v = 0.0;
          if (ax == 0) {
            if (Y0 + row < A.h && ib + cell < A.ph) v = ra_weight(B.y, ib + cell, Y0 + row, A.h);
          } else {
            if (X0 + row < A.w && jb + cell < A.pw) v = ra_weight(B.x, jb + cell, X0 + row, A.w);
          }
          wt[(ax * kRaTile + row) * kRaCol + cell] = v;
        }
        __syncthreads();
        if (t < 2 * kRaTile) {
          const double* w = wt + t * kRaCol;
          int a = kRaCells, b = -1;
          for (int k = 0; k < kRaCells; ++k)
            if (w[k] != 0.0) {
              a = min(a, k);
              b = k;
            }
          rng[2 * t] = a;
          rng[2 * t + 1] = b;
        }
        __syncthreads();
        const long long cot = (long long)r * A.oN + (long long)ib * A.oH + (long long)jb * A.oW;
#pragma unroll
        for (int e = 0; e < kRaAcc; ++e) {
          const int c = c_first + (CL ? 0 : e), p = p_first + (CL ? e : 0), py = p / kRaTile, px = p - py * kRaTile;
          if (c >= A.C) continue;
          const int ilo = rng[2 * py], ihi = rng[2 * py + 1], jlo = rng[2 * (kRaTile + px)], jhi = rng[2 * (kRaTile + px) + 1];
          if (ihi < ilo || jhi < jlo) continue;
          const double* wyr = wt + py * kRaCol;
          const double* wxr = wt + (kRaTile + px) * kRaCol;
          // two cell rows x four cell columns x two maps per trip (independent loads in flight); an index behind the range is
          // clamped to its end and gets a weight of 0; cell columns ascending inside a row, cell rows ascending
          const float* g0 = gout0 + cot + (long long)c * A.oC;
          const float* g1 = two ? gout1 + cot + (long long)c * A.oC : g0;
          double sum0 = 0.0, sum1 = 0.0;
          for (int ci = ilo; ci <= ihi; ci += 2) {
            const bool more = ci + 1 <= ihi;
            const int r0 = ci * oH, r1 = (more ? ci + 1 : ci) * oH;
            double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
            for (int cj = jlo; cj <= jhi; cj += 4) {
              float u[4], v[4], k0[4], k1[4];
              double wz[4];
#pragma unroll
              for (int z = 0; z < 4; ++z) {
                const int jz = min(cj + z, jhi), off = jz * oW;
                wz[z] = (cj + z <= jhi) ? wxr[jz] : 0.0;
                u[z] = g0[r0 + off];
                v[z] = g0[r1 + off];
                k0[z] = two ? g1[r0 + off] : 0.f;
                k1[z] = two ? g1[r1 + off] : 0.f;
              }
#pragma unroll
              for (int z = 0; z < 4; ++z) {
                a0 += wz[z] * (double)u[z];
                a1 += wz[z] * (double)v[z];
                b0 += wz[z] * (double)k0[z];
                b1 += wz[z] * (double)k1[z];
              }
            }
            const double w0 = wyr[ci], w1 = more ? wyr[ci + 1] : 0.0;
            sum0 += w0 * a0;
            sum0 += w1 * a1;
            sum1 += w0 * b0;
            sum1 += w1 * b1;
          }
          acc[0][e] += sum0;
          acc[1][e] += sum1;
        }
      }
    }
    }
  }
#pragma unroll
  for (int e = 0; e < kRaAcc; ++e) {
    const int c = c_first + (CL ? 0 : e), p = p_first + (CL ? e : 0), py = p / kRaTile, px = p - py * kRaTile;
    if (c < A.C && Y0 + py < A.h && X0 + px < A.w) {
      const long long o = (long long)n * A.sN + (long long)c * A.sC + (long long)(Y0 + py) * A.sH + (long long)(X0 + px) * A.sW;
      gmap0[o] = (float)acc[0][e];
      if (A.nmaps > 1) gmap1[o] = (float)acc[1][e];
    }
  }
}

// the largest offset four strides can form over (d0, d1, d2, d3) lies inside d0 d1 d2 d3 elements
static bool ra_inside(long long d0, long long d1, long long d2, long long d3, long long s0, long long s1, long long s2, long long s3) {
  const double elems = (double)d0 * (double)d1 * (double)d2 * (double)d3;
  if (s0 < 1 || s1 < 1 || s2 < 1 || s3 < 1 || elems > 9.0e18) return false;
  if (elems == 0.0) return true;
  return (double)(d0 - 1) * (double)s0 + (double)(d1 - 1) * (double)s1 + (double)(d2 - 1) * (double)s2 + (double)(d3 - 1) * (double)s3 < elems;
}

static int ra_check(const char* what, const float* rois, int bn, int NI, int C, int h, int w, int ph, int pw, float scale, int sampling,
                    long long sN, long long sC, long long sH, long long sW, long long oN, long long oC, long long oH, long long oW) {
  if (bn < 0 || NI < 1 || C < 1 || h < 1 || w < 1 || ph < 1 || pw < 1)
    return fail(EPROPNP_EINVAL, "%s: num_rois >= 0 and num_img, channels, height, width, out_height, out_width >= 1 required", what);
  if (sampling < 0 || sampling > kRaMaxSampling) return fail(EPROPNP_EINVAL, "%s: sampling_ratio %d outside 0 .. %d", what, sampling, kRaMaxSampling);
  if (!(fabsf(scale) <= 3.4028234663852886e38f)) return fail(EPROPNP_EINVAL, "%s: spatial_scale is not finite", what);
  if (!ra_inside(NI, C, h, w, sN, sC, sH, sW))
    return fail(EPROPNP_EINVAL, "%s: the map strides reach outside num_img * channels * height * width elements", what);
  if (!ra_inside(bn, C, ph, pw, oN, oC, oH, oW))
    return fail(EPROPNP_EINVAL, "%s: the output strides reach outside num_rois * channels * out_height * out_width elements", what);
  if ((long long)(h - 1) * sH + (long long)(w - 1) * sW > 0x7fffffffLL || (long long)(ph - 1) * oH + (long long)(pw - 1) * oW > 0x7fffffffLL)
    return fail(EPROPNP_EINVAL, "%s: one channel of one image (or of one RoI) spans more than 2^31 elements", what);
  if ((long long)bn * ph > 0x7fffffffLL || (pw + kRaCells - 1) / kRaCells > 65535)
    return fail(EPROPNP_EINVAL, "%s: num_rois * out_height exceeds 2^31 - 1 or out_width 65535 * %d", what, kRaCells);
  if (bn > 0 && !rois) return fail(EPROPNP_EINVAL, "%s: NULL rois", what);
  return EPROPNP_OK;
}

int launch_roi_align_forward(const float* map0, const float* map1, const float* rois, int bn, int NI, int C, int h, int w, int ph, int pw,
                             float scale, int sampling, int aligned, long long sN, long long sC, long long sH, long long sW,
                             long long oN, long long oC, long long oH, long long oW, float* out0, float* out1, hipStream_t st) {
  if (int rc = ra_check("roi_align_forward", rois, bn, NI, C, h, w, ph, pw, scale, sampling, sN, sC, sH, sW, oN, oC, oH, oW)) return rc;
  if (!map0 || (bn > 0 && !out0) || ((map1 != nullptr) != (out1 != nullptr) && bn > 0))
    return fail(EPROPNP_EINVAL, "roi_align_forward: NULL map or output (the second map and the second output come together)");
  if (bn == 0) return EPROPNP_OK;
  const RaArgs A = {rois, sN, sC, sH, sW, oN, oC, oH, oW, bn, NI, C, h, w, ph, pw, sampling, aligned ? 1 : 0, map1 ? 2 : 1, scale};
  const dim3 grid((unsigned)(bn * ph), (unsigned)((pw + kRaCells - 1) / kRaCells));
  if (sC == 1) {
    PNP_LAUNCH(roi_align_forward_kernel<true>, grid, dim3(kRaThreads), 0, st, A, map0, map1, out0, out1);
  } else {
    PNP_LAUNCH(roi_align_forward_kernel<false>, grid, dim3(kRaThreads), 0, st, A, map0, map1, out0, out1);
  }
  return check_launch("roi_align_forward_kernel");
}

int launch_roi_align_backward(const float* gout0, const float* gout1, const float* rois, int bn, int NI, int C, int h, int w, int ph,
                              int pw, float scale, int sampling, int aligned, long long sN, long long sC, long long sH, long long sW,
                              long long oN, long long oC, long long oH, long long oW, float* gmap0, float* gmap1, hipStream_t st) {
  if (int rc = ra_check("roi_align_backward", rois, bn, NI, C, h, w, ph, pw, scale, sampling, sN, sC, sH, sW, oN, oC, oH, oW)) return rc;
  if (!gmap0 || (bn > 0 && !gout0) || (gmap1 != nullptr && bn > 0 && !gout1) || (gout1 != nullptr && !gmap1))
    return fail(EPROPNP_EINVAL, "roi_align_backward: NULL cotangent or gradient (the second pair comes together)");
  const long long tiles = (long long)((h + kRaTile - 1) / kRaTile) * ((w + kRaTile - 1) / kRaTile);
  const long long planes = (long long)NI * ((C + kRaChan - 1) / kRaChan);
  if (tiles > 0x7fffffffLL || planes > 65535)
    return fail(EPROPNP_EINVAL, "roi_align_backward: more than 2^31 - 1 tiles per image or num_img * ceil(channels / %d) > 65535", kRaChan);
  const RaArgs A = {rois, sN, sC, sH, sW, oN, oC, oH, oW, bn, NI, C, h, w, ph, pw, sampling, aligned ? 1 : 0, gmap1 ? 2 : 1, scale};
  const dim3 grid((unsigned)tiles, (unsigned)planes);
  if (sC == 1) {
    PNP_LAUNCH(roi_align_backward_kernel<true>, grid, dim3(kRaThreads), 0, st, A, gout0, gout1, gmap0, gmap1);
  } else {
    PNP_LAUNCH(roi_align_backward_kernel<false>, grid, dim3(kRaThreads), 0, st, A, gout0, gout1, gmap0, gmap1);
  }
  return check_launch("roi_align_backward_kernel");
}

}  // namespace pnp
