// density_kernels.hip -- density pictures of the posterior, the weighted pose samples (S,B,P) + log-weights (S,B)
// (include/epropnp_hip.h: epropnp_orient_density, epropnp_bev_density):
//
//   orientation sphere : EPro-PnP-6DoF lib/utils/draw_orient_density.py:10-73 -- the three rotated object axes of every sample
//       splatted onto an orthographic view of the unit sphere, front and back hemisphere apart, box-filtered, composed into colour.
//   BEV grid           : EPro-PnP-Det core/visualizer/image_bev_vis.py:79-95 -- the samples of all objects of an image, weighted by
//       sample weight x object weight, splatted onto one bird's-eye grid and box-filtered.
//
// Both are ONE primitive, a list of weighted points (canvas, plane, pixel, weight) summed into pixels and box-summed, in two launches:
//
//   density_points_kernel : one workgroup per object.  The column's maximum and sum (block_max / block_sum: a fixed order), then per
//       sample the weight w = exp(logw - max) / sum [* obj_weight] (ONE rounding in the exponent's argument, as
//       posterior_summary_kernel) and the bin(s) the geometry decides: -1 for a dropped point.  Per object eight words of `info`:
//       the bounding box of its bins and whether its column is bad (a NaN / +inf log-weight, nothing but -inf).
//   density_tile_kernel   : one workgroup per (canvas, 32 x 32 pixel tile); the unfiltered tile plus the window's halo lives in LDS.
//       The objects of the canvas whose bounding box misses tile + halo are sorted out 256 at a time; the samples of the others are
//       scanned in chunks of 256, one sample per thread: a thread parks its points' cells and its weight in LDS and sets its bit in
//       the mask of the group of 16 threads that holds the cell's owner (dens_owner: one of the 256 threads per cell); every thread
//       then walks the set bits of its group's mask in ascending order and adds the entries whose cell it owns.  So a cell is only
//       ever touched by one thread, and its sum runs in sample order: no floating-point atomics, two
//       launches agree to the last bit (the bit masks are built with integer OR, which has no order).  After the last chunk the
//       zero-padded box sum runs in place in LDS -- along the rows with a lane per row, then down the columns with a lane per
//       column, each output a direct sum of its window; skipped for a tile nothing fell into -- and the epilogue (the BEV density;
//       the sphere's densities and colour composite) reads it.
// LDS does not depend on S or B; every output element is written; no allocation, no synchronisation.
#include "pnp_host.h"

namespace pnp {

constexpr int kDensTile = 32, kDensThreads = 256, kDensMaxWin = 9, kDensMaxSize = 4096;
constexpr int kDensEdge = kDensTile + kDensMaxWin - 1;      // a tile row with both halos
constexpr int kDensStride = kDensEdge + 1;                  // its stride in LDS: odd, so that the lanes of a row-per-lane pass hit 32 banks
constexpr int kDensCached = 4;                              // samples per thread the points kernel keeps in registers
constexpr int kDensInfo = 8;                                // words per object: xmin, -xmax, ymin, -ymax, bad, 3 spare
constexpr int kDensGroups = 16;                             // owner threads share a mask per group of 256 / 16 = 16
static_assert(kDensThreads == 256, "a cell's owner is one of 256 threads; eight 32-bit mask words per chunk");

// The thread that owns a cell of the LDS tile: a bijection of the low 8 bits that sends neighbouring cells to different groups,
// so that the hits of a compact blob spread over the groups' lists.
PNP_FN int dens_owner(int cell) { return (cell * 17) & (kDensThreads - 1); }

struct DensArgs {
  const float* pose; const float* logw; const float* obj_weight; const float* pose_opt; const int32_t* offsets;
  int32_t* info; float* wts; int32_t* bins;    // scratch, object-major: wts[b][j], bins[b][k][j] (a tile reads an object's column)
  int32_t* bins_out;                           // the caller's (S,B,K) bins or NULL
  float *out0, *out1, *image;                  // BEV: out0 = density.  sphere: front, back, image
  int S, B, P, H, W, kh, kw, ox, oy;
  float scale;                                 // BEV: pixels per unit.  sphere: 0.4 size
  float centre, sat, opac, intensity;
};

PNP_FN float dens_weight(float v, float M) { return (v == M) ? 1.0f : expf(v - M); }

// the pixel of a coordinate; false when it is off the canvas or not finite
PNP_FN bool dens_pixel(float f, int n, int& p) {
  const float r = rintf(f);                    // round half to even, as torch.round
  const bool in = r >= 0.f && r <= (float)(n - 1);
  p = in ? (int)r : 0;
  return in;
}

template <bool SPHERE>
__global__ __launch_bounds__(kDensThreads) void density_points_kernel(DensArgs a) {
  constexpr int K = SPHERE ? 3 : 1;
  __shared__ float red[kDensThreads / 64];
  __shared__ int box[4];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, S = a.S, B = a.B;
  if (tid < 4) box[tid] = 0x7fffffff;
  // ---- the column: maximum, then the sum of exp(logw - max).  The first kDensCached samples of a thread stay in registers, with
  // what the bins need of their poses: one round trip to memory for S <= 256 kDensCached ----
  constexpr int NV = SPHERE ? 4 : 2;
  float vc[kDensCached], pc[kDensCached][NV];
#pragma unroll
  for (int i = 0; i < kDensCached; ++i) {
    const int j = tid + i * kDensThreads;
    const size_t at = (size_t)(j < S ? j : 0) * B + b;
    vc[i] = (j < S) ? a.logw[at] : -INFINITY;
    const float* p = a.pose + at * a.P;
    if (SPHERE) { pc[i][0] = p[3]; pc[i][1] = p[4]; pc[i][2] = p[5]; pc[i][3] = p[6]; }
    else { pc[i][0] = p[0]; pc[i][1] = p[2]; }
  }
  float m = -INFINITY;
  bool poison = false;
#pragma unroll
  for (int i = 0; i < kDensCached; ++i) {
    poison = poison || (vc[i] != vc[i]) || (vc[i] == INFINITY);
    m = (vc[i] > m) ? vc[i] : m;
  }
  for (int j = tid + kDensCached * kDensThreads; j < S; j += kDensThreads) {
    const float v = a.logw[(size_t)j * B + b];
    poison = poison || (v != v) || (v == INFINITY);
    m = (v > m) ? v : m;
  }
  const float M = block_max(poison ? INFINITY : m, red);
  const bool bad = M == INFINITY || M == -INFINITY;
  float acc[1] = {0.f};
  if (!bad) {
#pragma unroll
    for (int i = 0; i < kDensCached; ++i) {
      vc[i] = dens_weight(vc[i], M);           // (a slot beyond S: exp(-inf) = 0)
      acc[0] += vc[i];
    }
    for (int j = tid + kDensCached * kDensThreads; j < S; j += kDensThreads) acc[0] += dens_weight(a.logw[(size_t)j * B + b], M);
  }
  block_sum<1>(acc, red);
  const float Wsum = acc[0];
  const float ow = (!SPHERE && a.obj_weight != nullptr) ? a.obj_weight[b] : 1.0f;
  // ---- per sample: weight and bins ----
  int xmin = 0x7fffffff, nxmax = 0x7fffffff, ymin = 0x7fffffff, nymax = 0x7fffffff;
  auto emit = [&](int j, float e, const float* q) {      // e = exp(logw - max); q: the quaternion / (x, z)
    const size_t at = (size_t)j * B + b;
    const float w = bad ? NAN : e / Wsum;
    a.wts[(size_t)b * S + j] = SPHERE ? w : mul_unfused(w, ow);
    if (SPHERE) {
      float R[9];
      quat_to_rot(q[0], q[1], q[2], q[3], R);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float fx = add_unfused(mul_unfused(R[k], a.scale), a.centre), fy = add_unfused(mul_unfused(R[3 + k], a.scale), a.centre);
        const float az = R[6 + k];
        int px, py;
        const bool okx = dens_pixel(fx, a.W, px), oky = dens_pixel(fy, a.H, py);
        const bool ok = okx && oky && fabsf(az) < INFINITY;
        const int bin = ok ? py * a.W + px + ((az <= 0.f) ? 0 : a.H * a.W) : -1;
        a.bins[((size_t)b * K + k) * S + j] = bin;
        if (a.bins_out != nullptr) a.bins_out[at * K + k] = bin;
        if (ok) { xmin = min(xmin, px); nxmax = min(nxmax, -px); ymin = min(ymin, py); nymax = min(nymax, -py); }
      }
    } else {
      const float rx = rintf(mul_unfused(q[1], a.scale)), ry = rintf(mul_unfused(q[0], a.scale));
      const bool fin = fabsf(rx) < 1e9f && fabsf(ry) < 1e9f;
      const long px = (long)(fin ? rx : 0.f) + a.ox, py = (long)(fin ? ry : 0.f) + a.oy;
      const bool ok = fin && px >= 0 && px < a.W && py >= 0 && py < a.H;
      const int bin = ok ? (int)(py * a.W + px) : -1;
      a.bins[(size_t)b * S + j] = bin;
      if (a.bins_out != nullptr) a.bins_out[at] = bin;
      if (ok) { xmin = min(xmin, (int)px); nxmax = min(nxmax, -(int)px); ymin = min(ymin, (int)py); nymax = min(nymax, -(int)py); }
    }
  };
#pragma unroll
  for (int i = 0; i < kDensCached; ++i)
    if (tid + i * kDensThreads < S) emit(tid + i * kDensThreads, vc[i], pc[i]);
  for (int j = tid + kDensCached * kDensThreads; j < S; j += kDensThreads) {
    const float* p = a.pose + ((size_t)j * B + b) * a.P;
    const float q[4] = {SPHERE ? p[3] : p[0], SPHERE ? p[4] : p[2], SPHERE ? p[5] : 0.f, SPHERE ? p[6] : 0.f};
    emit(j, bad ? 0.f : dens_weight(a.logw[(size_t)j * B + b], M), q);
  }
  __syncthreads();                             // box[] is initialised
  if (xmin != 0x7fffffff) {
    atomicMin(&box[0], xmin); atomicMin(&box[1], nxmax); atomicMin(&box[2], ymin); atomicMin(&box[3], nymax);
  }
  __syncthreads();
  if (tid < kDensInfo) a.info[(size_t)b * kDensInfo + tid] = (tid < 4) ? box[tid] : ((tid == 4 && bad) ? 1 : 0);
}

// squared distance of (x, y) from the segment (ox, oy) - (ex, ey)
PNP_FN float dens_segment_dist2(float x, float y, float ox, float oy, float ex, float ey) {
  const float dx = ex - ox, dy = ey - oy, qx = x - ox, qy = y - oy;
  const float len2 = dx * dx + dy * dy;
  float t = (len2 > 0.f) ? (qx * dx + qy * dy) / len2 : 0.f;
  t = fminf(fmaxf(t, 0.f), 1.f);
  const float rx = qx - t * dx, ry = qy - t * dy;
  return rx * rx + ry * ry;
}

// exponent of 2 of col ^ e: 0 for e == 0 whatever the colour (0 ^ 0 = 1, as torch.pow)
PNP_FN float dens_pow_term(float e, float lg) { return (e == 0.f) ? 0.f : e * lg; }

// line[i * stride] <- sum_{d < KW} line[(i + d) * stride] for the kDensTile outputs of a line with halo, in place: output i is
// written after the inputs i .. i + KW - 1 were read, and no later output reads position i.  A direct sum, left to right: a line
// of zeros stays exactly zero.
template <int KW>
PNP_FN void dens_box_line_k(float* line, int stride) {
  float w[KW];
#pragma unroll
  for (int d = 1; d < KW; ++d) w[d] = line[(d - 1) * stride];
#pragma unroll
  for (int i = 0; i < kDensTile; ++i) {
#pragma unroll
    for (int d = 0; d + 1 < KW; ++d) w[d] = w[d + 1];
    w[KW - 1] = line[(i + KW - 1) * stride];
    float s = w[0];
#pragma unroll
    for (int d = 1; d < KW; ++d) s += w[d];
    line[i * stride] = s;
  }
}

PNP_FN void dens_box_line(float* line, int stride, int k) {
  switch (k) {
    case 3: dens_box_line_k<3>(line, stride); break;
    case 5: dens_box_line_k<5>(line, stride); break;
    case 7: dens_box_line_k<7>(line, stride); break;
    case 9: dens_box_line_k<9>(line, stride); break;
    default: break;                            // 1: the line is its own sum
  }
}

template <bool SPHERE>
__global__ __launch_bounds__(kDensThreads) void density_tile_kernel(DensArgs a) {
  constexpr int K = SPHERE ? 3 : 1, NP = SPHERE ? 6 : 1;
  __shared__ float raw[NP * kDensEdge * kDensStride];
  __shared__ int cell[2][K][kDensThreads];
  __shared__ float cw[2][kDensThreads];
  __shared__ int pmask[3][kDensGroups][K][8], omask[8], hitlist[kDensThreads], anyhit;
  const int tid = (int)threadIdx.x, c = (int)blockIdx.y, S = a.S, B = a.B, H = a.H, W = a.W;
  const int tiles_x = (W + kDensTile - 1) / kDensTile;
  const int x0 = ((int)blockIdx.x % tiles_x) * kDensTile, y0 = ((int)blockIdx.x / tiles_x) * kDensTile;
  const int ph = a.kh / 2, pw = a.kw / 2, TH = kDensTile + 2 * ph, TW = kDensTile + 2 * pw;
  const int nchunk = (S + kDensThreads - 1) / kDensThreads;
  for (int i = tid; i < NP * TH * kDensStride; i += kDensThreads) raw[i] = 0.f;
  for (int i = tid; i < 3 * kDensGroups * K * 8; i += kDensThreads) (&pmask[0][0][0][0])[i] = 0;
  if (tid == 0) anyhit = 0;
  int ob0 = SPHERE ? c : a.offsets[c], ob1 = SPHERE ? c + 1 : a.offsets[c + 1];
  ob0 = max(0, min(ob0, B));
  ob1 = max(ob0, min(ob1, B));
  // a bad column: the sphere's canvas is NaN everywhere; a BEV object adds nothing
  const bool nan_canvas = SPHERE && a.info[(size_t)c * kDensInfo + 4] != 0;
  int step = 0;                                // chunks scanned so far: cell / cw of chunk `step` live in buffer step & 1, its masks in step % 3
  for (int oc = ob0; oc < ob1; oc += kDensThreads) {
    // ---- the objects of this round that reach the tile, in object order ----
    if (tid < 8) omask[tid] = 0;
    __syncthreads();
    bool mine = false;
    if (oc + tid < ob1) {
      const int32_t* in = a.info + (size_t)(oc + tid) * kDensInfo;
      mine = in[0] <= x0 + kDensTile - 1 + pw && -in[1] >= x0 - pw && in[2] <= y0 + kDensTile - 1 + ph && -in[3] >= y0 - ph && in[4] == 0;
      if (mine) atomicOr(&omask[tid >> 5], (int)(1u << (tid & 31)));
    }
    __syncthreads();
    int nhit = 0, before = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const unsigned m = (unsigned)omask[i];
      const int n = __builtin_popcount(m);
      before += (i < (tid >> 5)) ? n : ((i == (tid >> 5)) ? __builtin_popcount(m & ((1u << (tid & 31)) - 1u)) : 0);
      nhit += n;
    }
    if (mine) hitlist[before] = oc + tid;
    __syncthreads();
    // ---- their samples, 256 at a time.  One barrier per chunk: a thread parks its sample (loaded during the chunk before), the
    // block meets, every thread adds the entries whose cell it owns.  The buffers a chunk writes were last read two (cell, cw)
    // or three (masks, cleared behind the barrier of the chunk in between) chunks earlier.
    const int nwork = nhit * nchunk;
    float wn = 0.f;
    int bn[K];
#pragma unroll
    for (int k = 0; k < K; ++k) bn[k] = -1;
    auto fetch = [&](int it) {
      const int b = hitlist[it / nchunk], j = (it % nchunk) * kDensThreads + tid;
      const bool in = j < S;
      const size_t at = (size_t)b * S + (in ? j : 0);
      wn = in ? a.wts[at] : 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) bn[k] = in ? a.bins[at + (size_t)(b * (K - 1) + k) * S] : -1;
    };
    if (nwork > 0) fetch(0);
    for (int it = 0; it < nwork; ++it, ++step) {
      const int buf = step & 1, mb = step % 3;
      cw[buf][tid] = wn;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int bin = bn[k];
        int loc = -1;
        if (bin >= 0 && bin < (SPHERE ? 2 : 1) * H * W && wn != 0.f) {
          const int hemi = (bin >= H * W) ? 1 : 0, pix = bin - hemi * H * W;
          const int ly = pix / W - y0 + ph, lx = pix % W - x0 + pw;
          if (lx >= 0 && lx < TW && ly >= 0 && ly < TH) loc = ((hemi * K + k) * TH + ly) * kDensStride + lx;
        }
        cell[buf][k][tid] = loc;
        if (loc >= 0) {
          atomicOr(&pmask[mb][dens_owner(loc) >> 4][k][tid >> 5], (int)(1u << (tid & 31)));
          anyhit = 1;
        }
      }
      if (it + 1 < nwork) fetch(it + 1);
      __syncthreads();
      for (int i = tid; i < kDensGroups * K * 8; i += kDensThreads) (&pmask[(mb + 2) % 3][0][0][0])[i] = 0;
      // this thread's group's list, four entries at a time; consecutive hits of one cell are summed in a register, in list order
      int cur = -1;
      float sum = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        unsigned mw[8];
#pragma unroll
        for (int pd = 0; pd < 8; ++pd) mw[pd] = (unsigned)pmask[mb][tid >> 4][k][pd];
#pragma unroll 1
        for (int pd = 0; pd < 8; ++pd) {
          unsigned mk = mw[pd];
          while (mk != 0u) {
            int loc[4];
            float w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int e = pd * 32 + ((mk != 0u) ? __builtin_ctz(mk) : 0);
              loc[u] = (mk != 0u) ? cell[buf][k][e] : -1;
              w[u] = cw[buf][e];
              mk &= mk - 1u;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              if (loc[u] >= 0 && dens_owner(loc[u]) == tid) {
                if (loc[u] != cur) {
                  if (cur >= 0) raw[cur] = sum;
                  cur = loc[u];
                  sum = raw[cur];
                }
                sum += w[u];
              }
            }
          }
        }
      }
      if (cur >= 0) raw[cur] = sum;
    }
  }
  __syncthreads();
  // ---- the zero-padded box sum, in place: along the rows (a lane per row), then down the columns (a lane per column); a tile
  // that nothing fell into is all zeros already ----
  const bool hit = anyhit != 0;
  if (hit) {
    for (int i = tid; i < NP * TH; i += kDensThreads) dens_box_line(raw + i * kDensStride, 1, a.kw);
    __syncthreads();
    for (int i = tid; i < NP * kDensTile; i += kDensThreads)
      dens_box_line(raw + (i / kDensTile) * TH * kDensStride + i % kDensTile, kDensStride, a.kh);
    __syncthreads();
  }
  // ---- epilogue ----
  float lg_diag = 0.f, lg_off = 0.f, ax[3] = {0.f, 0.f, 0.f}, ay[3] = {0.f, 0.f, 0.f};
  const bool lines = SPHERE && a.pose_opt != nullptr;
  if (SPHERE) {
    lg_diag = log2f(a.sat + (1.0f - a.sat) * 0.5f);
    lg_off = log2f((1.0f - a.sat) * 0.5f);
    if (lines) {
      const float* p = a.pose_opt + (size_t)c * 7;
      float R[9];
      quat_to_rot(p[3], p[4], p[5], p[6], R);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        ax[k] = add_unfused(mul_unfused(R[k], a.scale), a.centre);
        ay[k] = add_unfused(mul_unfused(R[3 + k], a.scale), a.centre);
      }
    }
  }
  for (int p = tid; p < kDensTile * kDensTile; p += kDensThreads) {
    const int lx = p % kDensTile, ly = p / kDensTile, gx = x0 + lx, gy = y0 + ly;
    if (gx >= W || gy >= H) continue;
    float d[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) d[q] = nan_canvas ? NAN : raw[(q * TH + ly) * kDensStride + lx];
    const size_t at = ((size_t)c * H + gy) * W + gx;
    if (!SPHERE) {
      a.out0[at] = d[0];
      continue;
    }
    if (a.out0 != nullptr)
      for (int k = 0; k < 3; ++k) a.out0[at * 3 + k] = d[k];
    if (a.out1 != nullptr)
      for (int k = 0; k < 3; ++k) a.out1[at * 3 + k] = d[3 + k];
    if (a.image == nullptr) continue;
    // circle = 1 - 0.5 [(x - c)^2 + (y - c)^2 <= (0.4 size)^2], in the reference's normalised form
    const float ux = ((float)gx - a.centre) / a.scale, uy = ((float)gy - a.centre) / a.scale;      // (gx is the same for a thread's pixels)
    const float circle = (add_unfused(mul_unfused(ux, ux), mul_unfused(uy, uy)) <= 1.0f) ? 0.5f : 1.0f;
    int line = -1;
    if (lines) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (dens_segment_dist2((float)gx, (float)gy, a.centre, a.centre, ax[k], ay[k]) <= 2.25f) line = k;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float front_layer = 1.0f, back_layer = 1.0f;      // (an empty tile: every colour to the power 0)
      if (hit || nan_canvas) {
        float ef = 0.f, eb = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float lg = (k == ch) ? lg_diag : lg_off;
          ef += dens_pow_term(a.intensity * d[k], lg);
          eb += dens_pow_term(a.intensity * d[3 + k], lg);
        }
        front_layer = exp2f(ef);
        back_layer = exp2f(eb);
      }
      const float base = (line >= 0) ? ((line == ch) ? 1.0f : 0.0f)
                                     : add_unfused(mul_unfused(back_layer, a.opac), mul_unfused(circle, 1.0f - a.opac));
      a.image[at * 3 + ch] = mul_unfused(base, front_layer);
    }
  }
}

static size_t density_scratch_bytes(long S, long B, int K) {
  if (S < 1 || B < 1) return 0;
  return (size_t)B * kDensInfo * sizeof(int32_t) + (size_t)S * B * sizeof(float) + (size_t)S * B * K * sizeof(int32_t);
}
size_t orient_density_scratch_bytes(int S, int B) { return density_scratch_bytes(S, B, 3); }
size_t bev_density_scratch_bytes(int S, int B) { return density_scratch_bytes(S, B, 1); }

// info | weights | bins
static void density_carve(DensArgs& a, void* scratch, int32_t* bins_out) {
  char* p = (char*)scratch;
  a.info = (int32_t*)p;
  p += (size_t)a.B * kDensInfo * sizeof(int32_t);
  a.wts = (float*)p;
  p += (size_t)a.S * a.B * sizeof(float);
  a.bins = (int32_t*)p;
  a.bins_out = bins_out;
}

static bool density_window_ok(int k) { return k >= 1 && k <= kDensMaxWin && (k & 1) == 1; }

int launch_orient_density(const float* pose, const float* logw, const float* pose_opt, int S, int B, int dof, int size, int kh,
                          int kw, float saturation, float opacity, float intensity, void* scratch, size_t scratch_bytes,
                          float* image, float* front, float* back, int32_t* bins, hipStream_t st) {
  if (B < 0) return fail(EPROPNP_EINVAL, "epropnp_orient_density: num_obj must be >= 0, got %d", B);
  if (dof != 6) return fail(EPROPNP_EINVAL, "epropnp_orient_density: dof must be 6 (the sphere shows orientations), got %d", dof);
  if (S < 1) return fail(EPROPNP_EINVAL, "epropnp_orient_density: mc_samples must be >= 1, got %d", S);
  if (size < 1 || size > kDensMaxSize) return fail(EPROPNP_EINVAL, "epropnp_orient_density: size must be 1 .. %d, got %d", kDensMaxSize, size);
  if (!density_window_ok(kh) || !density_window_ok(kw))
    return fail(EPROPNP_EINVAL, "epropnp_orient_density: the window must be odd, 1 .. %d, got (%d, %d)", kDensMaxWin, kh, kw);
  if (B == 0) return EPROPNP_OK;
  if (B > 65535) return fail(EPROPNP_EINVAL, "epropnp_orient_density: num_obj = %d is more than the 65535 of one call", B);
  if (!pose || !logw || !scratch || (!image && !front && !back && !bins)) return fail(EPROPNP_EINVAL, "epropnp_orient_density: NULL pointer");
  if (scratch_bytes < orient_density_scratch_bytes(S, B))
    return fail(EPROPNP_EINVAL, "epropnp_orient_density: scratch of %zu bytes is smaller than epropnp_orient_density_scratch_bytes(%d, %d) = %zu",
                scratch_bytes, S, B, orient_density_scratch_bytes(S, B));
  DensArgs a{};
  a.pose = pose; a.logw = logw; a.pose_opt = pose_opt;
  a.S = S; a.B = B; a.P = 7; a.H = size; a.W = size; a.kh = kh; a.kw = kw;
  a.scale = (float)size * 0.4f;
  a.centre = (float)size * 0.5f - 0.5f;
  a.sat = saturation; a.opac = opacity; a.intensity = intensity;
  a.out0 = front; a.out1 = back; a.image = image;
  density_carve(a, scratch, bins);
  PNP_LAUNCH(density_points_kernel<true>, dim3((unsigned)B), dim3(kDensThreads), 0, st, a);
  int rc = check_launch("density_points_kernel");
  if (rc != EPROPNP_OK || (!image && !front && !back)) return rc;
  const int t = (size + kDensTile - 1) / kDensTile;
  PNP_LAUNCH(density_tile_kernel<true>, dim3((unsigned)(t * t), (unsigned)B), dim3(kDensThreads), 0, st, a);
  return check_launch("density_tile_kernel");
}

int launch_bev_density(const float* pose, const float* logw, const float* obj_weight, const int32_t* offsets, int S, int B, int G,
                       int dof, int H, int W, float scale, int ox, int oy, int window, void* scratch, size_t scratch_bytes,
                       float* density, int32_t* bins, hipStream_t st) {
  if (B < 0 || G < 0) return fail(EPROPNP_EINVAL, "epropnp_bev_density: num_obj and num_groups must be >= 0, got %d and %d", B, G);
  if (dof != 4 && dof != 6) return fail(EPROPNP_EINVAL, "epropnp_bev_density: dof must be 4 or 6, got %d", dof);
  if (S < 1) return fail(EPROPNP_EINVAL, "epropnp_bev_density: mc_samples must be >= 1, got %d", S);
  if (H < 1 || H > kDensMaxSize || W < 1 || W > kDensMaxSize)
    return fail(EPROPNP_EINVAL, "epropnp_bev_density: height and width must be 1 .. %d, got %d and %d", kDensMaxSize, H, W);
  if (!density_window_ok(window)) return fail(EPROPNP_EINVAL, "epropnp_bev_density: the window must be odd, 1 .. %d, got %d", kDensMaxWin, window);
  if (G > 65535) return fail(EPROPNP_EINVAL, "epropnp_bev_density: num_groups = %d is more than the 65535 of one call", G);
  if (B > 0 && (!pose || !logw || !scratch)) return fail(EPROPNP_EINVAL, "epropnp_bev_density: NULL pointer");
  if (G > 0 && (!offsets || !density)) return fail(EPROPNP_EINVAL, "epropnp_bev_density: NULL pointer");
  if (scratch_bytes < bev_density_scratch_bytes(S, B))
    return fail(EPROPNP_EINVAL, "epropnp_bev_density: scratch of %zu bytes is smaller than epropnp_bev_density_scratch_bytes(%d, %d) = %zu",
                scratch_bytes, S, B, bev_density_scratch_bytes(S, B));
  DensArgs a{};
  a.pose = pose; a.logw = logw; a.obj_weight = obj_weight; a.offsets = offsets;
  a.S = S; a.B = B; a.P = (dof == 6) ? 7 : 4; a.H = H; a.W = W; a.kh = window; a.kw = window; a.ox = ox; a.oy = oy;
  a.scale = scale;
  a.out0 = density;
  if (B > 0) {
    density_carve(a, scratch, bins);
    PNP_LAUNCH(density_points_kernel<false>, dim3((unsigned)B), dim3(kDensThreads), 0, st, a);
    const int rc = check_launch("density_points_kernel");
    if (rc != EPROPNP_OK) return rc;
  }
  if (G == 0) return EPROPNP_OK;
  const int tx = (W + kDensTile - 1) / kDensTile, ty = (H + kDensTile - 1) / kDensTile;
  PNP_LAUNCH(density_tile_kernel<false>, dim3((unsigned)(tx * ty), (unsigned)G), dim3(kDensThreads), 0, st, a);
  return check_launch("density_tile_kernel");
}

}  // namespace pnp
