// center_target_kernels.hip -- the centre targets of the detection head's training step (include/epropnp_hip.h:
// epropnp_volume_centers, epropnp_box_thickness): EPro-PnP-Det core/bbox_3d/center_target.py:42-259, VolumeCenter with the box mesh.
//
// The reference renders every ground-truth box with a mesh rasteriser, takes the depth thickness of each box along each render
// pixel's ray, resamples it at the output cells and returns the thickness-weighted 2D centre per object.  For the box mesh the
// rasteriser's near / far depth pair of a pixel is the ray-box slab intersection, so nothing is rendered here:
//
//   ct_table_kernel   : one thread per object.  A row of 16 words: cos / sin of the yaw, the camera centre in the box frame, the half
//       extents, a conservative rectangle of the box's projection in original-image pixels (infinite unless all eight corners lie
//       beyond z_clip), the image and a flag (not finite / in no image).
//   ct_partial_kernel : one workgroup per (image, 16 x 16 tile of output cells); a thread owns a cell, a wave four rows of it.  The
//       image's rows live in LDS, 128 objects at a time.  Per object a wave whose cells all miss the rectangle moves on; the others
//       take the four bilinear taps of their cell analytically -- a ray-box test per tap (ct_ray), plus the count of the image's
//       other fragments in front of the far face where faces_per_pixel can bind -- and reduce thickness, thickness x column,
//       thickness x row (tile-local, so that the fp32 wave sums stay short) and the four extents of the >= 0.5 valid cells
//       through wave_ops.h.  One partial row per (tile, object) goes to scratch, the four waves added in wave order in fp64.
//   ct_reduce_kernel  : one workgroup per object: its threads fetch the image's partial rows 256 at a time, thread 0 adds them in tile
//       order in fp64 and writes centre, box and valid.
//   ct_thickness_kernel : one thread per (object, render pixel): the same ct_ray written out, what the fused pass never stores.
//
// No floating-point atomics and every order fixed: two launches agree to the last bit.  No input value ever forms an address: the
// x2d maps only choose which rays are tested.  Every output element is written; no allocation, no synchronisation.
#include "pnp_host.h"

namespace pnp {

constexpr int kCtThreads = 256, kCtTile = 16, kCtRow = 16, kCtCap = 128, kCtMaxSize = 4096;
static_assert(kCtTile * kCtTile == kCtThreads, "a thread owns one cell of the tile");
// row words: 0 cos, 1 sin, 2..4 camera centre in the box frame, 5..7 half extents, 8..11 rectangle x0 x1 y0 y1, 12 image, 13 bad
constexpr int kCtImg = 12, kCtBad = 13;

struct CtArgs {
  const float* boxes3d; const float* boxes2d_in; const int32_t* offsets; const float* cam; const float* x2d; const float* mask;
  float* table; double* sums; int32_t* ext;      // scratch
  float* centers; float* boxes2d; uint8_t* valid;
  float* thick; uint8_t* tvalid;                 // epropnp_box_thickness
  int B, G, h, w, Hr, Wr, os, rs, K, want_box;
  float zc, min_box;
};

PNP_FN bool ct_finite(float x) { return fabsf(x) < INFINITY; }

// the objects of image g, clamped into [0, B]
PNP_FN void ct_range(const int32_t* off, int g, int B, int& o0, int& o1) {
  o0 = max(0, min(off[g], B));
  o1 = max(o0, min(off[g + 1], B));
}

// Ray (dx, dy, 1) from the camera against the box of `row`: its entry and exit parameters, which are camera depths.  false: a miss.
PNP_FN bool ct_slab(const float* row, float dx, float dy, float& lo, float& hi) {
  const float c = row[0], s = row[1];
  const float b[3] = {c * dx - s, dy, s * dx + c};
  lo = -INFINITY;
  hi = INFINITY;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float o = row[2 + k], e = row[5 + k];
    if (b[k] == 0.f) {
      if (fabsf(o) > e) return false;
    } else {
      const float t1 = (-e - o) / b[k], t2 = (e - o) / b[k];
      lo = fmaxf(lo, fminf(t1, t2));
      hi = fminf(hi, fmaxf(t1, t2));
    }
  }
  return lo <= hi;
}

PNP_FN bool ct_in_rect(const float* row, float u, float v, float margin) {
  return u + margin >= row[8] && u - margin <= row[9] && v + margin >= row[10] && v - margin <= row[11];
}

// The pixel whose centre lies at (u, v) in original-image coordinates, for the object `self` of the table `tab` (rows of the
// objects o0 .. o1 - 1 of its image, tab[0] the row of o0): true iff both faces of the box are fragments (beyond zc) and the far
// one is among the K nearest fragments of the image at that pixel (K == 0: no limit; bind == false: it cannot bind).
PNP_FN bool ct_ray(const float* tab, int o0, int o1, int self, float u, float v, float fx, float fy, float cx, float cy, float zc,
                   int K, bool bind, float& thick) {
  const float dx = (u - cx) / fx, dy = (v - cy) / fy;
  float lo, hi;
  thick = 0.f;
  if (!ct_slab(tab + (size_t)(self - o0) * kCtRow, dx, dy, lo, hi)) return false;
  if (!(hi > lo && lo > zc)) return false;
  if (bind) {
    int cnt = 1;                                 // the object's own near fragment
    for (int q = o0; q < o1 && cnt < K; ++q) {
      const float* r = tab + (size_t)(q - o0) * kCtRow;
      if (q == self || r[kCtBad] != 0.f || !ct_in_rect(r, u, v, 0.f)) continue;
      float l2, h2;
      if (!ct_slab(r, dx, dy, l2, h2)) continue;
      cnt += (l2 > zc && l2 < hi) ? 1 : 0;
      cnt += (h2 > zc && h2 < hi) ? 1 : 0;
    }
    if (cnt >= K) return false;
  }
  thick = hi - lo;
  return true;
}

__global__ __launch_bounds__(kCtThreads) void ct_table_kernel(CtArgs a) {
  const int b = (int)(blockIdx.x * kCtThreads + threadIdx.x);
  if (b >= a.B) return;
  float* row = a.table + (size_t)b * kCtRow;
  int g = -1;
  for (int i = 0; i < a.G && g < 0; ++i) {
    int o0, o1;
    ct_range(a.offsets, i, a.B, o0, o1);
    if (b >= o0 && b < o1) g = i;
  }
  const float* p = a.boxes3d + (size_t)b * 7;
  bool bad = g < 0;
#pragma unroll
  for (int k = 0; k < 7; ++k) bad = bad || !ct_finite(p[k]);
  float fx = 1.f, fy = 1.f, cx = 0.f, cy = 0.f;
  if (g >= 0) {
    const float* Km = a.cam + (size_t)g * 9;
    fx = Km[0]; fy = Km[4]; cx = Km[2]; cy = Km[5];
    bad = bad || !ct_finite(fx) || !ct_finite(fy) || !ct_finite(cx) || !ct_finite(cy) || fx == 0.f || fy == 0.f;
  }
  if (bad) {
#pragma unroll
    for (int k = 0; k < kCtRow; ++k) row[k] = 0.f;
    row[kCtImg] = (float)g;
    row[kCtBad] = 1.f;
    return;
  }
  const float c = cosf(p[6]), s = sinf(p[6]);
  const float ex = 0.5f * fabsf(p[0]), ey = 0.5f * fabsf(p[1]), ez = 0.5f * fabsf(p[2]);
  row[0] = c; row[1] = s;
  // R^T (0 - centre), R = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
  row[2] = -(c * p[3] - s * p[5]); row[3] = -p[4]; row[4] = -(s * p[3] + c * p[5]);
  row[5] = ex; row[6] = ey; row[7] = ez;
  // the rectangle of the eight projected corners, one pixel wider; infinite where a corner is not beyond z_clip or not finite
  float x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
  bool all_front = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float vx = (k & 1) ? ex : -ex, vy = (k & 2) ? ey : -ey, vz = (k & 4) ? ez : -ez;
    const float X = c * vx + s * vz + p[3], Y = vy + p[4], Z = -s * vx + c * vz + p[5];
    const float u = fx * X / Z + cx, v = fy * Y / Z + cy;
    all_front = all_front && Z > a.zc && ct_finite(u) && ct_finite(v);
    x0 = fminf(x0, u); x1 = fmaxf(x1, u); y0 = fminf(y0, v); y1 = fmaxf(y1, v);
  }
  if (all_front) {
    const float mx = 1.f + 1e-5f * fmaxf(fabsf(x0), fabsf(x1)), my = 1.f + 1e-5f * fmaxf(fabsf(y0), fabsf(y1));
    row[8] = x0 - mx; row[9] = x1 + mx; row[10] = y0 - my; row[11] = y1 + my;
  } else {
    row[8] = -INFINITY; row[9] = INFINITY; row[10] = -INFINITY; row[11] = INFINITY;
  }
  row[kCtImg] = (float)g;
  row[kCtBad] = 0.f;
  row[14] = 0.f; row[15] = 0.f;
}

__global__ __launch_bounds__(kCtThreads) void ct_partial_kernel(CtArgs a) {
  __shared__ float tab[kCtCap * kCtRow];
  __shared__ float wsum[kCtThreads / 64][kCtCap][3];
  __shared__ unsigned wext[kCtThreads / 64][kCtCap][4];
  const int tid = (int)threadIdx.x, g = (int)blockIdx.y, tile = (int)blockIdx.x, wv = wave_id(), lane = lane_id();
  const int tiles_x = (a.w + kCtTile - 1) / kCtTile;
  const int tx0 = (tile % tiles_x) * kCtTile, ty0 = (tile / tiles_x) * kCtTile;
  const int lx = tid & (kCtTile - 1), ly = tid / kCtTile, j = tx0 + lx, i = ty0 + ly;
  int ob0, ob1;
  ct_range(a.offsets, g, a.B, ob0, ob1);
  const int n = ob1 - ob0;
  const bool bind = a.K > 0 && 2 * n > a.K;
  const bool big = n > kCtCap;                   // the image's rows do not fit: the other objects of a pixel are read from memory
  const float* Km = a.cam + (size_t)g * 9;
  const float fx = Km[0], fy = Km[4], cx = Km[2], cy = Km[5];
  // ---- this thread's cell: coordinate, mask, the four taps ----
  const bool in = j < a.w && i < a.h;
  const size_t cell = (size_t)(in ? i : 0) * a.w + (in ? j : 0);
  const size_t plane = (size_t)a.h * a.w;
  const float x = in ? a.x2d[((size_t)g * 2) * plane + cell] : NAN, y = in ? a.x2d[((size_t)g * 2 + 1) * plane + cell] : NAN;
  const float m = in ? a.mask[(size_t)g * plane + cell] : 0.f;
  const float rsf = (float)a.rs;
  const float gx = (x + 0.5f) / rsf - 0.5f, gy = (y + 0.5f) / rsf - 0.5f;
  const bool live = in && m != 0.f && m == m && gx > -1.f && gx < (float)a.Wr && gy > -1.f && gy < (float)a.Hr;
  const float fx0 = live ? floorf(gx) : 0.f, fy0 = live ? floorf(gy) : 0.f;
  const int c0 = (int)fx0, r0 = (int)fy0;
  const float wx1 = live ? gx - fx0 : 0.f, wy1 = live ? gy - fy0 : 0.f, wx0 = 1.f - wx1, wy0 = 1.f - wy1;
  for (int oc = ob0; oc < ob1; oc += kCtCap) {
    const int nc = min(kCtCap, ob1 - oc);
    __syncthreads();                             // the chunk before has been written out
    for (int k = tid; k < nc * kCtRow; k += kCtThreads) tab[k] = a.table[(size_t)oc * kCtRow + k];
    for (int k = tid; k < (kCtThreads / 64) * kCtCap; k += kCtThreads) {
      float* s = &wsum[0][0][0] + (size_t)k * 3;
      unsigned* e = &wext[0][0][0] + (size_t)k * 4;
      s[0] = 0.f; s[1] = 0.f; s[2] = 0.f;
      e[0] = 0xffffffffu; e[1] = 0xffffffffu; e[2] = 0xffffffffu; e[3] = 0xffffffffu;
    }
    __syncthreads();
    for (int o = 0; o < nc; ++o) {
      const float* row = tab + o * kCtRow;
      if (row[kCtBad] != 0.f) continue;
      const bool hit = live && ct_in_rect(row, x, y, rsf);      // the taps lie within render_stride of the cell's coordinate
      if (wave_max(hit ? 1.f : 0.f) == 0.f) continue;           // wave-uniform: the reductions below are met by all lanes or none
      float t = 0.f, vm = 0.f;
      if (hit) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int c = c0 + (k & 1), r = r0 + (k >> 1);
          if (c < 0 || c >= a.Wr || r < 0 || r >= a.Hr) continue;
          const float u = rsf * ((float)c + 0.5f) - 0.5f, v = rsf * ((float)r + 0.5f) - 0.5f;
          float th;
          const bool ok = big ? ct_ray(a.table + (size_t)ob0 * kCtRow, ob0, ob1, oc + o, u, v, fx, fy, cx, cy, a.zc, a.K, bind, th)
                              : ct_ray(tab, ob0, ob1, oc + o, u, v, fx, fy, cx, cy, a.zc, a.K, bind, th);
          const float wt = ((k & 1) ? wx1 : wx0) * ((k >> 1) ? wy1 : wy0);
          t += wt * th;
          vm += ok ? wt : 0.f;
        }
        t *= m;
        vm *= m;
      }
      const float s0 = wave_sum(t), s1 = wave_sum(t * (float)lx), s2 = wave_sum(t * (float)ly);
      unsigned e0 = 0xffffffffu, e1 = 0xffffffffu, e2 = 0xffffffffu, e3 = 0xffffffffu;
      if (a.want_box) {
        const bool on = vm >= 0.5f;
        e0 = wave_min_u32(on ? (unsigned)j : 0xffffffffu);
        e1 = wave_min_u32(on ? (unsigned)(kCtMaxSize - j) : 0xffffffffu);
        e2 = wave_min_u32(on ? (unsigned)i : 0xffffffffu);
        e3 = wave_min_u32(on ? (unsigned)(kCtMaxSize - i) : 0xffffffffu);
      }
      if (lane == 0) {
        wsum[wv][o][0] = s0; wsum[wv][o][1] = s1; wsum[wv][o][2] = s2;
        wext[wv][o][0] = e0; wext[wv][o][1] = e1; wext[wv][o][2] = e2; wext[wv][o][3] = e3;
      }
    }
    __syncthreads();
    for (int o = tid; o < nc; o += kCtThreads) {
      double st = 0.0, sx = 0.0, sy = 0.0;
      unsigned e[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
#pragma unroll
      for (int q = 0; q < kCtThreads / 64; ++q) {
        st += (double)wsum[q][o][0]; sx += (double)wsum[q][o][1]; sy += (double)wsum[q][o][2];
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = min(e[k], wext[q][o][k]);
      }
      const size_t at = (size_t)tile * a.B + (oc + o);
      a.sums[at * 3] = st;
      a.sums[at * 3 + 1] = sx + (double)tx0 * st;      // in cells
      a.sums[at * 3 + 2] = sy + (double)ty0 * st;
#pragma unroll
      for (int k = 0; k < 4; ++k) a.ext[at * 4 + k] = (int32_t)e[k];
    }
  }
}

__global__ __launch_bounds__(kCtThreads) void ct_reduce_kernel(CtArgs a) {
  __shared__ double part[kCtThreads][3];
  __shared__ unsigned pext[kCtThreads][4];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const float* row = a.table + (size_t)b * kCtRow;
  const bool bad = row[kCtBad] != 0.f;           // (the same for the whole workgroup)
  const int tiles = ((a.w + kCtTile - 1) / kCtTile) * ((a.h + kCtTile - 1) / kCtTile);
  double st = 0.0, sx = 0.0, sy = 0.0;
  unsigned e[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  if (!bad) {
    // 256 tiles at a time: every thread fetches one partial row, thread 0 adds them in tile order
    for (int t0 = 0; t0 < tiles; t0 += kCtThreads) {
      const int nt = min(kCtThreads, tiles - t0);
      __syncthreads();
      if (tid < nt) {
        const size_t at = (size_t)(t0 + tid) * a.B + b;
#pragma unroll
        for (int k = 0; k < 3; ++k) part[tid][k] = a.sums[at * 3 + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) pext[tid][k] = (unsigned)a.ext[at * 4 + k];
      }
      __syncthreads();
      if (tid == 0) {
        for (int t = 0; t < nt; ++t) {
          st += part[t][0]; sx += part[t][1]; sy += part[t][2];
#pragma unroll
          for (int k = 0; k < 4; ++k) e[k] = min(e[k], pext[t][k]);
        }
      }
    }
  }
  if (tid != 0) return;
  const double os = (double)a.os;
  const bool some = st != 0.0 && st == st;
  a.centers[(size_t)b * 2] = some ? (float)(os * (sx / st) + 0.5 * os) : 0.f;
  a.centers[(size_t)b * 2 + 1] = some ? (float)(os * (sy / st) + 0.5 * os) : 0.f;
  float bx[4];
  if (a.want_box) {
    const bool any = e[0] != 0xffffffffu;
    bx[0] = any ? (float)((int)e[0] * a.os) : (float)(a.w * a.os);
    bx[1] = any ? (float)((int)e[2] * a.os) : (float)(a.h * a.os);
    bx[2] = any ? (float)((kCtMaxSize - (int)e[1]) * a.os + a.os) : (float)a.os;
    bx[3] = any ? (float)((kCtMaxSize - (int)e[3]) * a.os + a.os) : (float)a.os;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) bx[k] = a.boxes2d_in[(size_t)b * 4 + k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) a.boxes2d[(size_t)b * 4 + k] = bx[k];
  const bool ok = !bad && st >= 1e-6 && (bx[2] - bx[0]) >= a.min_box && (bx[3] - bx[1]) >= a.min_box;
  a.valid[b] = ok ? 1 : 0;
}

__global__ __launch_bounds__(kCtThreads) void ct_thickness_kernel(CtArgs a) {
  const int b = (int)blockIdx.y, pix = (int)(blockIdx.x * kCtThreads + threadIdx.x);
  if (pix >= a.Hr * a.Wr) return;
  const float* row = a.table + (size_t)b * kCtRow;
  const size_t at = (size_t)b * a.Hr * a.Wr + pix;
  float th = 0.f;
  bool ok = false;
  if (row[kCtBad] == 0.f) {
    const int g = (int)row[kCtImg];
    int ob0, ob1;
    ct_range(a.offsets, g, a.B, ob0, ob1);
    const float* Km = a.cam + (size_t)g * 9;
    const float rsf = (float)a.rs;
    const float u = rsf * ((float)(pix % a.Wr) + 0.5f) - 0.5f, v = rsf * ((float)(pix / a.Wr) + 0.5f) - 0.5f;
    ok = ct_ray(a.table + (size_t)ob0 * kCtRow, ob0, ob1, b, u, v, Km[0], Km[4], Km[2], Km[5], a.zc, a.K,
                a.K > 0 && 2 * (ob1 - ob0) > a.K, th);
  }
  a.thick[at] = th;
  a.tvalid[at] = ok ? 1 : 0;
}

static size_t ct_table_bytes(long B) { return (size_t)B * kCtRow * sizeof(float); }
static long ct_tiles(int h, int w) { return (long)((w + kCtTile - 1) / kCtTile) * ((h + kCtTile - 1) / kCtTile); }

size_t volume_centers_scratch_bytes(int B, int h, int w) {
  if (B < 1 || h < 0 || w < 0 || h > kCtMaxSize || w > kCtMaxSize) return 0;
  return ct_table_bytes(B) + (size_t)ct_tiles(h, w) * B * (3 * sizeof(double) + 4 * sizeof(int32_t));
}

static int ct_check_common(const char* who, int B, int G, int rs, int K, float zc) {
  if (B < 0 || G < 0) return fail(EPROPNP_EINVAL, "%s: num_obj and num_img must be >= 0, got %d and %d", who, B, G);
  if (G > 65535) return fail(EPROPNP_EINVAL, "%s: num_img = %d is more than the 65535 of one call", who, G);
  if (rs < 1) return fail(EPROPNP_EINVAL, "%s: render_stride must be >= 1, got %d", who, rs);
  if (K != 0 && K < 2) return fail(EPROPNP_EINVAL, "%s: faces_per_pixel must be >= 2, or 0 for no limit, got %d", who, K);
  if (!(zc >= 0.f)) return fail(EPROPNP_EINVAL, "%s: z_clip must be >= 0, got %g", who, (double)zc);
  return EPROPNP_OK;
}

static int ct_launch_table(CtArgs& a, void* scratch, hipStream_t st) {
  a.table = (float*)scratch;
  PNP_LAUNCH(ct_table_kernel, dim3((unsigned)((a.B + kCtThreads - 1) / kCtThreads)), dim3(kCtThreads), 0, st, a);
  return check_launch("ct_table_kernel");
}

int launch_volume_centers(const float* boxes3d, const float* boxes2d_in, const int32_t* offsets, const float* cam, const float* x2d,
                          const float* mask, int B, int G, int h, int w, int Hr, int Wr, int os, int rs, int K, float zc,
                          float min_box, int want_box, void* scratch, size_t scratch_bytes, float* centers, float* boxes2d,
                          uint8_t* valid, hipStream_t st) {
  const char* who = "epropnp_volume_centers";
  int rc = ct_check_common(who, B, G, rs, K, zc);
  if (rc != EPROPNP_OK) return rc;
  if (os < 1) return fail(EPROPNP_EINVAL, "%s: output_stride must be >= 1, got %d", who, os);
  if (h < 1 || h > kCtMaxSize || w < 1 || w > kCtMaxSize || Hr < 1 || Hr > kCtMaxSize || Wr < 1 || Wr > kCtMaxSize)
    return fail(EPROPNP_EINVAL, "%s: the output and render sizes must be 1 .. %d, got (%d, %d) and (%d, %d)", who, kCtMaxSize, h, w, Hr, Wr);
  if ((long)w * os > (1 << 24) || (long)h * os > (1 << 24))
    return fail(EPROPNP_EINVAL, "%s: output size x output_stride must stay within 2^24", who);
  if (B == 0) return EPROPNP_OK;
  if (!boxes3d || !offsets || !cam || !x2d || !mask || !scratch || !centers || !boxes2d || !valid || (!want_box && !boxes2d_in))
    return fail(EPROPNP_EINVAL, "%s: NULL pointer", who);
  if (G == 0) return fail(EPROPNP_EINVAL, "%s: %d objects but no image", who, B);
  if (scratch_bytes < volume_centers_scratch_bytes(B, h, w) || ((uintptr_t)scratch & 7u) != 0)
    return fail(EPROPNP_EINVAL, "%s: scratch of %zu bytes is smaller than epropnp_volume_centers_scratch_bytes(%d, %d, %d) = %zu, or not 8-byte aligned",
                who, scratch_bytes, B, h, w, volume_centers_scratch_bytes(B, h, w));
  CtArgs a{};
  a.boxes3d = boxes3d; a.boxes2d_in = boxes2d_in; a.offsets = offsets; a.cam = cam; a.x2d = x2d; a.mask = mask;
  a.centers = centers; a.boxes2d = boxes2d; a.valid = valid;
  a.B = B; a.G = G; a.h = h; a.w = w; a.Hr = Hr; a.Wr = Wr; a.os = os; a.rs = rs; a.K = K; a.want_box = want_box ? 1 : 0;
  a.zc = zc; a.min_box = min_box;
  rc = ct_launch_table(a, scratch, st);
  if (rc != EPROPNP_OK) return rc;
  const long tiles = ct_tiles(h, w);
  a.sums = (double*)((char*)scratch + ct_table_bytes(B));
  a.ext = (int32_t*)((char*)a.sums + (size_t)tiles * B * 3 * sizeof(double));
  PNP_LAUNCH(ct_partial_kernel, dim3((unsigned)tiles, (unsigned)G), dim3(kCtThreads), 0, st, a);
  rc = check_launch("ct_partial_kernel");
  if (rc != EPROPNP_OK) return rc;
  PNP_LAUNCH(ct_reduce_kernel, dim3((unsigned)B), dim3(kCtThreads), 0, st, a);
  return check_launch("ct_reduce_kernel");
}

int launch_box_thickness(const float* boxes3d, const int32_t* offsets, const float* cam, int B, int G, int Hr, int Wr, int rs, int K,
                         float zc, void* scratch, size_t scratch_bytes, float* thick, uint8_t* valid, hipStream_t st) {
  const char* who = "epropnp_box_thickness";
  int rc = ct_check_common(who, B, G, rs, K, zc);
  if (rc != EPROPNP_OK) return rc;
  if (Hr < 1 || Hr > kCtMaxSize || Wr < 1 || Wr > kCtMaxSize)
    return fail(EPROPNP_EINVAL, "%s: the render size must be 1 .. %d, got (%d, %d)", who, kCtMaxSize, Hr, Wr);
  if (B == 0) return EPROPNP_OK;
  if (B > 65535) return fail(EPROPNP_EINVAL, "%s: num_obj = %d is more than the 65535 of one call", who, B);
  if (!boxes3d || !offsets || !cam || !scratch || !thick || !valid) return fail(EPROPNP_EINVAL, "%s: NULL pointer", who);
  if (G == 0) return fail(EPROPNP_EINVAL, "%s: %d objects but no image", who, B);
  if (scratch_bytes < volume_centers_scratch_bytes(B, 0, 0))
    return fail(EPROPNP_EINVAL, "%s: scratch of %zu bytes is smaller than epropnp_volume_centers_scratch_bytes(%d, 0, 0) = %zu", who,
                scratch_bytes, B, volume_centers_scratch_bytes(B, 0, 0));
  CtArgs a{};
  a.boxes3d = boxes3d; a.offsets = offsets; a.cam = cam; a.thick = thick; a.tvalid = valid;
  a.B = B; a.G = G; a.Hr = Hr; a.Wr = Wr; a.rs = rs; a.K = K; a.zc = zc;
  rc = ct_launch_table(a, scratch, st);
  if (rc != EPROPNP_OK) return rc;
  PNP_LAUNCH(ct_thickness_kernel, dim3((unsigned)((Hr * Wr + kCtThreads - 1) / kCtThreads), (unsigned)B), dim3(kCtThreads), 0, st, a);
  return check_launch("ct_thickness_kernel");
}

}  // namespace pnp
