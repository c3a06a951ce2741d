// boxes_kernels.hip -- rotated bird's-eye-view boxes on the device (include/epropnp_hip.h: epropnp_bev_overlap, epropnp_bev_nms):
// pairwise / aligned overlap area and IoU of (cx, cy, dx, dy, angle) boxes and the greedy, grouped non-maximum suppression the
// detection head ends with (EPro-PnP-Det core/bbox_3d/misc.py:300-324 batched_bev_nms, ops/iou3d: nms_gpu, boxes_iou_bev -- there
// a CUDA extension whose suppression mask is reduced on the host).
//
//   bev_overlap_area : the ONE overlap routine of every kernel here.  A's corners are expressed in B's frame -- relative to B's
//       centre, A's half axes turned by angle_A - angle_B, so that the centres' magnitude never enters a product -- and
//           area(A n B) = | sum over A's 4 edges of  integral of clamp(y_e(x), -hy, hy) dx  over the edge's x inside [-hx, hx] |
//       (hx, hy: B's half sizes).  Per edge, taken left to right whichever way it runs: clamp its x range into [-hx, hx], clamp the
//       two x at which it crosses y = -hy and y = +hy into that range, and apply the trapezoid rule to the three pieces -- clamp(y) is
//       linear on each, the rule is exact.  No intersection points are collected or sorted, nothing is indexed at run time (no scratch
//       memory), no margins: the result is a continuous function of the ten inputs, and rounding on coincident edges moves it by
//       rounding only.  Identical boxes, a box against itself turned by a quarter or half turn, boxes sharing an edge or a corner
//       and a zero-width box give exactly area / 0: the relative angle is reduced by the ONE fp32 constant fl(pi/2), so that a
//       difference of exactly k fl(pi/2) is k quarter turns, and the two coincident edges of a degenerate box see identical operands.
//       Products are kept uncontracted: the pairwise, the aligned and the suppression kernels give the same bits for the same pair.
//   bev_overlap_kernel      : 64 x 64 tiles; row and column boxes staged in LDS in prepared form (centre, cos, sin, half sizes, area,
//       angle); a lane owns a column (its box in registers), a wave walks the tile's rows: coalesced stores.
//   bev_nms_mask_kernel     : one wave per 64 x 64 tile of the VISITING order, column tile >= row tile; column boxes gathered through
//       `order` into LDS; a lane owns a row and emits one 64-bit word (bit j: this row suppresses position 64 ct + j).  Pairs of
//       different groups or out of each other's reach are sorted out first; each lane then walks its own candidates.  The self
//       bit of a diagonal word flags a row that can never be kept (invalid box, order entry out of range).
//   bev_nms_reduce_kernel   : one workgroup; `removed` bitset in LDS; per row tile one wave resolves the 64 diagonal words serially in
//       registers (v_readlane), then all threads OR the kept rows' words into the later tiles' `removed` words (independent loads).
// No atomics, no cross-workgroup waiting, no allocation, no synchronisation: two launches agree to the last bit.
#include "pnp_host.h"

namespace pnp {

constexpr int kBevTile = EPROPNP_BEV_TILE;
constexpr int kBevOverlapThreads = 256, kBevReduceThreads = 256;
constexpr int kBevMaxTiles = 4096;             // the reduce launch's `removed` bitset: 32 KiB of LDS, 262144 boxes
static_assert(kBevTile == 64, "a tile is one wave wide: one mask word per row and tile");

// A box in the form the pair routine takes.  area is NaN for an invalid box (a component that is not finite, a negative size).
struct BevBox {
  float cx, cy, c, s, hx, hy, area, ang;
};

constexpr float kPio2Hi = 1.57079637050628662109375f, kPio2Lo = -4.371139000186241e-8f, kTwoOverPi = 0.636619772367581343f;

// cos and sin of r + q pi/2, |r| <= pi/4 (+ rounding): the Cephes single-precision kernels, exact at r == 0
PNP_FN void bev_sincos_quadrant(float r, int q, float& c, float& s) {
  const float z = r * r;
  const float sr = fmaf(r * z, fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f), r);
  const float cr = fmaf(z * z, fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f),
                        fmaf(-0.5f, z, 1.f));
  q &= 3;
  c = (q == 0) ? cr : (q == 1) ? -sr : (q == 2) ? -cr : sr;
  s = (q == 0) ? sr : (q == 1) ? cr : (q == 2) ? -sr : -cr;
}

PNP_FN float bev_quarter_turns(float a) { return fminf(fmaxf(rintf(a * kTwoOverPi), -1e9f), 1e9f); }

PNP_FN BevBox bev_prepare(const float* __restrict__ b) {
  const float cx = b[0], cy = b[1], dx = b[2], dy = b[3], a = b[4];
  const bool ok = fabsf(cx) < INFINITY && fabsf(cy) < INFINITY && dx >= 0.f && dx < INFINITY && dy >= 0.f && dy < INFINITY &&
                  fabsf(a) < INFINITY;
  BevBox o;
  const float ang = ok ? a : 0.f;
  const float k = bev_quarter_turns(ang);
  const float r = fmaf(-k, kPio2Lo, fmaf(-k, kPio2Hi, ang));      // the box's own angle: two-constant reduction
  bev_sincos_quadrant(r, (int)k, o.c, o.s);
  o.cx = cx; o.cy = cy;
  o.hx = 0.5f * dx; o.hy = 0.5f * dy;
  o.area = ok ? dx * dy : NAN;
  o.ang = ang;
  return o;
}

PNP_FN BevBox bev_no_box() {
  BevBox o;
  o.cx = o.cy = o.s = o.hx = o.hy = o.ang = 0.f;
  o.c = 1.f;
  o.area = NAN;
  return o;
}

PNP_FN float bev_clamp(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// integral of clamp(y(x), -hy, hy) dx along the edge (x0, y0) -> (x1, y1), over its x inside [-hx, hx]; signed by the edge's direction
PNP_FN float bev_edge(float x0, float y0, float x1, float y1, float hx, float hy) {
#pragma clang fp contract(off)
  const bool fwd = x1 >= x0;
  const float xa = fwd ? x0 : x1, ya = fwd ? y0 : y1, xb = fwd ? x1 : x0, yb = fwd ? y1 : y0;
  const float w = xb - xa, dy = yb - ya;
  // a vertical edge contributes nothing; neither does a slope whose quotient would not be finite
  const float m = (w > 1e-30f) ? dy / w : 0.f;                    // dy / dx
  const float n = (w > 1e-30f && dy != 0.f) ? w / dy : 0.f;       // dx / dy; a horizontal edge: the crossings collapse, clamp(y) is constant
  const float xl = fmaxf(xa, -hx), xr = fmaxf(fminf(xb, hx), xl);
  const float ca = fmaf(-hy - ya, n, xa), cb = fmaf(hy - ya, n, xa);
  const float c1 = bev_clamp(fminf(ca, cb), xl, xr), c2 = bev_clamp(fmaxf(ca, cb), xl, xr);
  const float y0c = bev_clamp(fmaf(xl - xa, m, ya), -hy, hy), y1c = bev_clamp(fmaf(c1 - xa, m, ya), -hy, hy);
  const float y2c = bev_clamp(fmaf(c2 - xa, m, ya), -hy, hy), y3c = bev_clamp(fmaf(xr - xa, m, ya), -hy, hy);
  const float sum = ((c1 - xl) * (y0c + y1c) + (c2 - c1) * (y1c + y2c)) + (xr - c2) * (y2c + y3c);
  const float v = (w > 1e-30f) ? 0.5f * sum : 0.f;
  return fwd ? v : -v;
}

// area(A n B); both boxes valid
PNP_FN float bev_overlap_area(const BevBox& A, const BevBox& B) {
#pragma clang fp contract(off)
  const float ddx = A.cx - B.cx, ddy = A.cy - B.cy;
  const float pu = ddx * B.c - ddy * B.s, pv = ddx * B.s + ddy * B.c;      // A's centre in B's frame
  const float da = A.ang - B.ang;
  const float k = bev_quarter_turns(da);
  float cd, sd;
  bev_sincos_quadrant(fmaf(-k, kPio2Hi, da), (int)k, cd, sd);           // ONE constant: k fl(pi/2) is exactly k quarter turns
  const float exx = A.hx * cd, exy = -(A.hx * sd), eyx = A.hy * sd, eyy = A.hy * cd;
  const float x0 = (pu + exx) + eyx, y0 = (pv + exy) + eyy;
  const float x1 = (pu + exx) - eyx, y1 = (pv + exy) - eyy;
  const float x2 = (pu - exx) - eyx, y2 = (pv - exy) - eyy;
  const float x3 = (pu - exx) + eyx, y3 = (pv - exy) + eyy;
  const float e0 = bev_edge(x0, y0, x1, y1, B.hx, B.hy), e1 = bev_edge(x1, y1, x2, y2, B.hx, B.hy);
  const float e2 = bev_edge(x2, y2, x3, y3, B.hx, B.hy), e3 = bev_edge(x3, y3, x0, y0, B.hx, B.hy);
  return fabsf(((e0 + e1) + e2) + e3);
}

PNP_FN float bev_iou_of(float overlap, float area_a, float area_b) {
#pragma clang fp contract(off)
  return overlap / fmaxf(area_a + area_b - overlap, 1e-8f);
}

// overlap or IoU of a pair; NaN as soon as one box is invalid
PNP_FN float bev_pair(const BevBox& A, const BevBox& B, int want_iou) {
  const float ov = bev_overlap_area(A, B);
  const float v = want_iou ? bev_iou_of(ov, A.area, B.area) : ov;
  return (A.area == A.area && B.area == B.area) ? v : NAN;
}

__global__ __launch_bounds__(kBevOverlapThreads) void bev_overlap_kernel(const float* __restrict__ boxes_a, int M,
                                                                         const float* __restrict__ boxes_b, int N, int want_iou,
                                                                         float* __restrict__ out) {
  __shared__ BevBox rows[kBevTile], cols[kBevTile];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = (int)blockIdx.y * kBevTile, c0 = (int)blockIdx.x * kBevTile;
  if (wave == 0) cols[lane] = (c0 + lane < N) ? bev_prepare(boxes_b + (size_t)(c0 + lane) * 5) : bev_no_box();
  if (wave == 1) rows[lane] = (r0 + lane < M) ? bev_prepare(boxes_a + (size_t)(r0 + lane) * 5) : bev_no_box();
  __syncthreads();
  const BevBox B = cols[lane];
  const int nrow = min(kBevTile, M - r0);
  if (c0 + lane >= N) return;
  // one pair at a time: two rows interleaved would come out as packed fp32 arithmetic (build.py: no compiler-formed v_pk_*)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
  for (int r = wave; r < nrow; r += kBevOverlapThreads / 64)
    out[(size_t)(r0 + r) * N + c0 + lane] = bev_pair(rows[r], B, want_iou);
}

__global__ __launch_bounds__(kBevOverlapThreads) void bev_overlap_aligned_kernel(const float* __restrict__ boxes_a,
                                                                                 const float* __restrict__ boxes_b, int N,
                                                                                 int want_iou, float* __restrict__ out) {
  const long i = (long)blockIdx.x * kBevOverlapThreads + (long)threadIdx.x;
  if (i >= N) return;
  const BevBox A = bev_prepare(boxes_a + (size_t)i * 5), B = bev_prepare(boxes_b + (size_t)i * 5);
  out[i] = bev_pair(A, B, want_iou);
}

__global__ __launch_bounds__(kBevTile) void bev_nms_mask_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ order,
                                                                 const int32_t* __restrict__ group, int N, int T, float thr,
                                                                 unsigned long long* __restrict__ mask) {
  const int rt = (int)blockIdx.y, ct = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (ct < rt) return;
  __shared__ BevBox cols[kBevTile];
  __shared__ float crad[kBevTile];             // half diagonal
  __shared__ int cgrp[kBevTile];
  // the column tile, gathered through `order`: an entry outside [0, N) is a position without a box
  {
    const int pos = ct * kBevTile + lane;
    const int idx = (pos < N) ? order[pos] : -1;
    const bool in = idx >= 0 && idx < N;
    const BevBox b = in ? bev_prepare(boxes + (size_t)idx * 5) : bev_no_box();
    cols[lane] = b;
    crad[lane] = sqrtf(b.hx * b.hx + b.hy * b.hy);
    cgrp[lane] = (in && group != nullptr) ? group[idx] : 0;
  }
  __syncthreads();
  const int rpos = rt * kBevTile + lane;
  BevBox A;
  float arad;
  int agrp;
  if (rt == ct) {
    A = cols[lane]; arad = crad[lane]; agrp = cgrp[lane];
  } else {
    // (rt < ct <= T - 1: every row of this tile is a position below N)
    const int idx = order[rpos];
    const bool in = idx >= 0 && idx < N;
    A = in ? bev_prepare(boxes + (size_t)idx * 5) : bev_no_box();
    arad = sqrtf(A.hx * A.hx + A.hy * A.hy);
    agrp = (in && group != nullptr) ? group[idx] : 0;
  }
  if (rpos >= N) return;
  const bool a_ok = A.area == A.area;
  unsigned long long word = 0ull;
  if (a_ok) {
    // pass 1, cheap and the same for every lane: the columns this row could suppress -- a later position, a box, the same group --
    // split into those close enough to touch and those whose IoU is 0 without any arithmetic
    unsigned long long near = 0ull, far = 0ull;
#pragma clang loop vectorize(disable) interleave(disable)
    for (int j = 0; j < kBevTile; ++j) {
      const bool pair = ct * kBevTile + j > rpos && cols[j].area == cols[j].area && cgrp[j] == agrp;
      const float ddx = A.cx - cols[j].cx, ddy = A.cy - cols[j].cy, reach = (arad + crad[j]) * 1.00001f;
      const bool apart = ddx * ddx + ddy * ddy > reach * reach;
      near |= (pair && !apart) ? 1ull << j : 0ull;
      far |= (pair && apart) ? 1ull << j : 0ull;
    }
    if (0.f > thr) word = far;                 // (a negative threshold: IoU 0 suppresses too, as in the reference)
    // pass 2: each lane walks its OWN candidates, so the wave runs max-over-lanes overlap evaluations, not one per column
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    while (near != 0ull) {
      const int j = __builtin_ctzll(near);
      near &= near - 1ull;
      const BevBox B = cols[j];
      if (bev_iou_of(bev_overlap_area(A, B), A.area, B.area) > thr) word |= 1ull << j;
    }
  } else if (rt == ct) {
    word = 1ull << lane;                       // never kept, suppresses nothing
  }
  mask[(size_t)rpos * T + ct] = word;
}

__global__ __launch_bounds__(kBevReduceThreads) void bev_nms_reduce_kernel(const int32_t* __restrict__ order, int N, int T,
                                                                           const unsigned long long* __restrict__ mask,
                                                                           int32_t* __restrict__ keep_index,
                                                                           uint8_t* __restrict__ keep_mask,
                                                                           int32_t* __restrict__ num_keep) {
  __shared__ unsigned long long removed[kBevMaxTiles];
  __shared__ unsigned long long kept_s;
  const int tid = (int)threadIdx.x;
  for (int t = tid; t < T; t += kBevReduceThreads) removed[t] = 0ull;
  for (int i = tid; i < N; i += kBevReduceThreads) keep_mask[i] = 0;
  __syncthreads();
  int count = 0;
  for (int rt = 0; rt < T; ++rt) {
    if (tid < kBevTile) {
      const int pos = rt * kBevTile + tid;
      const unsigned long long d = (pos < N) ? mask[(size_t)pos * T + rt] : (1ull << tid);
      const int dlo = (int)(unsigned)d, dhi = (int)(unsigned)(d >> 32);
      unsigned long long rem = removed[rt], kept = 0ull;
#pragma unroll
      for (int l = 0; l < kBevTile; ++l) {
        const unsigned long long w = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(dhi, l) << 32) |
                                     (unsigned long long)(unsigned)__builtin_amdgcn_readlane(dlo, l);
        if ((((rem | w) >> l) & 1ull) == 0ull) { rem |= w; kept |= 1ull << l; }
      }
      if ((kept >> tid) & 1ull) {
        const int idx = order[pos];            // a kept row is a box: idx lies inside [0, N) (checked all the same: the mask is memory)
        keep_index[count + __builtin_popcountll(kept & ((1ull << tid) - 1ull))] = idx;
        if ((unsigned)idx < (unsigned)N) keep_mask[idx] = 1;
      }
      if (tid == 0) kept_s = kept;
    }
    __syncthreads();
    const unsigned long long kept = kept_s;
    count += __builtin_popcountll(kept);
    if (kept != 0ull) {
      const int nrow = min(kBevTile, N - rt * kBevTile);
      for (int ct = rt + 1 + tid; ct < T; ct += kBevReduceThreads) {
        const unsigned long long* col = mask + (size_t)rt * kBevTile * T + ct;
        unsigned long long acc = 0ull;
        for (int l0 = 0; l0 < nrow; l0 += 16) {          // sixteen independent loads in flight, then their ORs
          unsigned long long w[16];
#pragma unroll
          for (int k = 0; k < 16; ++k) w[k] = (l0 + k < nrow) ? col[(size_t)(l0 + k) * T] : 0ull;
#pragma unroll
          for (int k = 0; k < 16; ++k) acc |= ((kept >> (l0 + k)) & 1ull) ? w[k] : 0ull;
        }
        removed[ct] |= acc;
      }
    }
    __syncthreads();
  }
  for (int i = count + tid; i < N; i += kBevReduceThreads) keep_index[i] = -1;
  if (tid == 0) num_keep[0] = count;
}

int launch_bev_overlap(const float* boxes_a, int M, const float* boxes_b, int N, int want_iou, int aligned, float* out,
                       hipStream_t st) {
  if (M < 0 || N < 0) return fail(EPROPNP_EINVAL, "epropnp_bev_overlap: box counts must be >= 0, got %d and %d", M, N);
  if (aligned && M != N) return fail(EPROPNP_EINVAL, "epropnp_bev_overlap: aligned needs num_a == num_b, got %d and %d", M, N);
  if (M == 0 || N == 0) return EPROPNP_OK;
  if (!boxes_a || !boxes_b || !out) return fail(EPROPNP_EINVAL, "epropnp_bev_overlap: NULL pointer");
  if (aligned) {
    const dim3 grid((unsigned)((N + kBevOverlapThreads - 1) / kBevOverlapThreads)), block(kBevOverlapThreads);
    PNP_LAUNCH(bev_overlap_aligned_kernel, grid, block, 0, st, boxes_a, boxes_b, N, want_iou ? 1 : 0, out);
    return check_launch("bev_overlap_aligned_kernel");
  }
  const long rt = ((long)M + kBevTile - 1) / kBevTile, ct = ((long)N + kBevTile - 1) / kBevTile;
  if (rt > 65535) return fail(EPROPNP_EINVAL, "epropnp_bev_overlap: num_a = %d is more than %d rows of one launch", M, 65535 * kBevTile);
  const dim3 grid((unsigned)ct, (unsigned)rt), block(kBevOverlapThreads);
  PNP_LAUNCH(bev_overlap_kernel, grid, block, 0, st, boxes_a, M, boxes_b, N, want_iou ? 1 : 0, out);
  return check_launch("bev_overlap_kernel");
}

size_t bev_nms_scratch_bytes(int N) {
  if (N < 1) return 0;
  const size_t T = ((size_t)N + kBevTile - 1) / kBevTile;
  return (size_t)N * T * sizeof(unsigned long long);      // the mask; the reduce launch needs nothing more (its bitset is LDS)
}

int launch_bev_nms(const float* boxes, const int32_t* order, const int32_t* group, int N, float thr, void* scratch,
                   size_t scratch_bytes, int32_t* keep_index, uint8_t* keep_mask, int32_t* num_keep, hipStream_t st) {
  if (N < 0) return fail(EPROPNP_EINVAL, "epropnp_bev_nms: num_boxes must be >= 0, got %d", N);
  if (!num_keep) return fail(EPROPNP_EINVAL, "epropnp_bev_nms: NULL num_keep");
  if (N > kBevMaxTiles * kBevTile)
    return fail(EPROPNP_EINVAL, "epropnp_bev_nms: %d boxes are more than the %d of one call", N, kBevMaxTiles * kBevTile);
  const int T = (N + kBevTile - 1) / kBevTile;
  // EPROPNP_TUNE="bev_nms_phase=mask" | "=reduce": one of the two launches alone, the other's scratch as it is (tools/boxes_timing.py)
  const char* only = tune_value("bev_nms_phase");
  const bool do_mask = !only || only[0] != 'r', do_reduce = !only || only[0] != 'm';
  if (N > 0) {
    if (!boxes || !order || !scratch || !keep_index || !keep_mask) return fail(EPROPNP_EINVAL, "epropnp_bev_nms: NULL pointer");
    if (scratch_bytes < bev_nms_scratch_bytes(N))
      return fail(EPROPNP_EINVAL, "epropnp_bev_nms: scratch of %zu bytes is smaller than epropnp_bev_nms_scratch_bytes(%d) = %zu",
                  scratch_bytes, N, bev_nms_scratch_bytes(N));
    if (do_mask) {
      const dim3 grid((unsigned)T, (unsigned)T), block(kBevTile);
      PNP_LAUNCH(bev_nms_mask_kernel, grid, block, 0, st, boxes, order, group, N, T, thr, (unsigned long long*)scratch);
      const int rc = check_launch("bev_nms_mask_kernel");
      if (rc != EPROPNP_OK) return rc;
    }
  }
  if (!do_reduce) return EPROPNP_OK;
  PNP_LAUNCH(bev_nms_reduce_kernel, dim3(1), dim3(kBevReduceThreads), 0, st, order, N, T, (const unsigned long long*)scratch,
             keep_index, keep_mask, num_keep);
  return check_launch("bev_nms_reduce_kernel");
}

}  // namespace pnp
