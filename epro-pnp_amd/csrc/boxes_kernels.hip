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
//   box_overlap_*_kernel    : rotated, 3D and image boxes under the four criteria, pairwise / aligned / segmented, around the same
//       bev_overlap_area (epropnp_box_overlap, epropnp_box_overlap_segmented): described where they stand, below the NMS launchers.
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

// ---- box overlaps: rotated, 3D and image boxes under the four criteria (epropnp_box_overlap, epropnp_box_overlap_segmented) ------------
// What EPro-PnP-Det's two numba-CUDA files put around the rotated intersection (core/bbox_3d/iou_calculators/rotate_iou_kernel.py,
// bbox3d_iou_calculator.py; core/evaluation/kitti_utils/rotate_iou.py, eval.py: image_box_overlap, d3_box_overlap_kernel).
//   box_prepare<KIND> : a box in the form the pair routine takes.  bev: BevBox as it is.  box3d: the BevBox of the two axes that are
//       not z_axis, and the height interval lo = z - h z_center, hi = z + h (1 - z_center).  image: (x1, y1, x2, y2) kept in the
//       BevBox's cx, cy, hx, hy.  `size` is the area / volume / image area, `ok` the validity (all numbers finite, sizes >= 0).
//   box_pair<KIND>    : the ONE pair function: intersection (bev_overlap_area, times the common height for box3d; iw ih for image),
//       then the criterion; products uncontracted.  NaN exactly where either box is invalid.
//   box_tile<KIND>    : the ONE tile body of the pairwise and the segmented kernel: up to 64 x 64 pairs, both sides' boxes prepared
//       into LDS, a lane owns a column, a wave walks the rows.  The aligned kernel calls box_pair on its own pair: the same bits.
//   segmented         : one workgroup per entry of a tile table built on the host (box_overlap_plan): six int32 per tile -- first row,
//       rows (1..64), first column, columns (1..64), output index of the tile's first element, row stride of its block.  The table is
//       memory: an entry that points outside the boxes or the output is skipped, nothing is read or written out of bounds.
constexpr int kBoxTileInts = EPROPNP_BOX_TILE_INTS;

struct OvBox {
  BevBox b;
  float lo, hi, size, ok;
};

struct OvMode {
  int crit, rule, z_axis;
  float z_center;
};

template <int KIND>
constexpr int box_floats() { return KIND == EPROPNP_BOX_BEV ? 5 : KIND == EPROPNP_BOX_3D ? 7 : 4; }

PNP_FN bool box_finite(float v) { return fabsf(v) < INFINITY; }

template <int KIND>
PNP_FN OvBox box_prepare(const float* __restrict__ p, const OvMode& m) {
#pragma clang fp contract(off)
  OvBox o;
  if (KIND == EPROPNP_BOX_IMAGE) {
    const float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
    o.b = bev_no_box();
    o.b.cx = x1; o.b.cy = y1; o.b.hx = x2; o.b.hy = y2;
    o.lo = o.hi = 0.f;
    o.size = (x2 - x1) * (y2 - y1);
    o.ok = (box_finite(x1) && box_finite(y1) && box_finite(x2) && box_finite(y2) && x2 >= x1 && y2 >= y1) ? 1.f : 0.f;
  } else if (KIND == EPROPNP_BOX_BEV) {
    o.b = bev_prepare(p);
    o.lo = o.hi = 0.f;
    o.size = o.b.area;
    o.ok = (o.b.area == o.b.area) ? 1.f : 0.f;
  } else {
    // the reference's bev_axes: the seven numbers without x[z_axis] and d[z_axis] -- [0, 2, 3, 5, 6] for z_axis = 1
    const int i0 = (m.z_axis == 0) ? 1 : 0, i1 = (m.z_axis == 2) ? 1 : 2;
    const float q0 = p[i0], q1 = p[i1], q2 = p[3 + i0], q3 = p[3 + i1], q4 = p[6];
    const float z = p[m.z_axis], h = p[3 + m.z_axis];
    const float bev[5] = {q0, q1, q2, q3, q4};
    o.b = bev_prepare(bev);
    o.lo = z - h * m.z_center;
    o.hi = z + h * (1.f - m.z_center);
    o.size = o.b.area * h;                     // (dx dy) h
    o.ok = (o.b.area == o.b.area && box_finite(z) && h >= 0.f && h < INFINITY) ? 1.f : 0.f;
  }
  return o;
}

PNP_FN OvBox box_no_box() {
  OvBox o;
  o.b = bev_no_box();
  o.lo = o.hi = o.size = o.ok = 0.f;
  return o;
}

template <int KIND>
PNP_FN float box_pair(const OvBox& A, const OvBox& B, const OvMode& m) {
#pragma clang fp contract(off)
  float inter;
  if (KIND == EPROPNP_BOX_IMAGE) {
    const float iw = fminf(A.b.hx, B.b.hx) - fmaxf(A.b.cx, B.b.cx), ih = fminf(A.b.hy, B.b.hy) - fmaxf(A.b.cy, B.b.cy);
    inter = (iw > 0.f && ih > 0.f) ? iw * ih : 0.f;
  } else {
    inter = bev_overlap_area(A.b, B.b);
    if (KIND == EPROPNP_BOX_3D) {
      // `interval`: the common part of the two height intervals.  `reference_torch`: the lower of the two bottoms where the higher
      // belongs (bbox3d_iou_calculator.py:151 takes torch.min; its numpy twin at :90 np.maximum)
      const float top = fminf(A.hi, B.hi);
      const float bottom = (m.rule == EPROPNP_BOX_HEIGHT_INTERVAL) ? fmaxf(A.lo, B.lo) : fminf(A.lo, B.lo);
      inter = inter * fmaxf(top - bottom, 0.f);
    }
  }
  float v = inter;
  if (m.crit != EPROPNP_BOX_CRIT_INTER) {
    const float den = (m.crit == EPROPNP_BOX_CRIT_IOU) ? A.size + B.size - inter : (m.crit == EPROPNP_BOX_CRIT_A) ? A.size : B.size;
    v = fminf(inter / fmaxf(den, 1e-8f), 1.f);
  }
  return (A.ok != 0.f && B.ok != 0.f) ? v : NAN;
}

// nrow x ncol pairs (1..64 each) of the boxes at a, b into out[r * stride + c]
template <int KIND>
PNP_FN void box_tile(const float* __restrict__ a, int nrow, const float* __restrict__ b, int ncol, const OvMode& m,
                     float* __restrict__ out, int stride, OvBox* rows, OvBox* cols) {
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (wave == 0) cols[lane] = (lane < ncol) ? box_prepare<KIND>(b + (size_t)lane * box_floats<KIND>(), m) : box_no_box();
  if (wave == 1) rows[lane] = (lane < nrow) ? box_prepare<KIND>(a + (size_t)lane * box_floats<KIND>(), m) : box_no_box();
  __syncthreads();
  const OvBox B = cols[lane];
  if (lane >= ncol) return;
  // one pair at a time, as in bev_overlap_kernel (build.py: no compiler-formed v_pk_*)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
  for (int r = wave; r < nrow; r += kBevOverlapThreads / 64) out[(size_t)r * (size_t)stride + lane] = box_pair<KIND>(rows[r], B, m);
}

template <int KIND>
__global__ __launch_bounds__(kBevOverlapThreads) void box_overlap_kernel(const float* __restrict__ boxes_a, int M,
                                                                         const float* __restrict__ boxes_b, int N, OvMode m,
                                                                         float* __restrict__ out) {
  __shared__ OvBox rows[kBevTile], cols[kBevTile];
  const int r0 = (int)blockIdx.y * kBevTile, c0 = (int)blockIdx.x * kBevTile;
  box_tile<KIND>(boxes_a + (size_t)r0 * box_floats<KIND>(), min(kBevTile, M - r0), boxes_b + (size_t)c0 * box_floats<KIND>(),
                 min(kBevTile, N - c0), m, out + (size_t)r0 * N + c0, N, rows, cols);
}

template <int KIND>
__global__ __launch_bounds__(kBevOverlapThreads) void box_overlap_aligned_kernel(const float* __restrict__ boxes_a,
                                                                                 const float* __restrict__ boxes_b, int N, OvMode m,
                                                                                 float* __restrict__ out) {
  const long i = (long)blockIdx.x * kBevOverlapThreads + (long)threadIdx.x;
  if (i >= N) return;
  const OvBox A = box_prepare<KIND>(boxes_a + (size_t)i * box_floats<KIND>(), m);
  const OvBox B = box_prepare<KIND>(boxes_b + (size_t)i * box_floats<KIND>(), m);
  out[i] = box_pair<KIND>(A, B, m);
}

template <int KIND>
__global__ __launch_bounds__(kBevOverlapThreads) void box_overlap_segmented_kernel(const float* __restrict__ boxes_a, int M,
                                                                                   const float* __restrict__ boxes_b, int N,
                                                                                   const int32_t* __restrict__ tiles, OvMode m,
                                                                                   float* __restrict__ out, long long num_out) {
  __shared__ OvBox rows[kBevTile], cols[kBevTile];
  const int32_t* t = tiles + (size_t)blockIdx.x * kBoxTileInts;
  const int r0 = t[0], nrow = t[1], c0 = t[2], ncol = t[3], o0 = t[4], stride = t[5];
  // the same for every thread of the workgroup: a tile outside the boxes or the output is skipped as a whole
  const bool inside = nrow >= 1 && nrow <= kBevTile && ncol >= 1 && ncol <= kBevTile && r0 >= 0 && r0 <= M - nrow && c0 >= 0 &&
                      c0 <= N - ncol && stride >= ncol && o0 >= 0 &&
                      (long long)o0 + (long long)(nrow - 1) * (long long)stride + (long long)ncol <= num_out;
  if (!inside) return;
  box_tile<KIND>(boxes_a + (size_t)r0 * box_floats<KIND>(), nrow, boxes_b + (size_t)c0 * box_floats<KIND>(), ncol, m, out + o0, stride,
                 rows, cols);
}

static int box_check(const char* who, int kind, int crit, int z_axis, float z_center, int rule) {
  if (kind != EPROPNP_BOX_BEV && kind != EPROPNP_BOX_3D && kind != EPROPNP_BOX_IMAGE)
    return fail(EPROPNP_EINVAL, "%s: unknown box kind %d", who, kind);
  if (crit != EPROPNP_BOX_CRIT_IOU && crit != EPROPNP_BOX_CRIT_A && crit != EPROPNP_BOX_CRIT_B && crit != EPROPNP_BOX_CRIT_INTER)
    return fail(EPROPNP_EINVAL, "%s: unknown criterion %d", who, crit);
  if (rule != EPROPNP_BOX_HEIGHT_INTERVAL && rule != EPROPNP_BOX_HEIGHT_REFERENCE_TORCH)
    return fail(EPROPNP_EINVAL, "%s: unknown height rule %d", who, rule);
  if (kind == EPROPNP_BOX_3D && (z_axis < 0 || z_axis > 2)) return fail(EPROPNP_EINVAL, "%s: z_axis must be 0, 1 or 2, got %d", who, z_axis);
  if (!(fabsf(z_center) < INFINITY)) return fail(EPROPNP_EINVAL, "%s: z_center is not finite", who);
  return EPROPNP_OK;
}

int launch_box_overlap(const float* boxes_a, int M, const float* boxes_b, int N, int kind, int crit, int z_axis, float z_center,
                       int rule, int aligned, float* out, hipStream_t st) {
  const char* who = "epropnp_box_overlap";
  if (M < 0 || N < 0) return fail(EPROPNP_EINVAL, "%s: box counts must be >= 0, got %d and %d", who, M, N);
  if (aligned && M != N) return fail(EPROPNP_EINVAL, "%s: aligned needs num_a == num_b, got %d and %d", who, M, N);
  if (int rc = box_check(who, kind, crit, z_axis, z_center, rule)) return rc;
  if (M == 0 || N == 0) return EPROPNP_OK;
  if (!boxes_a || !boxes_b || !out) return fail(EPROPNP_EINVAL, "%s: NULL pointer", who);
  const OvMode m{crit, rule, kind == EPROPNP_BOX_3D ? z_axis : 0, z_center};
  const dim3 block(kBevOverlapThreads);
  if (aligned) {
    const dim3 grid((unsigned)((N + kBevOverlapThreads - 1) / kBevOverlapThreads));
    if (kind == EPROPNP_BOX_BEV) {
      PNP_LAUNCH(box_overlap_aligned_kernel<EPROPNP_BOX_BEV>, grid, block, 0, st, boxes_a, boxes_b, N, m, out);
    } else if (kind == EPROPNP_BOX_3D) {
      PNP_LAUNCH(box_overlap_aligned_kernel<EPROPNP_BOX_3D>, grid, block, 0, st, boxes_a, boxes_b, N, m, out);
    } else {
      PNP_LAUNCH(box_overlap_aligned_kernel<EPROPNP_BOX_IMAGE>, grid, block, 0, st, boxes_a, boxes_b, N, m, out);
    }
    return check_launch("box_overlap_aligned_kernel");
  }
  const long rt = ((long)M + kBevTile - 1) / kBevTile, ct = ((long)N + kBevTile - 1) / kBevTile;
  if (rt > 65535) return fail(EPROPNP_EINVAL, "%s: num_a = %d is more than %d rows of one launch", who, M, 65535 * kBevTile);
  const dim3 grid((unsigned)ct, (unsigned)rt);
  if (kind == EPROPNP_BOX_BEV) {
    PNP_LAUNCH(box_overlap_kernel<EPROPNP_BOX_BEV>, grid, block, 0, st, boxes_a, M, boxes_b, N, m, out);
  } else if (kind == EPROPNP_BOX_3D) {
    PNP_LAUNCH(box_overlap_kernel<EPROPNP_BOX_3D>, grid, block, 0, st, boxes_a, M, boxes_b, N, m, out);
  } else {
    PNP_LAUNCH(box_overlap_kernel<EPROPNP_BOX_IMAGE>, grid, block, 0, st, boxes_a, M, boxes_b, N, m, out);
  }
  return check_launch("box_overlap_kernel");
}

int box_overlap_plan(const int32_t* counts_a, const int32_t* counts_b, int G, int32_t* tiles, long long capacity, long long* num_tiles,
                     long long* num_out) {
  const char* who = "epropnp_box_overlap_plan";
  if (G < 0) return fail(EPROPNP_EINVAL, "%s: num_segments must be >= 0, got %d", who, G);
  if (G > 0 && (!counts_a || !counts_b)) return fail(EPROPNP_EINVAL, "%s: NULL counts", who);
  if (tiles && capacity < 0) return fail(EPROPNP_EINVAL, "%s: negative table capacity", who);
  long long row = 0, col = 0, o = 0, nt = 0;
  for (int g = 0; g < G; ++g) {
    const long long na = counts_a[g], nb = counts_b[g];
    if (na < 0 || nb < 0) return fail(EPROPNP_EINVAL, "%s: segment %d has negative counts %lld and %lld", who, g, na, nb);
    if (row + na > INT32_MAX || col + nb > INT32_MAX) return fail(EPROPNP_EINVAL, "%s: more than 2^31 - 1 boxes", who);
    if (o + na * nb > (long long)INT32_MAX)
      return fail(EPROPNP_EINVAL, "%s: the output has 2^31 or more elements (segment %d: %lld x %lld)", who, g, na, nb);
    for (long long r = 0; r < na && nb > 0; r += kBevTile)
      for (long long c = 0; c < nb; c += kBevTile, ++nt) {
        if (!tiles) continue;
        if (nt >= capacity) return fail(EPROPNP_EINVAL, "%s: the table holds %lld tiles, more are needed", who, capacity);
        int32_t* t = tiles + nt * kBoxTileInts;
        t[0] = (int32_t)(row + r);
        t[1] = (int32_t)(na - r < kBevTile ? na - r : kBevTile);
        t[2] = (int32_t)(col + c);
        t[3] = (int32_t)(nb - c < kBevTile ? nb - c : kBevTile);
        t[4] = (int32_t)(o + r * nb + c);
        t[5] = (int32_t)nb;
      }
    row += na; col += nb; o += na * nb;
  }
  if (num_tiles) *num_tiles = nt;
  if (num_out) *num_out = o;
  return EPROPNP_OK;
}

int launch_box_overlap_segmented(const float* boxes_a, int M, const float* boxes_b, int N, int kind, int crit, int z_axis,
                                 float z_center, int rule, const int32_t* tiles, int num_tiles, float* out, long long num_out,
                                 hipStream_t st) {
  const char* who = "epropnp_box_overlap_segmented";
  if (M < 0 || N < 0) return fail(EPROPNP_EINVAL, "%s: box counts must be >= 0, got %d and %d", who, M, N);
  if (num_tiles < 0) return fail(EPROPNP_EINVAL, "%s: num_tiles must be >= 0, got %d", who, num_tiles);
  if (num_out < 0 || num_out > (long long)INT32_MAX)
    return fail(EPROPNP_EINVAL, "%s: num_out = %lld is outside 0 .. 2^31 - 1", who, num_out);
  if (int rc = box_check(who, kind, crit, z_axis, z_center, rule)) return rc;
  if (num_tiles == 0 || M == 0 || N == 0 || num_out == 0) return EPROPNP_OK;
  if (!boxes_a || !boxes_b || !tiles || !out) return fail(EPROPNP_EINVAL, "%s: NULL pointer", who);
  const OvMode m{crit, rule, kind == EPROPNP_BOX_3D ? z_axis : 0, z_center};
  const dim3 grid((unsigned)num_tiles), block(kBevOverlapThreads);
  if (kind == EPROPNP_BOX_BEV) {
    PNP_LAUNCH(box_overlap_segmented_kernel<EPROPNP_BOX_BEV>, grid, block, 0, st, boxes_a, M, boxes_b, N, tiles, m, out, num_out);
  } else if (kind == EPROPNP_BOX_3D) {
    PNP_LAUNCH(box_overlap_segmented_kernel<EPROPNP_BOX_3D>, grid, block, 0, st, boxes_a, M, boxes_b, N, tiles, m, out, num_out);
  } else {
    PNP_LAUNCH(box_overlap_segmented_kernel<EPROPNP_BOX_IMAGE>, grid, block, 0, st, boxes_a, M, boxes_b, N, tiles, m, out, num_out);
  }
  return check_launch("box_overlap_segmented_kernel");
}

}  // namespace pnp
