// amis_backward_mfma.hip -- backward of the AMIS log-weights with the pose x point projection on the matrix cores.
//
// Same contract as amis_backward_kernel (amis_kernels.hip): gradient of
//     sum_j a_j * cost(pose_j; x3d, x2d, w2d, delta),   a_j = -g_logw[j]  (+ g_init * cost(pose_init))
// w.r.t. the correspondences, recomputed from the points (the reference replays autograd through evaluate_pnp,
// epropnp/common.py:67-100, camera.py:21-30,81-93, cost_fun.py:45-61).  What differs is where the arithmetic runs:
//   * forward projection  h = (K R | K t)(X,Y,Z,1)^T of 16 poses x 16 points: three MFMAs (A = pose rows from LDS, B = point
//     tile in registers) -- v_mfma_f32_16x16x4_f32 as in amis_forward_mfma.hip, or (BF16, the default for <= 4 resident
//     point tiles) ONE v_mfma_f32_16x16x32_bf16 per image row on bf16x3-split operands: fp32-level accuracy at 55 % of the
//     matrix time (wave_ops.h: ProjOp; the points are split once per chunk, the pose rows once per compacted pose while the
//     table is built -- PRESPLIT below -- or, where the larger table would cost a workgroup per CU, on the fly: 21 instructions
//     per wave, pose tile and chunk);
//   * back-projection  g_x3d[n] += sum_j (K R)_j^T g_h[j,n] stays on the VALU (9 FMAs per pair).  It IS expressible as
//     the same MFMA with the roles swapped (A = the per-pair g_h values, which the forward MFMA leaves in exactly the
//     lane layout an A operand needs; B = pose rows indexed by output coordinate), and that variant was built and
//     measured: 12 more MFMAs per 16x16 tile for 3 useful output columns of 16, each waiting on VALU results and on
//     the previous accumulate -- 1.6-1.9 ms instead of 1.08 ms at C2 (profiles/r01_bwd_mfma_sweep.txt).  Dropped.  Round 6 built it
//     again on v_mfma_f32_4x4x1_16b_f32 (2 passes; a block of four lanes = four points, no wasted columns to speak of): 31 % fewer
//     packed instructions, 32 VGPRs less, 924-948 us against 780-793 -- vector arithmetic does not run underneath an MFMA on this
//     part, of its own wave or of a neighbour (profiles/r06_mfma_valu_overlap.txt, tools/ubench/mfma_4x4x1_layout.hip).  Dropped.
//   * the VALU keeps what is genuinely per pair: perspective divide, weighted residual, Huber weight, and the
//     accumulation of the gradients -- since round 6 on explicit 2-vectors: two point-poses per v_pk_*_f32 (22.6 wave-level
//     instructions per pair with four resident tiles, 2 of them transcendental; the loop is bound by how often a wave gets to issue, profiles/r06_bwd_packed.txt).
//     With the forward's sample costs at hand (DCOST below) the threshold's gradient needs no per-pair term: two clamped multiplies and
//     a packed fma per two pairs less (profiles/bwd_dcost_bench.txt).
// The weighted poses are built ONCE into an LDS table (compacted: the low-weight tail whose total |weight| is below
// drop_eps -- default 2^-24 -- of the object's total is dropped before tiling, mass_drop_threshold in amis_common.h;
// EPROPNP_BWD_DROP=0 keeps every non-zero sample), then every wave sweeps all pose tiles for its own points.
#include "amis_common.h"
#include "dispatch.h"
#include "tuning.h"

namespace pnp {

// Register budget (the packed pair loop of round 6 with pair accumulators, compiled WITHOUT the SLP vectoriser -- build.py): <= 2
// resident point tiles fit three waves per SIMD (bf16 projection: 152 VGPRs), four resident tiles are compiled for two (248 / 256
// VGPRs with the projection clamp, software pipeline over the tiles included) -- and are the faster shape at C2 all the same (launcher comment).
// Why no vectoriser: the packed fp32 instructions it forms include shapes that return wrong results on the MI355X while a bf16 MFMA of a
// neighbouring wave executes (profiles/r05_pk_opsel_erratum.txt) -- the run-to-run different gradients of round 5.  The packed
// arithmetic of this kernel is written by hand, on explicit 2-vectors, in shapes that the erratum does not touch (see the pair loop).
// Rules that stay: no scratch access inside a loop of this kernel (tools/scratch_audit.py --check), no packed instruction of the
// known-bad shape in ANY function of the library (tools/pk_opsel_fix.py --audit, run by the build), and every instantiation passes the
// repeated-launch test at full occupancy (tests/test_determinism_gpu.py) -- a defect of this kind is invisible to a tolerance.
template <int DOF, bool BOUNDS, int NPT, bool BF16>
constexpr int bwd_min_waves() { return (NPT <= 2) ? PNP_BWD_MINW : PNP_BWD_MINW4; }

// DCOST: d/d delta from the forward's sample costs instead of a per-pair term.  In the kernel's units (residuals / delta, s = |r|^2,
// c1 = min(1, 1 / rho)) the Huber value of a sample is  cost / delta^2 = sum_n m (rho - m / 2), m = min(rho, 1)
//                                                                     = sum_n c1 s - 1/2 sum_n min(s, 1)
// (inlier: s / 2 = s - s / 2; outlier: rho - 1/2 = rho - 1/2), hence  sum_j a_j sum_n min(s, 1) = 2 (sum_pairs coef s - sum_j a_j cost_j / delta^2)
// and the object's  sum_pairs coef s - sum_pairs a min(s, 1)  becomes  2 C_b - sum_pairs coef s,  C_b = sum_j a_j cost_j / delta^2:
// S multiply-adds per object while the pose table is built, where the pair loop spent two clamped multiplies and a packed fma per two
// pairs (`gsat2`).  cost_j is what the AMIS forward held when it wrote logweights (AmisParams.sample_costs), the cost of pose_init is
// the forward's cost_init.  grad_delta is then a difference of two sums computed by two kernels -- equal to the per-pair form within
// rounding, not bit for bit; the per-point gradients do not change.  Callers without costs launch the DCOST = false instantiations.
// PRESPLIT (BF16 only): the bf16-split A operands of the projection come out of the pose table.  The table build, one thread per
// compacted pose, also stores the split words of the pose's 12 components of (K R | K t) -- wave_ops.h: bf16_split_a_words -- and the
// sweep reads them back (one 16-byte and one 2-byte LDS read per lane and pose tile, three v_perm) where every wave split three fp32
// entries per pose tile and chunk (21 instructions).  The same dwords reach the matrix instruction: every output keeps its bits.
// Layout: qtab[pose][k] = {w0 of the x, y, z row | a3 of the x and y rows as two halves}, ztab[pose][k] = a3 of the z row (16 bits):
// 18 dwords per pose next to the 15 of the fp32 table, whose K R rows the back-projection still reads (its K t slots are then dead).
// Storing (a3, a3) as a word would take 24: 89.8 KB per workgroup at C2, where two workgroups per CU leave 80.
// ZFREE: a second body of the sweep without the depth clamp, taken for an object whose every table pose keeps every point in front of
// z_min -- five of the 38 wave-level instructions per two pairs (two v_max_i32 in front of the reciprocals, then two clamped fmas and a
// packed multiply for the 0/1 front factor) that return their input and multiply by 1 there.  The choice is per OBJECT and costs no
// pass, barrier or branch of its own inside a loop: Rmax = max |x3d| (two points per thread at N = 512) rides through the block
// reduction of amax; the table build, which holds (K R | K t) of its pose anyway, evaluates depth_clamp_clear (pnp_math.h: the bound,
// its slack and why the bits are the same) and a thread whose pose fails clears an LDS word (red[kClearWord]) that the barrier behind
// the build publishes; one scalar branch in front of the chunk loop picks the body.  Outputs are the clamped body's bits for every
// input, NaN and inf included (those fail the bound).  Launched only where plan_amis_backward says it can pay; EPROPNP_TUNE=zfree=0 | 1.
constexpr int kClearWord = 72;      // of red[80]: behind the compaction's 65 lane counts, beyond what the block reductions use
template <int DOF, bool BOUNDS, int NPT, bool BF16 = false, bool DCOST = false, bool PRESPLIT = false, bool ZFREE = false>
__global__ __launch_bounds__(512, (bwd_min_waves<DOF, BOUNDS, NPT, BF16>())) void amis_backward_mfma_kernel(Problem p, const float* __restrict__ pose_samples,
                                                                     const float* __restrict__ g_logw, int S,
                                                                     const float* __restrict__ pose_init,
                                                                     const float* __restrict__ g_init, int P16,
                                                                     float* __restrict__ gx3d, float* __restrict__ gx2d,
                                                                     float* __restrict__ gw2d, float* __restrict__ gdelta,
                                                                     int nsplit, float drop_eps, int gw_rows,
                                                                     const float* __restrict__ sample_costs,
                                                                     const float* __restrict__ cost_init) {
  constexpr int PL = PoseLen<DOF>::value;
  typedef ProjOp<BF16> Proj;      // the projection MFMA: fp32 16x16x4, or the bf16x3 split on 16x16x32 (wave_ops.h)
  static_assert(!PRESPLIT || BF16, "the pre-split pose rows are operands of the bf16 projection");
  // nsplit > 1 (few objects): an object's point chunks are dealt to nsplit workgroups (v = b * nsplit + part), each with
  // its own copy of the pose table; per-point gradients are disjoint, grad_delta comes out as nsplit partials per object
  const int v = object_of_block(p.B * nsplit);
  if (v >= p.B * nsplit) return;
  const int b = v / nsplit, part = v - b * nsplit;
  const int T = (int)blockDim.x, tid = (int)threadIdx.x, lane = lane_id(), wv = wave_id(), W = T >> 6;

  PNP_PHASES_BEGIN(6);      // (tuning builds: cycles in [weights | drop threshold | compaction | pose rows | sweep + outputs | tail])
  PNP_DYN_SMEM(float, smem);
  float* ptab = smem;                                   // [P16 / 4][12][4]  (K R | K t) of the compacted poses, four poses per component (below)
  u32x4* qtab = reinterpret_cast<u32x4*>(ptab + 12 * P16);                                 // [P16][4]  (PRESPLIT) split words, above
  unsigned short* ztab = reinterpret_cast<unsigned short*>(qtab + (PRESPLIT ? 4 * P16 : 0));  // [P16][4]  (PRESPLIT)
  float* wtab = reinterpret_cast<float*>(ztab + (PRESPLIT ? 4 * P16 : 0));                   // [P16]      weights of the compacted poses
  float* wraw = wtab + P16;                             // [P16]      weights by sample index (0 = dropped)
  int* idx = reinterpret_cast<int*>(wraw + P16);        // [P16]      sample index of compacted pose c
  float* red = reinterpret_cast<float*>(idx + P16);     // [80]       reductions, lane counts, active count
  float* hist = red + 80;                               // [kDropHistFloats] weight histogram of the drop threshold
  // [gw_rows][2] this object's grad_w2d, parked until the threshold's gradient (one number per object, known only after the
  // last chunk) can be added on the way out: the fold below then costs no second pass over grad_w2d in global memory
  float* gwl = hist + kDropHistFloats;
  const bool fold = (p.delta_stats != nullptr) && (nsplit == 1);
  const bool park = fold && (gw_rows >= p.N);

  float Kc[9], delta;
  Bounds bd;
  load_camera<BOUNDS>(p, b, Kc, bd, delta);
  // Residuals in units of delta (weights pre-multiplied by 1 / delta, huber_scale): min(rho, delta) becomes the clamp
  // modifier of a full-rate multiply (sat_mul); the Huber weight `coef` is unchanged, the accumulators come out scaled
  // by 1 / delta (A1, d/d delta) or 1 / delta^2 (A2, the back-projection) and are rescaled once per point at the end.
  const HuberScale hs = huber_scale(delta);
  const float zmin_v = to_vgpr(p.z_min), one_v = to_vgpr(1.0f);
  // "in front of the depth clamp" as a 0/1 factor from ONE full-rate instruction: clamp((h_z - z_lo) * 2^60, 0, 1) with z_lo
  // the float just below z_min is 1 exactly when h_z >= z_min (compare + two selects issue at half rate, tools/ubench)
  const float front_scale = to_vgpr(0x1p60f);
  const float front_off = to_vgpr(-nextafterf(p.z_min, -1.0f) * 0x1p60f);
  const float tiny_v = to_vgpr(1e-30f);     // keeps rsq finite at a zero residual; folded into the norm's first fma

  const bool with_init = (pose_init != nullptr) && (g_init != nullptr);
  const int P = S + (with_init ? 1 : 0);      // pose index S = pose_init
  // g_init[b] is wave-uniform, i.e. a SCALAR load: inside the per-lane (m >= S) arm below the compiler does not branch
  // around it when no lane takes the arm (scalar loads ignore EXEC), and a NULL g_init faulted.  Fetch it under a
  // uniform branch instead.
  const float g_init_b = with_init ? g_init[b] : 0.f;

  // DCOST: the cost of pose_init in the kernel's units.  cost_init was evaluated at the caller's threshold; one that huber_scale
  // carries as 1e-12 (delta = 0: cost_init is exactly 0 there) does not give the kernel's Huber value, so in that case -- degenerate
  // objects -- the workgroup evaluates it here, one pass over the object's points.
  float cinit_u = 0.f;
  if (DCOST && with_init) {
    if (hs.inv_delta < 1e12f) {
      cinit_u = (cost_init[b] * hs.inv_delta) * hs.inv_delta;
    } else {
      float ps[PL], R[9], KR[9], Kt[3];
#pragma unroll
      for (int i = 0; i < PL; ++i) ps[i] = pose_init[(size_t)b * PL + i];
      pose_to_rot<DOF>(ps, R);
      compose_kr_kt(Kc, R, ps, KR, Kt);
      float c[1] = {0.f};
      for (int n = tid; n < p.N; n += T) {
        SweepPoint q = to_sweep_point(load_point(p, b, n));
        q.wu *= hs.inv_delta; q.wv *= hs.inv_delta; q.cu *= hs.inv_delta; q.cv *= hs.inv_delta;
        c[0] += sweep_cost<BOUNDS>(q, KR, Kt, p.z_min, 1.0f, bd);
      }
      block_sum<1>(c, red);
      cinit_u = c[0];
    }
  }

  // ---- weights, drop threshold (mass_drop_threshold, amis_common.h), compaction ----
  float amax = 0.f;
  for (int m = tid; m < P; m += T) {
    const float w = (m < S) ? -g_logw[(size_t)m * p.B + b] : g_init_b;        // logw = -cost - const
    wraw[m] = w;
    if (m < S) amax = fmaxf(amax, fabsf(w));
  }
  float Rmax = 0.f;
  if constexpr (ZFREE) {      // the object's largest |x3d|, for the table build's bound: one more value through the reduction of amax
    float r2 = 0.f;
    for (int n = tid; n < p.N; n += T) {
      const float* x = p.x3d + ((size_t)b * p.N + n) * 3;
      r2 = fmaxf(r2, depth_r2(x[0], x[1], x[2]));
    }
    block_max2(amax, r2, red);
    Rmax = depth_rmax_up(r2);
  } else {
    amax = block_max(amax, red);          // (barriers inside: wraw is visible to every wave afterwards)
  }
  __syncthreads();
  PNP_PHASE(0);
  const float askip = mass_drop_threshold([&](int m) { return fabsf(wraw[m]); }, S, amax, drop_eps, hist);
  for (int m = tid; m < S; m += T)
    if (fabsf(wraw[m]) <= askip) wraw[m] = 0.f;
  __syncthreads();
  PNP_PHASE(1);
  if (wv == 0) {     // ordered compaction by one wave: lane l owns the contiguous samples [l*seg, (l+1)*seg)
    const int seg = (P + 63) >> 6;
    const int m0 = lane * seg, m1 = min(P, m0 + seg);
    int cnt = 0;
    for (int m = m0; m < m1; ++m) cnt += (wraw[m] != 0.f) ? 1 : 0;
    int* lcnt = reinterpret_cast<int*>(red);
    lcnt[lane] = cnt;
    wave_lds_fence();
    int off = 0, total = 0;
    for (int l = 0; l < 64; ++l) {
      const int c = lcnt[l];
      off += (l < lane) ? c : 0;
      total += c;
    }
    for (int m = m0; m < m1; ++m)
      if (wraw[m] != 0.f) idx[off++] = m;
    if (lane == 0) lcnt[64] = total;
    if (ZFREE && lane == 0) lcnt[kClearWord] = 1;      // "every pose of the table clears z_min" until a build thread says otherwise
  }
  __syncthreads();
  PNP_PHASE(2);
  const int nact = reinterpret_cast<const int*>(red)[64];
  const int ntile = (nact + 15) >> 4;
  // Pose table layout: [group of 4 poses][component row * 4 + k][pose in group] -- component (row, k) of (K R | K t), k = 3 the
  // translation column.  The sweep's lanes each own one group (poses g4 .. g4 + 3 of a tile): a float4 read is one component of the
  // lane's four poses, i.e. two aligned register PAIRS (poses 0, 1 | 2, 3) -- the operands of the packed pair loop below.
  // DCOST: C_b = sum over the KEPT samples of weight x cost / delta^2 rides along -- dropped and zero-weight samples are not in idx, so
  // their costs (possibly inf) are never read and no 0 * inf appears
  float csum[1] = {0.f};
  for (int c = tid; c < ntile * 16; c += T) {
    float* dst = ptab + (c >> 2) * 48 + (c & 3);
    float comp[12];      // (K R | K t), component 4 * row + k
    if (c < nact) {
      const int m = idx[c];
      if (DCOST) {
        const float cu = (m < S) ? (sample_costs[(size_t)m * p.B + b] * hs.inv_delta) * hs.inv_delta : cinit_u;
        csum[0] = fmaf(wraw[m], cu, csum[0]);
      }
      const float* src = (m < S) ? pose_samples + ((size_t)m * p.B + b) * PL : pose_init + (size_t)b * PL;
      float ps[PL], R[9], KR[9], Kt[3];
#pragma unroll
      for (int i = 0; i < PL; ++i) ps[i] = src[i];
      pose_to_rot<DOF>(ps, R);
      compose_kr_kt(Kc, R, ps, KR, Kt);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        comp[4 * r] = KR[3 * r]; comp[4 * r + 1] = KR[3 * r + 1]; comp[4 * r + 2] = KR[3 * r + 2];
        comp[4 * r + 3] = Kt[r];
      }
      wtab[c] = wraw[m];
      // ZFREE: a pose that may put a point behind z_min clears the word.  Every such thread stores the same 0 -- a benign race --
      // and the barrier behind the build publishes it.
      if constexpr (ZFREE) {
        if (!depth_clamp_clear(KR[6], KR[7], KR[8], Kt[2], Rmax, p.z_min)) reinterpret_cast<int*>(red)[kClearWord] = 0;
      }
    } else {     // padding of the last tile: a harmless pose (depth 1; ZFREE: a depth that passes the bound for any z_min) with zero weight
      const float pad_z = ZFREE ? fmaxf(1.f, 2.f * p.z_min) : 1.f;
#pragma unroll
      for (int k = 0; k < 12; ++k) comp[k] = (k == 11) ? pad_z : 0.f;
      wtab[c] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) dst[k * 4] = comp[k];
    if constexpr (PRESPLIT) {
      unsigned zh[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        unsigned w0x, w0y, w0z, w3x, w3y, w3z;
        bf16_split_a_words(comp[k], w0x, w3x);
        bf16_split_a_words(comp[4 + k], w0y, w3y);
        bf16_split_a_words(comp[8 + k], w0z, w3z);
        qtab[c * 4 + k] = u32x4{w0x, w0y, w0z, bf16_a3_half(w3x) | (bf16_a3_half(w3y) << 16)};
        zh[k] = bf16_a3_half(w3z);
      }
      *reinterpret_cast<u32x2*>(ztab + c * 4) = u32x2{zh[0] | (zh[1] << 16), zh[2] | (zh[3] << 16)};
    }
  }
  __syncthreads();
  // workgroup-uniform, read before the block sum below reuses `red`
  const bool clear = ZFREE && __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(red)[kClearWord]) != 0;
  float Cb = 0.f;
  if (DCOST) {      // one block sum in a fixed order (wave_ops.h); the total is wave-uniform: kept in a scalar register across the sweep
    block_sum<1>(csum, red);
    Cb = bits_f32((unsigned)__builtin_amdgcn_readfirstlane((int)f32_bits(csum[0])));
  }
  PNP_PHASE(3);

  const int col = lane & 15, kk = lane >> 4, g4 = kk * 4;
  float gd = 0.f;
  const int chunk_pts = W * NPT * 16;
  // The sweep over the chunks, once with the depth clamp and -- ZFREE -- once without: `clear` chooses per object, outside every loop.
  // CLAMP = false drops clamp_below in front of the reciprocal (which then reads the matrix instruction's result directly) and the
  // 0/1 front factor of ghz2: where depth_clamp_clear (pnp_math.h) holds for every pose of the table both are the identity, bit for bit.
  // It is ONE text, amis_backward_sweep.inc, included once per body with CLAMP set -- not a function or a lambda: with the chunk loop
  // in a lambda (by reference or by value, inlined by force or not) the instantiations without a second body no longer compiled to
  // the code they had (two VGPRs more at four tiles, another schedule).  As it is, their device code is unchanged.
  if constexpr (ZFREE) {
    if (clear) {
      constexpr bool CLAMP = false;
#include "amis_backward_sweep.inc"
    } else {
      constexpr bool CLAMP = true;
#include "amis_backward_sweep.inc"
    }
  } else {
    constexpr bool CLAMP = true;
#include "amis_backward_sweep.inc"
  }
  PNP_PHASE(4);
  if (DCOST && part == 0 && tid == 0) gd += 2.0f * Cb;      // (split launch: the partials of the other parts stay partials)
  float one[1] = {gd * hs.delta};
  block_sum<1>(one, red);
  if (tid == 0) gdelta[v] = one[0];
  // delta = mean(w2d) * std * rel came from THIS w2d (Problem.delta_stats): its gradient reaches w2d as one number per
  // object, added here to what this workgroup has just written instead of by three launches of the caller's autograd.
  // (With the object split over workgroups the sum of the parts is not known here: delta_path_kernel, amis_kernels.hip.)
  if (fold) {
    const float add = (one[0] * p.delta_stats[(size_t)b * 4 + 1]) * (p.delta_relative / (2.0f * (float)p.N));
    __syncthreads();        // this workgroup's gw2d values (LDS or global) are visible to all of its threads behind the barrier
    float* row = gw2d + (size_t)b * p.N * 2;
    if (park) {
      for (int i = tid; i < 2 * p.N; i += T) row[i] = gwl[i] + add;       // the only pass over grad_w2d, coalesced
    } else {                // (no LDS left for the rows: read back what was just written)
      for (int i = tid; i < 2 * p.N; i += T) row[i] += add;
    }
  }
  PNP_PHASE(5);
  PNP_PHASES_FLUSH(6);
}

// per-phase cycle totals of this file's kernel (tuning builds; -1 otherwise)
int tuning_bwd_phase_cycles(unsigned long long* out, int reset) { return tuning::read_cycles(out, reset, false); }

template <class F>
static int dispatch_bwd_npt(int npt, F&& f) {
  switch (npt) {
    case 1: return f(ic<1>{});
    case 2: return f(ic<2>{});
    default: return f(ic<4>{});
  }
}

struct BwdPlan {
  int waves, npt, P16, gw_rows;
  size_t smem;
  bool bf16, presplit, zfree;
};

// Which instantiation launch_amis_backward_mfma launches, and with what shape: a pure host function of the sizes, the tuning
// variables and the CU count (launches nothing, reads no device memory), shared by the launcher below and by
// epropnp_plan_amis_backward (c_api.hip) so that the two cannot drift.  Returns 1 when the shape is not supported (the
// pose table does not fit LDS: the caller falls back to amis_backward_kernel).
static int plan_amis_backward(const epropnp_problem* prob, int mc_samples, bool with_init, int nsplit, BwdPlan* out) {
  const int B = prob->num_obj, N = prob->num_pts;
  const int P = mc_samples + (with_init ? 1 : 0);
  const int P16 = ((P + 15) / 16) * 16 + 16;
  size_t smem = sizeof(float) * (15 * (size_t)P16 + 80 + kDropHistFloats);
  if (smem > 160 * 1024) return 1;
  // grad_w2d rows parked in LDS while the threshold's gradient is folded in (kernel comment): when the fold applies and the
  // rows fit next to three workgroups' pose tables per CU
  int gw_rows = 0;
  if (prob->delta_stats != nullptr && nsplit == 1 && 3 * (smem + sizeof(float) * 2 * (size_t)N) <= 160 * 1024) {
    gw_rows = N;
    smem += sizeof(float) * 2 * (size_t)N;
  }
  // 4 waves x NPT <= 4 point tiles of 16 per chunk; larger N loops over chunks of 256 points against the LDS-resident pose table.
  // Measured at C2 in round 1: 4x4 (2 chunks) 1.07 ms, 4x8 1.11, 8x4 1.22.
  // Few objects (fewer than two waves per SIMD otherwise): 8 waves, one chunk of 512 points (B = 32 / 256: -7..9 %).
  const int ptiles = (N + 15) / 16;
  int waves = (B < 512 && ptiles > 16) ? 8 : 4, npt = 1;
  while (npt < 4 && waves * npt < ptiles) npt *= 2;
  // Round 6, packed pair loop with pair accumulators (same-box A/Bs, profiles/r06_bwd_packed.txt): without a projection clamp 4 x 4
  // wins -- 784 ... 819 us at 206-248 VGPRs (two waves per SIMD) against 808 ... 838 us for 4 x 2 at 152 VGPRs (three): with two point-poses
  // per instruction the fewer instructions per pair of the four-tile loop (22.6 against 24.0) weigh more than the third wave.  With the
  // clamp the four-tile loop needs 218 VGPRs and two tiles win where the grid fills the chip: 913 against 945 us.  (The scalar loop of
  // round 5 preferred two tiles either way: 905 at 4 x 4, 868 at 4 x 2 with four waves.)  EPROPNP_TUNE=bwd_mfma=<waves>,<tiles> overrides.
  if (has_bounds(prob) && waves == 4 && npt == 4 && B >= 2 * device_cu_count() && 3 * smem <= 160 * 1024) npt = 2;
  if (nsplit > 1) {      // 4 waves x the fewest tiles that still cover N with nsplit chunks in flight
    waves = 4; npt = 1;
    while (npt < 4 && waves * npt * nsplit < ptiles) npt *= 2;
  }
  { int ov[2]; if (tune_ints("bwd_mfma", ov, 2) && ov[0] >= 1 && ov[0] <= 8 && (ov[1] == 1 || ov[1] == 2 || ov[1] == 4)) { waves = ov[0]; npt = ov[1]; } }
  // Projection on the bf16 matrix path (kernel comment) wherever the split operands fit the register budget of three waves per
  // SIMD (<= 4 resident point tiles: 4 VGPRs per tile instead of 1).  C2 backward 0.954 -> 0.899 ms, bounded 1.111 -> 1.037 ms,
  // Det shape neutral (profiles/r04_bwd_bf16_projection.txt).  EPROPNP_BWD_PROJ=f32 | bf16 forces either.
  // (With a projection clamp and four resident tiles the bf16 instantiation is a two-waves-per-SIMD kernel, see above.  It is taken
  // whatever the grid: which projection arithmetic an object gets must not depend on how many objects share the launch or on how
  // its points are split over workgroups -- the per-point gradients of the split and the unsplit launch are the same bits.)
  bool bf16 = true;
  if (const char* e = getenv("EPROPNP_BWD_PROJ")) bf16 = (e[0] == 'f') ? false : (e[0] == 'b' ? true : bf16);
  // Pose rows split to bf16 once, by the table build (kernel comment: PRESPLIT): 18 dwords per pose more.  Taken only where the larger
  // table does not lower the workgroups per CU of the shape -- two for four resident tiles, three for one and two (the register budgets
  // above) -- with the parked grad_w2d rows kept where they are parked today: C2 (S = 512, four tiles) 76.8 KB per workgroup, the Det
  // shape (S = 128, two tiles) fits three; two tiles at S = 512 keep the split on the fly.  EPROPNP_TUNE=bwd_presplit=0 forces that path.
  bool presplit = false;
  if (bf16) {
    const size_t pre = smem + sizeof(float) * 18 * (size_t)P16;
    presplit = (size_t)(npt == 4 ? 2 : 3) * pre <= 160 * 1024;
    { int ov[1]; if (tune_ints("bwd_presplit", ov, 1) && ov[0] == 0) presplit = false; }
    if (presplit) smem = pre;
  }
  // The sweep with a second, clamp-free body (kernel comment: ZFREE) exists for the pre-split instantiations of the unsplit launch.
  // It is taken where it was measured to pay (profiles/zfree_bench.txt): 6-DoF without a projection clamp, four resident tiles, and a
  // grid that fills the device at the two workgroups per CU of that shape -- with fewer objects the per-object set-up (the pass for
  // Rmax) is not hidden behind other workgroups' sweeps.  EPROPNP_TUNE=zfree=0 never takes it (the A/B switch, the tests' reference),
  // zfree=1 takes it wherever it exists, whatever the grid: the outputs are the same bits either way.
  bool zfree = presplit && nsplit == 1 && prob->dof == 6 && !has_bounds(prob) && npt == 4 && B >= 2 * device_cu_count();
  { int ov[1]; if (tune_ints("zfree", ov, 1)) zfree = presplit && nsplit == 1 && ov[0] != 0; }
  out->zfree = zfree;
  out->waves = waves; out->npt = npt; out->P16 = P16; out->gw_rows = gw_rows; out->smem = smem; out->bf16 = bf16; out->presplit = presplit;
  return 0;
}

// epropnp_plan_amis_backward: {waves, tiles, bf16, rows parked in LDS, VALU fallback}; with the fallback the first four are zero
int plan_amis_backward_record(const epropnp_problem* prob, int mc_samples, int with_init, int nsplit, int32_t* out) {
  BwdPlan plan;
  // (the split entry point never falls back: without an LDS pose table it fails, amis_kernels.hip)
  const bool valu = (backward_valu_forced() && nsplit == 1) || plan_amis_backward(prob, mc_samples, with_init != 0, nsplit, &plan) != 0;
  out[0] = valu ? 0 : plan.waves; out[1] = valu ? 0 : plan.npt; out[2] = valu ? 0 : plan.bf16; out[3] = valu ? 0 : plan.gw_rows > 0;
  out[4] = valu;
  return EPROPNP_OK;
}

// returns 1 when the shape is not supported (caller falls back to amis_backward_kernel)
int launch_amis_backward_mfma(const epropnp_problem* prob, const float* pose_samples, const float* grad_logweights,
                              int mc_samples, const float* pose_init, const float* grad_cost_init, float* grad_x3d,
                              float* grad_x2d, float* grad_w2d, float* grad_delta, int nsplit, hipStream_t st,
                              const float* sample_costs, const float* cost_init) {
  const Problem d = to_device_problem(prob);
  BwdPlan plan;
  const bool with_init = pose_init && grad_cost_init;
  if (plan_amis_backward(prob, mc_samples, with_init, nsplit, &plan)) return 1;
  // d/d delta from the forward's costs (kernel comment: DCOST) when the caller hands them over -- the costs of the samples and, with a
  // pose_init term, cost_init; otherwise the per-pair instantiation, to the bits of the entries without costs.  The launch shape is
  // the plan's either way.  EPROPNP_TUNE=bwd_dcost=0 keeps the per-pair path (A/B).
  bool dcost = sample_costs != nullptr && mc_samples > 0 && (!with_init || cost_init != nullptr);
  { int ov[1]; if (tune_ints("bwd_dcost", ov, 1) && ov[0] == 0) dcost = false; }
  const int waves = plan.waves, npt = plan.npt, P16 = plan.P16, gw_rows = plan.gw_rows;
  const size_t smem = plan.smem;
  const bool bf16 = plan.bf16;
  const dim3 grid(padded_object_grid(d.B * nsplit)), block(64 * waves);
  dispatch_dof_bounds(prob->dof, has_bounds(prob), [&](auto DOF, auto BND) -> int {
    auto launch = [&](auto kern) -> int {
      allow_dynamic_lds((const void*)kern, smem);
      PNP_LAUNCH(kern, grid, block, smem, st, d, pose_samples, grad_logweights, mc_samples, pose_init, grad_cost_init, P16,
                 grad_x3d, grad_x2d, grad_w2d, grad_delta, nsplit, backward_drop_eps(), gw_rows, sample_costs, cost_init);
      return 0;
    };
    return dispatch_bwd_npt(npt, [&](auto NPT) -> int {
      constexpr int kDof = decltype(DOF)::value, kNpt = decltype(NPT)::value;
      constexpr bool kBnd = decltype(BND)::value;
      if (plan.zfree)
        return dcost ? launch(amis_backward_mfma_kernel<kDof, kBnd, kNpt, true, true, true, true>)
                     : launch(amis_backward_mfma_kernel<kDof, kBnd, kNpt, true, false, true, true>);
      if (plan.presplit)
        return dcost ? launch(amis_backward_mfma_kernel<kDof, kBnd, kNpt, true, true, true>)
                     : launch(amis_backward_mfma_kernel<kDof, kBnd, kNpt, true, false, true>);
      if (dcost)
        return bf16 ? launch(amis_backward_mfma_kernel<kDof, kBnd, kNpt, true, true>)
                    : launch(amis_backward_mfma_kernel<kDof, kBnd, kNpt, false, true>);
      return bf16 ? launch(amis_backward_mfma_kernel<kDof, kBnd, kNpt, true>) : launch(amis_backward_mfma_kernel<kDof, kBnd, kNpt, false>);
    });
  });
  return check_launch("amis_backward_mfma_kernel");
}

}  // namespace pnp
