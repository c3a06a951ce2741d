// amis_backward_sweep.inc -- the chunk loop of amis_backward_mfma_kernel (amis_backward_mfma.hip): every wave sweeps all pose tiles
// of the LDS table for its own points, chunk by chunk, and writes the chunk's gradients.  Included inside the kernel body, once per
// body of the sweep, with `constexpr bool CLAMP` in scope: true keeps the camera's depth clamp, false (ZFREE, for an object whose
// every pose clears z_min) drops it.  Everything else it names is the kernel's.
  for (int c0 = part * chunk_pts; c0 < p.N; c0 += nsplit * chunk_pts) {
    // this wave's point tiles q = wv + W * i of the chunk; lane = (point column, k)
    typename Proj::T rB[NPT];
    float4 rW[NPT];
    // per resident tile: the four sums behind d/du, d/dw and the back-projected gradient, as PAIRS over the lane's poses (0, 2 | 1, 3):
    // folded once per chunk (below).  14 VGPRs per tile instead of 7 -- the two-tile instantiation has them to spare below the
    // three-waves-per-SIMD budget of 168, and they save 3.5 wave-level instructions per pair (8 scalar fmacs -> 4 packed fmas per two
    // pairs, no folding adds per pose tile).
    f32x2 A1x[NPT], A1y[NPT], A2x[NPT], A2y[NPT];
    f32x2 gXv[NPT], gYv[NPT], gZv[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      const Point q = load_point(p, b, c0 + (wv + W * i) * 16 + col);      // zero weight beyond N
      rB[i] = Proj::b((kk == 0) ? q.X : (kk == 1) ? q.Y : (kk == 2) ? q.Z : 1.0f);
      const float wu = q.wu * hs.inv_delta, wv = q.wv * hs.inv_delta;
      rW[i] = make_float4(wu, -q.u * wu, wv, -q.v * wv);      // (w_u, c_u | w_v, c_v): the factors in the low halves of their pairs
      A1x[i] = A1y[i] = A2x[i] = A2y[i] = f32x2{0.f, 0.f};
      gXv[i] = gYv[i] = gZv[i] = f32x2{0.f, 0.f};
    }
    f32x2 gsat2 = {0.f, 0.f};   // sum_pairs a_j min(|r|^2, 1): the second term of d/d delta (below), poses (0, 2) | (1, 3) of the lanes
    const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x2 tiny2 = {tiny_v, tiny_v};
    // The pair loop on 2-VECTORS: a lane's four poses of a tile are two register pairs (MFMA result elements 0, 1 | 2, 3; the pose
    // table above delivers every per-pose operand as such pairs), and every multiply / fma below is ONE v_pk_*_f32 for two pairs.  Packed
    // fp32 issues at half the rate of the scalar form, so the arithmetic throughput is the same -- but this loop is not bound by that:
    // it is bound by how often a wave gets to issue (profiles/r06_bwd_probe.txt: 10 % fewer instructions changed nothing, a fourth wave
    // per SIMD gave 6 %), and the packed form needs ~40 % fewer issues per pair.  Shapes: plain operands, broadcasts from the LOW half of
    // a pair (op_sel_hi) and negations only -- never the (lo, hi) source selection of profiles/r05_pk_opsel_erratum.txt; the build's
    // assembly gate (tools/pk_opsel_fix.py --audit) and tests/test_erratum_gpu.py hold that line.
    // (Round 6 tried a second loop body without the depth clamp, chosen per pose TILE by a bound on |X|: no gain on the scalar loop of
    // that time, which was bound by issue slots as said above, and 10-20 us more per launch at the few-object shapes for the bound's
    // extra pass, barriers and per-tile branch; removed.  On this packed loop the count matters: the body is back as CLAMP = false,
    // chosen per OBJECT in front of the chunk loop -- kernel comment: ZFREE; -47 us at C2, profiles/zfree_bench.txt.)
    for (int t = 0; t < ntile; ++t) {
      typename Proj::T ax, ay, az;
      if constexpr (PRESPLIT) {      // A operands rebuilt from the stored words of pose (tile t, row col), k-slice kk
        const u32x4 q = qtab[(t * 16 + col) * 4 + kk];
        const unsigned z = ztab[(t * 16 + col) * 4 + kk];
        ax = bf16_a_from_words(q[0], bf16_dup_lo(q[3]));
        ay = bf16_a_from_words(q[1], bf16_dup_hi(q[3]));
        az = bf16_a_from_words(q[2], bf16_dup_lo(z));
      } else {
        const float* grp = ptab + (t * 4 + (col >> 2)) * 48 + (col & 3);
        ax = Proj::a(grp[kk * 4]); ay = Proj::a(grp[(4 + kk) * 4]); az = Proj::a(grp[(8 + kk) * 4]);
      }
      const float4 aw4 = *reinterpret_cast<const float4*>(wtab + t * 16 + g4);
      // this lane's 4 poses: rows of K R (the back-projection), one float4 = one component of the four poses
      const float4* rows = reinterpret_cast<const float4*>(ptab + (t * 4 + kk) * 48);
      const float4 kxx = rows[0], kxy = rows[1], kxz = rows[2], kyx = rows[4], kyy = rows[5], kyz = rows[6], kzx = rows[8], kzy = rows[9],
                   kzz = rows[10];
      // Four resident tiles (two waves per SIMD, registers to spare): a software pipeline over the tiles -- tile i + 1's three
      // projections are issued in front of tile i's pair work, so that no wave waits out an MFMA's result latency in s_nops (29 -> 1
      // per pose tile).  With one or two tiles the compiler's own placement is the better one (the fence costs it its freedom).
      constexpr bool kPipe = (NPT == 4);
      floatx4 hxn = zero, hyn = zero, hzn = zero;
      if (kPipe) {
        hxn = Proj::mma(ax, rB[0], zero); hyn = Proj::mma(ay, rB[0], zero); hzn = Proj::mma(az, rB[0], zero);
      }
#pragma unroll
      for (int i = 0; i < NPT; ++i) {
        floatx4 hx, hy, hz;
        if (kPipe) {
          hx = hxn; hy = hyn; hz = hzn;
          if (i + 1 < NPT) {
            hxn = Proj::mma(ax, rB[i + 1], zero);
            hyn = Proj::mma(ay, rB[i + 1], zero);
            hzn = Proj::mma(az, rB[i + 1], zero);
            sched_fence();
          }
        } else {
          hx = Proj::mma(ax, rB[i], zero);
          hy = Proj::mma(ay, rB[i], zero);
          hz = Proj::mma(az, rB[i], zero);
        }
        const float4 w4 = rW[i];
        const f32x2 wu2 = {w4.x, w4.x}, cu2 = {w4.y, w4.y}, wv2 = {w4.z, w4.z}, cv2 = {w4.w, w4.w};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x2 hx2 = {hx[2 * h], hx[2 * h + 1]}, hy2 = {hy[2 * h], hy[2 * h + 1]};
          const float hz0 = hz[2 * h], hz1 = hz[2 * h + 1];
          const f32x2 aw2 = h ? f32x2{aw4.z, aw4.w} : f32x2{aw4.x, aw4.y};
          const f32x2 rz2 = {fast_rcp(CLAMP ? clamp_below(hz0, zmin_v) : hz0), fast_rcp(CLAMP ? clamp_below(hz1, zmin_v) : hz1)};
          f32x2 rx2, ry2, ghx2, ghy2, ghz2;
          // Huber weight min(1, delta / rho) = min(1, rs) straight from the reciprocal norm (rho * rs = 1): ONE clamped multiply where
          // rho, min(rho, 1) and their product with rs took three.
          // d huber / d delta = max(rho - delta, 0) (/ delta) = coef |r|^2 - a min(|r|^2, 1) (residuals in units of delta; outlier:
          // a rho - a, inlier: a rho^2 - a rho^2 = 0): the first term is what A2x + A2y accumulate anyway, the second costs one clamped
          // multiply per pair and a packed fma (`gsat2`) where rho, rho (1 - c1) and the accumulation took three instructions per pair.
          f32x2 coef2, crx2, cry2;
          if (!BOUNDS) {
            // no projection clamp: the weight goes into the reciprocal depth once (w / z), which serves the residual and the
            // gradient w.r.t. (h_x, h_y) -- one multiply per pair less than projecting first
            const f32x2 wrx2 = rz2 * wu2, wry2 = rz2 * wv2;
            rx2 = fma2(hx2, wrx2, cu2);
            ry2 = fma2(hy2, wry2, cv2);
            const f32x2 s22 = fma2(rx2, rx2, fma2(ry2, ry2, tiny2));      // |r|^2 + 1e-30: one v_max less per pair than clamping
            const f32x2 c12 = {sat_mul(fast_rsqrt(s22[0]), one_v), sat_mul(fast_rsqrt(s22[1]), one_v)};
            coef2 = aw2 * c12;
            if (!DCOST) gsat2 = fma2(aw2, f32x2{sat_mul(s22[0], one_v), sat_mul(s22[1], one_v)}, gsat2);
            crx2 = coef2 * rx2;
            cry2 = coef2 * ry2;
            ghx2 = crx2 * wrx2;
            ghy2 = cry2 * wry2;
            ghz2 = -rz2 * fma2(ghx2, hx2, ghy2 * hy2);                      // = -(ghx p_x + ghy p_y)
          } else {
            const f32x2 ppx2 = hx2 * rz2, ppy2 = hy2 * rz2;                 // un-clamped projection
            const f32x2 px2 = {clamp_lu(ppx2[0], bd.lbx, bd.ubx), clamp_lu(ppx2[1], bd.lbx, bd.ubx)};
            const f32x2 py2 = {clamp_lu(ppy2[0], bd.lby, bd.uby), clamp_lu(ppy2[1], bd.lby, bd.uby)};
            rx2 = fma2(px2, wu2, cu2);
            ry2 = fma2(py2, wv2, cv2);
            const f32x2 s22 = fma2(rx2, rx2, fma2(ry2, ry2, tiny2));
            const f32x2 c12 = {sat_mul(fast_rsqrt(s22[0]), one_v), sat_mul(fast_rsqrt(s22[1]), one_v)};
            coef2 = aw2 * c12;
            if (!DCOST) gsat2 = fma2(aw2, f32x2{sat_mul(s22[0], one_v), sat_mul(s22[1], one_v)}, gsat2);
            crx2 = coef2 * rx2;
            cry2 = coef2 * ry2;
            f32x2 gpx2 = crx2 * wu2, gpy2 = cry2 * wv2;
            // the clamp passes no gradient where it is active: inside [lb, ub] <=> clamp(x) == x
            gpx2 = f32x2{(px2[0] == ppx2[0]) ? gpx2[0] : 0.f, (px2[1] == ppx2[1]) ? gpx2[1] : 0.f};
            gpy2 = f32x2{(py2[0] == ppy2[0]) ? gpy2[0] : 0.f, (py2[1] == ppy2[1]) ? gpy2[1] : 0.f};
            ghx2 = gpx2 * rz2;
            ghy2 = gpy2 * rz2;
            ghz2 = fma2(-ghx2, ppx2, -(ghy2 * ppy2));
          }
          // "in front of the depth clamp" as a 0/1 factor from ONE full-rate instruction per pair (front_scale above)
          if constexpr (CLAMP) ghz2 = ghz2 * f32x2{sat_fma(hz0, front_scale, front_off), sat_fma(hz1, front_scale, front_off)};
          // d/dw = crx * (px - u) = crx * rx / w and d/du = -crx * w: the per-point factors are applied once at the end
          A2x[i] = fma2(crx2, rx2, A2x[i]);
          A2y[i] = fma2(cry2, ry2, A2y[i]);
          A1x[i] = fma2(coef2, rx2, A1x[i]);
          A1y[i] = fma2(coef2, ry2, A1y[i]);
          const f32x2 kxx2 = h ? f32x2{kxx.z, kxx.w} : f32x2{kxx.x, kxx.y}, kyx2 = h ? f32x2{kyx.z, kyx.w} : f32x2{kyx.x, kyx.y},
                      kzx2 = h ? f32x2{kzx.z, kzx.w} : f32x2{kzx.x, kzx.y};
          const f32x2 kxy2 = h ? f32x2{kxy.z, kxy.w} : f32x2{kxy.x, kxy.y}, kyy2 = h ? f32x2{kyy.z, kyy.w} : f32x2{kyy.x, kyy.y},
                      kzy2 = h ? f32x2{kzy.z, kzy.w} : f32x2{kzy.x, kzy.y};
          const f32x2 kxz2 = h ? f32x2{kxz.z, kxz.w} : f32x2{kxz.x, kxz.y}, kyz2 = h ? f32x2{kyz.z, kyz.w} : f32x2{kyz.x, kyz.y},
                      kzz2 = h ? f32x2{kzz.z, kzz.w} : f32x2{kzz.x, kzz.y};
          gXv[i] = fma2(kxx2, ghx2, fma2(kyx2, ghy2, fma2(kzx2, ghz2, gXv[i])));
          gYv[i] = fma2(kxy2, ghx2, fma2(kyy2, ghy2, fma2(kzy2, ghz2, gYv[i])));
          gZv[i] = fma2(kxz2, ghx2, fma2(kyz2, ghy2, fma2(kzz2, ghz2, gZv[i])));
        }
      }
    }
    const float gsat = gsat2[0] + gsat2[1];
    {   // d/d delta of this chunk: sum_pairs coef |r|^2 (= the sums behind d/dw, before their per-point factors) - sum_pairs a min(|r|^2, 1)
        // (DCOST: 2 C_b - sum_pairs coef |r|^2, the object's C_b added once behind the chunk loop)
      float a2 = 0.f;
#pragma unroll
      for (int i = 0; i < NPT; ++i) a2 += (A2x[i][0] + A2x[i][1]) + (A2y[i][0] + A2y[i][1]);
      gd += DCOST ? -a2 : a2 - gsat;
    }
    // ---- outputs of this chunk: sums over the 4 pose groups of a point via MFMAs against indicator columns ----
    // The lane geometry is re-derived here behind an opaque copy of the lane index: as invariants of the chunk loop the four
    // indicator columns and the three 64-bit output addresses were hoisted in front of it and stayed live across the pose-tile
    // loop -- 10 VGPRs, which cost the bf16 instantiation 7 spilled dwords per lane (33 MB of scratch traffic per launch at C2).
    const int laneE = (int)f32_bits(to_vgpr(bits_f32((unsigned)lane)));
    const int colE = laneE & 15, g4E = (laneE >> 4) * 4;
    const float ind0 = (colE == 0) ? 1.f : 0.f, ind1 = (colE == 1) ? 1.f : 0.f, ind2 = (colE == 2) ? 1.f : 0.f,
                ind3 = (colE == 3) ? 1.f : 0.f;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      floatx4 D1 = zero;
      D1 = mfma_16x16x4((gXv[i][0] + gXv[i][1]) * hs.delta_sq, ind0, D1);
      D1 = mfma_16x16x4((gYv[i][0] + gYv[i][1]) * hs.delta_sq, ind1, D1);
      D1 = mfma_16x16x4((gZv[i][0] + gZv[i][1]) * hs.delta_sq, ind2, D1);
      const float4 w4 = rW[i];
      floatx4 D2 = zero;
      const float a1x = A1x[i][0] + A1x[i][1], a1y = A1y[i][0] + A1y[i][1], a2x = A2x[i][0] + A2x[i][1], a2y = A2y[i][0] + A2y[i][1];
      D2 = mfma_16x16x4(-w4.x * a1x * hs.delta_sq, ind0, D2);                               // d/du
      D2 = mfma_16x16x4(-w4.z * a1y * hs.delta_sq, ind1, D2);                               // d/dv
      D2 = mfma_16x16x4((w4.x != 0.f) ? a2x * hs.delta / w4.x : 0.f, ind2, D2);             // d/dwu
      D2 = mfma_16x16x4((w4.z != 0.f) ? a2y * hs.delta / w4.z : 0.f, ind3, D2);             // d/dwv
      const int nb = c0 + (wv + W * i) * 16 + g4E;    // D rows: points nb + r; column = lane & 15
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = nb + r;
        if (n < p.N) {
          const size_t o = (size_t)b * p.N + n;
          if (colE < 3) gx3d[o * 3 + colE] = D1[r];
          if (colE < 2) gx2d[o * 2 + colE] = D2[r];
          else if (colE < 4) {
            if (park) gwl[n * 2 + (colE - 2)] = D2[r]; else gw2d[o * 2 + (colE - 2)] = D2[r];
          }
        }
      }
    }
  }
