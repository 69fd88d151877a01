// Body of bwd_first_kernel (kernels_bwd.hip.h); LDS: sX, sXg, smem, sKp, sWt: textually included by the one-launch-per-layer kernel (where its LDS arrays are separate __shared__ objects,
// exactly as before the layers could be fused - passing them to a function instead changed the register allocation of the
// hot instantiations) and by the stage function of the fused launches (where they are slices of the launch's one LDS array).
// In scope at the point of inclusion: the template parameters, `a`, the LDS arrays named below.
  constexpr int CIN = C1;
  constexpr int CPI = pitch(CIN), CPO = pitch(COUT);
  constexpr int RA = TT + K - 1;
  constexpr int TAIL = S > 1 ? K - 1 : 0;        // extra a0 / g0 rows of a single-tile window ("tail rows", see fwd_first_body.inc)
  constexpr int TAILK = (TAIL + 3) / 4 * 4;   // rows behind the tile that the tail k-steps of dW1 read (whole k-steps of 4 rows)
  constexpr int XR = (TT + TAILK - 1) * S + K1;   // x rows the dW1 contraction of one tile reads
  constexpr int NT1 = C1 / 16;
  constexpr int M1 = K1 * FBINS;                 // rows of W1
  constexpr int MT1 = (M1 + 15) / 16;            // m-tiles of dW1
  constexpr int MPW = (MT1 + 3) / 4;             // m-tiles per wave
  constexpr int MT = CIN / 16, NT = COUT / 16, KSO = COUT / 4;
  constexpr int NCH = nchunks(CIN), L = chunk_len(CIN);
  constexpr int QI = CIN / 4;
  constexpr int RAP = halo_rows_padded(CIN, K), TTP = tile_rows_padded(CIN);
  constexpr int OFF_A = 0, OFF_DP = OFF_A + RAP * CPI, OFF_U = OFF_DP + TT * CPO, OFF_DU = OFF_U + TTP * CPI;
  // X6 (common.hip.h "fp32-grade products on the bf16 matrix pipe"): dW1 = im2col(x)^T g0 as six bf16 slice products per fp32
  // product.  Both operands are contracted over the time rows, which is the strided dimension of their tiles, so they are staged
  // row-major as bf16 slice planes and read with ds_read_b64_tr_b16 (lds_read_tr16): x as three planes of 96-byte rows, g0 as three
  // planes of 64-byte rows whose two 16-channel halves swap places in rows with bit 2 set (conflict-free transpose reads) - in the
  // space of the dp tile (and, for 32 pointwise filters, the start of the u tile behind it), dead once the pointwise phase is over.  No g0 tile of its own then.
  constexpr int PB = 96, PLB = XR * PB, GPB = 2 * CIN, GPL = TT * GPB;
  static_assert(!X6 || (S == 1 && CIN == 32 && (K1 * FBINS) % 8 == 0 && 3 * GPL <= (TT * CPO + TTP * CPI) * 4 && TTP == TT), "the x6 form serves the stride-1 first convolutions");
  constexpr int OFF_G0 = OFF_DU + RAP * CPI, OFF_END = X6 ? OFF_G0 : OFF_G0 + (TTP + TAILK) * CPI;
  static_assert(TAIL <= NCH && TTP + TAIL <= RAP, "tail rows");
  constexpr int PX = FBINS + 1;                  // odd pitch of the staged x rows (see fwd_first_kernel)
  static_assert(OFF_END >= 4 * CIN * COUT && OFF_END >= NCH * (K + 1) * CIN, "scratch aliasing");
  static_assert(TT >= K - 1, "shape");

  float* sA = smem + OFF_A;
  float* sDP = smem + OFF_DP;
  float* sU = smem + OFF_U;
  float* sDU = smem + OFF_DU;
  float* sG0 = smem + OFF_G0;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g = lane >> 4;
  const int c = tid % CIN, chunk = tid / CIN;
  const bool dw_active = chunk < NCH;
  const int Ta = (a.T - K1) / S + 1;
  MWW_PC_DECL
  MWW_PC_AT(0);   // kernel entry (profiling builds only: tools/phase_clocks.py)

  const bool tailmode = TAIL > 0 && Ta > TT && Ta <= TT + TAIL;   // the window is one tile: rows [TT, Ta) ride behind the TT tile rows
  const int ntiles = tailmode ? 1 : (Ta + TT - 1) / TT;
  const int nsamp = (int)blockIdx.x < a.B ? (a.B - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x : 0;
  const int nitems = nsamp * ntiles;
  XStage<XR, PX, MWW_AUX_LD_XB> xs;
  DpStage<COUT, false, SB> dps;
  constexpr int NA = (RA * QI + kThreads - 1) / kThreads;
  float4 pre_a[NA];
  // LATE: group A (x and a0, committed in P0) is requested again in front of barrier 1, group B (the dp rows) is committed and
  // requested again behind P1: sDP is first read in the pointwise phase, and the g0 planes the x6 form keeps in its space are last
  // read in front of the tile's last barrier.  (The x rows stay in group A: their LDS tile is read up to that last barrier, so
  // they could only move towards the dW1 phase, where they would be requested - and waited for - behind both other groups.)
  // `live` false: a request behind the last tile (the window slot of the last one, no rows, empty descriptors).  LATE requests
  // its groups unconditionally: each wait then counts the loads known to follow its group instead of draining them.
  auto issue_a = [&](int it, bool live) {
    const int s = live ? it / ntiles : nsamp - 1, b = blockIdx.x + s * gridDim.x, t0 = (it % ntiles) * TT;
    const int nrx = live ? ((tailmode ? Ta : min(TT, Ta - t0)) - 1) * S + K1 : 0;
    xs.issue(a.x, a.xg, sXg, s, b, a.T, t0 * S, nrx, tid);
    const BufRsrc ra = tile_rsrc(a.a0 + ((size_t)b * Ta + t0) * CIN, live ? min(RA, Ta - t0) * QI * 16 : 0);
#pragma unroll
    for (int j = 0; j < NA; ++j) pre_a[j] = tile_load4<MWW_AUX_LD_A0>(ra, (tid + j * kThreads) * 16);
  };
  auto issue_b = [&](int it, bool live) {
    const int b = blockIdx.x + (it / ntiles) * gridDim.x, t0 = (it % ntiles) * TT;
    const int nvk = live ? max(0, min(TT, a.Tout - t0)) * (COUT / 4) : 0;
    const size_t koff = ((size_t)b * a.Tout + t0) * COUT;
    dps.issue(elem_ptr<SB>(a.pk, koff), elem_ptr<SB>(a.gk, koff), nvk, tid);
  };
  // per-lane offsets of the dW1 rows this wave owns: row m = j*40+f of W1 reads x[s*S+j][f]
  int offm[MPW];
  bool okm[MPW];
  // X6: byte offsets of this lane's share of a transpose read (lane 16 g + p points at row 4 g + (p >> 2) of a 16-row half
  // k-block, four columns from 4 (p & 3) of the 16-column tile): x rows are shifted by the tap j of the lane's column group
  // m = 16 mt + 4 (p & 3) = j * 40 + f (groups past K1 * 40 read the last real one: their dW1 rows are not stored)
  int xoff[MPW], goff[NT1];
  if constexpr (X6) {
    const int rowl = 4 * g + (r16 >> 2), cg = 4 * (r16 & 3);
#pragma unroll
    for (int mi = 0; mi < MPW; ++mi) {
      const int m = min((wave * MPW + mi) * 16 + cg, M1 - 4);
      xoff[mi] = (rowl + m / FBINS) * PB + (m % FBINS) * 2;
    }
#pragma unroll
    for (int nt = 0; nt < NT1; ++nt) goff[nt] = rowl * GPB + ((nt * 16 + cg) ^ ((rowl & 4) ? 16 : 0)) * 2;
  } else {
#pragma unroll
  for (int mi = 0; mi < MPW; ++mi) {
    const int m = (wave * MPW + mi) * 16 + r16;
    okm[mi] = m < M1;
    offm[mi] = okm[mi] ? (m / FBINS) * PX + (m % FBINS) : 0;
  }
  }
  if (a.xg.win) xgather_setup(a.xg, sXg, nsamp, tid);
  stagger_start<MWW_STAGGER_BWD>();
  if (nitems > 0) {
    issue_a(0, true);
    issue_b(0, true);
  }

  // every global load of the prologue first (see WeightStage) ...
  WeightStage<CIN, COUT, 0, pitch_wt(CIN, BF)> wst;
  wst.load(a.pw_w, nullptr, tid);
  float dww[K], accw[K];
  float accb = 0.f, dwb = 0.f;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    dww[i] = dw_active ? a.dw_w[i * CIN + c] : 0.f;
    accw[i] = 0.f;
  }
  if (dw_active) dwb = a.dw_b[c];
  // ... then BN_1's backward coefficients
  for (int i = tid; i < COUT; i += kThreads) {
    const float krs = a.k_rstd[i];
    const float kmean = a.k_mean[i];
    float c1, mg, mgx;
    if (a.gfold.acc) {
      bn_grad_fold_channel(a.gfold, COUT, i, krs, c1, mg, mgx);
    } else {
      c1 = a.k_c1[i];
      mg = a.k_mg[i];
      mgx = a.k_mgx[i];
    }
    const float kA = -c1 * krs * mgx;
    sKp[0 * COUT + i] = c1;
    sKp[1 * COUT + i] = kA;
    sKp[2 * COUT + i] = -c1 * mg - kA * kmean;
    sKp[5 * COUT + i] = 0.f;
    sKp[6 * COUT + i] = 0.f;
  }
  wst.store(sWt, nullptr, tid);
  for (int i = RA * CPI + tid; i < RAP * CPI; i += kThreads) {
    sA[i] = 0.f;
    sDU[i] = 0.f;
  }
  // g0 rows behind the tile: the tail k-step reads four of them, the tail rows [TT, Ta) are rewritten per window, the rest stays zero
  if constexpr (!X6)
    for (int i = TTP * CPI + tid; i < (TTP + TAILK) * CPI; i += kThreads) sG0[i] = 0.f;
#pragma unroll
  for (int i = 0; i < K; ++i) pin(dww[i]);
  pin(dwb);
  f32x4 dwacc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) dwacc[mt][nt] = zero4();
  f32x4 w1acc[MPW][NT1];
#pragma unroll
  for (int mi = 0; mi < MPW; ++mi)
#pragma unroll
    for (int nt = 0; nt < NT1; ++nt) w1acc[mi][nt] = zero4();
  __syncthreads();

  MWW_PC_AT(1);   // prologue done
  MWW_PC_START(MWW_ABLATE(a, 16) && tid == 0);
  for (int it = 0; it < nitems; ++it) {
    rotate_priority(it, 2);
    const int t0 = (it % ntiles) * TT;
    const int nrows_new = max(0, min(TT, a.Tout - t0));
    const int rows_da = min(TT, Ta - t0);
    // ---- P0: commit x (odd pitch), a0 rows [t0, t0+RA) (zero past the sample), dp; roll the du ring
    if constexpr (X6) xs.template commit_planes<PB, PLB>(reinterpret_cast<unsigned*>(sX), a.xg, sXg, it / ntiles, t0 * S, tid);
    else xs.commit(sX, a.xg, sXg, it / ntiles, t0 * S, tid);
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int i = tid + j * kThreads;
      if (i < RA * QI) {
        const int r = i / QI, q = i - r * QI;
        *reinterpret_cast<float4*>(sA + r * CPI + q * 4) = pre_a[j];
      }
    }
    MWW_PC_MARK(0);   // commit of group A (incl. the wait for the prefetched x / a0 rows)
    if constexpr (!LATE) dps.commit(sDP, sKp, 0.f, nrows_new * (COUT / 4), tid);
    carry_du<K, CPI>(sDU, t0 == 0, tid);
    if constexpr (LATE) issue_a(it + 1, it + 1 < nitems);
    MWW_PC_MARK(LATE ? 0 : 8);   // !LATE: commit of group B (incl. the wait for the dp rows) + ring roll
    __syncthreads();
    MWW_PC_MARK(1);   // barrier 1
    if constexpr (!LATE) {
      if (it + 1 < nitems) {
        issue_a(it + 1, true);
        issue_b(it + 1, true);
      }
    }
    // ---- P1: u = depthwise(a0) + bias
    if (dw_active) {
      if (chunk * L < nrows_new) {
        float o[L];
        dw_chunk<K, L>(sA, CPI, chunk * L, c, dww, dwb, o);
#pragma unroll
        for (int t = 0; t < L; ++t) {
          const int tl = chunk * L + t;
          sU[tl * CPI + c] = (tl < nrows_new) ? o[t] : 0.f;
        }
      } else {
#pragma unroll
        for (int t = 0; t < L; ++t) sU[(chunk * L + t) * CPI + c] = 0.f;
      }
    }
    MWW_PC_MARK(2);   // issue + P1 (u recompute)
    if constexpr (LATE) {
      dps.commit(sDP, sKp, 0.f, nrows_new * (COUT / 4), tid);
      issue_b(it + 1, it + 1 < nitems);
      MWW_PC_MARK(8);   // commit of group B (incl. the wait for the dp rows) + its next request
    }
    __syncthreads();
    MWW_PC_MARK(3);   // barrier 2
    pointwise_backward_tile<CIN, COUT, K, BF>(sU, sDP, sDU, wave, r16, g, sWt, dwacc, wave * 16 < nrows_new);
    MWW_PC_MARK(4);   // MFMA (dW_pw, du)
    __syncthreads();
    MWW_PC_MARK(5);   // barrier 3
    // ---- P4: depthwise backward -> g0 = da * relu'(a0) kept in LDS
    if (dw_active) {
      // one pass over LDS for the whole phase (see bwd_block_body.inc)
      float wdu[L + K - 1], wa[L + K - 1];
#pragma unroll
      for (int j = 0; j < L + K - 1; ++j) wdu[j] = sDU[(chunk * L + j) * CPI + c];
#pragma unroll
      for (int j = 0; j < L + K - 1; ++j) wa[j] = sA[(chunk * L + j) * CPI + c];
      lds_reads_first();
#pragma unroll
      for (int t = 0; t < L; ++t) {
        const int sl = chunk * L + t;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < K; ++i) acc = fmaf(dww[K - 1 - i], wdu[t + i], acc);
        const float gv = (sl < rows_da && wa[t] > 0.f) ? acc : 0.f;
        if constexpr (X6) {
          unsigned h0, h1, h2;
          split3(gv, h0, h1, h2);
          unsigned short* gp = reinterpret_cast<unsigned short*>(sDP) + sl * CIN + (c ^ ((sl & 4) ? 16 : 0));
          gp[0] = (unsigned short)(h0 >> 16);
          gp[GPL / 2] = (unsigned short)(h1 >> 16);
          gp[GPL] = (unsigned short)(h2 >> 16);
        } else {
          sG0[sl * CPI + c] = gv;
        }
      }
      if (chunk * L < nrows_new) {
#pragma unroll
        for (int t = 0; t < L; ++t) {
          const float dut = wdu[K - 1 + t];
          accb += dut;
#pragma unroll
          for (int i = 0; i < K; ++i) accw[i] = fmaf(dut, wa[t + i], accw[i]);
        }
      }
      if constexpr (TAIL > 0) {
        if (tailmode && chunk < TAIL) {
          // input-gradient rows [TT, Ta) of a single-tile window: one row per chunk (du rows past the tile are zero: the
          // ring ends at row RAP)
          const int sl = TT + chunk;
          float acc = 0.f;
#pragma unroll
          for (int j = 0; j < K; ++j) acc = fmaf(dww[K - 1 - j], sl + j < RAP ? sDU[(sl + j) * CPI + c] : 0.f, acc);
          sG0[sl * CPI + c] = (sl < Ta && sA[sl * CPI + c] > 0.f) ? acc : 0.f;
        }
      }
    }
    MWW_PC_MARK(6);   // P4 (depthwise backward, g0)
    __syncthreads();
    // ---- dW1 += im2col(x)^T g0 : A[m][k=s] = x[s*S + m/40][m%40], B[k=s][n] = g0[s][n]
    // (operands one k-step ahead of their MFMAs, schedule pinned: see pointwise_backward_tile)
    if constexpr (X6) {
      // per k-block of 32 rows (k-slot 8 g + 4 h + e of the MFMA = row 32 kb + 16 h + 4 g + e, the same for both operands):
      // the three slice quads of g0's column tile, then per m-tile those of x and the six products
      const char* xb = reinterpret_cast<const char*>(sX);
      const char* gb = reinterpret_cast<const char*>(sDP);
#pragma unroll
      for (int kb = 0; kb < TT / 32; ++kb)
#pragma unroll
        for (int nt = 0; nt < NT1; ++nt) {
          u32x4v gq[3];
#pragma unroll
          for (int p = 0; p < 3; ++p) {
            const u32x2v lo = lds_read_tr16(gb + goff[nt] + p * GPL + (32 * kb) * GPB), hi = lds_read_tr16(gb + goff[nt] + p * GPL + (32 * kb + 16) * GPB);
            gq[p] = u32x4v{lo.x, lo.y, hi.x, hi.y};
          }
#pragma unroll
          for (int mi = 0; mi < MPW; ++mi) {
            u32x4v xq[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) {
              const u32x2v lo = lds_read_tr16(xb + xoff[mi] + p * PLB + (32 * kb) * S * PB), hi = lds_read_tr16(xb + xoff[mi] + p * PLB + (32 * kb + 16) * S * PB);
              xq[p] = u32x4v{lo.x, lo.y, hi.x, hi.y};
            }
            w1acc[mi][nt] = mfma_x6(xq, gq, w1acc[mi][nt]);
          }
        }
    } else {
      float av[2][MPW], bv[2][NT1];
      auto load_w1 = [&](int kk, int sl) {
        const int s = kk * 4 + g;
#pragma unroll
        for (int nt = 0; nt < NT1; ++nt) bv[sl][nt] = sG0[s * CPI + nt * 16 + r16];
#pragma unroll
        for (int mi = 0; mi < MPW; ++mi) {
          const float v = sX[s * S * PX + offm[mi]];   // (rows past M1 read offset 0 and are zeroed: no conditional load)
          av[sl][mi] = okm[mi] ? v : 0.f;
        }
      };
      load_w1(0, 0);
#pragma unroll
      for (int kk = 0; kk < TT / 4; ++kk) {
        if (kk + 1 < TT / 4) load_w1(kk + 1, (kk + 1) & 1);
#pragma unroll
        for (int mi = 0; mi < MPW; ++mi)
#pragma unroll
          for (int nt = 0; nt < NT1; ++nt) w1acc[mi][nt] = mfma4(av[kk & 1][mi], bv[kk & 1][nt], w1acc[mi][nt]);
      }
      __builtin_amdgcn_sched_group_barrier(0x100, MPW + NT1, 0);
      sched_read_mfma_groups<TT / 4 - 1, MPW + NT1, MPW * NT1>();
      sched_read_mfma_groups<1, 0, MPW * NT1>();
      if constexpr (TAIL > 0) {
        if (tailmode) {   // the tail rows [TT, Ta): one or two more k-steps (g0 rows past Ta are zero)
#pragma unroll
          for (int ks = 0; ks < TAILK / 4; ++ks) {
            load_w1(TT / 4 + ks, 0);
#pragma unroll
            for (int mi = 0; mi < MPW; ++mi)
#pragma unroll
              for (int nt = 0; nt < NT1; ++nt) w1acc[mi][nt] = mfma4(av[0][mi], bv[0][nt], w1acc[mi][nt]);
          }
        }
      }
    }
    MWW_PC_MARK(7);   // barrier 4 + the conv1 weight gradient
    __syncthreads();
    MWW_PC_MARK(5);   // its barrier: counted with barrier 3
  }
  MWW_PC_AT(2);   // tile loop done
  float* gdst = a.grad_part + (size_t)blockIdx.x * (M1 * C1 + (K + 1) * CIN + CIN * COUT);
#pragma unroll
  for (int mi = 0; mi < MPW; ++mi)
#pragma unroll
    for (int nt = 0; nt < NT1; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = (wave * MPW + mi) * 16 + g * 4 + r;
        if (m < M1) gdst[m * C1 + nt * 16 + r16] = w1acc[mi][nt][r];
      }
  write_block_grad_partials<CIN, COUT, K>(smem, gdst + M1 * C1, dwacc, accw, accb, dw_active, c, chunk, tid, wave, r16, g);
  MWW_PC_AT(3);   // epilogue done
  MWW_PC_DUMP(a.phase_clk ? a.phase_clk + (size_t)blockIdx.x * kClkSlots : nullptr);
