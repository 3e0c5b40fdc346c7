// ba_big.inc -- the reduced pose system beyond the LDS-resident limit (more than MAX_FREE_KF_LDS free key frames; included by ba.hip).
// The kernels first, the host side (pair lists, the Schur complement + solve part of a slot) at the end of the file.
//
// Same mathematics as k_ba_schur_c / k_ba_solve_c (BlockSolver::solve with the Schur complement, block_solver.hpp:354-486,
// dense LDL^T without pivoting) and the same place in a slot of the device-resident schedule: every kernel reads the
// Levenberg-Marquardt state from BACtl and does nothing in a slot that only linearises or after the schedule has finished.
// The reduced system S (P6 x P6) lives in HBM and everything is a deterministic gather:
//   k_ba_dinv            lane per landmark: (Hll + lambda I)^-1
//   k_ba_schur_gather    one wave per non-zero 6x6 block (pr <= pc) of S: sum over the landmarks seen by both key frames of
//                        (W_a D^-1) W_b^T; the (block -> edge pair) lists are built once per BA on the host
//   k_ba_rhs_gather      one wave per free key frame: r_a = sum over its edges of (W_a D^-1) b_l
//   k_big_assemble       M = diagonal blocks of Hpp + HppO + lambda I - S (lower triangle), rhs = bp - r
//   k_big_panel          one workgroup: right-looking LDL^T of a 48x48 diagonal block in LDS, then the panel below it
//   k_big_update         trailing update M22 -= L21 D L21^T, one 48x48 tile per workgroup, lower triangle only
//   k_big_solve          one workgroup: blocked forward / diagonal / backward substitution, vector in LDS; the triangular
//                        solve inside a panel runs in one wave with shuffles

// (BIG_NB, the panel width, is in ba_plan.h: the plan sizes U by it.)
__device__ __forceinline__ bool big_idle(const BACtl *c) { return c->phase == 2 || c->needInit; }  // no trial in this slot

__global__ __launch_bounds__(256) void k_ba_dinv(BADev D, Lb2 lb, const BACtl *c, double *Dinv) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (big_idle(c) || l >= D.npt) return;
  const LinBuf &B = lb.b[c->cur];
  const double lambda = c->lambda;
  double M[9];
#pragma unroll
  for (int i = 0; i < 9; i++) M[i] = B.Hll[(size_t)9 * l + i];
  M[0] += lambda; M[4] += lambda; M[8] += lambda;
  const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
  const double det = M[0] * c00 + M[1] * c01 + M[2] * c02;
  const double id = 1.0 / det;
  double *Di = Dinv + (size_t)9 * l;
  Di[0] = c00 * id; Di[1] = (M[2] * M[7] - M[1] * M[8]) * id; Di[2] = (M[1] * M[5] - M[2] * M[4]) * id;
  Di[3] = c01 * id; Di[4] = (M[0] * M[8] - M[2] * M[6]) * id; Di[5] = (M[2] * M[3] - M[0] * M[5]) * id;
  Di[6] = c02 * id; Di[7] = (M[1] * M[6] - M[0] * M[7]) * id; Di[8] = (M[0] * M[4] - M[1] * M[3]) * id;
}

struct BigLists {  // device CSR: block -> (row edge, column edge) pairs, row block <= column block
  int nBlocks;
  const int *blk_start;  // [nBlocks + 1]
  const int *blk_pr, *blk_pc;
  const int *ent_er, *ent_ec;
};

__global__ __launch_bounds__(256) void k_ba_schur_gather(BADev D, Lb2 lb, const BACtl *c, const double *Dinv, BigLists Lst, double *S, int P6) {
  const int blk = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (big_idle(c) || blk >= Lst.nBlocks) return;
  const LinBuf &B = lb.b[c->cur];
  double acc[36];
#pragma unroll
  for (int i = 0; i < 36; i++) acc[i] = 0;
  for (int q = Lst.blk_start[blk] + lane; q < Lst.blk_start[blk + 1]; q += 64) {
    const int er = Lst.ent_er[q], ec = Lst.ent_ec[q];
    if (D.e_level[er] != 0 || D.e_level[ec] != 0) continue;
    const double *Di = Dinv + (size_t)9 * D.e_pt[er];
    const double *Wr = B.W + (size_t)er * 18, *Wc = B.W + (size_t)ec * 18;
    double wc[18];
#pragma unroll
    for (int i = 0; i < 18; i++) wc[i] = Wc[i];
#pragma unroll
    for (int i = 0; i < 6; i++) {
      const double w0 = Wr[i * 3], w1 = Wr[i * 3 + 1], w2 = Wr[i * 3 + 2];
      const double y0 = w0 * Di[0] + w1 * Di[3] + w2 * Di[6];
      const double y1 = w0 * Di[1] + w1 * Di[4] + w2 * Di[7];
      const double y2 = w0 * Di[2] + w1 * Di[5] + w2 * Di[8];
#pragma unroll
      for (int j = 0; j < 6; j++) acc[i * 6 + j] += y0 * wc[j * 3] + y1 * wc[j * 3 + 1] + y2 * wc[j * 3 + 2];
    }
  }
#pragma unroll
  for (int i = 0; i < 36; i++) acc[i] = wave_sum(acc[i]);
  if (lane == 0) {
    const int pr = Lst.blk_pr[blk], pc = Lst.blk_pc[blk];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int j = 0; j < 6; j++) S[(size_t)(6 * pr + i) * P6 + 6 * pc + j] = acc[i * 6 + j];
  }
}

__global__ __launch_bounds__(256) void k_ba_rhs_gather(BADev D, Lb2 lb, const BACtl *c, const double *Dinv, double *r) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (big_idle(c) || k >= D.np) return;
  const LinBuf &B = lb.b[c->cur];
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int c = D.ps_start[k] + lane; c < D.ps_start[k + 1]; c += 64) {
    const int e = D.ps_edges[c];
    if (D.e_level[e] != 0) continue;
    const int l = D.e_pt[e];
    const double *Di = Dinv + (size_t)9 * l, *W = B.W + (size_t)e * 18;
    const double b0 = B.bl[(size_t)3 * l], b1 = B.bl[(size_t)3 * l + 1], b2 = B.bl[(size_t)3 * l + 2];
    const double t0 = Di[0] * b0 + Di[1] * b1 + Di[2] * b2, t1 = Di[3] * b0 + Di[4] * b1 + Di[5] * b2,
                 t2 = Di[6] * b0 + Di[7] * b1 + Di[8] * b2;
#pragma unroll
    for (int i = 0; i < 6; i++) acc[i] += W[i * 3] * t0 + W[i * 3 + 1] * t1 + W[i * 3 + 2] * t2;
  }
#pragma unroll
  for (int i = 0; i < 6; i++) acc[i] = wave_sum(acc[i]);
  if (lane == 0)
#pragma unroll
    for (int i = 0; i < 6; i++) r[6 * k + i] = acc[i];
}

// M (lower triangle, row-major, ld = P6) = Hpp + lambda I - S ; rhs = bp - r, formed as solve_lookahead forms them: the
// dense Hpp is not materialised, B.Hpp holds the key frames' diagonal blocks and HppO (exchange block of the accepted
// linearisation) the pose-pose blocks.  S, Hpp and HppO are read in their UPPER triangle.
__global__ void k_big_assemble(Lb2 lb, const BACtl *c, XBLay xb, const double *S, const double *r, double *M, double *rhs, int P6, double *okFlag) {
  if (big_idle(c)) return;
  const LinBuf &B = lb.b[c->cur];
  const double *HppO = xb.at(c->cur) + xb.oH;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < (long long)P6 * P6) {
    const int i = (int)(idx / P6), j = (int)(idx % P6);
    if (j <= i) {
      double h = HppO[(size_t)j * P6 + i] - S[(size_t)j * P6 + i];
      if (i / 6 == j / 6) h += B.Hpp[(size_t)j * P6 + i];  // same key frame: the diagonal block
      if (i == j) h += c->lambda;
      M[(size_t)i * P6 + j] = h;
    }
  }
  if (idx < P6) rhs[idx] = B.bp[idx] - r[idx];
  if (idx == 0) *okFlag = 1.0;  // cleared by k_big_panel on a zero pivot
}

// LDL^T of the diagonal block [k0, k0+kw) and the panel below it.  On exit M holds unit-lower L (below the diagonal) and
// D (on it) in these columns; U[row][c] = L[row][k0+c] * d_c for the trailing update.
__global__ __launch_bounds__(256) void k_big_panel(const BACtl *c, double *M, int P6, int k0, int kw, double *U, double *okFlag) {
  __shared__ double Ld[BIG_NB][BIG_NB + 1];
  __shared__ double dd[BIG_NB];
  __shared__ int s_neg;
  static_assert(sizeof(Ld) + sizeof(dd) + sizeof(s_neg) == STATIC_BIG_PANEL, "ba_plan.h states this kernel's static LDS");
  if (big_idle(c)) return;
  const int tid = threadIdx.x;
  if (tid == 0) s_neg = 0;
  for (int i = tid; i < kw * kw; i += 256) {
    const int rr = i / kw, cc = i % kw;
    Ld[rr][cc] = cc <= rr ? M[(size_t)(k0 + rr) * P6 + k0 + cc] : 0.0;
  }
  __syncthreads();
  for (int c = 0; c < kw; c++) {  // right-looking: column c is final when its turn comes
    const double dc = Ld[c][c];
    const double inv = dc != 0 ? 1.0 / dc : 0.0;
    if (tid == 0) { dd[c] = dc; if (dc == 0) s_neg = 1; }  // SimplicialLDLT rule (see solve_lookahead)
    const int m = kw - c - 1;  // trailing size
    for (int rr = tid >> 4; rr < m; rr += 16) {
      const double lr = Ld[c + 1 + rr][c] * inv;
      for (int ss = tid & 15; ss <= rr; ss += 16) Ld[c + 1 + rr][c + 1 + ss] -= lr * Ld[c + 1 + ss][c];
    }
    __syncthreads();
    for (int rr = tid; rr < m; rr += 256) Ld[c + 1 + rr][c] *= inv;
    __syncthreads();
  }
  for (int i = tid; i < kw * kw; i += 256) {
    const int rr = i / kw, cc = i % kw;
    if (cc < rr) M[(size_t)(k0 + rr) * P6 + k0 + cc] = Ld[rr][cc];
    else if (cc == rr) M[(size_t)(k0 + rr) * P6 + k0 + cc] = dd[rr];
  }
  // rows below the block: u = a L11^-T (forward substitution), l = u / d
  for (int row = k0 + kw + tid; row < P6; row += 256) {
    double u[BIG_NB];
#pragma unroll
    for (int c = 0; c < BIG_NB; c++) {
      if (c < kw) {
        double v = M[(size_t)row * P6 + k0 + c];
        for (int m = 0; m < c; m++) v -= u[m] * Ld[c][m];
        u[c] = v;
      }
    }
#pragma unroll
    for (int c = 0; c < BIG_NB; c++) {
      if (c < kw) {
        U[(size_t)row * BIG_NB + c] = u[c];
        M[(size_t)row * P6 + k0 + c] = dd[c] != 0 ? u[c] / dd[c] : 0.0;
      }
    }
  }
  if (tid == 0 && s_neg) *okFlag = 0.0;
}

// trailing update of the lower triangle: tile (bi, bj), bj <= bi, of the rows >= k0 + kw
__global__ __launch_bounds__(256) void k_big_update(const BACtl *c, double *M, int P6, int k0, int kw, const double *U) {
  __shared__ double Lt[BIG_NB][BIG_NB + 1], Ut[BIG_NB][BIG_NB + 1];
  static_assert(sizeof(Lt) + sizeof(Ut) == STATIC_BIG_UPDATE, "ba_plan.h states this kernel's static LDS");
  if (big_idle(c)) return;
  const int t0 = k0 + kw;
  const int nb = (P6 - t0 + BIG_NB - 1) / BIG_NB;
  int bi = 0, rem = blockIdx.x;  // blockIdx.x enumerates (bi, bj <= bi)
  while (rem > bi) { rem -= bi + 1; bi++; }
  const int bj = rem;
  if (bi >= nb) return;
  const int r0 = t0 + bi * BIG_NB, c0 = t0 + bj * BIG_NB;
  const int tid = threadIdx.x;
  for (int i = tid; i < BIG_NB * BIG_NB; i += 256) {
    const int rr = i / BIG_NB, cc = i % BIG_NB;
    Lt[rr][cc] = (r0 + rr < P6 && cc < kw) ? M[(size_t)(r0 + rr) * P6 + k0 + cc] : 0.0;
    Ut[rr][cc] = (c0 + rr < P6 && cc < kw) ? U[(size_t)(c0 + rr) * BIG_NB + cc] : 0.0;
  }
  __syncthreads();
  for (int i = tid; i < BIG_NB * BIG_NB; i += 256) {
    const int rr = i / BIG_NB, cc = i % BIG_NB;
    const int gr = r0 + rr, gc = c0 + cc;
    if (gr >= P6 || gc >= P6 || gc > gr) continue;
    double acc = 0;
#pragma unroll
    for (int m = 0; m < BIG_NB; m++) acc += Lt[rr][m] * Ut[cc][m];
    M[(size_t)gr * P6 + gc] -= acc;
  }
}

// L y = b, z = D^-1 y, L^T x = z.  One workgroup, the vector in LDS (P6 <= 4096).
__global__ __launch_bounds__(256) void k_big_solve(const BACtl *c, const double *M, const double *rhs, int P6, double *xp) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  if (big_idle(c)) return;
  double *y = reinterpret_cast<double *>(smem);   // [P6]
  __shared__ double Lp[BIG_NB][BIG_NB + 1];       // diagonal block of the current panel
  static_assert(sizeof(Lp) == STATIC_BIG_SOLVE, "ba_plan.h states this kernel's static LDS");
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < P6; i += 256) y[i] = rhs[i];
  const int nblk = (P6 + BIG_NB - 1) / BIG_NB;
  for (int kb = 0; kb < nblk; kb++) {  // forward
    const int k0 = kb * BIG_NB, kw = min(BIG_NB, P6 - k0);
    __syncthreads();
    for (int i = tid; i < kw * kw; i += 256) {
      const int rr = i / kw, cc = i % kw;
      Lp[rr][cc] = cc < rr ? M[(size_t)(k0 + rr) * P6 + k0 + cc] : 0.0;
    }
    __syncthreads();
    if (tid < 64) {  // in-panel forward substitution in one wave
      double yv = lane < kw ? y[k0 + lane] : 0.0;
      for (int c = 0; c < kw; c++) {
        const double yc = __shfl(yv, c, 64);
        if (lane > c && lane < kw) yv -= Lp[lane][c] * yc;
      }
      if (lane < kw) y[k0 + lane] = yv;
    }
    __syncthreads();
    for (int row = k0 + kw + tid; row < P6; row += 256) {
      double acc = 0;
      for (int c = 0; c < kw; c++) acc += M[(size_t)row * P6 + k0 + c] * y[k0 + c];
      y[row] -= acc;
    }
  }
  __syncthreads();
  for (int i = tid; i < P6; i += 256) {
    const double d = M[(size_t)i * P6 + i];
    y[i] = d != 0 ? y[i] / d : 0.0;
  }
  for (int kb = nblk - 1; kb >= 0; kb--) {  // backward
    const int k0 = kb * BIG_NB, kw = min(BIG_NB, P6 - k0);
    __syncthreads();
    for (int i = tid; i < kw * kw; i += 256) {
      const int rr = i / kw, cc = i % kw;
      Lp[rr][cc] = cc < rr ? M[(size_t)(k0 + rr) * P6 + k0 + cc] : 0.0;
    }
    __syncthreads();
    if (tid < 64) {
      double xv = lane < kw ? y[k0 + lane] : 0.0;
      for (int c = kw - 1; c >= 0; c--) {
        const double xc = __shfl(xv, c, 64);
        if (lane < c) xv -= Lp[c][lane] * xc;
      }
      if (lane < kw) y[k0 + lane] = xv;
    }
    __syncthreads();
    for (int k = tid; k < k0; k += 256) {
      double acc = 0;
      for (int c = 0; c < kw; c++) acc += M[(size_t)(k0 + c) * P6 + k] * y[k0 + c];
      y[k] -= acc;
    }
  }
  __syncthreads();
  for (int i = tid; i < P6; i += 256) xp[i] = y[i];
}

// ---- host side of the HBM-resident path -----------------------------------------------------------------------------------
namespace {
struct BigSys {
  double *S = nullptr, *M = nullptr, *U = nullptr;  // S | r,  M | rhs,  the panel's L D: slots of the call's scratch block
  fb::DevBuf blkStart, blkPr, blkPc, entEr, entEc;
  BigLists lists{};
};

// (row key frame <= column key frame) -> the edge pairs of the landmarks both observe; counting sort by block.  Reads the
// HOST copy of the staged graph.
int big_prepare(BigSys &B, int np, int npt, const int *poseIdx, const int *e_kf, const int *lm_start, const int *lm_edges) {
  std::vector<int> cnt((size_t)np * np + 1, 0);
  auto for_pairs = [&](auto &&f) {
    for (int l = 0; l < npt; l++)
      for (int a = lm_start[l]; a < lm_start[l + 1]; a++) {
        const int pa = poseIdx[e_kf[lm_edges[a]]];
        if (pa < 0) continue;
        for (int b2 = a; b2 < lm_start[l + 1]; b2++) {
          const int pb = poseIdx[e_kf[lm_edges[b2]]];
          if (pb < 0) continue;
          if (pa <= pb) f(pa, pb, lm_edges[a], lm_edges[b2]);
          else f(pb, pa, lm_edges[b2], lm_edges[a]);
        }
      }
  };
  for_pairs([&](int pr, int pc, int, int) { cnt[(size_t)pr * np + pc + 1]++; });
  std::vector<int> blkStart(1, 0), blkPr, blkPc, slot((size_t)np * np, -1);
  for (size_t key = 0; key < (size_t)np * np; key++)
    if (cnt[key + 1] > 0) {
      slot[key] = (int)blkPr.size();
      blkPr.push_back((int)(key / np));
      blkPc.push_back((int)(key % np));
      blkStart.push_back(blkStart.back() + cnt[key + 1]);
    }
  std::vector<int> fillp(blkStart.begin(), blkStart.end() - 1), entEr(blkStart.back()), entEc(blkStart.back());
  for_pairs([&](int pr, int pc, int er, int ec) {
    const int q = fillp[slot[(size_t)pr * np + pc]]++;
    entEr[q] = er;
    entEc[q] = ec;
  });
  BA_UP(B.blkStart, blkStart); BA_UP(B.blkPr, blkPr); BA_UP(B.blkPc, blkPc); BA_UP(B.entEr, entEr); BA_UP(B.entEc, entEc);
  B.lists.nBlocks = (int)blkPr.size();
  B.lists.blk_start = B.blkStart.as<int>(); B.lists.blk_pr = B.blkPr.as<int>(); B.lists.blk_pc = B.blkPc.as<int>();
  B.lists.ent_er = B.entEr.as<int>(); B.lists.ent_ec = B.entEc.as<int>();
  return FB_OK;
}

// The Schur complement + solve part of a slot (the HBM-resident twin of k_ba_schur_c / k_ba_sumparts_c / k_ba_solve_c): at
// the accepted linearisation and lambda of BACtl, the pose increment lands in xp, the LDL^T status in *okFlag.  Sharded: the
// reduced system S | r is summed over the ranks on the stream (exchange 1).
int big_slot_solve(const BigSys &B, const BADev &D, const Lb2 &lb, const BACtl *ctl, const XBLay &xr, int P6, double *Dinv, double *xp, double *okFlag,
                   const Xchg &X, std::vector<double> &hostScratch, hipStream_t s0) {
  double *S = B.S, *rS = S + (size_t)P6 * P6, *M = B.M, *rhs = M + (size_t)P6 * P6;
  const size_t nS = (size_t)P6 * P6 + P6;
  { fb::ProfScope pr(fb::P_BA_SCHUR, s0);
    FB_HIP(hipMemsetAsync(S, 0, nS * 8, s0));  // blocks without a shared landmark stay 0
    if (D.npt > 0) k_ba_dinv<<<(D.npt + 255) / 256, 256, 0, s0>>>(D, lb, ctl, Dinv);
    if (B.lists.nBlocks > 0) k_ba_schur_gather<<<(B.lists.nBlocks + 3) / 4, 256, 0, s0>>>(D, lb, ctl, Dinv, B.lists, S, P6);
    if (D.np > 0) k_ba_rhs_gather<<<(D.np + 3) / 4, 256, 0, s0>>>(D, lb, ctl, Dinv, rS); }
  fb::ProfScope pr(fb::P_BA_SOLVE, s0);
  FB_TRY(X.sum_dev(S, nS, s0, hostScratch));
  k_big_assemble<<<(unsigned)(((long long)P6 * P6 + 255) / 256), 256, 0, s0>>>(lb, ctl, xr, S, rS, M, rhs, P6, okFlag);
  for (int k0 = 0; k0 < P6; k0 += BIG_NB) {
    const int kw = std::min(BIG_NB, P6 - k0);
    k_big_panel<<<1, 256, 0, s0>>>(ctl, M, P6, k0, kw, B.U, okFlag);
    const int nbt = (P6 - k0 - kw + BIG_NB - 1) / BIG_NB;
    if (nbt > 0) k_big_update<<<nbt * (nbt + 1) / 2, 256, 0, s0>>>(ctl, M, P6, k0, kw, B.U);
  }
  k_big_solve<<<1, 256, (size_t)P6 * 8, s0>>>(ctl, M, rhs, P6, xp);
  return FB_OK;
}
}  // namespace
