// ba_graph.inc -- the staged graph of a bundle adjustment (included by ba.hip): the argument agreement and the builders that
// fill the one block that travels to the device (GraphLayout in ba_plan.h): header,
// host builder (fb_local_ba & co.), k_bld_* + device builder (fb_local_ba_dev), odometry edges and their CSR.
namespace {

BADims dims_of(const fb_local_ba_args *A, int rank) {
  BADims d;
  d.odom = A->with_odom != 0;
  d.n_kf = A->n_kf; d.n_mp = A->n_mp; d.npt = A->n_mp + A->n_mpb;
  d.nF = A->n_obs; d.nB = d.odom ? A->n_bobs : 0; d.nE = d.nF + d.nB; d.nOAll = d.odom ? A->n_odom : 0; d.nO = rank == 0 ? d.nOAll : 0;
  d.np = 0;
  for (int k = 0; k < d.n_kf; k++) d.np += A->kf_fixed[k] ? 0 : 1;
  return d;
}

// ---- index predicates: the agreement block and the builder pass ask the same questions ------------------------------
inline bool obs_in_range(const fb_local_ba_args *A, int i) {
  return A->obs_mp[i] >= 0 && A->obs_mp[i] < A->n_mp && A->obs_kf[i] >= 0 && A->obs_kf[i] < A->n_kf;
}
inline bool bobs_in_range(const fb_local_ba_args *A, int i) {
  return A->bobs_mpb[i] >= 0 && A->bobs_mpb[i] < A->n_mpb && A->bobs_kf[i] >= 0 && A->bobs_kf[i] < A->n_kf;
}
inline bool odom_in_range(const fb_local_ba_args *A, int i) {
  return A->odom_kf_i[i] >= 0 && A->odom_kf_i[i] < A->n_kf && A->odom_kf_j[i] >= 0 && A->odom_kf_j[i] < A->n_kf;
}

// Sharded: a rank must not return alone on ITS argument error -- the others would wait for it in the first exchange.
// Every rank checks its arguments completely here (the builder asks the same predicates again, where they can no longer
// fail) and the verdict is reduced, so all ranks refuse together.
int agree_on_arguments(const fb_local_ba_args *A, int rank, const Xchg &X) {
  const bool argsOk = A && A->n_kf > 0 && A->n_mp >= 0 && A->n_mpb >= 0 && A->n_obs >= 0 && A->kf_Tcw && A->kf_fixed;
  if (!X.active()) {  // alone: the index checks ride in the building pass
    FB_ARG(argsOk);
    return FB_OK;
  }
  int bad = argsOk ? 0 : 1;
  if (!bad) {
    const bool od = A->with_odom != 0;
    int free = 0;
    for (int k = 0; k < A->n_kf; k++) free += A->kf_fixed[k] ? 0 : 1;
    if (6 * free > MAX_P6) bad = 1;
    std::vector<long long> pairs;
    pairs.reserve((size_t)A->n_obs + (od ? A->n_bobs : 0));
    for (int i = 0; i < A->n_obs && !bad; i++) {
      if (!obs_in_range(A, i)) bad = 1;
      else pairs.push_back(((long long)A->obs_mp[i] << 32) | (unsigned)A->obs_kf[i]);
    }
    for (int i = 0; od && i < A->n_bobs && !bad; i++) {
      if (!bobs_in_range(A, i)) bad = 1;
      else pairs.push_back(((long long)(A->n_mp + A->bobs_mpb[i]) << 32) | (unsigned)A->bobs_kf[i]);
    }
    for (int i = 0; od && rank == 0 && i < A->n_odom && !bad; i++)
      if (!odom_in_range(A, i)) bad = 1;
    if (!bad) {
      std::sort(pairs.begin(), pairs.end());
      if (std::adjacent_find(pairs.begin(), pairs.end()) != pairs.end()) bad = 1;
    }
  }
  double v = bad;
  FB_TRY(X.reduce_host(&v, 1, 1));
  if (v > 0.0) {
    fb::set_error(bad ? "fb_local_ba_sharded: bad arguments on this rank" : "fb_local_ba_sharded: another rank rejected its arguments");
    return FB_ERR_ARG;
  }
  return FB_OK;
}

void stage_header(const fb_local_ba_args *A, const BADims &d, const GraphLayout &G, uint8_t *hs, bool anything) {
  int *poseIdx = G.poseIdx.at(hs);
  for (int k = 0, free = 0; k < d.n_kf; k++) poseIdx[k] = A->kf_fixed[k] ? -1 : free++;
  memcpy(G.fixed.at(hs), A->kf_fixed, d.n_kf);
  // initial Levenberg-Marquardt control block + abort word of the device-resident schedule
  BACtl init;
  memset(&init, 0, sizeof(init));
  init.phase = anything ? 0 : 2;
  init.needInit = 1;
  memcpy(G.ctl.at(hs), &init, sizeof(init));
  const int abort0 = (A->stop_flag && *A->stop_flag) ? 1 : 0;  // sharded: raised before the call on this rank only
  memset(G.abort.at(hs), 0, 16);
  memcpy(G.abort.at(hs), &abort0, sizeof(int));
}

// One pass over the observations validates them, fills the per-edge arrays and counts the two CSR structures, a second
// one scatters.  (fb_local_ba from host pointers is a timed path: no separate validation pass.)
int build_graph_host(const fb_local_ba_args *A, const BADims &d, const GraphLayout &G, uint8_t *hs, bool sharded, int rank, int world) {
  const int n_kf = d.n_kf, n_mp = d.n_mp, npt = d.npt, np = d.np, nF = d.nF, nB = d.nB, nE = d.nE;
  const bool odom = d.odom;
  const int *poseIdx = G.poseIdx.at(hs);
  int *e_pt = G.e_pt.at(hs), *e_kf = G.e_kf.at(hs), *e_pj = G.e_pj.at(hs), *lm_start = G.lm_start.at(hs), *lm_edges = G.lm_edges.at(hs),
      *ps_start = G.ps_start.at(hs), *ps_edges = G.ps_edges.at(hs);
  uint8_t *e_type = G.e_type.at(hs), *e_level = G.e_level.at(hs);
  float *e_meas = G.e_meas.at(hs);
  double *e_info = G.e_info.at(hs), *pts = G.pts.at(hs);
  SE3 *poses = G.poses.at(hs);
  memcpy(G.kfT.at(hs), A->kf_Tcw, (size_t)n_kf * 48);
  for (int l = 0; l <= npt; l++) lm_start[l] = 0;
  for (int k = 0; k <= np; k++) ps_start[k] = 0;
  const double wFd = (double)A->wF, wBd = (double)A->wB;
  // Observations usually arrive grouped by point (the reference walks its local map points): then the CSR by landmark is
  // the edge order itself and the duplicate check (a key frame sees a point at most once) rides in this pass.
  static thread_local std::vector<int> seen;
  seen.assign(n_kf, -1);
  bool grouped = true, dup = false;
  int prevPt = -1;
  for (int i = 0; i < nF; i++) {
    FB_ARG(obs_in_range(A, i));
    const int pt = A->obs_mp[i], kf = A->obs_kf[i];
    grouped = grouped && pt >= prevPt;
    prevPt = pt;
    dup = dup || seen[kf] == pt;
    seen[kf] = pt;
    e_pt[i] = pt; e_kf[i] = kf; e_type[i] = T_PROJ;
    e_meas[3 * i] = A->obs_uv[2 * i]; e_meas[3 * i + 1] = A->obs_uv[2 * i + 1]; e_meas[3 * i + 2] = 0.0f;
    e_info[i] = odom ? (1.0 * (double)A->obs_inv_sigma2[i]) * wFd : (double)A->obs_inv_sigma2[i];
    e_level[i] = (sharded && pt % world != rank) ? 2 : 0;  // 2 = not this rank's landmark
    const int pj = poseIdx[kf];
    e_pj[i] = pj;
    lm_start[pt + 1]++;
    if (pj >= 0) ps_start[pj + 1]++;
  }
  for (int i = 0; i < nB; i++) {
    FB_ARG(bobs_in_range(A, i));
    const int e = nF + i, pt = n_mp + A->bobs_mpb[i], kf = A->bobs_kf[i];
    grouped = grouped && pt >= prevPt;
    prevPt = pt;
    dup = dup || seen[kf] == pt;
    seen[kf] = pt;
    e_pt[e] = pt; e_kf[e] = kf; e_type[e] = T_XYZ;
    for (int k = 0; k < 3; k++) e_meas[3 * e + k] = A->bobs_xc[3 * i + k];
    e_info[e] = (1.0 * (double)A->bobs_inv_sigma2[i]) * wBd;
    e_level[e] = (sharded && pt % world != rank) ? 2 : 0;
    const int pj = poseIdx[kf];
    e_pj[e] = pj;
    lm_start[pt + 1]++;
    if (pj >= 0) ps_start[pj + 1]++;
  }
  for (int l = 0; l < npt; l++) lm_start[l + 1] += lm_start[l];
  for (int k = 0; k < np; k++) ps_start[k + 1] += ps_start[k];
  static thread_local std::vector<int> fillL, fillP;
  fillP.assign(ps_start, ps_start + np);
  if (grouped) {
    for (int e = 0; e < nE; e++) {
      lm_edges[e] = e;
      if (e_pj[e] >= 0) ps_edges[fillP[e_pj[e]]++] = e;
    }
  } else {
    fillL.assign(lm_start, lm_start + npt);
    for (int e = 0; e < nE; e++) {
      lm_edges[fillL[e_pt[e]]++] = e;
      if (e_pj[e] >= 0) ps_edges[fillP[e_pj[e]]++] = e;
    }
    // a keyframe observes a point at most once (map<KeyFrame*,size_t>): stamp per key frame = last landmark seen
    dup = false;
    seen.assign(n_kf, -1);
    for (int l = 0; l < npt && !dup; l++)
      for (int c = lm_start[l]; c < lm_start[l + 1]; c++) {
        int &sk = seen[e_kf[lm_edges[c]]];
        dup = dup || sk == l;
        sk = l;
      }
  }
  if (dup) { fb::set_error("fb_local_ba: duplicate (keyframe, point) observation"); return FB_ERR_ARG; }
  for (int k = 0; k < n_kf; k++) poses[k] = fb::se3_from_float12(A->kf_Tcw + 12 * k);
  for (int i = 0; i < 3 * n_mp; i++) pts[i] = A->mp_xw[i];
  for (int i = 0; i < 3 * A->n_mpb; i++) pts[3 * n_mp + i] = A->mpb_xw[i];
  return FB_OK;
}

// the odometry edges and, per free pose, its incident edges in ascending edge index
int stage_odometry(const fb_local_ba_args *A, const BADims &d, const GraphLayout &G, uint8_t *hs) {
  const int *poseIdx = G.poseIdx.at(hs);
  int *o_i = G.o_i.at(hs), *o_j = G.o_j.at(hs), *od_start = G.od_start.at(hs), *od_edges = G.od_edges.at(hs);
  double *o_info = G.o_info.at(hs);
  SE3 *oZinv = G.o_Zinv.at(hs);
  for (int i = 0; i < d.nO; i++) {
    FB_ARG(odom_in_range(A, i));
    o_i[i] = A->odom_kf_i[i]; o_j[i] = A->odom_kf_j[i]; o_info[i] = A->odom_info[i];
    oZinv[i] = fb::se3_inverse(fb::se3_from_float12(A->odom_Tij + 12 * i));
  }
  std::vector<std::vector<int>> inc(d.np);
  for (int e = 0; e < d.nO; e++) {
    const int pi = poseIdx[o_i[e]], pj = poseIdx[o_j[e]];
    if (pi >= 0) inc[pi].push_back(e);
    if (pj >= 0 && pj != pi) inc[pj].push_back(e);
  }
  od_start[0] = 0;
  int q = 0;
  for (int k = 0; k < d.np; k++) { for (int e : inc[k]) od_edges[q++] = e; od_start[k + 1] = q; }
  return FB_OK;
}
}  // namespace

// ---- device-side graph builder (fb_local_ba_dev): what build_graph_host does, as kernels ---- ----------------------
namespace {
struct BuildIn {
  const int32_t *obs_kf, *obs_mp; const float *obs_uv, *obs_inv;
  const int32_t *bobs_kf, *bobs_mpb; const float *bobs_xc, *bobs_inv;
  const float *kf_Tcw, *mp_xw, *mpb_xw;
  int nF, nB, n_kf, n_mp, n_mpb, odom;
  double wF, wB;
};
// per edge: the flat edge record (Optimizer.cc:2346-2367, 2399-2414) + the counts of the two CSR structures
__global__ void k_bld_edges(BuildIn I, const int *poseIdx, int *e_pt, int *e_kf, int *e_pj, uint8_t *e_type, uint8_t *e_level,
                            float *e_meas, double *e_info, int *lm_cnt, int *ps_cnt, int *bad) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= I.nF + I.nB) return;
  int pt, kf;
  if (e < I.nF) {
    pt = I.obs_mp[e]; kf = I.obs_kf[e];
    if (!(pt >= 0 && pt < I.n_mp && kf >= 0 && kf < I.n_kf)) { atomicOr(bad, 1); pt = 0; kf = 0; }
    e_type[e] = T_PROJ;
    e_meas[3 * e] = I.obs_uv[2 * e]; e_meas[3 * e + 1] = I.obs_uv[2 * e + 1]; e_meas[3 * e + 2] = 0.0f;
    e_info[e] = I.odom ? (1.0 * (double)I.obs_inv[e]) * I.wF : (double)I.obs_inv[e];
  } else {
    const int i = e - I.nF;
    int pb = I.bobs_mpb[i];
    kf = I.bobs_kf[i];
    if (!(pb >= 0 && pb < I.n_mpb && kf >= 0 && kf < I.n_kf)) { atomicOr(bad, 1); pb = 0; kf = 0; }
    pt = I.n_mp + pb;
    e_type[e] = T_XYZ;
    for (int k = 0; k < 3; k++) e_meas[3 * e + k] = I.bobs_xc[3 * i + k];
    e_info[e] = (1.0 * (double)I.bobs_inv[i]) * I.wB;
  }
  e_pt[e] = pt; e_kf[e] = kf; e_level[e] = 0;
  const int pj = poseIdx[kf];
  e_pj[e] = pj;
  atomicAdd(&lm_cnt[pt + 1], 1);
  if (pj >= 0) atomicAdd(&ps_cnt[pj + 1], 1);
}
__global__ void k_bld_state(BuildIn I, SE3 *poses, double *pts, float *kfT) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < I.n_kf) {
    poses[i] = fb::se3_from_float12(I.kf_Tcw + 12 * i);
    for (int k = 0; k < 12; k++) kfT[12 * i + k] = I.kf_Tcw[12 * i + k];
  }
  if (i < 3 * I.n_mp) pts[i] = I.mp_xw[i];
  if (i < 3 * I.n_mpb) pts[3 * I.n_mp + i] = I.mpb_xw[i];
}
// in-place: cnt[0] = 0, cnt[i + 1] = count of bucket i  ->  exclusive starts; one workgroup, n up to millions
__global__ __launch_bounds__(1024) void k_bld_scan(int *cnt, int n, int *fill) {
  __shared__ int s_w[16], s_run;
  static_assert(sizeof(s_w) + sizeof(s_run) == STATIC_BLD_SCAN, "ba_plan.h states this kernel's static LDS");
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) s_run = 0;
  __syncthreads();
  for (int base = 0; base <= n; base += 1024) {
    const int i = base + tid;
    const int v = i <= n ? cnt[i] : 0;
    const int inc = fb::wave_incl_scan(v);
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    int off = s_run;
    for (int w = 0; w < wv; w++) off += s_w[w];
    const int incl = off + inc;
    if (i <= n) { cnt[i] = incl; if (fill && i < n) fill[i] = incl; }  // start of bucket i = inclusive sum up to cnt[i] (cnt[0] = 0)
    __syncthreads();
    if (tid == 1023) s_run = incl;
    __syncthreads();
  }
}
__global__ void k_bld_scatter(int nE, const int *e_pt, const int *e_pj, int *fillL, int *fillP, int *lm_edges, int *ps_edges) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nE) return;
  lm_edges[atomicAdd(&fillL[e_pt[e]], 1)] = e;
  if (e_pj[e] >= 0) ps_edges[atomicAdd(&fillP[e_pj[e]], 1)] = e;
}
// a landmark's edges in ascending edge index (the order the host builder produces: sums must not depend on the atomics'
// order) + a key frame observes a point at most once (map<KeyFrame*, size_t>)
__global__ void k_bld_sort_lm(int npt, const int *lm_start, int *lm_edges, const int *e_kf, int *bad) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= npt) return;
  const int a0 = lm_start[l], a1 = lm_start[l + 1];
  for (int i = a0 + 1; i < a1; i++) {
    const int v = lm_edges[i];
    int j = i - 1;
    while (j >= a0 && lm_edges[j] > v) { lm_edges[j + 1] = lm_edges[j]; j--; }
    lm_edges[j + 1] = v;
  }
  for (int i = a0; i < a1; i++)
    for (int j = i + 1; j < a1; j++)
      if (e_kf[lm_edges[i]] == e_kf[lm_edges[j]]) atomicOr(bad, 2);
}
// a key frame's edges in ascending edge index: bitonic sort of its segment in LDS (one workgroup per free key frame)
__global__ __launch_bounds__(1024) void k_bld_sort_ps(const int *ps_start, int *ps_edges, int cap, int *bad) {
  extern __shared__ int s_v[];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int a0 = ps_start[k], n = ps_start[k + 1] - a0;
  int m = 1;
  while (m < n) m <<= 1;
  if (m > cap) { if (tid == 0) atomicOr(bad, 4); return; }  // one key frame with more observations than the LDS sort holds
  for (int i = tid; i < m; i += 1024) s_v[i] = i < n ? ps_edges[a0 + i] : 0x7fffffff;
  __syncthreads();
  fb::bitonic_sort(s_v, m, tid, 1024);
  for (int i = tid; i < n; i += 1024) ps_edges[a0 + i] = s_v[i];
}
__global__ void k_bld_check(const int *bad, BACtl *c) {
  if (*bad) { c->badArgs = *bad; c->phase = 2; }
}
}  // namespace
namespace {
// fb_local_ba_dev: the big arrays of the arguments are device pointers; nothing of them is read on the host
int check_device_inputs(const fb_local_ba_args *A, const BADims &d) {
  FB_ARG(A->kf_Tcw && (d.n_mp == 0 || A->mp_xw) && (A->n_mpb == 0 || A->mpb_xw));
  FB_ARG(d.nF == 0 || (A->obs_kf && A->obs_mp && A->obs_uv && A->obs_inv_sigma2 && A->obs_outlier));
  FB_ARG(d.nB == 0 || (A->bobs_kf && A->bobs_mpb && A->bobs_xc && A->bobs_inv_sigma2 && A->bobs_outlier));
  return FB_OK;
}
// the builder's scratch: fill cursors of both CSR structures and the verdict word k_bld_check hands to the control block
int *builder_verdict(const fb::DevBuf &d_bld, const BADims &d) { return d_bld.as<int>() + d.npt + 1 + d.np + 1; }

// The edge records, both CSR structures and the double-precision state, built on stream s0 into the device block `dsb`
// from the caller's device arrays: the same contents as build_graph_host, incl. the ascending edge order inside a
// landmark / a key frame that the sums depend on.  The header (poseIdx) must have been enqueued before.
int build_graph_device(const fb_local_ba_args *A, const BADims &d, const GraphLayout &G, uint8_t *dsb, fb::DevBuf &d_bld, hipStream_t s0) {
  const int n_kf = d.n_kf, n_mp = d.n_mp, npt = d.npt, np = d.np, nE = d.nE;
  FB_TRY(d_bld.alloc(((size_t)npt + np + 2) * 4 + 16));
  int *fillL = d_bld.as<int>(), *fillP = fillL + npt + 1, *badDev = builder_verdict(d_bld, d);
  FB_HIP(hipMemsetAsync(G.lm_start.at(dsb), 0, G.e_pt.off - G.lm_start.off, s0));   // lm_start | ps_start (counts accumulate into them)
  FB_HIP(hipMemsetAsync(d_bld.p, 0, d_bld.bytes, s0));
  BuildIn I;
  I.obs_kf = A->obs_kf; I.obs_mp = A->obs_mp; I.obs_uv = A->obs_uv; I.obs_inv = A->obs_inv_sigma2;
  I.bobs_kf = A->bobs_kf; I.bobs_mpb = A->bobs_mpb; I.bobs_xc = A->bobs_xc; I.bobs_inv = A->bobs_inv_sigma2;
  I.kf_Tcw = A->kf_Tcw; I.mp_xw = A->mp_xw; I.mpb_xw = A->mpb_xw;
  I.nF = d.nF; I.nB = d.nB; I.n_kf = n_kf; I.n_mp = n_mp; I.n_mpb = A->n_mpb; I.odom = d.odom ? 1 : 0; I.wF = (double)A->wF; I.wB = (double)A->wB;
  int *dlms = G.lm_start.at(dsb), *dpss = G.ps_start.at(dsb), *dept = G.e_pt.at(dsb), *dekf = G.e_kf.at(dsb), *depj = G.e_pj.at(dsb),
      *dlme = G.lm_edges.at(dsb), *dpse = G.ps_edges.at(dsb);
  int segCap = 1;
  while (segCap < std::max(nE, 1) && segCap < 32768) segCap <<= 1;  // observations of ONE key frame: at most 32768 (128 KB of LDS)
  fb::ProfScope pr(fb::P_BA_MISC, s0);
  if (nE > 0) k_bld_edges<<<(nE + 255) / 256, 256, 0, s0>>>(I, G.poseIdx.at(dsb), dept, dekf, depj, G.e_type.at(dsb), G.e_level.at(dsb), G.e_meas.at(dsb),
                                                          G.e_info.at(dsb), dlms, dpss, badDev);
  k_bld_state<<<(std::max(n_kf, 3 * std::max(n_mp, A->n_mpb)) + 255) / 256, 256, 0, s0>>>(I, G.poses.at(dsb), G.pts.at(dsb), G.kfT.at(dsb));
  k_bld_scan<<<1, 1024, 0, s0>>>(dlms, npt, fillL);
  k_bld_scan<<<1, 1024, 0, s0>>>(dpss, np, fillP);
  if (nE > 0) {
    k_bld_scatter<<<(nE + 255) / 256, 256, 0, s0>>>(nE, dept, depj, fillL, fillP, dlme, dpse);
    k_bld_sort_lm<<<(npt + 255) / 256, 256, 0, s0>>>(npt, dlms, dlme, dekf, badDev);
    if (np > 0) {
      FB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_bld_sort_ps), hipFuncAttributeMaxDynamicSharedMemorySize, segCap * 4));
      k_bld_sort_ps<<<np, 1024, (size_t)segCap * 4, s0>>>(dpss, dpse, segCap, badDev);
    }
  }
  FB_HIP(hipGetLastError());
  return FB_OK;
}
}  // namespace
