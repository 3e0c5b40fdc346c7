// ba_driver.inc -- the host driver of every bundle adjustment entry point (included by ba.hip).  local_ba_impl is the table of
// contents: agreement -> plan -> stage/build -> bind -> the device-resident Levenberg-Marquardt schedule -> results.
// Everything a call owns sits in one BACtx; the stages are free functions over it.  Every size, LDS byte count and path choice
// comes from plan() of ba_plan.h; a call owns three device blocks: the staged graph, the device builder's cursors, the scratch.
struct DevIn { hipStream_t stream = nullptr; };  // fb_local_ba_dev: the big arrays of fb_local_ba_args are DEVICE pointers

// per host thread and device: the side stream for the abort request (does not synchronise with the null stream), the pinned
// mirror of the control block and the event the host waits on (concurrent callers must not share them; a stream belongs
// to its device).  fb_shutdown releases the calling thread's set through fb::ba_release_thread.
struct PerDev { hipStream_t sAux = nullptr; BACtl *hCtl = nullptr; hipEvent_t evDone = nullptr; };
static thread_local PerDev g_perDev[64];

namespace fb {
void ba_release_thread() {
  int cur = 0;
  const bool have = hipGetDevice(&cur) == hipSuccess;
  for (int d = 0; d < 64; d++) {
    PerDev &pd = g_perDev[d];
    if (!pd.sAux && !pd.hCtl && !pd.evDone) continue;
    if (hipSetDevice(d) != hipSuccess) continue;
    if (pd.evDone) (void)hipEventDestroy(pd.evDone);
    if (pd.hCtl) (void)hipHostFree(pd.hCtl);
    if (pd.sAux) (void)hipStreamDestroy(pd.sAux);
    pd = PerDev();
  }
  if (have) (void)hipSetDevice(cur);
}
}  // namespace fb

namespace {

struct BAEnv {  // what the environment says about a call, read once beside the plan
  int nwgCap;          // FB_BA_NWG: the most workgroups of k_ba_schur_c (256)
  bool timing, trace;  // FB_BA_TIMING (host-side phase times on stderr), FB_BA_TRACE (one line per slot; implies paced)
  bool paced;          // FB_BA_HOST_LM: one slot per batch, the control block read back after each
};
BAEnv read_env() {
  BAEnv e;
  const char *nwg = getenv("FB_BA_NWG");
  e.nwgCap = std::max(1, nwg ? atoi(nwg) : 256);
  e.timing = getenv("FB_BA_TIMING") != nullptr;
  e.trace = getenv("FB_BA_TRACE") != nullptr;
  e.paced = e.trace || getenv("FB_BA_HOST_LM") != nullptr;
  return e;
}

// Once work has been enqueued on the call's stream, a return that has not waited for it must do so before the device
// blocks go back to the pool: fb::pool_give does not synchronise and another host thread may be handed the block.
struct StreamDrain {
  hipStream_t stream = nullptr;
  bool pending = false;
  void arm(hipStream_t s) { stream = s; pending = true; }
  void done() { pending = false; }  // the caller has just seen the stream idle
  ~StreamDrain() {
    if (pending) { (void)hipStreamSynchronize(stream); (void)hipGetLastError(); }
  }
};

struct BACtx {  // one call
  const fb_local_ba_args *A;
  const Xchg &X;
  const BASched sc;
  const double delta;  // Huber delta: sqrt(5.991) local (Optimizer.cc:2290), sqrt(5.99) global (:1836)
  hipStream_t s0;
  std::chrono::steady_clock::time_point tStart;
  const BAEnv env = read_env();
  BAPlan P;
  GraphLayout G;
  ScratchLayout C;
  uint8_t *hs = nullptr;  // host copy of the staged graph (device input: only its header is filled)
  fb::DevBuf d_stage, d_bld, d_scratch;  // device blocks; they return to the pool when the context goes
  BigSys bigSys;
  BADev D;
  St2 st2;
  Lb2 lb2;
  StreamDrain drain;  // LAST member: destroyed first, before any block above is given back
  BACtx(const fb_local_ba_args *a, const Xchg &x, const BASched &s, double dl, hipStream_t st)
      : A(a), X(x), sc(s), delta(dl), s0(st), tStart(std::chrono::steady_clock::now()) {}
  uint8_t *ds() const { return d_stage.as<uint8_t>(); }
  uint8_t *dc() const { return d_scratch.as<uint8_t>(); }
  BACtl *ctl() const { return G.ctl.at(ds()); }
  int *abortWord() const { return G.abort.at(ds()); }
  void lap(const char *what) const {
    if (env.timing) fprintf(stderr, "[fb_local_ba] %-28s %8.1f us\n", what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tStart).count());
  }
};

int make_plan(BACtx &c, int rank, bool devIn) {
  const BADims d = dims_of(c.A, rank);
  if (6 * d.np > MAX_P6) { fb::set_error("fb_local_ba: more than %d free keyframes", MAX_P6 / 6); return FB_ERR_CAPACITY; }
  c.P = plan(d, c.X.active(), devIn, rank, c.X.world, c.env.nwgCap);
  if (devIn && c.P.big) { fb::set_error("fb_local_ba_dev: more than %d free key frames (use fb_local_ba)", MAX_FREE_KF_LDS); return FB_ERR_CAPACITY; }
  return FB_OK;
}

// ---- stage / build: the graph on the host, then on the device ---------------------------------------------------------------
int stage_graph(BACtx &c) {
  const BADims &d = c.P.d;
  if (c.P.devIn) FB_TRY(check_device_inputs(c.A, d));  // every argument check of the device path precedes its first enqueue
  static thread_local std::vector<uint8_t> stage;
  c.G = graph_layout(d);
  if (stage.size() < c.G.bytes) stage.resize(c.G.bytes);
  c.hs = stage.data();
  stage_header(c.A, d, c.G, c.hs, c.P.anything);
  if (!c.P.devIn) FB_TRY(build_graph_host(c.A, d, c.G, c.hs, c.P.sharded, c.P.rank, c.P.world));
  FB_TRY(stage_odometry(c.A, d, c.G, c.hs));
  c.lap("host preprocessing done");
  if (!c.P.devIn) {
    FB_TRY(c.d_stage.upload(c.hs, c.G.bytes));
  } else {  // only the header travels
    FB_TRY(c.d_stage.alloc(c.G.bytes));
    c.drain.arm(c.s0);
    FB_HIP(hipMemcpyAsync(c.d_stage.p, c.hs, c.G.headerBytes, hipMemcpyHostToDevice, c.s0));
    FB_TRY(build_graph_device(c.A, d, c.G, c.ds(), c.d_bld, c.s0));
  }
  c.lap("graph uploaded");
  return FB_OK;
}

// ---- bind: the scratch block and the pointer structs the kernels take -------------------------------------------------------
int bind_device(BACtx &c) {
  const BAPlan &P = c.P;
  const BADims &d = P.d;
  const GraphLayout &G = c.G;
  const ScratchLayout &C = c.C = scratch_layout(P);
  FB_TRY(c.d_scratch.alloc(C.bytes));
  uint8_t *ds = c.ds(), *dc = c.dc();
  if (P.big) {
    FB_TRY(big_prepare(c.bigSys, d.np, d.npt, G.poseIdx.at(c.hs), G.e_kf.at(c.hs), G.lm_start.at(c.hs), G.lm_edges.at(c.hs)));
    c.bigSys.S = C.bigS.at(dc); c.bigSys.M = C.bigM.at(dc); c.bigSys.U = C.bigU.at(dc);
  }
  BADev &D = c.D;
  D.n_kf = d.n_kf; D.np = d.np; D.npt = d.npt; D.nE = d.nE; D.nO = d.nO; D.quat = d.odom ? 1 : 0;
  D.fx = c.A->fx; D.fy = c.A->fy; D.cx = c.A->cx; D.cy = c.A->cy; D.delta = c.delta;
  D.poseIdx = G.poseIdx.at(ds); D.e_pt = G.e_pt.at(ds); D.e_kf = G.e_kf.at(ds); D.e_pj = G.e_pj.at(ds);
  D.e_type = G.e_type.at(ds); D.e_meas = G.e_meas.at(ds); D.e_info = G.e_info.at(ds);
  D.e_level = G.e_level.at(ds); D.e_chi2 = C.e_chi2.at(dc);
  D.lm_start = G.lm_start.at(ds); D.lm_edges = G.lm_edges.at(ds);
  D.ps_start = G.ps_start.at(ds); D.ps_edges = G.ps_edges.at(ds);
  D.o_i = G.o_i.at(ds); D.o_j = G.o_j.at(ds); D.o_Zinv = G.o_Zinv.at(ds); D.o_info = G.o_info.at(ds);
  D.od_start = G.od_start.at(ds); D.od_edges = G.od_edges.at(ds);
  // state 0 = the staged copy, state 1 starts as the same poses / points (dev_lm_prepare copies them)
  c.st2.s[0].pose = G.poses.at(ds); c.st2.s[0].pt = G.pts.at(ds);
  c.st2.s[1].pose = C.pose1.at(dc); c.st2.s[1].pt = C.pt1.at(dc);
  for (int q = 0; q < 2; q++) {
    LinBuf &b = c.lb2.b[q];
    b.Hll = C.lin[q].Hll.at(dc); b.bl = C.lin[q].bl.at(dc); b.W = C.lin[q].W.at(dc);
    b.Hpp = C.lin[q].Hpp.at(dc); b.bp = C.lin[q].bp.at(dc); b.chiPart = C.lin[q].chiPart.at(dc); b.maxPart = C.lin[q].maxPart.at(dc);
  }
  return FB_OK;
}

// ---- results ------------------------------------------------------------------------------------------------------------------
struct HostResult { std::vector<uint8_t> flags; std::vector<float> po; };
int fetch_results(BACtx &c, HostResult &r) {
  r.flags.resize(std::max(c.P.d.nE, 1));
  FB_HIP(hipMemcpy(r.flags.data(), c.C.flags.at(c.dc()), std::max(c.P.d.nE, 1), hipMemcpyDeviceToHost));
  r.po.resize((size_t)std::max(c.P.d.npt, 1) * 3);
  if (c.P.d.npt > 0) FB_HIP(hipMemcpy(r.po.data(), c.C.ptOut.at(c.dc()), (size_t)c.P.d.npt * 12, hipMemcpyDeviceToHost));
  return FB_OK;
}
// the one place where a BA writes into the caller's host arrays
int results_to_host(BACtx &c, const HostResult &r) {
  const fb_local_ba_args *A = c.A;
  const BADims &d = c.P.d;
  if (c.sc.gate) {  // the global BA classifies nothing
    for (int i = 0; i < d.nF; i++) A->obs_outlier[i] = r.flags[i];
    for (int i = 0; i < d.nB; i++) A->bobs_outlier[i] = r.flags[d.nF + i];
  }
  FB_HIP(hipMemcpy(A->kf_Tcw, c.C.kfT.at(c.dc()), (size_t)d.n_kf * 48, hipMemcpyDeviceToHost));
  for (int i = 0; i < 3 * d.n_mp; i++) A->mp_xw[i] = r.po[i];
  for (int i = 0; i < 3 * A->n_mpb; i++) A->mpb_xw[i] = r.po[3 * d.n_mp + i];
  return FB_OK;
}
int results_to_device(BACtx &c) {
  const fb_local_ba_args *A = c.A;
  const BADims &d = c.P.d;
  hipStream_t s0 = c.s0;
  const uint8_t *flags = c.C.flags.at(c.dc());
  const float *ptOut = c.C.ptOut.at(c.dc());
  if (c.sc.gate) {
    if (d.nF > 0) FB_HIP(hipMemcpyAsync(A->obs_outlier, flags, (size_t)d.nF, hipMemcpyDeviceToDevice, s0));
    if (d.nB > 0) FB_HIP(hipMemcpyAsync(A->bobs_outlier, flags + d.nF, (size_t)d.nB, hipMemcpyDeviceToDevice, s0));
  }
  FB_HIP(hipMemcpyAsync(A->kf_Tcw, c.C.kfT.at(c.dc()), (size_t)d.n_kf * 48, hipMemcpyDeviceToDevice, s0));
  if (d.n_mp > 0) FB_HIP(hipMemcpyAsync(A->mp_xw, ptOut, (size_t)d.n_mp * 12, hipMemcpyDeviceToDevice, s0));
  if (A->n_mpb > 0) FB_HIP(hipMemcpyAsync(A->mpb_xw, ptOut + (size_t)3 * d.n_mp, (size_t)A->n_mpb * 12, hipMemcpyDeviceToDevice, s0));
  FB_HIP(hipStreamSynchronize(s0));  // the scratch goes back to the pool when the call returns
  c.drain.done();
  return FB_OK;
}

// ---- device-resident Levenberg-Marquardt: no read-back inside a batch of slots.  Sharded: two all-reduces per slot on this
//      stream (the Schur-reduced system; the exchange block of the linearisation), every rank enqueues the same slots and
//      takes the same decisions from the reduced values.
using SchurKernel = void (*)(BADev, Lb2, const BACtl *, double *, double *, int, int, int);
struct DevLm {
  PerDev *pd = nullptr;
  SchurKernel schurC = nullptr;
  XBLay xb, xr;              // raw and reduced exchange blocks (the same unless sharded)
  double *Dinv, *Spart, *xp, *scale, *okFlag;
  OdomLin *ol;               // the odometry records on the HBM route, else null
  std::vector<double> hostScratch;
  int rcSlot = FB_OK;
};

int per_device(PerDev *&out) {
  int devId = 0;
  FB_HIP(hipGetDevice(&devId));
  if (devId < 0 || devId >= 64) { fb::set_error("fb_local_ba: device id %d", devId); return FB_ERR_NODEVICE; }
  PerDev &pd = g_perDev[devId];
  if (!pd.sAux) FB_HIP(hipStreamCreateWithFlags(&pd.sAux, hipStreamNonBlocking));
  if (!pd.hCtl) FB_HIP(hipHostMalloc(reinterpret_cast<void **>(&pd.hCtl), sizeof(BACtl), hipHostMallocDefault));
  if (!pd.evDone) FB_HIP(hipEventCreateWithFlags(&pd.evDone, hipEventDisableTiming));
  out = &pd;
  return FB_OK;
}
// every kernel of this call whose dynamic LDS may exceed the 64 KiB default, with the bytes its launch will ask for
template <typename K> int allow_lds(K kernel, size_t bytes) {
  FB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return FB_OK;
}
int opt_in_lds(const BAPlan &P, SchurKernel schurC) {
  if (P.big) return allow_lds(k_big_solve, (size_t)P.P6 * 8);
  FB_TRY(allow_lds(schurC, P.schurLds));
  FB_TRY(allow_lds(k_ba_solve_c, P.solveLds));
  return P.odomHome == ODOM_LDS ? allow_lds(k_ba_lin_c<false>, P.linLds) : FB_OK;
}

// the per-device objects, the LDS opt-ins, the copies and memsets the schedule starts from
int dev_lm_prepare(BACtx &c, DevLm &L) {
  const BAPlan &P = c.P;
  const BADims &d = P.d;
  const GraphLayout &G = c.G;
  const ScratchLayout &C = c.C;
  uint8_t *ds = c.ds(), *dc = c.dc();
  hipStream_t s0 = c.s0;
  FB_TRY(per_device(L.pd));
  L.schurC = P.schur == SCHUR_T9 ? k_ba_schur_c<schur_maxt(SCHUR_T9)> : k_ba_schur_c<schur_maxt(SCHUR_T20)>;
  FB_TRY(opt_in_lds(P, L.schurC));
  L.Dinv = C.Dinv.at(dc); L.Spart = C.Spart.at(dc); L.xp = C.xp.at(dc); L.scale = C.scale.at(dc); L.okFlag = C.ok.at(dc);
  L.ol = P.odomHome == ODOM_HBM ? C.ol.at(dc) : nullptr;
  // sharded: the kernels of a linearisation fill the RAW blocks; exchange 2 sums BOTH raw blocks into the REDUCED ones out of
  // place (which of the two the slot wrote is device-side knowledge; the raw block of the accepted linearisation is not
  // touched until it is overwritten, so re-reducing it is idempotent); k_ba_control and the solve read the reduced blocks.
  L.xb = P.xb;
  L.xb.base = C.xb.at(dc);
  L.xr = L.xb;
  if (P.sharded) L.xr.base = L.xb.base + (size_t)2 * L.xb.stride;
  c.drain.arm(s0);
  if (P.devIn) {  // a rejected graph (index out of range, duplicate observation) ends the schedule before it starts
    k_bld_check<<<1, 1, 0, s0>>>(builder_verdict(c.d_bld, d), c.ctl());
    FB_HIP(hipGetLastError());
  }
  // what the kernels rely on (ScratchLayout in ba_plan.h): e_chi2, the first partial of Spart, the exchange blocks
  FB_HIP(hipMemsetAsync(C.e_chi2.at(dc), 0, (size_t)std::max(d.nE, 1) * 8, s0));
  if (!P.big) FB_HIP(hipMemsetAsync(L.Spart, 0, (size_t)P.nS * 8, s0));
  FB_HIP(hipMemsetAsync(L.xb.base, 0, (size_t)(P.sharded ? 4 : 2) * L.xb.stride * 8, s0));
  FB_HIP(hipMemcpyAsync(C.pose1.at(dc), G.poses.at(ds), (size_t)d.n_kf * sizeof(SE3), hipMemcpyDeviceToDevice, s0));
  FB_HIP(hipMemcpyAsync(C.pt1.at(dc), G.pts.at(ds), (size_t)std::max(d.npt, 1) * 24, hipMemcpyDeviceToDevice, s0));
  FB_HIP(hipMemcpyAsync(C.kfT.at(dc), G.kfT.at(ds), (size_t)d.n_kf * 48, hipMemcpyDeviceToDevice, s0));
  return FB_OK;
}

// one slot: a trial (or the opening linearisation) and the decision of k_ba_control
void dev_lm_slot(BACtx &c, DevLm &L) {
  if (L.rcSlot != FB_OK) return;
  const BAPlan &P = c.P;
  const BADev &D = c.D;
  const Lb2 &lb2 = c.lb2;
  hipStream_t s0 = c.s0;
  BACtl *ctl = c.ctl();
  int *d_abort = c.abortWord();
  const int nLin256 = P.nLin256;
  if (P.big) {
    L.rcSlot = big_slot_solve(c.bigSys, D, lb2, ctl, L.xr, P.P6, L.Dinv, L.xp, L.okFlag, c.X, L.hostScratch, s0);
  } else {
    { fb::ProfScope pr(fb::P_BA_SCHUR, s0);
      L.schurC<<<P.nWg, SCHUR_THREADS, P.schurLds, s0>>>(D, lb2, ctl, L.Dinv, L.Spart, P.P6, P.NT, P.lmPerWg); }
    fb::ProfScope pr(fb::P_BA_SOLVE, s0);
    k_ba_sumparts_c<<<(P.nS + SUMPARTS_ELEMS - 1) / SUMPARTS_ELEMS, 256, 0, s0>>>(ctl, L.Spart, P.nWg, P.nS, P.rows);
    if (P.sharded) L.rcSlot = c.X.sum_dev(L.Spart, (size_t)P.nS, s0, L.hostScratch);  // exchange 1: the Schur-reduced system
    k_ba_solve_c<<<1, SOLVE_C_THREADS, P.solveLds, s0>>>(lb2, ctl, L.Spart, P.P6, P.NT, L.xp, L.okFlag, L.xr);
  }
  { fb::ProfScope pr(fb::P_BA_UPDATE, s0);
    k_ba_update_c<<<P.nUpdBlocks, LIN_THREADS, 0, s0>>>(D, lb2, c.st2, ctl, L.Dinv, L.xp, L.scale, P.rank == 0 ? 1 : 0); }
  { fb::ProfScope pr(fb::P_BA_LINEARIZE, s0);
    if (L.ol) k_ba_lin_c<true><<<P.linGrid, LIN_C_THREADS, 0, s0>>>(D, c.st2, lb2, ctl, c.sc, P.P6, nLin256, nLin256, L.ol, L.xb);
    else k_ba_lin_c<false><<<P.linGrid, LIN_C_THREADS, P.linLds, s0>>>(D, c.st2, lb2, ctl, c.sc, P.P6, nLin256, nLin256, nullptr, L.xb); }
  { fb::ProfScope pr(fb::P_BA_MISC, s0);
    if (P.sharded) {
      k_ba_prex<<<1, 256, 0, s0>>>(D, lb2, ctl, nLin256, nLin256, L.scale, P.nUpdBlocks, L.xb, d_abort, P.rank, P.world);
      // exchange 2: both raw blocks -> the reduced blocks, one all-reduce
      if (L.rcSlot == FB_OK) L.rcSlot = c.X.sum_dev(L.xr.at(0), (size_t)2 * L.xb.stride, s0, L.hostScratch, L.xb.at(0));
      k_ba_control<true><<<1, 256, 0, s0>>>(D, lb2, ctl, c.sc, nLin256, nLin256, L.scale, P.nUpdBlocks, L.okFlag, P.P6, L.xr, d_abort, P.world);
    } else {
      k_ba_control<false><<<1, 256, 0, s0>>>(D, lb2, ctl, c.sc, nLin256, nLin256, L.scale, P.nUpdBlocks, L.okFlag, P.P6, L.xb, d_abort, P.world);
    } }
}

// the results of the state that is current now (final when the schedule has finished, which is the common case) and the
// control block into its pinned mirror, the event behind them
int dev_lm_export(BACtx &c, DevLm &L) {
  const BAPlan &P = c.P;
  const int n_kf = P.d.n_kf, npt = P.d.npt, nE = P.d.nE;
  hipStream_t s0 = c.s0;
  BACtl *ctl = c.ctl();
  uint8_t *flags = c.C.flags.at(c.dc());
  float *ptOut = c.C.ptOut.at(c.dc());
  double *ex = c.C.ex.at(c.dc());
  if (nE > 0) k_ba_gate_final_c<<<(nE + 255) / 256, 256, 0, s0>>>(c.D, c.st2, ctl, flags);
  k_ba_export_c<<<(n_kf + npt * 3 + 255) / 256, 256, 0, s0>>>(n_kf, npt, c.st2, ctl, c.G.fixed.at(c.ds()), c.C.kfT.at(c.dc()), ptOut);
  if (P.sharded) {  // every rank returns the complete result
    const int nx = npt * 3 + nE;
    k_ba_final_pack<<<(nx + 255) / 256, 256, 0, s0>>>(npt, nE, P.rank, P.world, ptOut, flags, ex);
    FB_TRY(c.X.sum_dev(ex, (size_t)nx, s0, L.hostScratch));
    k_ba_final_unpack<<<(nx + 255) / 256, 256, 0, s0>>>(npt, nE, ex, ptOut, flags);
  }
  if (hipGetLastError() != hipSuccess) { fb::set_error("fb_local_ba: kernel launch failed"); return FB_ERR_HIP; }
  if (hipMemcpyAsync(L.pd->hCtl, ctl, sizeof(BACtl), hipMemcpyDeviceToHost, s0) != hipSuccess || hipEventRecord(L.pd->evDone, s0) != hipSuccess) {
    fb::set_error("fb_local_ba: control block read-back failed");
    return FB_ERR_HIP;
  }
  return FB_OK;
}

// wait for the event; meanwhile forward pbStopFlag (the control kernel sees it at the end of the slot that is running)
int dev_lm_wait(BACtx &c, DevLm &L, bool &abortSent) {
  static const int one = 1;
  const fb_local_ba_args *A = c.A;
  if (!A->stop_flag) {  // nothing to forward: block in the driver instead of holding a host core
    const hipError_t q = hipEventSynchronize(L.pd->evDone);
    if (q != hipSuccess) { fb::set_error("fb_local_ba: %s", hipGetErrorString(q)); return FB_ERR_HIP; }
    return FB_OK;
  }
  for (;;) {
    const hipError_t q = hipEventQuery(L.pd->evDone);
    if (q == hipSuccess) return FB_OK;
    if (q != hipErrorNotReady) { fb::set_error("fb_local_ba: %s", hipGetErrorString(q)); return FB_ERR_HIP; }
    if (!abortSent && *A->stop_flag) {
      (void)hipMemcpyAsync(c.abortWord(), &one, sizeof(int), hipMemcpyHostToDevice, L.pd->sAux);
      abortSent = true;
    }
    // a BA lasts milliseconds and the flag only has to reach the device before the running slot (~0.1 ms) ends:
    // poll every 20 us instead of spinning on the LocalMapping thread's core
    std::this_thread::sleep_for(std::chrono::microseconds(20));
  }
}

// FB_BA_TRACE: the slot that took the control block from `was` to `now`, in the format of the oracle's trace (se3_oracle.h)
void trace_slot(const BACtl &was, const BACtl &now, const BASched &sc) {
  if (was.phase == 2 || now.badArgs) return;  // the slot did nothing
  if (was.needInit) fprintf(stderr, "[hip] optimize(%d) chi0=%.17g maxDiag=%.17g\n", was.phase == 0 ? sc.its1 : sc.its2, now.trChi, now.trScale);
  else fprintf(stderr, "[hip]  it=%d q=%d lambda=%.17g tempChi=%.17g scale=%.17g rho=%.17g ok=%d\n", was.it, was.qmax, was.lambda, now.trChi, now.trScale,
               now.trRho, now.trChi != 1.7976931348623157e308 ? 1 : 0);
}

int run_device_lm(BACtx &c) {
  const BASched &sc = c.sc;
  DevLm L;
  FB_TRY(dev_lm_prepare(c, L));
  bool abortSent = false;
  // Paced (FB_BA_HOST_LM, FB_BA_TRACE): the host looks at the control block after every slot
  int batch = c.P.anything ? first_batch(sc) : 0;
  if (c.env.paced) batch = std::min(batch, 1);
  const int maxSlots = max_slots(sc);
  c.lap("buffers ready");
  const BACtl *hCtl = L.pd->hCtl;
  BACtl was = *c.G.ctl.at(c.hs);
  for (int enqueued = 0;;) {
    for (int i = 0; i < batch; i++) dev_lm_slot(c, L);
    enqueued += batch;
    FB_TRY(L.rcSlot);
    c.lap("slots enqueued");
    FB_TRY(dev_lm_export(c, L));
    FB_TRY(dev_lm_wait(c, L, abortSent));
    if (c.env.trace) trace_slot(was, *hCtl, sc);
    was = *hCtl;
    if (hCtl->phase == 2 || enqueued >= maxSlots) break;
    batch = c.env.paced ? 1 : 6;
  }
  c.drain.done();  // the event was the last thing on the stream
  c.lap("schedule finished");
  if (hCtl->phase != 2) { fb::set_error("fb_local_ba: the LM schedule did not finish"); return FB_ERR_HIP; }
  if (c.P.devIn) {
    if (hCtl->badArgs & 4) { fb::set_error("fb_local_ba_dev: a key frame with more than 32768 observations (use fb_local_ba)"); return FB_ERR_CAPACITY; }
    if (hCtl->badArgs) {
      fb::set_error(hCtl->badArgs & 1 ? "fb_local_ba_dev: observation index out of range" : "fb_local_ba_dev: duplicate (keyframe, point) observation");
      return FB_ERR_ARG;
    }
    c.drain.arm(c.s0);
    FB_TRY(results_to_device(c));
    c.lap("results copied (device)");
    return FB_OK;
  }
  HostResult r;
  FB_TRY(fetch_results(c, r));
  FB_TRY(results_to_host(c, r));
  c.lap("results copied out");
  return FB_OK;
}

}  // namespace

static int local_ba_impl(const fb_local_ba_args *A, int rank, const Xchg &X, const BASched &sc, double delta, const DevIn *dv = nullptr) {
  FB_TRY(fb::check_device());
  const bool devIn = dv != nullptr;  // observations / poses / points / result arrays live in HBM (fb_local_ba_dev)
  BACtx c(A, X, sc, delta, devIn ? dv->stream : nullptr);
  FB_ARG(!(devIn && X.active()));
  FB_TRY(agree_on_arguments(A, rank, X));
  // Optimizer.cc:902-906 / 2498-2500.  Sharded: a rank must not leave on its OWN view of the flag (the others would wait for
  // it in the first exchange): every stop decision of the schedule goes through a reduction
  if (!X.active() && A->stop_flag && *A->stop_flag) return FB_OK;
  FB_TRY(make_plan(c, rank, devIn));
  FB_TRY(stage_graph(c));
  FB_TRY(bind_device(c));
  return run_device_lm(c);
}

static const BASched kLocalSchedule = {5, 1, 1, 10};
static const double kLocalDelta = (double)(float)sqrt(5.991);

extern "C" int fb_local_ba(const fb_local_ba_args *A) { return local_ba_impl(A, 0, Xchg(), kLocalSchedule, kLocalDelta); }
extern "C" int fb_local_ba_dev(const fb_local_ba_args *A, void *stream) {
  DevIn dv;
  dv.stream = fb::as_stream(stream);
  return local_ba_impl(A, 0, Xchg(), kLocalSchedule, kLocalDelta, &dv);
}

extern "C" int fb_global_ba(const fb_local_ba_args *A, int n_iterations, int robust) {
  FB_ARG(n_iterations >= 0);
  const BASched sc = {n_iterations, robust ? 1 : 0, 0, 0};
  return local_ba_impl(A, 0, Xchg(), sc, (double)(float)sqrt(5.99));
}

// Landmark-partitioned BA (SURVEY 8e): rank r owns the landmarks l with l % world == r and all their edges, the
// odometry edges live on rank 0, the keyframe state is replicated.  Per LM trial two small all-reduces: the
// Schur-reduced system (after k_ba_schur_c / the gathers of ba_big.inc) and the exchange block (after the linearisation at the trial state).
extern "C" int fb_local_ba_sharded(const fb_local_ba_args *A, int rank, int world, fb_allreduce_fn allreduce, void *ctx) {
  FB_ARG(world >= 1 && rank >= 0 && rank < world && (world == 1 || allreduce));
  Xchg X;
  X.world = world; X.cb = allreduce; X.ctx = ctx;
  return local_ba_impl(A, rank, X, kLocalSchedule, kLocalDelta);
}

extern "C" int fb_local_ba_sharded_rccl(const fb_local_ba_args *A, int rank, int world, void *comm) {
  FB_ARG(world >= 1 && rank >= 0 && rank < world && comm);
  if (!rccl_api()) { fb::set_error("fb_local_ba_sharded_rccl: no RCCL in this process"); return FB_ERR_NODEVICE; }
  Xchg X;
  X.world = world; X.comm = comm;
  return local_ba_impl(A, rank, X, kLocalSchedule, kLocalDelta);
}
