// ba_driver.inc -- the host driver of every bundle adjustment entry point (included by ba.hip).  local_ba_impl is the table of
// contents: agreement -> plan -> stage/build -> bind -> the device-resident Levenberg-Marquardt schedule -> results.
// Everything a call owns sits in one BACtx; the stages are free functions over it.
// optimisation schedule: LocalBundleAdjustment[WithOdom] = optimize(5) robust, chi2 gate, optimize(10) plain
// (Optimizer.cc:2504-2560); BundleAdjustmentWithOdom = ONE optimize(nIterations), robust iff bRobust, no gate (:2048-2050)
struct BASchedule {
  int its1, robust1;
  bool gate;
  int its2;
  double delta;  // Huber delta: sqrt(5.991) local (:2290), sqrt(5.99) global (:1836)
};
struct DevIn { hipStream_t stream = nullptr; };  // fb_local_ba_dev: the big arrays of fb_local_ba_args are DEVICE pointers

// per host thread and device: the side stream for the abort request (does not synchronise with the null stream), the pinned
// mirror of the control block and the event the host waits on (concurrent callers must not share them; a stream belongs
// to its device).  fb_shutdown releases the calling thread's set.
struct PerDev { hipStream_t sAux = nullptr; BACtl *hCtl = nullptr; hipEvent_t evDone = nullptr; };
static thread_local PerDev g_perDev[64];

namespace {

struct BAPlan {
  BADims d;
  bool sharded, devIn;
  int rank, world;
  int P6, NT, rows;
  int nLinBlocks, nUpdBlocks;  // LIN_THREADS landmarks each (sizes the chi2 / max partials); k_ba_update_c: four lanes per landmark + one per key frame
  int nWg, lmPerWg;            // k_ba_schur_c: workgroups and landmarks of each (a multiple of CHUNK)
  size_t schurLds, solveLds;
  bool big;       // beyond ~23 free key frames the reduced system no longer fits LDS: HBM-resident path of ba_big.inc
  bool anything;  // (sharded: nE is this rank's view; every rank holds all edges, so this agrees across the ranks)
  bool timing, trace;  // FB_BA_TIMING (host-side phase times on stderr), FB_BA_TRACE (one line per slot; implies paced)
  bool paced;          // FB_BA_HOST_LM: one slot per batch, the control block read back after each
};

int plan(const fb_local_ba_args *A, int rank, const Xchg &X, bool devIn, BAPlan &P) {
  P.d = dims_of(A, rank);
  const BADims &d = P.d;
  P.sharded = X.active(); P.devIn = devIn; P.rank = rank; P.world = X.world;
  P.P6 = 6 * d.np;
  if (P.P6 > 4096) { fb::set_error("fb_local_ba: more than 682 free keyframes"); return FB_ERR_CAPACITY; }
  P.NT = (P.P6 + 1 + 15) / 16;
  P.rows = P.NT * 16;
  P.nLinBlocks = (d.npt + LIN_THREADS - 1) / LIN_THREADS;
  P.nUpdBlocks = (4 * d.npt + d.n_kf + LIN_THREADS - 1) / LIN_THREADS;
  const char *nwg = getenv("FB_BA_NWG");
  P.nWg = std::min(nwg ? atoi(nwg) : 256, std::max(1, (d.npt + CHUNK - 1) / CHUNK));
  P.lmPerWg = ((d.npt + P.nWg - 1) / P.nWg + CHUNK - 1) / CHUNK * CHUNK;
  P.nWg = std::max(1, (d.npt + P.lmPerWg - 1) / std::max(P.lmPerWg, 1));
  P.schurLds = (size_t)2 * P.rows * KPAD * 8;
  P.solveLds = ((size_t)(P.P6 + 1) * (P.P6 + 1) + (size_t)(P.P6 + 1) * 6 + 96 + P.P6 + 2) * 8;  // solve_lookahead
  P.big = P.schurLds > 160 * 1024 || P.solveLds > 160 * 1024 || P.P6 + 1 > 256;
  if (devIn && P.big) { fb::set_error("fb_local_ba_dev: more than 23 free key frames (use fb_local_ba)"); return FB_ERR_CAPACITY; }
  P.anything = d.nE + (d.odom ? A->n_odom : 0) > 0 && (d.np > 0 || d.npt > 0);
  P.timing = getenv("FB_BA_TIMING") != nullptr;
  P.trace = getenv("FB_BA_TRACE") != nullptr;
  P.paced = P.trace || getenv("FB_BA_HOST_LM") != nullptr;
  return FB_OK;
}

struct ScratchLayout {  // the second device block: everything the schedule writes
  Slot<double> e_chi2;
  Slot<SE3> pose1;  // state 1 (state 0 is the staged copy)
  Slot<double> pt1;
  struct { Slot<double> Hll, bl, W, Hpp, bp, chiPart, maxPart; } lin[2];
  size_t bytes;
};
ScratchLayout scratch_layout(const BAPlan &P) {
  const size_t nE1 = std::max(P.d.nE, 1), npt1 = std::max(P.d.npt, 1), P6 = P.P6;
  ScratchLayout C;
  Carver c;
  C.e_chi2 = c.take<double>(nE1);
  C.pose1 = c.take<SE3>(P.d.n_kf); C.pt1 = c.take<double>(3 * npt1);
  for (auto &l : C.lin) {
    l.Hll = c.take<double>(9 * npt1); l.bl = c.take<double>(3 * npt1); l.W = c.take<double>(18 * nE1);
    l.Hpp = c.take<double>(std::max<size_t>(P6 * P6, 1)); l.bp = c.take<double>(std::max<size_t>(P6, 1));
    l.chiPart = c.take<double>(2 * P.nLinBlocks + 2); l.maxPart = c.take<double>(2 * P.nLinBlocks + 2);
  }
  C.bytes = c.bytes;
  return C;
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
  const BASchedule &sc;
  hipStream_t s0;
  std::chrono::steady_clock::time_point tStart;
  BAPlan P;
  GraphLayout G;
  uint8_t *hs = nullptr;  // host copy of the staged graph (device input: only its header is filled)
  // device blocks; they return to the pool when the context goes
  fb::DevBuf d_stage, d_bld, d_scratch, d_Dinv, d_Spart, d_xp, d_ok, d_scale, d_ol;
  BigSys bigSys;
  fb::DevBuf d_xb, d_olDev, d_ex;        // exchange blocks, odometry records, sharded result
  fb::DevBuf d_flags, d_kfT, d_ptOut;    // results
  BADev D;
  State st[2];
  LinBuf lb[2];
  const uint8_t *d_fixed = nullptr;
  const float *d_kfT0 = nullptr;
  BACtl *ctl = nullptr;
  int *d_abort = nullptr;
  OdomLin *olGlobal = nullptr;  // long odometry chains: per-edge linearisations in HBM
  size_t odomLds = 0;
  StreamDrain drain;  // LAST member: destroyed first, before any block above is given back
  BACtx(const fb_local_ba_args *a, const Xchg &x, const BASchedule &s, hipStream_t st) : A(a), X(x), sc(s), s0(st), tStart(std::chrono::steady_clock::now()) {}
  void lap(const char *what) const {
    if (P.timing) fprintf(stderr, "[fb_local_ba] %-28s %8.1f us\n", what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tStart).count());
  }
};

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
    FB_TRY(build_graph_device(c.A, d, c.G, c.d_stage.as<uint8_t>(), c.d_bld, c.s0));
  }
  c.lap("graph uploaded");
  return FB_OK;
}

// ---- bind: the scratch block and the pointer structs the kernels take -------------------------------------------------------
int bind_device(BACtx &c) {
  const BAPlan &P = c.P;
  const BADims &d = P.d;
  const GraphLayout &G = c.G;
  const ScratchLayout C = scratch_layout(P);
  FB_TRY(c.d_scratch.alloc(C.bytes));
  uint8_t *ds = c.d_stage.as<uint8_t>(), *dc = c.d_scratch.as<uint8_t>();
  hipStream_t s0 = c.s0;
  c.drain.arm(s0);
  FB_HIP(hipMemsetAsync(C.e_chi2.at(dc), 0, (size_t)std::max(d.nE, 1) * 8, s0));
  // state 0 = the staged copy, state 1 starts as the same poses / points
  FB_HIP(hipMemcpyAsync(C.pose1.at(dc), G.poses.at(ds), (size_t)d.n_kf * sizeof(SE3), hipMemcpyDeviceToDevice, s0));
  FB_HIP(hipMemcpyAsync(C.pt1.at(dc), G.pts.at(ds), (size_t)std::max(d.npt, 1) * 24, hipMemcpyDeviceToDevice, s0));
  c.d_fixed = G.fixed.at(ds);
  c.d_kfT0 = G.kfT.at(ds);
  c.ctl = G.ctl.at(ds);
  c.d_abort = G.abort.at(ds);
  BADev &D = c.D;
  D.n_kf = d.n_kf; D.np = d.np; D.npt = d.npt; D.nE = d.nE; D.nO = d.nO; D.quat = d.odom ? 1 : 0;
  D.fx = c.A->fx; D.fy = c.A->fy; D.cx = c.A->cx; D.cy = c.A->cy; D.delta = c.sc.delta;
  D.poseIdx = G.poseIdx.at(ds); D.e_pt = G.e_pt.at(ds); D.e_kf = G.e_kf.at(ds); D.e_pj = G.e_pj.at(ds);
  D.e_type = G.e_type.at(ds); D.e_meas = G.e_meas.at(ds); D.e_info = G.e_info.at(ds);
  D.e_level = G.e_level.at(ds); D.e_chi2 = C.e_chi2.at(dc);
  D.lm_start = G.lm_start.at(ds); D.lm_edges = G.lm_edges.at(ds);
  D.ps_start = G.ps_start.at(ds); D.ps_edges = G.ps_edges.at(ds);
  D.o_i = G.o_i.at(ds); D.o_j = G.o_j.at(ds); D.o_Zinv = G.o_Zinv.at(ds); D.o_info = G.o_info.at(ds);
  D.od_start = G.od_start.at(ds); D.od_edges = G.od_edges.at(ds);
  c.st[0].pose = G.poses.at(ds); c.st[0].pt = G.pts.at(ds);
  c.st[1].pose = C.pose1.at(dc); c.st[1].pt = C.pt1.at(dc);
  for (int q = 0; q < 2; q++) {
    LinBuf &b = c.lb[q];
    b.Hll = C.lin[q].Hll.at(dc); b.bl = C.lin[q].bl.at(dc); b.W = C.lin[q].W.at(dc);
    b.Hpp = C.lin[q].Hpp.at(dc); b.bp = C.lin[q].bp.at(dc); b.chiPart = C.lin[q].chiPart.at(dc); b.maxPart = C.lin[q].maxPart.at(dc);
  }
  return FB_OK;
}

int alloc_solver(BACtx &c) {
  const BAPlan &P = c.P;
  const BADims &d = P.d;
  const int P6 = P.P6;
  FB_TRY(c.d_Dinv.alloc((size_t)d.npt * 9 * 8));
  FB_TRY(c.d_Spart.alloc(P.big ? 8 : (size_t)P.nWg * P.rows * P.rows * 8));
  if (P.big) {
    const GraphLayout &G = c.G;
    FB_TRY(big_prepare(c.bigSys, d.np, d.npt, P6, G.poseIdx.at(c.hs), G.e_kf.at(c.hs), G.lm_start.at(c.hs), G.lm_edges.at(c.hs)));
  }
  FB_TRY(c.d_xp.alloc((size_t)std::max(P6, 1) * 8)); FB_TRY(c.d_ok.alloc(8)); FB_TRY(c.d_scale.alloc((size_t)P.nUpdBlocks * 8));
  c.odomLds = (size_t)std::max(d.nO, 1) * sizeof(OdomLin);
  if (c.odomLds > 150 * 1024) {  // long odometry chains: per-edge linearisations in HBM
    FB_TRY(c.d_ol.alloc(c.odomLds));
    c.olGlobal = c.d_ol.as<OdomLin>();
    c.odomLds = 0;
  }
  return FB_OK;
}

// ---- results ------------------------------------------------------------------------------------------------------------------
struct HostResult { std::vector<uint8_t> flags; std::vector<float> po; };
int fetch_results(BACtx &c, HostResult &r) {
  r.flags.resize(std::max(c.P.d.nE, 1));
  FB_TRY(c.d_flags.download(r.flags.data(), std::max(c.P.d.nE, 1)));
  r.po.resize((size_t)std::max(c.P.d.npt, 1) * 3);
  return c.d_ptOut.download(r.po.data(), (size_t)c.P.d.npt * 12);
}
// the one place where a BA writes into the caller's host arrays
int results_to_host(BACtx &c, const HostResult &r) {
  const fb_local_ba_args *A = c.A;
  const BADims &d = c.P.d;
  if (c.sc.gate) {  // the global BA classifies nothing
    for (int i = 0; i < d.nF; i++) A->obs_outlier[i] = r.flags[i];
    for (int i = 0; i < d.nB; i++) A->bobs_outlier[i] = r.flags[d.nF + i];
  }
  FB_TRY(c.d_kfT.download(A->kf_Tcw, (size_t)d.n_kf * 48));
  for (int i = 0; i < 3 * d.n_mp; i++) A->mp_xw[i] = r.po[i];
  for (int i = 0; i < 3 * A->n_mpb; i++) A->mpb_xw[i] = r.po[3 * d.n_mp + i];
  return FB_OK;
}
int results_to_device(BACtx &c) {
  const fb_local_ba_args *A = c.A;
  const BADims &d = c.P.d;
  hipStream_t s0 = c.s0;
  if (c.sc.gate) {
    if (d.nF > 0) FB_HIP(hipMemcpyAsync(A->obs_outlier, c.d_flags.p, (size_t)d.nF, hipMemcpyDeviceToDevice, s0));
    if (d.nB > 0) FB_HIP(hipMemcpyAsync(A->bobs_outlier, c.d_flags.as<uint8_t>() + d.nF, (size_t)d.nB, hipMemcpyDeviceToDevice, s0));
  }
  FB_HIP(hipMemcpyAsync(A->kf_Tcw, c.d_kfT.p, (size_t)d.n_kf * 48, hipMemcpyDeviceToDevice, s0));
  if (d.n_mp > 0) FB_HIP(hipMemcpyAsync(A->mp_xw, c.d_ptOut.p, (size_t)d.n_mp * 12, hipMemcpyDeviceToDevice, s0));
  if (A->n_mpb > 0) FB_HIP(hipMemcpyAsync(A->mpb_xw, c.d_ptOut.as<float>() + (size_t)3 * d.n_mp, (size_t)A->n_mpb * 12, hipMemcpyDeviceToDevice, s0));
  FB_HIP(hipStreamSynchronize(s0));  // the scratch goes back to the pool when the call returns
  c.drain.done();
  return FB_OK;
}

// ---- device-resident Levenberg-Marquardt: no read-back inside a batch of slots.  Sharded: two all-reduces per slot on this
//      stream (the Schur-reduced system; the exchange block of the linearisation), every rank enqueues the same slots and
//      takes the same decisions from the reduced values.
struct DevLm {
  PerDev *pd = nullptr;
  BASched sched;
  St2 st2;
  Lb2 lb2;
  void (*schurC)(BADev, Lb2, const BACtl *, double *, double *, int, int, int) = nullptr;
  int nS, nLin256, linGrid;  // nLin256: four lanes per landmark; chi2 slot of the odometry role = nLin256
  XBLay xb, xr;              // raw and reduced exchange blocks (the same unless sharded)
  size_t linLds;
  bool linGlobal;
  OdomLin *ol;
  std::vector<double> hostScratch;
  int rcSlot = FB_OK;
};

int dev_lm_prepare(BACtx &c, DevLm &L) {
  const BAPlan &P = c.P;
  const BADims &d = P.d;
  hipStream_t s0 = c.s0;
  int devId = 0;
  FB_HIP(hipGetDevice(&devId));
  if (devId < 0 || devId >= 64) { fb::set_error("fb_local_ba: device id %d", devId); return FB_ERR_NODEVICE; }
  PerDev &pd = g_perDev[devId];
  if (!pd.sAux) FB_HIP(hipStreamCreateWithFlags(&pd.sAux, hipStreamNonBlocking));
  if (!pd.hCtl) FB_HIP(hipHostMalloc(reinterpret_cast<void **>(&pd.hCtl), sizeof(BACtl), hipHostMallocDefault));
  if (!pd.evDone) FB_HIP(hipEventCreateWithFlags(&pd.evDone, hipEventDisableTiming));
  L.pd = &pd;
  if (P.devIn) {  // a rejected graph (index out of range, duplicate observation) ends the schedule before it starts
    k_bld_check<<<1, 1, 0, s0>>>(builder_verdict(c.d_bld, d), c.ctl);
    FB_HIP(hipGetLastError());
  }
  L.sched = {c.sc.its1, c.sc.robust1, c.sc.gate ? 1 : 0, c.sc.its2};
  L.st2.s[0] = c.st[0]; L.st2.s[1] = c.st[1];
  L.lb2.b[0] = c.lb[0]; L.lb2.b[1] = c.lb[1];
  L.nS = P.rows * P.rows;
  if (P.big) {
    FB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_big_solve), hipFuncAttributeMaxDynamicSharedMemorySize, P.P6 * 8));
  } else {
    // accumulator tiles per wave: NT<=8 -> 9, NT<=12 -> 20, NT<=16 -> 34
    L.schurC = P.NT <= 8 ? k_ba_schur_c<9> : (P.NT <= 12 ? k_ba_schur_c<20> : k_ba_schur_c<34>);
    FB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(L.schurC), hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.schurLds));
    FB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_ba_solve_c), hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.solveLds));
    FB_HIP(hipMemsetAsync(c.d_Spart.p, 0, (size_t)L.nS * 8, s0));  // the lower tiles of the summed system are never written: keep them finite
  }
  L.nLin256 = (4 * d.npt + 255) / 256;
  XBLay &xb = L.xb;
  xb.oH = d.np * POSE_PARTS * 27; xb.oB = xb.oH + P.P6 * P.P6; xb.oS = xb.oB + P.P6; xb.oM = xb.oS + 4; xb.stride = xb.oM + P.world;
  // sharded: the kernels of a linearisation fill the RAW blocks; exchange 2 sums BOTH raw blocks into the REDUCED ones out of
  // place (which of the two the slot wrote is device-side knowledge; the raw block of the accepted linearisation is not
  // touched until it is overwritten, so re-reducing it is idempotent); k_ba_control and the solve read the reduced blocks.
  // The blocks start cleared: the odometry role relies on it for HppO
  FB_TRY(c.d_xb.alloc((size_t)(P.sharded ? 4 : 2) * xb.stride * 8));
  FB_HIP(hipMemsetAsync(c.d_xb.p, 0, (size_t)(P.sharded ? 4 : 2) * xb.stride * 8, s0));
  xb.base = c.d_xb.as<double>();
  L.xr = xb;
  if (P.sharded) L.xr.base = xb.base + (size_t)2 * xb.stride;
  L.ol = c.olGlobal;
  L.linLds = L.ol ? 0 : c.odomLds + (size_t)std::max(d.nO, 1) * 108 * 8;
  L.linGlobal = L.ol != nullptr;
  if (!L.linGlobal && L.linLds > 150 * 1024) {  // the products' scratch does not fit next to the records: HBM records, serial products
    FB_TRY(c.d_olDev.alloc((size_t)std::max(d.nO, 1) * sizeof(OdomLin)));
    L.ol = c.d_olDev.as<OdomLin>();
    L.linGlobal = true;
  }
  if (!L.linGlobal) FB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_ba_lin_c<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.linLds));
  L.linGrid = L.nLin256 + POSE_PARTS * d.np + 1;
  FB_TRY(c.d_flags.alloc(std::max(d.nE, 1)));
  FB_TRY(c.d_kfT.alloc((size_t)d.n_kf * 48));
  FB_HIP(hipMemcpyAsync(c.d_kfT.p, c.d_kfT0, (size_t)d.n_kf * 48, hipMemcpyDeviceToDevice, s0));
  FB_TRY(c.d_ptOut.alloc((size_t)std::max(d.npt, 1) * 12));
  if (P.sharded) FB_TRY(c.d_ex.alloc(((size_t)d.npt * 3 + d.nE + 1) * 8));
  return FB_OK;
}

// one slot: a trial (or the opening linearisation) and the decision of k_ba_control
void dev_lm_slot(BACtx &c, DevLm &L) {
  if (L.rcSlot != FB_OK) return;
  const BAPlan &P = c.P;
  const BADev &D = c.D;
  hipStream_t s0 = c.s0;
  double *Dinv = c.d_Dinv.as<double>(), *Spart = c.d_Spart.as<double>(), *xp = c.d_xp.as<double>(), *scale = c.d_scale.as<double>(),
         *okFlag = c.d_ok.as<double>();
  BACtl *ctl = c.ctl;
  const int nLin256 = L.nLin256;
  if (P.big) {
    L.rcSlot = big_slot_solve(c.bigSys, D, L.lb2, ctl, L.xr, P.P6, Dinv, xp, okFlag, c.X, L.hostScratch, s0);
  } else {
    { fb::ProfScope pr(fb::P_BA_SCHUR, s0);
      L.schurC<<<P.nWg, SCHUR_THREADS, P.schurLds, s0>>>(D, L.lb2, ctl, Dinv, Spart, P.P6, P.NT, P.lmPerWg); }
    fb::ProfScope pr(fb::P_BA_SOLVE, s0);
    k_ba_sumparts_c<<<(L.nS + SUMPARTS_ELEMS - 1) / SUMPARTS_ELEMS, 256, 0, s0>>>(ctl, Spart, P.nWg, L.nS, P.rows);
    if (P.sharded) L.rcSlot = c.X.sum_dev(Spart, (size_t)L.nS, s0, L.hostScratch);  // exchange 1: the Schur-reduced system
    k_ba_solve_c<<<1, SOLVE_C_THREADS, P.solveLds, s0>>>(L.lb2, ctl, Spart, P.P6, P.NT, xp, okFlag, L.xr);
  }
  { fb::ProfScope pr(fb::P_BA_UPDATE, s0);
    k_ba_update_c<<<P.nUpdBlocks, LIN_THREADS, 0, s0>>>(D, L.lb2, L.st2, ctl, Dinv, xp, scale, P.rank == 0 ? 1 : 0); }
  { fb::ProfScope pr(fb::P_BA_LINEARIZE, s0);
    if (L.linGlobal) k_ba_lin_c<true><<<L.linGrid, 256, 0, s0>>>(D, L.st2, L.lb2, ctl, L.sched, P.P6, nLin256, nLin256, L.ol, L.xb);
    else k_ba_lin_c<false><<<L.linGrid, 256, L.linLds, s0>>>(D, L.st2, L.lb2, ctl, L.sched, P.P6, nLin256, nLin256, nullptr, L.xb); }
  { fb::ProfScope pr(fb::P_BA_MISC, s0);
    if (P.sharded) {
      k_ba_prex<<<1, 256, 0, s0>>>(D, L.lb2, ctl, nLin256, nLin256, scale, P.nUpdBlocks, L.xb, c.d_abort, P.rank, P.world);
      // exchange 2: both raw blocks -> the reduced blocks, one all-reduce
      if (L.rcSlot == FB_OK) L.rcSlot = c.X.sum_dev(L.xr.at(0), (size_t)2 * L.xb.stride, s0, L.hostScratch, L.xb.at(0));
      k_ba_control<true><<<1, 256, 0, s0>>>(D, L.lb2, ctl, L.sched, nLin256, nLin256, scale, P.nUpdBlocks, okFlag, P.P6, L.xr, c.d_abort, P.world);
    } else {
      k_ba_control<false><<<1, 256, 0, s0>>>(D, L.lb2, ctl, L.sched, nLin256, nLin256, scale, P.nUpdBlocks, okFlag, P.P6, L.xb, c.d_abort, P.world);
    } }
}

// the results of the state that is current now (final when the schedule has finished, which is the common case) and the
// control block into its pinned mirror, the event behind them
int dev_lm_export(BACtx &c, DevLm &L) {
  const BAPlan &P = c.P;
  const int n_kf = P.d.n_kf, npt = P.d.npt, nE = P.d.nE;
  hipStream_t s0 = c.s0;
  if (nE > 0) k_ba_gate_final_c<<<(nE + 255) / 256, 256, 0, s0>>>(c.D, L.st2, c.ctl, c.d_flags.as<uint8_t>());
  k_ba_export_c<<<(n_kf + npt * 3 + 255) / 256, 256, 0, s0>>>(n_kf, npt, L.st2, c.ctl, c.d_fixed, c.d_kfT.as<float>(), c.d_ptOut.as<float>());
  if (P.sharded) {  // every rank returns the complete result
    const int nx = npt * 3 + nE;
    k_ba_final_pack<<<(nx + 255) / 256, 256, 0, s0>>>(npt, nE, P.rank, P.world, c.d_ptOut.as<float>(), c.d_flags.as<uint8_t>(), c.d_ex.as<double>());
    FB_TRY(c.X.sum_dev(c.d_ex.as<double>(), (size_t)nx, s0, L.hostScratch));
    k_ba_final_unpack<<<(nx + 255) / 256, 256, 0, s0>>>(npt, nE, c.d_ex.as<double>(), c.d_ptOut.as<float>(), c.d_flags.as<uint8_t>());
  }
  if (hipGetLastError() != hipSuccess) { fb::set_error("fb_local_ba: kernel launch failed"); return FB_ERR_HIP; }
  if (hipMemcpyAsync(L.pd->hCtl, c.ctl, sizeof(BACtl), hipMemcpyDeviceToHost, s0) != hipSuccess || hipEventRecord(L.pd->evDone, s0) != hipSuccess) {
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
      (void)hipMemcpyAsync(c.d_abort, &one, sizeof(int), hipMemcpyHostToDevice, L.pd->sAux);
      abortSent = true;
    }
    // a BA lasts milliseconds and the flag only has to reach the device before the running slot (~0.1 ms) ends:
    // poll every 20 us instead of spinning on the LocalMapping thread's core
    std::this_thread::sleep_for(std::chrono::microseconds(20));
  }
}

// FB_BA_TRACE: the slot that took the control block from `was` to `now`, in the format of the oracle's trace (se3_oracle.h)
void trace_slot(const BACtl &was, const BACtl &now, const BASchedule &sc) {
  if (was.phase == 2 || now.badArgs) return;  // the slot did nothing
  if (was.needInit) fprintf(stderr, "[hip] optimize(%d) chi0=%.17g maxDiag=%.17g\n", was.phase == 0 ? sc.its1 : sc.its2, now.trChi, now.trScale);
  else fprintf(stderr, "[hip]  it=%d q=%d lambda=%.17g tempChi=%.17g scale=%.17g rho=%.17g ok=%d\n", was.it, was.qmax, was.lambda, now.trChi, now.trScale,
               now.trRho, now.trChi != 1.7976931348623157e308 ? 1 : 0);
}

int run_device_lm(BACtx &c) {
  const BASchedule &sc = c.sc;
  DevLm L;
  FB_TRY(dev_lm_prepare(c, L));
  bool abortSent = false;
  // a typical schedule takes one trial per iteration: its1 + its2 trials + the two opening linearisations; the longest one
  // ten trials per iteration.  Paced (FB_BA_HOST_LM, FB_BA_TRACE): the host looks at the control block after every slot
  int batch = c.P.anything ? sc.its1 + (sc.gate ? sc.its2 + 1 : 0) + 1 + 2 : 0;
  if (c.P.paced) batch = std::min(batch, 1);
  const int maxSlots = 2 + 10 * (sc.its1 + (sc.gate ? sc.its2 : 0));
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
    if (c.P.trace) trace_slot(was, *hCtl, sc);
    was = *hCtl;
    if (hCtl->phase == 2 || enqueued >= maxSlots) break;
    batch = c.P.paced ? 1 : 6;
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

static int local_ba_impl(const fb_local_ba_args *A, int rank, const Xchg &X, const BASchedule &sc, const DevIn *dv = nullptr) {
  FB_TRY(fb::check_device());
  const bool devIn = dv != nullptr;  // observations / poses / points / result arrays live in HBM (fb_local_ba_dev)
  BACtx c(A, X, sc, devIn ? dv->stream : nullptr);
  FB_ARG(!(devIn && X.active()));
  FB_TRY(agree_on_arguments(A, rank, X));
  // Optimizer.cc:902-906 / 2498-2500.  Sharded: a rank must not leave on its OWN view of the flag (the others would wait for
  // it in the first exchange): every stop decision of the schedule goes through a reduction
  if (!X.active() && A->stop_flag && *A->stop_flag) return FB_OK;
  FB_TRY(plan(A, rank, X, devIn, c.P));
  FB_TRY(stage_graph(c));
  FB_TRY(bind_device(c));
  FB_TRY(alloc_solver(c));
  return run_device_lm(c);
}

static const BASchedule kLocalSchedule = {5, 1, true, 10, (double)(float)sqrt(5.991)};

extern "C" int fb_local_ba(const fb_local_ba_args *A) { return local_ba_impl(A, 0, Xchg(), kLocalSchedule); }
extern "C" int fb_local_ba_dev(const fb_local_ba_args *A, void *stream) {
  DevIn dv;
  dv.stream = fb::as_stream(stream);
  return local_ba_impl(A, 0, Xchg(), kLocalSchedule, &dv);
}

extern "C" int fb_global_ba(const fb_local_ba_args *A, int n_iterations, int robust) {
  FB_ARG(n_iterations >= 0);
  const BASchedule sc = {n_iterations, robust ? 1 : 0, false, 0, (double)(float)sqrt(5.99)};
  return local_ba_impl(A, 0, Xchg(), sc);
}

// Landmark-partitioned BA (SURVEY 8e): rank r owns the landmarks l with l % world == r and all their edges, the
// odometry edges live on rank 0, the keyframe state is replicated.  Per LM trial two small all-reduces: the
// Schur-reduced system (after k_ba_schur_c / the gathers of ba_big.inc) and the exchange block (after the linearisation at the trial state).
extern "C" int fb_local_ba_sharded(const fb_local_ba_args *A, int rank, int world, fb_allreduce_fn allreduce, void *ctx) {
  FB_ARG(world >= 1 && rank >= 0 && rank < world && (world == 1 || allreduce));
  Xchg X;
  X.world = world; X.cb = allreduce; X.ctx = ctx;
  return local_ba_impl(A, rank, X, kLocalSchedule);
}

extern "C" int fb_local_ba_sharded_rccl(const fb_local_ba_args *A, int rank, int world, void *comm) {
  FB_ARG(world >= 1 && rank >= 0 && rank < world && comm);
  if (!rccl_api()) { fb::set_error("fb_local_ba_sharded_rccl: no RCCL in this process"); return FB_ERR_NODEVICE; }
  Xchg X;
  X.world = world; X.comm = comm;
  return local_ba_impl(A, rank, X, kLocalSchedule);
}

extern "C" int fb_shutdown(void) {
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
  fb::pool_release();
  return FB_OK;
}
