// covis_correct.inc -- the two places where the loop closer rewrites the map, on the tables the handle's callers keep in
// HBM (included at the end of covis.hip, after covis_tree.inc: it shares Gr, Index, row_sorted and same_map).
//
// Replaces (reference file:line):
//   LoopClosing::CorrectLoop, the Sim3 propagation and the pose write     src/LoopClosing.cc:438-541
//   MapPoint::UpdateNormalAndDepth as that loop calls it                   src/MapPoint.cc:330-371
//   KeyFrame::SetPose (Twc, Ow)                                            src/KeyFrame.cc:104-118
//   LoopClosing::RunGlobalBundleAdjustment, the map update                 src/LoopClosing.cc:714-825
//   g2o::Sim3 (constructor from a matrix, map, inverse, operator*)        Thirdparty/g2o/g2o/types/sim3.h:64, :144, :233, :266
//
// No branch depends on a float: NULL, bad, holder rank, flag.  The integer outputs are compared for equality with
// tests/map_correct_ref.py, the float ones to rounding (cv::Mat products accumulate in double and round once, the
// project's convention; the Sim3 algebra is double and uses the quaternion helpers of fb_se3.h).
//
// Quirks of the reference kept as they are:
//  * the point loop of CorrectLoop iterates a std::map<KeyFrame*, Sim3>: ascending kf_order, not list order.  A point is
//    moved by the first set member in that order that holds it (mnCorrectedByKF): a minimum over set positions.
//  * UpdateNormalAndDepth runs inside that loop and sees a half-corrected map: an observer that is a set member EARLIER in
//    that order than the point's holder has its corrected pose already (SetPose ends its turn), every other observer, the
//    holder included, still has its old one.
//  * line :523 compares where it means to assign, so a bird point is never marked: EVERY set member that holds it moves it
//    again, once per feature it is held at, each applying its own CorrectedSwi o Siw to the result of the one before.  One
//    thread per bird point walks its holders in that order.
//  * RunGlobalBundleAdjustment reads Twc of a parent before the parent's SetPose (:721 before :737): both factors of
//    Tchild * Twc_parent are OLD poses, only TcwGBA of the parent comes from the walk.
#include "fb_frame_geom.h"
#include "fb_se3.h"

namespace {

constexpr int CL_NT = 256;
constexpr int32_t CL_NONE = 0x7f7f7f7f;                // memset(0x7f): the point has no holder in the set
enum { CH_NSET = 0 };

struct ClEntry {        // one set member, at its position in ascending kf_order
  double siw_q[4], siw_t[3];                           // NonCorrectedSim3 (s = 1)
  double inv_q[4], inv_t[3], inv_s;                    // CorrectedSim3.inverse()
  float ow_new[3];                                     // Ow of the corrected pose
  float Tcw[12];                                       // [R(CorrectedSiw) | t / s]
  int32_t slot;
};

struct ClS {            // the scratch of one call, behind the index
  int32_t *hdr;         // [64]
  int32_t *pos;         // [K] slot -> position in the set, -1 = not a member
  ClEntry *tab;         // [K]
  float *ow_old;        // [K][3] Ow of every key frame's pose as it came in
  int32_t *owner;       // [n_mp] the smallest set position among the point's holders
  int32_t *bhead;       // [n_mpb] } the (set position, feature) pairs that hold a bird point, as a linked list:
  int32_t *bnext;       // [K][BS] } pair = position * BS + feature
};

static_assert(sizeof(ClEntry) == CL_ENTRY_BYTES, "plan_correct_loop sizes the table by it");
void cl_map(uint8_t *b, const ClOff &o, ClS *S) {
  S->hdr = (int32_t *)(b + o.hdr); S->pos = (int32_t *)(b + o.pos); S->tab = (ClEntry *)(b + o.tab); S->ow_old = (float *)(b + o.ow_old);
  S->owner = (int32_t *)(b + o.owner); S->bhead = (int32_t *)(b + o.bhead); S->bnext = (int32_t *)(b + o.bnext);
}

using fb::Sim3d; using fb::sim3_map; using fb::sim3_mul; using fb::sim3_inverse;  // g2o::Sim3 in double, fb_se3.h

// Sim3(Matrix3d(R of a CV_32F pose), Vector3d(t), 1.0): Quaterniond(R) is not normalised (sim3.h:64)
__device__ __forceinline__ Sim3d sim3_from_pose(const float *T) {
  const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
  Sim3d S;
  S.r = fb::quat_from_R(R);
  S.t[0] = T[3]; S.t[1] = T[7]; S.t[2] = T[11];
  S.s = 1.0;
  return S;
}
// rows 0..2 of Twc as KeyFrame::SetPose leaves it (KeyFrame.cc:108-115): Rwc = Rcw.t(), Ow = -Rwc*tcw
__device__ __forceinline__ void pose_inverse(const float *T, float *Twc) {
  float Ow[3];
  fb::camera_centre(T, Ow);
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) Twc[r * 4 + c] = T[c * 4 + r];
    Twc[r * 4 + 3] = Ow[r];
  }
}
// rows 0..2 of the CV_32F 4x4 product A*B (the fourth rows are 0 0 0 1): double accumulation, rounded once
__device__ __forceinline__ void pose_mul(const float *A, const float *B, float *Cm) {
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 3; k++) s += (double)A[r * 4 + k] * (double)B[k * 4 + c];
      if (c == 3) s += (double)A[r * 4 + 3];
      Cm[r * 4 + c] = (float)s;
    }
}
// R*x + t with R | t the rows of a pose: the product rounds to CV_32F, then a CV_32F addition
__device__ __forceinline__ void pose_apply(const float *T, const float x[3], float o[3]) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) s += (double)T[r * 4 + k] * (double)x[k];
    o[r] = (float)s + T[r * 4 + 3];
  }
}

// ---- CorrectLoop -----------------------------------------------------------------------------------------------------------
// The set (:438-439) in ascending kf_order, NonCorrectedSim3 / CorrectedSim3 (:450-472) and the corrected poses (:529-535)
// of its members, and Ow of every key frame, all from the poses as they came in.  One workgroup.
__global__ __launch_bounds__(CV_NT) void k_cl_set(Gr G, const float *kf_Tcw, fb_correct_loop_args A, ClS S) {
  __shared__ uint32_t s_key[CV_MAXK];
  __shared__ int s_wv[CV_NT / 64];
  const int tid = threadIdx.x, K = G.K, cur = A.cur_slot;
  int n2 = 2;
  while (n2 < K) n2 <<= 1;
  const uint16_t *row = G.W + (size_t)cur * K;
  int cnt = 0;
  for (int i = tid; i < n2; i += CV_NT) {
    uint32_t key = KEY_NONE32;
    if (i < K) {
      const uint32_t v = row[i];
      if (i == cur || ((v & CV_MEMBER) && (v & CV_W))) { key = (uint32_t)G.rank[i]; cnt++; }
      S.pos[i] = -1;
      fb::camera_centre(kf_Tcw + (size_t)i * 12, S.ow_old + (size_t)i * 3);
    }
    s_key[i] = key;
  }
  const int n = fb::block_sum<CV_NT>(cnt, s_wv);
  __syncthreads();
  fb::bitonic_sort(s_key, n2, tid, CV_NT);
  if (tid == 0) { S.hdr[CH_NSET] = n; *A.d_n_set = n; }
  Sim3d Scw;
  Scw.r.x = A.q[0]; Scw.r.y = A.q[1]; Scw.r.z = A.q[2]; Scw.r.w = A.q[3];
  Scw.t[0] = A.t[0]; Scw.t[1] = A.t[1]; Scw.t[2] = A.t[2]; Scw.s = A.s;
  float Twc[12];
  pose_inverse(kf_Tcw + (size_t)cur * 12, Twc);                         // :443
  for (int p = tid; p < n; p += CV_NT) {
    const int slot = G.inv[s_key[p]];
    const float *Tiw = kf_Tcw + (size_t)slot * 12;
    S.pos[slot] = p;
    A.d_set_slots[p] = slot;
    ClEntry &E = S.tab[p];
    E.slot = slot;
    Sim3d cor = Scw;                                                    // :442
    if (slot != cur) {                                                  // :456-465
      float Tic[12];
      pose_mul(Tiw, Twc, Tic);
      cor = sim3_mul(sim3_from_pose(Tic), Scw);
    }
    const Sim3d siw = sim3_from_pose(Tiw), inv = sim3_inverse(cor);     // :467-471, :479
    E.siw_q[0] = siw.r.x; E.siw_q[1] = siw.r.y; E.siw_q[2] = siw.r.z; E.siw_q[3] = siw.r.w;
    E.inv_q[0] = inv.r.x; E.inv_q[1] = inv.r.y; E.inv_q[2] = inv.r.z; E.inv_q[3] = inv.r.w;
    double R[9];
    fb::quat_to_R(cor.r, R);
    const double is = 1. / cor.s;                                       // :533
    for (int r = 0; r < 3; r++) {
      E.siw_t[r] = siw.t[r]; E.inv_t[r] = inv.t[r];
      for (int c = 0; c < 3; c++) E.Tcw[r * 4 + c] = (float)R[r * 3 + c];
      E.Tcw[r * 4 + 3] = (float)(cor.t[r] * is);
    }
    E.inv_s = inv.s;
    fb::camera_centre(E.Tcw, E.ow_new);
    if (A.d_set_Scw) {                                                  // Converter::toCvMat(CorrectedSim3): s * R | t, cast once
      float *o = A.d_set_Scw + (size_t)p * 12;
      for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) o[r * 4 + c] = (float)(cor.s * R[r * 3 + c]);
        o[r * 4 + 3] = (float)cor.t[r];
      }
    }
  }
}

// mnCorrectedByKF as a minimum: block p takes the features of the set member at position p
__global__ __launch_bounds__(CL_NT) void k_cl_owner(fb_covis_map M, ClS S, int32_t *err) {
  const int p = blockIdx.x;
  if (p >= S.hdr[CH_NSET]) return;
  const int slot = S.tab[p].slot, N = min(max(M.kf_n[slot], 0), M.kp_stride);
  const int32_t *mps = M.kf_mp + (size_t)slot * M.kp_stride;
  for (int i = threadIdx.x; i < N; i += CL_NT) {
    const int mp = mps[i];
    if (mp < 0) continue;                                               // :487
    if (mp >= M.n_mp) { atomicAdd(err, 1); continue; }
    if (M.mp_bad[mp]) continue;                                         // :489
    atomicMin(&S.owner[mp], p);
  }
}

__device__ __forceinline__ void cl_move(const ClEntry &E, float *X) {   // :495-500
  Sim3d siw, inv;
  siw.r.x = E.siw_q[0]; siw.r.y = E.siw_q[1]; siw.r.z = E.siw_q[2]; siw.r.w = E.siw_q[3]; siw.s = 1.0;
  inv.r.x = E.inv_q[0]; inv.r.y = E.inv_q[1]; inv.r.z = E.inv_q[2]; inv.r.w = E.inv_q[3]; inv.s = E.inv_s;
  for (int r = 0; r < 3; r++) { siw.t[r] = E.siw_t[r]; inv.t[r] = E.inv_t[r]; }
  const double P[3] = {X[0], X[1], X[2]};
  double c[3], w[3];
  sim3_map(siw, P, c);
  sim3_map(inv, c, w);
  X[0] = (float)w[0]; X[1] = (float)w[1]; X[2] = (float)w[2];
}

// One thread per map point: the move by its holder, then UpdateNormalAndDepth (MapPoint.cc:330-371) over its live edges in
// ascending kf_order (a selection over the point's few edges: the sum of CV_32F unit vectors depends on the order).  The
// arithmetic is nd_unit / nd_finish of covis_points.inc, the one copy k_pt_refresh uses too.
__global__ __launch_bounds__(CL_NT) void k_cl_move(fb_covis_map M, Gr G, const int32_t *start, const int32_t *csr, fb_correct_loop_args A,
                                                   float *mp_xw, int n_levels, ClS S) {
  const int mp = blockIdx.x * CL_NT + threadIdx.x;
  if (mp >= M.n_mp) return;
  const int p = S.owner[mp];
  if (p == CL_NONE) { A.d_mp_corrected_ref[mp] = -1; return; }
  const ClEntry &E = S.tab[p];
  float X[3] = {mp_xw[(size_t)mp * 3], mp_xw[(size_t)mp * 3 + 1], mp_xw[(size_t)mp * 3 + 2]};
  cl_move(E, X);
  mp_xw[(size_t)mp * 3] = X[0]; mp_xw[(size_t)mp * 3 + 1] = X[1]; mp_xw[(size_t)mp * 3 + 2] = X[2];
  A.d_mp_corrected_ref[mp] = E.slot;                                    // :502
  const int p0 = start[mp], p1 = start[mp + 1];
  if (p0 == p1) return;                                                 // observations.empty()
  const int ref = A.mp_ref_kf[mp];
  if (ref < 0 || ref >= G.K) { atomicAdd(G.err, 1); return; }           // the reference dereferences pRefKF
  auto centre = [&](int kf) {                                           // GetCameraCenter() at this moment of the loop
    const int q = S.pos[kf];
    return (q >= 0 && q < p) ? S.tab[q].ow_new : S.ow_old + (size_t)kf * 3;
  };
  int ref_idx = 0;                                                      // observations[pRefKF] inserts 0 when it is not there
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  int n = 0, last = -1;
  for (;;) {
    int best = INT_MAX, be = -1;
    for (int q = p0; q < p1; q++) {
      const int e = csr[q], r = G.rank[M.obs_kf[e]];                    // in [0, K): the index holds checked edges only
      if (r > last && (r < best || (r == best && e > be))) { best = r; be = e; }   // (a repeated (mp, kf) edge, which fb_covis_map
                                                                                    // rules out: the later entry, whatever csr's order)
    }
    if (be < 0) break;
    last = best;
    const int kf = M.obs_kf[be];
    if (kf == ref) ref_idx = M.obs_idx[be];
    float u[3];
    nd_unit(X, centre(kf), u);
    nx = nx + u[0]; ny = ny + u[1]; nz = nz + u[2];                     // :355
    n++;
  }
  const int level = M.kf_octave[(size_t)ref * M.kp_stride + ref_idx];   // :361
  if (level >= n_levels) { atomicAdd(G.err, 1); return; }
  const float sum[3] = {nx, ny, nz};
  nd_finish(X, centre(ref), A.scale_factors[level], A.scale_factors[n_levels - 1], sum, n, A.mp_normal + (size_t)mp * 3, A.mp_min_dist + mp,
            A.mp_max_dist + mp);
}

// the (set member, bird feature) pairs of every bird point: block p links the features of the member at position p
__global__ __launch_bounds__(CL_NT) void k_cl_bird_link(fb_covis_kf_tables T, ClS S, int32_t *err) {
  const int p = blockIdx.x;
  if (p >= S.hdr[CH_NSET]) return;
  const int slot = S.tab[p].slot, BS = T.bird_stride, N = min(max(T.kf_nb[slot], 0), BS);
  const int32_t *mps = T.kf_mpb + (size_t)slot * BS;
  for (int i = threadIdx.x; i < N; i += CL_NT) {
    const int mp = mps[i];
    if (mp < 0) continue;                                               // :510
    if (mp >= T.n_mpb) { atomicAdd(err, 1); continue; }
    if (T.mpb_bad[mp]) continue;                                        // :512
    const int pair = p * BS + i;
    S.bnext[pair] = atomicExch(&S.bhead[mp], pair);
  }
}

// One thread per bird point, serial over its holders in ascending kf_order (:506-525; the == at :523 marks nothing).  The
// pairs of one member apply the same transform, so only their number matters.
__global__ __launch_bounds__(CL_NT) void k_cl_bird_move(fb_covis_kf_tables T, ClS S) {
  const int mp = blockIdx.x * CL_NT + threadIdx.x;
  if (mp >= T.n_mpb) return;
  const int head = S.bhead[mp], BS = T.bird_stride;
  if (head < 0) return;
  float X[3] = {T.mpb_xw[(size_t)mp * 3], T.mpb_xw[(size_t)mp * 3 + 1], T.mpb_xw[(size_t)mp * 3 + 2]};
  int last = -1;
  for (;;) {
    int best = INT_MAX, times = 0;
    for (int pair = head; pair >= 0; pair = S.bnext[pair]) {
      const int p = pair / BS;
      if (p <= last) continue;
      if (p < best) { best = p; times = 1; }
      else if (p == best) times++;
    }
    if (best == INT_MAX) break;
    last = best;
    for (int k = 0; k < times; k++) cl_move(S.tab[best], X);
  }
  T.mpb_xw[(size_t)mp * 3] = X[0]; T.mpb_xw[(size_t)mp * 3 + 1] = X[1]; T.mpb_xw[(size_t)mp * 3 + 2] = X[2];
}

// SetPose(correctedTiw) of every set member (:529-537), after every read of an old pose
__global__ __launch_bounds__(CL_NT) void k_cl_poses(float *kf_Tcw, ClS S) {
  const int p = blockIdx.x * CL_NT + threadIdx.x;
  if (p >= S.hdr[CH_NSET]) return;
  const ClEntry &E = S.tab[p];
  float *T = kf_Tcw + (size_t)E.slot * 12;
#pragma unroll
  for (int i = 0; i < 12; i++) T[i] = E.Tcw[i];
}

// ---- RunGlobalBundleAdjustment, the map update ----------------------------------------------------------------------------------
// The breadth-first walk (:715-740), level-synchronous over parent[] by one workgroup.  kf_Tcw is read-only until the walk
// has ended, so every Tchild * Twc_parent is of old poses.
__global__ __launch_bounds__(CV_NT) void k_gba_walk(Gr G, float *kf_Tcw, fb_propagate_gba_args A) {
  __shared__ int s_level[CV_MAXK];
  __shared__ int s_wv[CV_NT / 64];
  const int tid = threadIdx.x, K = G.K;
  for (int i = tid; i < K; i += CV_NT) s_level[i] = -1;
  __syncthreads();
  for (int j = tid; j < A.n_origins; j += CV_NT) {                      // mvpKeyFrameOrigins: distinct roots, or counted and left out
    const int o = A.origins[j];
    if (o < 0 || o >= K || G.parent[o] != -1 || atomicCAS(&s_level[o], -1, 0) != -1) atomicAdd(G.err, 1);
  }
  __syncthreads();
  int added = 1;
  for (int depth = 1; depth <= K && added; depth++) {
    int mine = 0;
    for (int c = tid; c < K; c += CV_NT) {
      if (s_level[c] != -1) continue;
      const int a = G.parent[c];
      if (a < 0 || a == c || !G.linked[c] || s_level[a] != depth - 1) continue;   // GetChilds() of a key frame of the level before
      if (!A.kf_gba[c]) {                                               // :726-731
        float Twc[12], Tchildc[12], Tp[12], Tg[12];
        pose_inverse(kf_Tcw + (size_t)a * 12, Twc);
        pose_mul(kf_Tcw + (size_t)c * 12, Twc, Tchildc);
        for (int i = 0; i < 12; i++) Tp[i] = ld(&A.kf_Tcw_gba[(size_t)a * 12 + i]);
        pose_mul(Tchildc, Tp, Tg);
        for (int i = 0; i < 12; i++) st(&A.kf_Tcw_gba[(size_t)c * 12 + i], Tg[i]);
        A.kf_gba[c] = 1;
      }
      mine++;
    }
    added = fb::block_sum<CV_NT>(mine, s_wv);
    __syncthreads();
    for (int c = tid; c < K; c += CV_NT) {                              // after the tests of this level: a level is read, never its own
      if (s_level[c] != -1) continue;
      const int a = G.parent[c];
      if (a >= 0 && a != c && G.linked[c] && s_level[a] == depth - 1) s_level[c] = depth;
    }
    group_sync();
  }
  if (added && tid == 0) atomicAdd(G.err, 1);                           // deeper than K levels: not a tree
  for (int i = tid; i < K; i += CV_NT) {                                // :736-737
    const bool in = s_level[i] >= 0;
    A.d_reached[i] = in ? 1 : 0;
    if (!in) continue;
    for (int k = 0; k < 12; k++) {
      A.kf_Tcw_bef[(size_t)i * 12 + k] = kf_Tcw[(size_t)i * 12 + k];
      kf_Tcw[(size_t)i * 12 + k] = A.kf_Tcw_gba[(size_t)i * 12 + k];
    }
  }
}

// :747-779 (bird = 0) and :784-825 (bird = 1, where a reference of -1 is pRefKF == NULL): one thread per point
__global__ __launch_bounds__(CL_NT) void k_gba_points(int K, int n, const uint8_t *bad, float *xw, const uint8_t *flag, const float *pos_gba,
                                                      const int32_t *ref_kf, const uint8_t *kf_gba, const float *kf_Tcw, const float *kf_Tcw_bef,
                                                      int bird, int32_t *err) {
  const int i = blockIdx.x * CL_NT + threadIdx.x;
  if (i >= n) return;
  if (bad[i]) return;
  float *X = xw + (size_t)i * 3;
  if (flag[i]) {
    X[0] = pos_gba[(size_t)i * 3]; X[1] = pos_gba[(size_t)i * 3 + 1]; X[2] = pos_gba[(size_t)i * 3 + 2];
    return;
  }
  const int ref = ref_kf[i];
  if (bird && ref == -1) return;                                        // :799-803
  if (ref < 0 || ref >= K) { atomicAdd(err, 1); return; }               // the reference dereferences pRefKF
  if (!kf_gba[ref]) return;                                             // :764, :810
  const float P[3] = {X[0], X[1], X[2]};
  float Xc[3], Twc[12], W[3];
  pose_apply(kf_Tcw_bef + (size_t)ref * 12, P, Xc);                     // :768-770
  pose_inverse(kf_Tcw + (size_t)ref * 12, Twc);                         // :773-775
  pose_apply(Twc, Xc, W);
  X[0] = W[0]; X[1] = W[1]; X[2] = W[2];
}

bool cl_has_bird(const fb_covis_kf_tables *T) { return T->kf_mpb != nullptr; }

int check_correct_loop(const fb_covis *g, const fb_covis_map *M, const fb_covis_kf_tables *T, const fb_correct_loop_args *a) {
  FB_ARG(T && a);
  FB_ARG(a->cur_slot >= 0 && a->cur_slot < g->K);
  FB_ARG(a->reuse_index == 0 || a->reuse_index == 1);
  FB_ARG(T->kf_Tcw && T->n_levels >= 1 && T->n_levels <= FB_MAX_LEVELS && a->scale_factors);
  FB_ARG(a->d_n_set && a->d_set_slots);
  FB_ARG(M->n_mp == 0 || (T->mp_xw && a->mp_ref_kf && a->mp_normal && a->mp_min_dist && a->mp_max_dist && a->d_mp_corrected_ref));
  if (cl_has_bird(T)) {
    FB_ARG(T->bird_stride >= 1 && T->bird_stride <= FB_COVIS_MAX_STRIDE && T->n_mpb >= 0 && T->n_mpb < INT_MAX && T->kf_nb);
    FB_ARG((size_t)g->K * (size_t)T->bird_stride < (size_t)INT_MAX);    // a (position, feature) pair is an int
    FB_ARG(T->n_mpb == 0 || (T->mpb_bad && T->mpb_xw));
  }
  return FB_OK;
}

int check_propagate_gba(const fb_covis_map *M, const fb_covis_kf_tables *T, const fb_propagate_gba_args *a) {
  FB_ARG(T && a);
  FB_ARG(a->n_origins >= 0 && (a->n_origins == 0 || a->origins));
  FB_ARG(T->kf_Tcw && a->kf_gba && a->kf_Tcw_gba && a->kf_Tcw_bef && a->d_reached);
  FB_ARG(M->n_mp == 0 || (T->mp_xw && a->mp_gba && a->mp_pos_gba && a->mp_ref_kf));
  if (T->mpb_xw) {
    FB_ARG(T->n_mpb >= 0 && T->n_mpb < INT_MAX);
    FB_ARG(T->n_mpb == 0 || (T->mpb_bad && a->mpb_gba && a->mpb_pos_gba && a->mpb_ref_kf));
  }
  return FB_OK;
}

}  // namespace

extern "C" {

int fb_covis_reserve_correct_loop(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_q, int32_t n_mpb, int32_t bird_stride) {
  FB_ARG(g);
  FB_ARG(n_mp >= 0 && n_mp < INT_MAX && n_obs >= 0 && n_q >= 0 && n_q <= g->K && n_mpb >= 0 && n_mpb < INT_MAX);
  FB_ARG(bird_stride >= 0 && bird_stride <= FB_COVIS_MAX_STRIDE);
  ClOff co;
  return g->reserve(plan_map_call(g->K, n_mp, n_obs, n_q, plan_correct_loop(g->K, n_mp, n_mpb, bird_stride, &co)));
}

int fb_covis_correct_loop_dev(fb_covis *g, const fb_covis_map *M, const fb_covis_kf_tables *T, const fb_correct_loop_args *a, void *stream) {
  FB_ARG(g);
  FB_TRY(check_map(g, M));
  FB_TRY(check_correct_loop(g, M, T, a));
  FB_TRY(g->ensure());
  hipStream_t s = fb::as_stream(stream);
  const bool bird = cl_has_bird(T);
  const size_t K = g->K, n_mp = M->n_mp, n_mpb = bird ? T->n_mpb : 0, BS = bird ? T->bird_stride : 0;
  ClOff co;
  IndexAsk ask;
  ask.reuse = a->reuse_index != 0; ask.tail = plan_correct_loop(K, n_mp, n_mpb, BS, &co);
  Index ix;
  uint8_t *tail;
  FB_TRY(g->acquire(*M, ask, &ix, &tail, s));
  ClS S;
  cl_map(tail, co, &S);
  k_cl_set<<<1, CV_NT, 0, s>>>(g->G, T->kf_Tcw, *a, S);
  if (n_mp) {
    FB_HIP(hipMemsetAsync(S.owner, 0x7f, n_mp * 4, s));
    k_cl_owner<<<(unsigned)K, CL_NT, 0, s>>>(*M, S, g->G.err);
    k_cl_move<<<(unsigned)((n_mp + CL_NT - 1) / CL_NT), CL_NT, 0, s>>>(*M, g->G, ix.start, ix.csr, *a, T->mp_xw, T->n_levels, S);
  }
  if (n_mpb) {
    FB_HIP(hipMemsetAsync(S.bhead, 0xff, n_mpb * 4, s));
    k_cl_bird_link<<<(unsigned)K, CL_NT, 0, s>>>(*T, S, g->G.err);
    k_cl_bird_move<<<(unsigned)((n_mpb + CL_NT - 1) / CL_NT), CL_NT, 0, s>>>(*T, S);
  }
  k_cl_poses<<<(unsigned)((K + CL_NT - 1) / CL_NT), CL_NT, 0, s>>>(T->kf_Tcw, S);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_correct_loop(fb_covis *g, const fb_covis_map *HM, const fb_covis_kf_tables *HT, const fb_correct_loop_args *ha) {
  FB_ARG(g);
  FB_TRY(check_map(g, HM));
  FB_TRY(check_correct_loop(g, HM, HT, ha));
  FB_TRY(g->ensure());
  fb_covis_map M = *HM;
  fb_covis_kf_tables T;
  memset(&T, 0, sizeof(T));                                             // the fields the call does not read stay NULL
  fb_correct_loop_args A = *ha;
  const size_t K = g->K, n_mp = M.n_mp;
  T.kf_Tcw = HT->kf_Tcw; T.n_levels = HT->n_levels; T.mp_xw = HT->mp_xw;
  fb::Stager st;
  stage_map(st, M);
  st.in(A.scale_factors, (size_t)T.n_levels * 4); st.in(A.mp_ref_kf, n_mp * 4);
  // copy-in: what the call leaves alone keeps the caller's contents
  st.out(T.kf_Tcw, K * 48, true); st.out(T.mp_xw, n_mp * 12, true);
  st.out(A.mp_normal, n_mp * 12, true); st.out(A.mp_min_dist, n_mp * 4, true); st.out(A.mp_max_dist, n_mp * 4, true);
  st.out(A.d_mp_corrected_ref, n_mp * 4, false); st.out(A.d_n_set, 4, false); st.out(A.d_set_slots, K * 4, true);
  st.out(A.d_set_Scw, K * 48, true);
  if (cl_has_bird(HT)) {
    T.bird_stride = HT->bird_stride; T.n_mpb = HT->n_mpb; T.kf_nb = HT->kf_nb; T.kf_mpb = HT->kf_mpb; T.mpb_bad = HT->mpb_bad;
    T.mpb_xw = HT->mpb_xw;
    st.in(T.kf_nb, K * 4); st.in(T.kf_mpb, K * (size_t)T.bird_stride * 4); st.in(T.mpb_bad, (size_t)T.n_mpb);
    st.out(T.mpb_xw, (size_t)T.n_mpb * 12, true);
  }
  FB_TRY(st.commit(nullptr));
  A.reuse_index = 0;   // the staged arrays are new device arrays every call
  IndexDropGuard drop(g->state);
  FB_TRY(fb_covis_correct_loop_dev(g, &M, &T, &A, nullptr));
  return st.fetch(nullptr);
}

int fb_covis_propagate_gba_dev(fb_covis *g, const fb_covis_map *M, const fb_covis_kf_tables *T, const fb_propagate_gba_args *a, void *stream) {
  FB_ARG(g);
  FB_TRY(check_map(g, M));
  FB_TRY(check_propagate_gba(M, T, a));
  FB_TRY(g->ensure());
  hipStream_t s = fb::as_stream(stream);
  k_gba_walk<<<1, CV_NT, 0, s>>>(g->G, T->kf_Tcw, *a);
  if (M->n_mp)
    k_gba_points<<<(unsigned)((M->n_mp + CL_NT - 1) / CL_NT), CL_NT, 0, s>>>(g->K, M->n_mp, M->mp_bad, T->mp_xw, a->mp_gba, a->mp_pos_gba,
                                                                              a->mp_ref_kf, a->kf_gba, T->kf_Tcw, a->kf_Tcw_bef, 0, g->G.err);
  if (T->mpb_xw && T->n_mpb)
    k_gba_points<<<(unsigned)((T->n_mpb + CL_NT - 1) / CL_NT), CL_NT, 0, s>>>(g->K, T->n_mpb, T->mpb_bad, T->mpb_xw, a->mpb_gba, a->mpb_pos_gba,
                                                                               a->mpb_ref_kf, a->kf_gba, T->kf_Tcw, a->kf_Tcw_bef, 1, g->G.err);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_covis_propagate_gba(fb_covis *g, const fb_covis_map *HM, const fb_covis_kf_tables *HT, const fb_propagate_gba_args *ha) {
  FB_ARG(g);
  FB_TRY(check_map(g, HM));
  FB_TRY(check_propagate_gba(HM, HT, ha));
  FB_TRY(g->ensure());
  fb_covis_map M = *HM;
  fb_covis_kf_tables T;
  memset(&T, 0, sizeof(T));
  fb_propagate_gba_args A = *ha;
  const size_t K = g->K, n_mp = M.n_mp;
  T.kf_Tcw = HT->kf_Tcw; T.mp_xw = HT->mp_xw;
  fb::Stager st;
  stage_map(st, M);
  st.in(A.origins, (size_t)A.n_origins * 4);
  st.in(A.mp_gba, n_mp); st.in(A.mp_pos_gba, n_mp * 12); st.in(A.mp_ref_kf, n_mp * 4);
  st.out(T.kf_Tcw, K * 48, true); st.out(T.mp_xw, n_mp * 12, true);
  st.out(A.kf_gba, K, true); st.out(A.kf_Tcw_gba, K * 48, true); st.out(A.kf_Tcw_bef, K * 48, true); st.out(A.d_reached, K, false);
  if (HT->mpb_xw) {
    T.n_mpb = HT->n_mpb; T.mpb_bad = HT->mpb_bad; T.mpb_xw = HT->mpb_xw;
    const size_t n_mpb = T.n_mpb;
    st.in(T.mpb_bad, n_mpb); st.in(A.mpb_gba, n_mpb); st.in(A.mpb_pos_gba, n_mpb * 12); st.in(A.mpb_ref_kf, n_mpb * 4);
    st.out(T.mpb_xw, n_mpb * 12, true);
  } else {
    A.mpb_gba = nullptr; A.mpb_pos_gba = nullptr; A.mpb_ref_kf = nullptr;
  }
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_covis_propagate_gba_dev(g, &M, &T, &A, nullptr));
  return st.fetch(nullptr);
}

}  // extern "C"
