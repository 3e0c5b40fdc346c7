// track_stages.inc -- the stages of the tracking chain on a frame handle: each fills the argument block of a matcher / the
// pose optimiser from the handle's pointer blocks, launches the glue kernel around it and says which stream it runs on
// (part of track.hip, after struct fb_frame; the C entry points that check arguments and call these follow there).
namespace {

MapDev map_dev(const fb_map_points *m) {
  MapDev M;
  M.stride = m->stride; M.n = m->n; M.bad = m->bad; M.obs_pos = m->obs_pos; M.xw = m->xw; M.normal = m->normal;
  M.max_dist = m->max_dist; M.min_dist = m->min_dist; M.desc = m->desc;
  return M;
}
BirdMapDev bird_dev(const fb_map_points_bird *m) {
  BirdMapDev M;
  M.stride = m->stride; M.n = m->n; M.xw = m->xw; M.desc = m->desc;
  return M;
}
bool map_ok(const fb_frame *f, const fb_map_points *m) {
  return m && m->stride > 0 && m->stride <= f->P.map_cap && m->n && m->bad && m->obs_pos && m->xw && m->normal && m->max_dist && m->min_dist &&
         m->desc && ((uintptr_t)m->desc % 16 == 0);
}
bool bird_ok(const fb_map_points_bird *m) { return m && m->stride > 0 && m->n && m->xw && m->desc && ((uintptr_t)m->desc % 16 == 0); }
dim3 slot_grid(const fb_frame *f) { return dim3((f->cap + TT - 1) / TT, f->B); }

int edges_and_pose(fb_frame *f, const fb_map_points *map, const fb_map_points_bird *mpb, int mode, float wB, float wF, int which,
                   const Commit &C, hipStream_t s) {
  const EdgeOut &E = f->E;
  {
    fb::ProfScope prof_(fb::P_GATHER, s);
    k_edges<<<slot_grid(f), TT, 0, s>>>(f->F, map_dev(map), bird_dev(mpb), f->sig, E, C);
    FB_HIP(hipGetLastError());
  }
  fb_pose_opt_args A;
  memset(&A, 0, sizeof(A));
  A.batch = f->B; A.mode = mode; A.front_stride = f->cap; A.bird_stride = f->cap;
  A.fx = f->P.K[0]; A.fy = f->P.K[1]; A.cx = f->P.K[2]; A.cy = f->P.K[3];
  A.wF = wF; A.wB = wB;
  A.n_front = f->F.n; A.front_xw = E.fxw; A.front_obs = E.fobs; A.front_inv_sigma2 = E.finf; A.front_valid = E.fvalid;
  A.n_bird = f->F.nb; A.bird_xw = E.bxw; A.bird_xc = E.bxc; A.bird_inv_sigma2 = E.binf; A.bird_valid = E.bvalid;
  A.bird_outlier = f->F.boutlier;
  A.Tcw = f->F.Tcw; A.front_outlier = f->F.outlier;
  A.ninliers = f->cnt(which ? FB_CNT_POSE2_INLIERS : FB_CNT_POSE1_INLIERS);
  return fb_pose_opt_batch_dev(&A, s);
}

// A matcher leaves its result in the frame's match buffer; `defer` = the pose optimisation that follows folds it into
// mvpMapPoints / mvpMapPointsBird inside its edge kernel (fb_frame_track_dev), otherwise a commit launch does it here.
int launch_commit(fb_frame *f, const Commit &C, hipStream_t s) {
  fb::ProfScope prof_(fb::P_TRACK_GLUE, s);
  k_commit<<<slot_grid(f), TT, 0, s>>>(f->F, C);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

Commit commit_m9(const fb_frame *cur, const int32_t *d_local) {
  Commit C;
  memset(&C, 0, sizeof(C));
  C.kind = 1; C.match = nullptr; C.match_bird = cur->m_bird; C.local_mpb = d_local; C.lcap_mpb = cur->P.local_mpb_cap;
  return C;
}

int m9_impl(fb_frame *cur, const fb_map_points_bird *mpb, const int32_t *d_local, const int32_t *d_n_local, int window_size,
            float filter_size, const fb_matcher_params *matcher, hipStream_t s) {
  const int B = cur->B, cap = cur->cap, lcap = cur->P.local_mpb_cap;
  const FrameDev &F = cur->F;
  const M9Scratch &S = cur->m9;
  fb_bird_mp_args A;
  memset(&A, 0, sizeof(A));
  { fb::ProfScope prof_(fb::P_TRACK_GLUE, s);
  if (d_local) {
    k_m9_prepare<<<dim3((std::max(lcap, cap) + TT - 1) / TT, B), TT, 0, s>>>(bird_dev(mpb), d_local, d_n_local, lcap, S.valid, S.xw, S.desc,
                                                                          S.n, cur->m_bird, cap);
    A.ref_stride = lcap; A.ref_valid = S.valid; A.ref_xw = S.xw; A.ref_desc = S.desc;
  } else {
    k_m9_prepare_all<<<slot_grid(cur), TT, 0, s>>>(bird_dev(mpb), S.n, cur->m_bird, cap);
    A.ref_stride = mpb->stride; A.ref_valid = S.ones; A.ref_xw = mpb->xw; A.ref_desc = mpb->desc;
  }
  }
  FB_HIP(hipGetLastError());
  A.batch = B; A.cur_stride = cap;
  A.n_cur = F.nb; A.cur_kps = F.bkps; A.cur_desc = F.bdesc;
  A.cur_cam_xyz = F.bcam; A.cur_cell_start = cur->bcs; A.cur_cell_items = cur->bci;
  A.cur_Tcw = F.Tcw; A.n_ref = S.n;
  memcpy(A.Tbc, cur->P.Tbc, sizeof(A.Tbc));
  A.bird_cols = cur->P.bird_width; A.bird_rows = cur->P.bird_height;
  A.meter2pixel = cur->P.meter2pixel; A.rear_axle_to_center = cur->P.rear_axle_to_center;
  A.grid = cur->gB; A.window_size = window_size; A.filter_size = filter_size; A.matcher = *matcher;
  A.match_cur_to_ref = cur->m_bird; A.ninliers = cur->cnt(FB_CNT_BIRD_KF_MATCHES);
  return fb_match_bird_mappoints_dev(&A, s);
}

int m3_impl(fb_frame *cur, const fb_frame *last, const fb_map_points *map, float th, const fb_matcher_params *matcher, hipStream_t s,
            int retry_below = 0) {
  const FrameDev &F = cur->F;
  const M3Scratch &S = cur->m3;
  { fb::ProfScope prof_(fb::P_TRACK_GLUE, s);
    k_m3_prepare<<<slot_grid(cur), TT, 0, s>>>(F, last->F, map_dev(map), S); }
  FB_HIP(hipGetLastError());
  fb_proj_frame_args A;
  memset(&A, 0, sizeof(A));
  A.batch = cur->B; A.cur_stride = cur->cap; A.last_stride = cur->cap;
  A.n_cur = F.n; A.cur_kps = F.kps_un; A.cur_desc = F.desc;
  A.cur_cell_start = cur->cs; A.cur_cell_items = cur->ci; A.cur_blocked = nullptr;
  A.cur_Tcw = F.Tcw;
  A.n_last = last->F.n; A.last_valid = S.valid; A.last_obs_pos = S.obs; A.last_xw = S.xw; A.last_desc = S.desc;
  A.last_octave = S.oct; A.last_angle = S.ang;
  A.cam = cur->cam; A.grid = cur->gF;
  for (int i = 0; i < FB_MAX_LEVELS; i++) A.scale_factors[i] = cur->tab.scale_factor[i];
  A.th = th; A.matcher = *matcher;
  A.match_cur_to_last = cur->m_front; A.nmatches = cur->cnt(FB_CNT_PROJ_MATCHES);
  A.retry_below = retry_below; A.retry_th = 2.0f * th;   // Tracking.cc:1342-1349
  A.retried = retry_below > 0 ? cur->cnt(FB_CNT_PROJ_RETRIED) : nullptr;
  return fb_match_projection_frame_dev(&A, s);
}

int local_impl(fb_frame *f, const fb_map_points *map, const int32_t *d_local, const int32_t *d_n_local, float th,
               const fb_matcher_params *matcher, hipStream_t s, const int32_t *gate_row = nullptr, int gate_min = 0) {
  const int B = f->B, cap = f->cap, lcap = f->P.local_mp_cap;
  const FrameDev &F = f->F;
  const LocalScratch &S = f->loc;
  FrustumK K{f->cam, f->logScale, f->P.orb.nlevels};
  {
    fb::ProfScope prof_(fb::P_FRUSTUM, s);
    k_local_points<<<B, WG, 0, s>>>(F, map_dev(map), d_local, d_n_local, lcap, K, S, f->counts, B, gate_row, gate_min);
    FB_HIP(hipGetLastError());
  }
  fb_proj_points_args A;
  memset(&A, 0, sizeof(A));
  A.batch = B; A.cur_stride = cap; A.mp_stride = lcap;
  A.n_cur = F.n; A.cur_kps = F.kps_un; A.cur_desc = F.desc;
  A.cur_cell_start = f->cs; A.cur_cell_items = f->ci; A.cur_blocked = S.blocked;
  A.n_mp = S.n_eff; A.mp_track = S.inview; A.mp_obs_pos = S.obs; A.mp_proj = S.proj; A.mp_level = S.level; A.mp_view_cos = S.cosv;
  A.mp_desc = S.desc; A.grid = f->gF;
  for (int i = 0; i < FB_MAX_LEVELS; i++) A.scale_factors[i] = f->tab.scale_factor[i];
  A.th = th; A.matcher = *matcher;
  A.match_cur_to_mp = f->m_local; A.nmatches = f->cnt(FB_CNT_LOCAL_MATCHES);
  A.workspace = f->m2_ws; A.workspace_bytes = f->plan.r[FR_m2_ws].bytes;
  return fb_match_projection_points_dev(&A, s);
}

int bird_points_impl(fb_frame *cur, fb_frame *ref, fb_map_points_bird *mpb, int window_size, float filter_size,
                     const fb_matcher_params *matcher, int only_below, hipStream_t s, const int32_t *gate_row = nullptr, int gate_min = 0) {
  const FrameDev &F = cur->F, &R = ref->F;
  const M8Scratch &S = cur->m8;
  fb_birdview_args A;
  memset(&A, 0, sizeof(A));
  A.batch = cur->B; A.cur_stride = cur->cap; A.ref_stride = cur->cap;
  A.n_cur = F.nb; A.cur_kps = F.bkps; A.cur_desc = F.bdesc;
  A.cur_cell_start = cur->bcs; A.cur_cell_items = cur->bci;
  A.n_ref = R.nb; A.ref_kps = R.bkps; A.ref_desc = R.bdesc;
  A.grid = cur->gB; A.window_size = window_size; A.matcher = *matcher;
  A.match_ref_to_cur = S.m12; A.match_dist = S.dist;
  A.nmatches = S.n; A.n_dmatches = S.nd;
  FB_TRY(fb_match_birdview_dev(&A, s));
  const size_t lds = (size_t)cur->cap * 4;
  if (lds > 150 * 1024) { fb::set_error("fb_frame_match_bird_points: %d key points per frame beyond the LDS slot table", cur->cap); return FB_ERR_CAPACITY; }
  FB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_bird_commit), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  fb::ProfScope prof_(fb::P_TRACK_GLUE, s);
  k_bird_commit<<<cur->B, WG, lds, s>>>(F, R, bird_dev(mpb), S.m12, filter_size, cur->counts, cur->B, only_below, gate_row, gate_min, S.n);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int discard_impl(fb_frame *f, const fb_map_points *map, int src_slot, int gate_min, hipStream_t s) {
  fb::ProfScope prof_(fb::P_TRACK_GLUE, s);
  k_discard<<<f->B, WG, 0, s>>>(f->F, map_dev(map), f->counts, f->B, src_slot, gate_min);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

fb_feature_vector frame_fv(const fb_frame *f) {
  fb_feature_vector v;
  v.node_stride = f->cap; v.item_stride = f->cap;
  v.n_nodes = f->bw.fv_nn; v.node_ids = f->bw.fv_ids; v.node_start = f->bw.fv_start; v.items = f->bw.fv_items;
  return v;
}

// SearchByBoW(pKF, F, vpMapPointMatches) (ORBmatcher.cc:160-289): result in cur->m_front, count in FB_CNT_BOW_MATCHES
int bow_impl(fb_frame *cur, const fb_frame *kf, const fb_map_points *map, const fb_matcher_params *matcher, hipStream_t s) {
  { fb::ProfScope prof_(fb::P_TRACK_GLUE, s);
    k_bow_prepare<<<slot_grid(cur), TT, 0, s>>>(kf->F, map_dev(map), cur->bow_has_mp); }
  FB_HIP(hipGetLastError());
  fb_bow_args A;
  memset(&A, 0, sizeof(A));
  A.batch = cur->B; A.kf_stride = cur->cap; A.f_stride = cur->cap;
  A.n_kf = kf->F.n; A.kf_kps = kf->F.kps_un; A.kf_desc = kf->F.desc;
  A.kf_has_mp = cur->bow_has_mp; A.kf_fv = frame_fv(kf);
  A.n_f = cur->F.n; A.f_kps = cur->F.kps; A.f_desc = cur->F.desc; A.f_fv = frame_fv(cur);  // F.mvKeys, :258
  A.matcher = *matcher;
  A.match_f_to_kf = cur->m_front; A.nmatches = cur->cnt(FB_CNT_BOW_MATCHES);
  return fb_match_bow_dev(&A, s);
}

Commit commit_bow(const fb_frame *cur, const fb_frame *kf, int min_matches) {
  Commit C;
  memset(&C, 0, sizeof(C));
  C.kind = 3; C.match = cur->m_front; C.src_mp = kf->F.mp; C.src_stride = cur->cap;
  C.gate = min_matches > 0 ? cur->cnt(FB_CNT_BOW_MATCHES) : nullptr; C.gate_min = min_matches;
  return C;
}

bool track_args_ok(const fb_frame *cur, const fb_track_args *T) {
  return T && map_ok(cur, &T->map) && bird_ok(&T->mpb) && (!T->d_local_mp || T->d_n_local_mp) && (!T->d_local_mpb || T->d_n_local_mpb) &&
         (T->d_local_mp || T->map.stride <= cur->P.local_mp_cap) && (T->d_local_mpb || T->mpb.stride <= cur->P.local_mpb_cap);
}

const fb_matcher_params M09 = {0.9f, 1};  // ORBmatcher matcher(0.9,true), Tracking.cc:1325,2001,2726
const fb_matcher_params M08 = {0.8f, 1};  // ORBmatcher matcher(0.8), Tracking.cc:1988
const fb_matcher_params M07 = {0.7f, 1};  // ORBmatcher matcher(0.7,true), Tracking.cc:1207

// The bird-side step of a stage runs on the handle's own stream beside the front-side step: fork after the producer of what
// both need, join before the edge kernel.  Between the two, the caller's stream writes FRONT scratch and the front members,
// the handle's stream BIRD scratch and the bird members (track_plan.h); both only read the pose, and each writes counter
// rows of its own.  Not while every kernel is bracketed for the per-kernel table (the table shows each kernel on its own).
struct SideStream {
  fb_frame *f; hipStream_t s; bool on;
  SideStream(fb_frame *f_, hipStream_t s_) : f(f_), s(s_), on(!(fb::g_prof_on && fb::g_prof_only < 0) && !getenv("FB_TRACK_NO_FORK")) {}
  hipStream_t side() const { return on ? f->sBird : s; }
  int fork() { if (on) { FB_HIP(hipEventRecord(f->evFork, s)); FB_HIP(hipStreamWaitEvent(f->sBird, f->evFork, 0)); } return FB_OK; }
  int join() { if (on) { FB_HIP(hipEventRecord(f->evJoin, f->sBird)); FB_HIP(hipStreamWaitEvent(s, f->evJoin, 0)); } return FB_OK; }
};

// TrackWithMotionModel (Tracking.cc:1312-1385)
int motion_model_impl(fb_frame *cur, fb_frame *last, const fb_track_args *T, hipStream_t s) {
  fb_map_points_bird mpb = T->mpb;
  FB_TRY(fb_frame_predict_pose_dev(cur, last, T->d_delta, s));                                         // :1314-1320
  SideStream side(cur, s);
  FB_TRY(side.fork());
  FB_TRY(m9_impl(cur, &mpb, T->d_local_mpb, T->d_n_local_mpb, 10, 0.05f, &M09, side.side()));          // :1322-1323 -> :1999-2012
  FB_TRY(m3_impl(cur, last, &T->map, 15.0f, &M09, s, 20));                                             // :1339-1349 (incl. the 2 * th retry)
  FB_TRY(side.join());
  Commit C1 = commit_m9(cur, T->d_local_mpb);
  C1.match = cur->m_front; C1.src_mp = last->F.mp; C1.src_stride = cur->cap;
  // if (nmatches < 20) return false (:1351): the matches are committed, but such a sequence gets no edges (the optimiser leaves
  // its pose and flags alone) and no discard loop
  C1.gate = cur->cnt(FB_CNT_PROJ_MATCHES); C1.gate_min = 20;
  FB_TRY(edges_and_pose(cur, &T->map, &mpb, FB_POSE_FRONT_BIRD, T->wB, T->wF, 0, C1, s));              // :1353
  return discard_impl(cur, &T->map, FB_CNT_PROJ_MATCHES, 20, s);                                       // :1358-1376
}

int finish_impl(fb_frame *f, const fb_map_points *map, const int32_t *gate_row, int gate_min, int keep_outliers, hipStream_t s,
                int min_inliers = 0) {
  f->minInliers = min_inliers > 0 ? min_inliers : 30;
  fb::ProfScope prof_(fb::P_TRACK_GLUE, s);
  k_finish<<<f->B, WG, 0, s>>>(f->F, map_dev(map), f->counts, f->B, gate_row, gate_min, f->minInliers, keep_outliers);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

// TrackLocalMap (Tracking.cc:1387-1441) + the end of Track (:1411-1424, 690-701, 721-725).  gated: a sequence whose first
// stage failed (nmatchesMap < 10: TrackWithMotionModel :1384 / TrackReferenceKeyFrame :1243 returned false; the counter is
// still 0 when the stage returned early) is left alone, as if (bOK) of Tracking.cc:642 leaves it
int local_map_impl(fb_frame *cur, fb_frame *ref, const fb_track_args *T, hipStream_t s, bool gated) {
  fb_map_points_bird mpb = T->mpb;
  const int32_t *gr = gated ? cur->cnt(FB_CNT_MATCHES_MAP) : nullptr;
  const int gm = 10;
  SideStream side(cur, s);
  FB_TRY(side.fork());
  FB_TRY(bird_points_impl(cur, ref, &mpb, 10, 0.05f, &M09, 0, side.side(), gr, gm));                   // :1392 -> :2724-2733
  FB_TRY(local_impl(cur, &T->map, T->d_local_mp, T->d_n_local_mp, 1.0f, &M08, s, gr, gm));             // :1396 -> :1947-1997
  FB_TRY(side.join());
  Commit C2;
  memset(&C2, 0, sizeof(C2));
  C2.kind = 2; C2.match = cur->m_local; C2.src_mp = T->d_local_mp; C2.src_stride = cur->P.local_mp_cap;
  C2.gate = gr; C2.gate_min = gm;
  FB_TRY(edges_and_pose(cur, &T->map, &mpb, FB_POSE_FRONT_BIRD, T->wB, T->wF, 1, C2, s));              // :1400
  return finish_impl(cur, &T->map, gr, gm, T->defer_outlier_drop, s, T->min_inliers);
}

}  // namespace
