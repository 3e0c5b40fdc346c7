// The covisibility handle's memory plan and scratch state (fishbirdeyevisualslam_amd/csrc/covis_plan.h) on the CPU.
// Sweep: K x n_mp x n_obs x n_q x batch x recent_cap x n_features x {no bird side, bird side}.  Per case: every region of
// every part is 256-byte aligned, inside its part and disjoint from the others; the parts of a call follow each other and the
// tail begins at the index's end; the totals of every fb_covis_reserve* equal the size formulas the handle had before the plan
// (copied below from commit 36a7271: that list is the specification); the window's key-frame offsets do not depend on the
// point counts.  Then the state sequences, with no device.
// usage: covis_plan_test   -> prints "cases=<n> failures=<n>", exit status 1 if failures > 0
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../fishbirdeyevisualslam_amd/csrc/covis_plan.h"

static long g_failures = 0, g_cases = 0;
#define CHECK(cond, ...)                                      \
  do {                                                        \
    if (!(cond)) {                                            \
      if (g_failures++ < 20) {                                \
        std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
        std::printf(__VA_ARGS__);                             \
        std::printf("\n");                                    \
      }                                                       \
    }                                                         \
  } while (0)

// ---- the size formulas of commit 36a7271 (covis.hip, covis_window.inc, covis_tree.inc, covis_correct.inc, covis_points.inc),
// literally; OLD_CV_SCAN_TILE = 1024 * 4, PT_NT = 256, LM_EXPAND = 80, LM_NEIGH = 10, LM_HDR = 64, sizeof(ClEntry) = 184
static size_t old_up256(size_t v) { return (v + 255) & ~(size_t)255; }
static const size_t OLD_TILE = 4096;
static size_t old_scratch_bytes(size_t n_mp, size_t n_obs, size_t n_q, size_t k) {
  const size_t nb = (n_mp + 1 + OLD_TILE - 1) / OLD_TILE;
  return old_up256((n_mp + 1) * 4) + 2 * old_up256(n_mp * 4) + 2 * old_up256(n_obs * 4) + old_up256(nb * 4) + old_up256(n_q * k * 2) + 256;
}
static size_t old_win_side_bytes(size_t n_pt) {
  const size_t nb = (n_pt + 1 + OLD_TILE - 1) / OLD_TILE;
  return 2 * old_up256(n_pt * 4) + old_up256((n_pt + 1) * 4) + old_up256(nb * 4);
}
static size_t old_win_head_bytes(size_t K, size_t n_mp, size_t n_mpb) {
  return 256 + 4 * old_up256(K * 4) + old_up256(K) + old_up256(K * 8) + old_win_side_bytes(n_mp) + old_win_side_bytes(n_mpb);
}
static size_t old_lm_list(size_t K) { return K > 84 ? K : 84; }
static size_t old_lm_bytes(size_t batch, size_t K, size_t n_mp) {
  return batch * (old_up256(64 * 4) + old_up256(80 * 4) + old_up256((size_t)80 * 10 * 4) + old_up256(old_lm_list(K) * 4)) +
         old_up256(old_lm_list(K) * 4) + 2 * old_up256(n_mp * 4);
}
static size_t old_cl_bytes(size_t K, size_t n_mp, size_t n_mpb, size_t BS) {
  return 256 + old_up256(K * 4) + old_up256(K * 184) + old_up256(K * 12) + old_up256(n_mp * 4) + old_up256(n_mpb * 4) + old_up256(K * BS * 4);
}
static size_t old_mpc_bytes(size_t n_mp, size_t cap) { return old_up256(n_mp * 4) + 3 * old_up256(cap * 4) + old_up256(((cap + 256 - 1) / 256) * 12 + 12); }
static size_t old_pnk_bytes(size_t n_features) { return 2 * old_up256(n_features * 4) + 256; }
static size_t old_graph_bytes(size_t k) {   // fb_covis::ensure(): oFirst + up256(k)
  const size_t oRank = old_up256(k * k * 2), oInv = oRank + old_up256(k * 4), oErr = oInv + old_up256(k * 4), oPar = oErr + 256,
               oLink = oPar + old_up256(k * 4), oFirst = oLink + old_up256(k);
  return oFirst + old_up256(k);
}

struct Reg { const char *name; size_t off, bytes; };

// aligned, inside [0, total), pairwise disjoint
static void check_regions(const char *tag, const char *part, const std::vector<Reg> &R, size_t total) {
  CHECK(total % 256 == 0, "%s: %s has %zu bytes", tag, part, total);
  for (size_t i = 0; i < R.size(); i++) {
    CHECK(R[i].off % 256 == 0 && R[i].off + R[i].bytes <= total, "%s: %s.%s is [%zu, +%zu) of %zu", tag, part, R[i].name, R[i].off, R[i].bytes, total);
    for (size_t j = 0; j < i; j++)
      CHECK(!(R[i].off < R[j].off + R[j].bytes && R[j].off < R[i].off + R[i].bytes), "%s: %s.%s and %s.%s overlap", tag, part, R[j].name, part, R[i].name);
  }
}

static void check_call(const char *tag, const char *what, const CallPlan &c, size_t head, size_t front, size_t bird, size_t tail, size_t old_total) {
  CHECK(c.head == 0 && c.front == head && c.bird == head + front && c.tail == head + front + bird && c.total == head + front + bird + tail,
        "%s: %s: parts at %zu %zu %zu %zu, total %zu", tag, what, c.head, c.front, c.bird, c.tail, c.total);
  CHECK(c.total == old_total, "%s: %s: %zu bytes, the formula gave %zu", tag, what, c.total, old_total);
  CHECK(c.front % 256 == 0 && c.bird % 256 == 0 && c.tail % 256 == 0, "%s: %s: a part is not 256-aligned", tag, what);
}

static void check_plan(size_t K, size_t n_mp, size_t n_obs, size_t n_q, size_t batch, size_t cap, size_t NF, size_t n_mpb, size_t n_bobs, size_t BS) {
  char tag[160];
  std::snprintf(tag, sizeof(tag), "K=%zu n_mp=%zu n_obs=%zu n_q=%zu batch=%zu cap=%zu NF=%zu n_mpb=%zu BS=%zu", K, n_mp, n_obs, n_q, batch, cap, NF, n_mpb, BS);
  g_cases++;
  const size_t nb = (n_mp + 1 + 4095) / 4096, nbb = (n_mpb + 1 + 4095) / 4096, L = old_lm_list(K);

  GraphOff go;
  const size_t graph = plan_graph(K, &go);
  check_regions(tag, "graph", {{"W", go.W, K * K * 2}, {"rank", go.rank, K * 4}, {"inv", go.inv, K * 4}, {"err", go.err, 4}, {"parent", go.parent, K * 4},
                               {"linked", go.linked, K}, {"first", go.first, K}}, graph);
  CHECK(graph == old_graph_bytes(K), "%s: graph %zu, was %zu", tag, graph, old_graph_bytes(K));

  IndexOff io;
  const size_t index = plan_index(n_mp, n_obs, n_q, K, &io);
  check_regions(tag, "index", {{"start", io.start, (n_mp + 1) * 4}, {"fill", io.fill, n_mp * 4}, {"nobs", io.nobs, n_mp * 4}, {"csr", io.csr, n_obs * 4},
                               {"dead", io.dead, n_obs * 4}, {"bsum", io.bsum, nb * 4}, {"counter", io.counter, n_q * K * 2}}, index);
  CHECK(io.start == 0 && io.fill == old_up256((n_mp + 1) * 4) && io.nobs == io.fill + old_up256(n_mp * 4), "%s: one memset of [start, nobs) clears start and fill", tag);
  IndexOff io0;
  const size_t index0 = plan_index(n_mp, n_obs, 0, K, &io0);   // a reuse maps the index without knowing its n_q
  CHECK(index0 <= index && io0.start == io.start && io0.fill == io.fill && io0.nobs == io.nobs && io0.csr == io.csr && io0.dead == io.dead &&
        io0.bsum == io.bsum, "%s: the index arrays move with n_q", tag);
  IndexOff iob;
  const size_t indexb = plan_index(n_mpb, n_bobs, 0, K, &iob);

  WinOff wo, wk, w0;
  const size_t win = plan_window(K, n_mp, n_mpb, &wo);
  std::vector<Reg> wr = {{"hdr", wo.hdr, 256}, {"lpos", wo.lpos, K * 4}, {"widx", wo.widx, K * 4}, {"wslot", wo.wslot, K * 4}, {"rowcnt", wo.rowcnt, K * 4},
                         {"wfixed", wo.wfixed, K}, {"fixkey", wo.fixkey, K * 8}};
  const size_t npt[2] = {n_mp, n_mpb}, nbs[2] = {nb, nbb};
  for (int sd = 0; sd < 2; sd++) {
    wr.push_back({"ptkey", wo.side[sd].ptkey, npt[sd] * 4}); wr.push_back({"plist", wo.side[sd].plist, npt[sd] * 4});
    wr.push_back({"eoff", wo.side[sd].eoff, (npt[sd] + 1) * 4}); wr.push_back({"bsum", wo.side[sd].bsum, nbs[sd] * 4});
  }
  check_regions(tag, "window", wr, win);
  CHECK(win == old_win_head_bytes(K, n_mp, n_mpb), "%s: window head %zu, was %zu", tag, win, old_win_head_bytes(K, n_mp, n_mpb));
  Regions rk;
  memset(&wk, 0xff, sizeof(wk));
  win_kf_regions(rk, K, &wk);
  plan_window(K, 0, 0, &w0);
  CHECK(wk.hdr == wo.hdr && wk.wslot == wo.wslot && wk.wfixed == wo.wfixed && w0.hdr == wo.hdr && w0.wslot == wo.wslot && w0.wfixed == wo.wfixed &&
        rk.off <= wo.side[0].ptkey, "%s: the window's key-frame arrays depend on the point counts", tag);

  LmOff lo;
  const size_t lm = plan_local_map(batch, K, n_mp, &lo);
  check_regions(tag, "local map", {{"hdr", lo.hdr, batch * 256}, {"voters", lo.voters, batch * old_up256(80 * 4)}, {"rows", lo.rows, batch * old_up256(80 * 10 * 4)},
                                   {"wslot", lo.wslot, batch * old_up256(L * 4)}, {"rowcnt", lo.rowcnt, L * 4}, {"ptkey", lo.ptkey, n_mp * 4},
                                   {"plist", lo.plist, n_mp * 4}}, lm);
  CHECK(lm == old_lm_bytes(batch, K, n_mp) && (size_t)lo.list == L, "%s: local map %zu (list %d), was %zu (%zu)", tag, lm, lo.list, old_lm_bytes(batch, K, n_mp), L);

  ClOff co;
  const size_t cl = plan_correct_loop(K, n_mp, n_mpb, BS, &co);
  check_regions(tag, "correct loop", {{"hdr", co.hdr, 256}, {"pos", co.pos, K * 4}, {"tab", co.tab, K * 184}, {"ow_old", co.ow_old, K * 12},
                                      {"owner", co.owner, n_mp * 4}, {"bhead", co.bhead, n_mpb * 4}, {"bnext", co.bnext, K * BS * 4}}, cl);
  CHECK(cl == old_cl_bytes(K, n_mp, n_mpb, BS) && co.tab % 8 == 0, "%s: correct loop %zu, was %zu", tag, cl, old_cl_bytes(K, n_mp, n_mpb, BS));

  MpcOff mo;
  const size_t mpc = plan_point_culling(n_mp, cap, &mo);
  const size_t blocks = (cap + 255) / 256;   // k_mpc_count writes 3 ints per block of PT_NT entries
  check_regions(tag, "point culling", {{"first", mo.first, n_mp * 4}, {"val", mo.val, cap * 4}, {"dec", mo.dec, cap * 4}, {"rowbase", mo.rowbase, cap * 4},
                                       {"bcnt", mo.bcnt, blocks * 12}}, mpc);
  CHECK(mpc == old_mpc_bytes(n_mp, cap), "%s: point culling %zu, was %zu", tag, mpc, old_mpc_bytes(n_mp, cap));

  PnkOff po;
  const size_t pnk = plan_new_keyframe(NF, &po);
  check_regions(tag, "new key frame", {{"gain", po.gain, NF * 4}, {"gain_idx", po.gain_idx, NF * 4}, {"n_gain", po.n_gain, 4}}, pnk);
  CHECK(pnk == old_pnk_bytes(NF), "%s: new key frame %zu, was %zu", tag, pnk, old_pnk_bytes(NF));

  // the seven reserves
  const size_t sb = old_scratch_bytes(n_mp, n_obs, n_q, K);
  CHECK(index == sb, "%s: index %zu, was %zu", tag, index, sb);
  check_call(tag, "reserve / reserve_refresh_points", plan_map_call(K, n_mp, n_obs, n_q, 0), 0, index, 0, 0, sb);
  check_call(tag, "reserve_window", plan_window_call(K, n_mp, n_obs, n_mpb, n_bobs), win, index0, indexb, 0,
             old_win_head_bytes(K, n_mp, n_mpb) + old_scratch_bytes(n_mp, n_obs, 0, K) + old_scratch_bytes(n_mpb, n_bobs, 0, K));
  WinOff w1;
  for (int ww = 0; ww < 2; ww++)
    check_call(tag, "reserve_local_map", plan_local_map_call(K, n_mp, n_obs, n_q, batch, ww != 0), ww ? plan_window(K, n_mp, 0, &w1) : 0, index, 0, lm,
               (ww ? old_win_head_bytes(K, n_mp, 0) : 0) + sb + old_lm_bytes(batch, K, n_mp));
  check_call(tag, "reserve_correct_loop", plan_map_call(K, n_mp, n_obs, n_q, cl), 0, index, 0, cl, sb + old_cl_bytes(K, n_mp, n_mpb, BS));
  check_call(tag, "reserve_process_new_keyframe", plan_map_call(K, n_mp, n_obs, n_q, pnk), 0, index, 0, pnk, sb + old_pnk_bytes(NF));
  check_call(tag, "reserve_map_point_culling", plan_map_call(K, n_mp, n_obs, n_q, mpc), 0, index, 0, mpc, sb + old_mpc_bytes(n_mp, cap));

  // a call on an empty scratch: the index at its head, the tail at the index's end, the total the plan's
  ScratchState S{};
  fb_covis_map M;
  memset(&M, 0, sizeof(M));
  const IndexStep st = scratch_decide(S, true, M, win, index, lm);
  CHECK(!st.reuse && !st.refused && st.index_at == win && st.tail_at == win + index && st.total == win + index + lm, "%s: a first call", tag);
}

// ---- the state ------------------------------------------------------------------------------------------------------------
static fb_covis_map a_map(int n_mp, const void *arrays) {
  fb_covis_map M;
  memset(&M, 0, sizeof(M));
  M.max_keyframes = 64; M.kp_stride = 100; M.n_mp = n_mp; M.n_obs = 5000;
  M.kf_n = static_cast<const int32_t *>(arrays); M.kf_mp = M.kf_n; M.obs_mp = M.kf_n; M.obs_kf = M.kf_n; M.obs_idx = M.kf_n;
  return M;
}

// what fb_covis::acquire does with the state, without the device: `enqueue_ok` stands for the build's result
static IndexStep acquire(ScratchState &S, bool reuse, const fb_covis_map &M, size_t head, size_t index_bytes, size_t tail, bool kept = true, bool enqueue_ok = true) {
  const IndexStep st = scratch_decide(S, reuse, M, head, index_bytes, tail);
  if (st.refused || st.reuse) return st;
  if (st.total > S.capacity) scratch_grown(S, st.total);
  scratch_build_begins(S, st.index_at, kept);
  if (enqueue_ok) scratch_build_done(S, st.index_at, st.tail_at, M, kept);
  return st;
}

static void check_states() {
  static int32_t arrays_a[4], arrays_b[4];
  const size_t K = 64, n_mp = 1000, n_obs = 5000, n_mpb = 300, n_bobs = 900;
  const fb_covis_map A = a_map((int)n_mp, arrays_a), B = a_map((int)n_mp, arrays_b), Bird = a_map((int)n_mpb, arrays_b);
  IndexOff io;
  WinOff wo;
  LmOff lo;
  const size_t index = plan_index(n_mp, n_obs, 0, K, &io), bindex = plan_index(n_mpb, n_bobs, 0, K, &io), head = plan_window(K, n_mp, n_mpb, &wo),
               lm = plan_local_map(1, K, n_mp, &lo);
  auto window = [&](ScratchState &S, bool bird) {   // fb_covis_local_window_dev
    const CallPlan c = plan_call(head, index, bird ? bindex : plan_index(0, 0, 0, K, &io), 0);
    scratch_window_begins(S);
    acquire(S, false, A, c.front, index, c.total - c.bird);
    if (bird) acquire(S, false, Bird, c.bird, bindex, 0, false);
    scratch_window_done(S, c.front, 40);
    return c;
  };

  {  // window -> reuse with a tail that fits keeps both
    g_cases++;
    ScratchState S{};
    scratch_grown(S, head + index + bindex + lm);
    const CallPlan c = window(S, false);
    CHECK(S.win_valid && S.win_bytes == head && S.win_cap_kf == 40 && S.index_valid && S.index_head == head && S.index_end == c.bird, "a window leaves its head and its front index");
    const IndexStep st = acquire(S, true, A, 0, index, lm);
    CHECK(st.reuse && st.index_at == head && st.tail_at == c.bird && S.win_valid && S.index_valid, "a reuse behind the window keeps both");
  }
  {  // window -> index at head 0 drops the window (update_connections, keyframe_culling, any rebuild)
    g_cases++;
    ScratchState S{};
    scratch_grown(S, head + index + bindex + lm);
    window(S, false);
    const IndexStep st = acquire(S, false, A, 0, index, 0);
    CHECK(!st.reuse && st.index_at == 0 && !S.win_valid && S.index_valid && S.index_head == 0 && S.index_end == index, "an index at offset 0 ends the window");
  }
  {  // growth drops both
    g_cases++;
    ScratchState S{};
    const CallPlan c = window(S, false);   // grows from nothing to the window's total
    CHECK(S.capacity == c.total && S.win_valid && S.index_valid, "the window sized the scratch");
    const IndexStep st = scratch_decide(S, true, A, 0, index, lm);   // the tail does not fit behind the window's index
    CHECK(!st.reuse && !st.refused && st.index_at == 0 && st.total == index + lm, "a reuse whose tail does not fit is a rebuild");
    scratch_grown(S, c.total + 256);
    CHECK(!S.win_valid && !S.index_valid && S.capacity == c.total + 256, "growing the scratch leaves nothing");
  }
  {  // reuse with a different map is refused
    g_cases++;
    ScratchState S{};
    acquire(S, false, A, 0, index, lm);
    const ScratchState before = S;
    const IndexStep st = acquire(S, true, B, 0, index, lm);
    CHECK(st.refused && !st.reuse && memcmp(&before, &S, sizeof(S)) == 0, "another map is refused and nothing changes");
    CHECK(acquire(S, true, A, 0, index, lm).reuse, "the same map is reused");
  }
  {  // a failed build leaves the index invalid
    g_cases++;
    ScratchState S{};
    acquire(S, false, A, 0, index, lm);
    CHECK(S.index_valid, "built");
    acquire(S, false, A, 0, index, lm, true, false);
    CHECK(!S.index_valid && !acquire(S, true, A, 0, index, lm).reuse && S.index_valid, "a build that was not enqueued leaves no index; the next call rebuilds");
  }
  {  // a guard on an error path invalidates
    g_cases++;
    ScratchState S{};
    auto twin = [&](bool fail) {
      IndexDropGuard drop(S);
      acquire(S, false, A, 0, index, lm);
      if (fail) return 1;   // a launch after the index failed
      return 0;
    };
    CHECK(twin(true) == 1 && !S.index_valid, "the guard drops the index on the error path");
    CHECK(twin(false) == 0 && !S.index_valid, "and on the success path");
  }
  {  // after a bird window the kept index is the front one
    g_cases++;
    ScratchState S{};
    const CallPlan c = window(S, true);
    CHECK(S.win_valid && S.index_valid && S.index_head == c.front && S.index_end == c.bird && same_map(S.index_map, A), "the front index is kept");
    CHECK(acquire(S, true, Bird, 0, bindex, 0).refused, "the bird side's map is not the index's");
  }
  {  // an editing call invalidates the index afterwards
    g_cases++;
    ScratchState S{};
    acquire(S, false, A, 0, index, lm);
    scratch_drop_index(S);   // process_new_keyframe, map_point_culling
    const IndexStep st = acquire(S, true, A, 0, index, lm);
    CHECK(!st.reuse && !st.refused && S.index_valid, "after an edit reuse_index rebuilds");
  }
}

int main() {
  for (size_t K : {1, 2, 64, 65, 500, 4096})
    for (size_t n_mp : {0, 1, 4094, 4095, 4096, 100000})
      for (size_t n_obs : {0, 1, 63, 600000})
        for (size_t qi = 0; qi < 3; qi++)
          for (size_t batch : {1, 2, 3})
            for (size_t cap : {0, 1, 255, 256, 257})
              for (size_t NF : {0, 1, 2000})
                for (int bird = 0; bird < 2; bird++) {
                  const size_t n_q = qi == 0 ? 0 : qi == 1 ? 1 : K;
                  check_plan(K, n_mp, n_obs, n_q, batch, cap, NF, bird ? 777 : 0, bird ? 3001 : 0, bird ? 300 : 0);
                }
  check_states();
  std::printf("cases=%ld failures=%ld\n", g_cases, g_failures);
  return g_failures ? 1 : 0;
}
