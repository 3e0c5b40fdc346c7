// The frame handle's memory plan (fishbirdeyevisualslam_amd/csrc/track_plan.h) on the CPU: plan_frame() over a sweep of
// batches, extractor capacities and map / list capacities.  Checks that every region is 256-byte aligned and inside its
// arena, that regions of one arena are disjoint except the two declared aliases, that no front-side scratch overlaps
// bird-side scratch, that the byte counts are the ones the handle allocated buffer by buffer before it had a plan (written
// out below: that list is the specification), the member and BoW lists, that a refusal leaves the caller's plan alone, and
// that a handle does not hold more device memory than its separate power-of-two buffers did.
// usage: track_plan_test   -> prints "cases=<n> failures=<n>", exit status 1 if failures > 0
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../fishbirdeyevisualslam_amd/csrc/track_plan.h"

static std::string g_error;
namespace fb {
void set_error(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error = buf;
}
}  // namespace fb

// match.hip: M2_K = 8 candidates of 4 bytes and one count byte per local map point, 16 bytes of slack
extern "C" size_t fb_match_projection_points_workspace(int batch, int mp_stride) {
  if (batch <= 0 || mp_stride <= 0) return 0;
  return (size_t)batch * mp_stride * (8 * 4 + 1) + 16;
}

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

struct Spec { const char *name; size_t bytes; };

// The buffers of a handle and their sizes as fb_frame_create / fb_frame_compute_bow_dev allocated them one by one.
static std::vector<Spec> buffer_sizes(size_t B, size_t cap, size_t map_cap, size_t lm, size_t lb) {
  const size_t KP = sizeof(fb_keypoint);
  return {
      {"n", B * 4}, {"kps", B * cap * KP}, {"kps_un", B * cap * KP}, {"desc", B * cap * 32}, {"cs", B * (64 * 48 + 1) * 4}, {"ci", B * cap * 4},
      {"mp", B * cap * 4}, {"outlier", B * cap},
      {"nb", B * 4}, {"bkps", B * cap * KP}, {"bdesc", B * cap * 32}, {"bcam", B * cap * 12}, {"bcs", B * (32 * 32 + 1) * 4}, {"bci", B * cap * 4},
      {"mpb", B * cap * 4}, {"boutlier", B * cap}, {"nb_pre", B * 4}, {"bkps_pre", B * cap * KP}, {"bdesc_pre", B * cap * 32},
      {"Tcw", B * 48}, {"counts", B * 16 * 4}, {"seen_mark", B * map_cap},
      {"m3_valid", B * cap}, {"m3_obs", B * cap}, {"m3_xw", B * cap * 12}, {"m3_desc", B * cap * 32}, {"m3_oct", B * cap * 4}, {"m3_ang", B * cap * 4},
      {"m_front", B * cap * 4},
      {"m9_valid", B * lb}, {"m9_xw", B * lb * 12}, {"m9_desc", B * lb * 32}, {"m9_n", B * 4}, {"m_bird", B * cap * 4}, {"ones", B * lb},
      {"e_fxw", B * cap * 12}, {"e_fobs", B * cap * 8}, {"e_finf", B * cap * 4}, {"e_fvalid", B * cap},
      {"e_bxw", B * cap * 12}, {"e_bxc", B * cap * 12}, {"e_binf", B * cap * 4}, {"e_bvalid", B * cap},
      {"m8_m12", B * cap * 4}, {"m8_dist", B * cap * 4}, {"m8_n", B * 4}, {"m8_nd", B * 4},
      {"l_seen", B * map_cap}, {"l_blocked", B * cap}, {"l_inview", B * lm}, {"l_obs", B * lm}, {"l_proj", B * lm * 8},
      {"l_level", B * lm * 4}, {"l_cos", B * lm * 4}, {"l_desc", B * lm * 32}, {"l_n", B * 4}, {"m_local", B * cap * 4},
      {"m2_ws", B * lm * 33 + 16},
      {"bow_nw", B * 4}, {"bow_ids", B * cap * 4}, {"bow_vals", B * cap * 8}, {"fv_nn", B * 4}, {"fv_ids", B * cap * 4},
      {"fv_start", B * (cap + 1) * 4}, {"fv_items", B * cap * 4}};
}

static const char *const MEMBERS[19] = {"n", "kps", "kps_un", "desc", "cs", "ci", "mp", "outlier", "nb", "bkps", "bdesc", "bcam", "bcs", "bci",
                                        "mpb", "boutlier", "Tcw", "counts", "seen_mark"};
static const char *const BOW[7] = {"bow_nw", "bow_ids", "bow_vals", "fv_nn", "fv_ids", "fv_start", "fv_items"};
struct Fill { const char *name; int byte; };
static const Fill FILLS[10] = {{"counts", 0}, {"seen_mark", 0}, {"n", 0}, {"nb", 0}, {"Tcw", 0}, {"outlier", 0}, {"mp", 0xff}, {"mpb", 0xff},
                               {"ones", 1}, {"boutlier", 1}};
struct Alias { const char *name, *host; int side; };
static const Alias ALIASES[2] = {{"guidance_keep", "l_blocked", FS_BIRD}, {"bow_has_mp", "m3_valid", FS_FRONT}};

static fb_frame_params params(int batch, int nfeatures, int nlevels, int map_cap, int lm, int lb) {
  fb_frame_params p;
  memset(&p, 0, sizeof(p));
  p.batch = batch; p.front_width = 640; p.front_height = 480; p.bird_width = 384; p.bird_height = 384;
  p.orb.nfeatures = nfeatures; p.orb.scale_factor = 1.2f; p.orb.nlevels = nlevels; p.orb.ini_th_fast = 15; p.orb.min_th_fast = 5;
  p.map_cap = map_cap; p.local_mp_cap = lm; p.local_mpb_cap = lb;
  return p;
}
static int capacity(const fb_frame_params &p) { return p.orb.nfeatures + 8 * p.orb.nlevels; }  // fb_orb_capacity

static const FrameRegion *find(const FramePlan &P, const std::string &name) {
  for (int i = 0; i < FR_COUNT; i++)
    if (name == P.r[i].name) return &P.r[i];
  return nullptr;
}
static bool is_alias(const FrameRegion &R) { return R.alias_of >= 0; }
static bool overlap(const FrameRegion &a, const FrameRegion &b) { return a.arena == b.arena && a.off < b.off + b.bytes && b.off < a.off + a.bytes; }

static void check_plan(const fb_frame_params &p, const char *tag) {
  FramePlan P;
  g_cases++;
  const int cap = capacity(p);
  if (plan_frame(p, cap, &P) != FB_OK) { CHECK(false, "%s: refused: %s", tag, g_error.c_str()); return; }
  // inside the arena, aligned, named once
  for (int i = 0; i < FR_COUNT; i++) {
    const FrameRegion &R = P.r[i];
    CHECK(R.name && R.arena >= 0 && R.arena < FA_COUNT, "%s: region %d has no name or arena", tag, i);
    if (!R.name) return;
    CHECK(R.off % 256 == 0 && R.bytes > 0 && R.off + R.bytes <= P.arena_bytes[R.arena], "%s: %s is [%zu, +%zu) of %zu", tag, R.name, R.off, R.bytes, P.arena_bytes[R.arena]);
    CHECK(find(P, R.name) == &R, "%s: the name %s appears twice", tag, R.name);
    CHECK((R.arena == FA_SCRATCH) == (R.side != FS_NONE), "%s: %s: arena %d with side %d", tag, R.name, R.arena, R.side);
  }
  for (int a = 0; a < FA_COUNT; a++) CHECK(P.arena_bytes[a] > 0 && P.arena_bytes[a] % 256 == 0, "%s: arena %d has %zu bytes", tag, a, P.arena_bytes[a]);
  // disjoint, except that an alias IS its host (and nothing but its host); front scratch never meets bird scratch
  int naliases = 0;
  for (int i = 0; i < FR_COUNT; i++) {
    const FrameRegion &R = P.r[i];
    if (is_alias(R)) {
      naliases++;
      const FrameRegion &H = P.r[R.alias_of];
      CHECK(!is_alias(H) && R.arena == H.arena && R.off == H.off && R.bytes == H.bytes && R.fill == FILL_NONE, "%s: alias %s is not its host %s", tag, R.name, H.name);
    }
    for (int j = 0; j < i; j++) {
      const FrameRegion &Q = P.r[j];
      const bool declared = (is_alias(R) && R.alias_of == j) || (is_alias(Q) && Q.alias_of == i);
      CHECK(declared || !overlap(R, Q), "%s: %s and %s overlap", tag, Q.name, R.name);
      if (!is_alias(R) && !is_alias(Q) && R.side != FS_NONE && Q.side != FS_NONE && R.side != Q.side)
        CHECK(!overlap(R, Q), "%s: front-side %s meets bird-side %s", tag, Q.name, R.name);
    }
  }
  CHECK(naliases == 2, "%s: %d aliases", tag, naliases);
  for (const Alias &A : ALIASES) {
    const FrameRegion *R = find(P, A.name);
    CHECK(R && is_alias(*R) && std::string(P.r[R->alias_of].name) == A.host && R->side == A.side, "%s: alias %s", tag, A.name);
  }
  // the byte counts of the separate buffers
  const std::vector<Spec> spec = buffer_sizes(p.batch, cap, p.map_cap, p.local_mp_cap, p.local_mpb_cap);
  CHECK((int)spec.size() + 2 == FR_COUNT, "%s: %zu buffers, %d regions", tag, spec.size(), (int)FR_COUNT);
  for (const Spec &s : spec) {
    const FrameRegion *R = find(P, s.name);
    CHECK(R && !is_alias(*R) && R->bytes == s.bytes, "%s: %s has %zu bytes, the buffer had %zu", tag, s.name, R ? R->bytes : 0, s.bytes);
  }
  // members and bow: exactly these, in this order, contiguous from the start of their arena
  auto check_list = [&](int arena, const char *const *names, int n) {
    size_t off = 0;
    int seen = 0;
    for (int i = 0; i < FR_COUNT; i++) {
      const FrameRegion &R = P.r[i];
      if (R.arena != arena) continue;
      CHECK(seen < n && std::string(R.name) == names[seen] && R.off == off, "%s: arena %d entry %d is %s at %zu", tag, arena, seen, R.name, R.off);
      off += (R.bytes + 255) & ~(size_t)255;
      seen++;
    }
    CHECK(seen == n && off == P.arena_bytes[arena], "%s: arena %d has %d entries, %zu of %zu bytes", tag, arena, seen, off, P.arena_bytes[arena]);
  };
  check_list(FA_MEMBERS, MEMBERS, 19);
  check_list(FA_BOW, BOW, 7);
  // what create fills, and with what; everything else starts uninitialised
  int nfill = 0;
  for (int i = 0; i < FR_COUNT; i++) nfill += P.r[i].fill != FILL_NONE;
  CHECK(nfill == 10, "%s: %d regions are filled", tag, nfill);
  for (const Fill &F : FILLS) {
    const FrameRegion *R = find(P, F.name);
    CHECK(R && R->fill == F.byte, "%s: %s is filled with %d", tag, F.name, R ? R->fill : -2);
  }
}

static size_t size_class(size_t bytes) {  // what the pool grants a request without the exact-size path
  size_t cls = 256;
  while (cls < bytes) cls <<= 1;
  return cls;
}

// device bytes of a handle: one size-class block per buffer before, the arenas at their exact (256-byte granular) size now
static void check_granted(const fb_frame_params &p, const char *what) {
  FramePlan P;
  const int cap = capacity(p);
  CHECK(plan_frame(p, cap, &P) == FB_OK, "%s is planned", what);
  size_t before = 0, before_bow = 0;
  for (const Spec &s : buffer_sizes(p.batch, cap, p.map_cap, p.local_mp_cap, p.local_mpb_cap))
    (find(P, s.name)->arena == FA_BOW ? before_bow : before) += size_class(s.bytes);
  const size_t now = P.arena_bytes[FA_MEMBERS] + P.arena_bytes[FA_SCRATCH], now_bow = P.arena_bytes[FA_BOW];
  std::printf("granted bytes per handle, %s: %zu separate buffers -> %zu arenas (with BoW: %zu -> %zu)\n", what, before, now, before + before_bow, now + now_bow);
  CHECK(now <= before && now_bow <= before_bow, "%s: the handle grew", what);
}

int main() {
  char tag[128];
  const int caps[] = {1, 7, 2000, 4096};
  for (int batch : {1, 2, 3, 256})
    for (int nf : {50, 500, 1000, 2000})
      for (int nl = 1; nl <= 8; nl++)
        for (int mc : caps)
          for (int lm : caps)
            for (int lb : caps) {
              std::snprintf(tag, sizeof(tag), "B=%d nf=%d nl=%d map_cap=%d lm=%d lb=%d", batch, nf, nl, mc, lm, lb);
              check_plan(params(batch, nf, nl, mc, lm, lb), tag);
            }
  // a refusal leaves a filled plan byte for byte as it was
  {
    FramePlan P;
    CHECK(plan_frame(params(2, 2000, 8, 2064, 2064, 4128), 2064, &P) == FB_OK, "the test configuration is planned");
    std::vector<uint8_t> object(sizeof(P));
    memcpy(object.data(), static_cast<const void *>(&P), sizeof(P));
    for (const fb_frame_params &bad : {params(0, 2000, 8, 2064, 2064, 4128), params(2, 2000, 8, 0, 2064, 4128), params(2, 2000, 8, 2064, 0, 4128),
                                       params(2, 2000, 8, 2064, 2064, 0), params(65536, 2000, 8, 2064, 2064, 4128)}) {
      g_error.clear();
      CHECK(plan_frame(bad, 2064, &P) == FB_ERR_ARG && !g_error.empty(), "a bad parameter set is refused with a message");
      CHECK(memcmp(object.data(), static_cast<const void *>(&P), sizeof(P)) == 0, "the refusal changed the plan");
    }
    CHECK(plan_frame(params(2, 2000, 8, 2064, 2064, 4128), 0, &P) == FB_ERR_ARG, "capacity 0 is refused");
  }
  // the configurations of the GPU tests (map_cap = capacity, bird table 2 x capacity) and of the bench (2 x and 8 x)
  fb_frame_params p = params(2, 2000, 8, 2064, 2064, 2 * 2064);
  check_granted(p, "640x480 + 384x384, default extractor, batch 2");
  p = params(3, 2000, 8, 2064, 2064, 2 * 2064);
  check_granted(p, "640x480 + 384x384, default extractor, batch 3");
  p = params(2, 2000, 8, 2064, 2064, 2 * 2064);
  p.front_width = 1280; p.front_height = 720; p.bird_width = 512; p.bird_height = 512;
  check_granted(p, "1280x720 + 512x512, batch 2");
  p = params(256, 2000, 8, 2 * 2064, 2 * 2064, 8 * 2064);
  p.front_width = 1280; p.front_height = 720; p.bird_width = 512; p.bird_height = 512; p.bird_nfeatures = 1000;
  check_granted(p, "1280x720 + 512x512, batch 256, 1000 bird features");
  std::printf("cases=%ld failures=%ld\n", g_cases, g_failures);
  return g_failures ? 1 : 0;
}
