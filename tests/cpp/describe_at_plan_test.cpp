// The host path of fb_orb_describe (fishbirdeyevisualslam_amd/csrc/orb_describe_at_plan.h) on the CPU: the LDS layout the
// launcher and k_describe_at share, the argument checks of both entry points and the bytes the host entry point stages.
// Stand-alone, so that it can be built with -fsanitize=address,undefined (tests/test_describe_at_plan.py does): every staged
// size is used to allocate, fill and read back a buffer of exactly that size.
// usage: describe_at_plan_test   -> prints "cases=<n> failures=<n>", exit status 1 if failures > 0
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../fishbirdeyevisualslam_amd/csrc/orb_describe_at_plan.h"

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

static long g_failures = 0, g_cases = 0;
#define CHECK(cond, ...)                                                \
  do {                                                                  \
    g_cases++;                                                          \
    if (!(cond)) {                                                      \
      if (g_failures++ < 20) {                                          \
        std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
        std::printf(__VA_ARGS__);                                       \
        std::printf("\n");                                              \
      }                                                                 \
    }                                                                   \
  } while (0)

static constexpr int LAST = 2;  // images of the last extract call in the argument checks

int main() {
  // the layout: slices of whole 16 bytes, the raw patch only in IC mode, inside what a launch gets without an opt-in
  for (int mode : {FB_DESCRIBE_KEEP_ANGLE, FB_DESCRIBE_IC_ANGLE}) {
    DescAtLds L;
    size_t bytes = 0;
    CHECK(plan_describe_at(mode, "test", &bytes) == FB_OK, "mode %d is planned", mode);
    CHECK(describe_at_layout(L, mode) == bytes && bytes == L.slice * DESCAT_WAVES && bytes <= DESCAT_LDS_MAX, "mode %d: %zu B", mode, bytes);
    CHECK(L.slice % 16 == 0 && L.blur % 16 == 0 && L.raw % 16 == 0, "mode %d: alignment", mode);
    CHECK(L.raw >= L.blur + (size_t)DESCAT_BL_ROWS * DESCAT_BL_DW * 4, "mode %d: the raw patch starts behind the blurred one", mode);
    const size_t need = mode == FB_DESCRIBE_IC_ANGLE ? L.raw + (size_t)DESCAT_RAW_ROWS * DESCAT_RAW_DW * 4 : L.raw;
    CHECK(L.slice >= need && L.slice < need + 16, "mode %d: slice %zu for %zu B", mode, L.slice, need);
  }
  size_t bytes = 0;
  for (int bad : {-1, 2, 1000}) {
    g_error.clear();
    CHECK(plan_describe_at(bad, "test", &bytes) == FB_ERR_ARG && !g_error.empty(), "angle mode %d is refused with a message", bad);
  }
  // the argument checks, against a last extract call of 2 images of 157 x 120
  constexpr int W = 157, H = 120;
  int32_t n[3] = {5, 0, 7};
  std::vector<fb_keypoint> kps(3 * 8);
  std::vector<uint8_t> desc(3 * 8 * 32), status(3 * 8), img((size_t)2 * (W * H + 1));
  fb_orb_describe_args ok;
  memset(&ok, 0, sizeof(ok));
  ok.batch = 2; ok.kp_stride = 8; ok.n = n; ok.kps = kps.data(); ok.desc = desc.data(); ok.status = status.data();
  ok.angle_mode = FB_DESCRIBE_IC_ANGLE; ok.images = img.data(); ok.stride = W; ok.image_stride = (size_t)W * H + 1;
  auto rc = [&](const fb_orb_describe_args &a, int last = LAST) { g_error.clear(); return check_describe_at(&a, last, W, H, "test", &bytes); };
  CHECK(rc(ok) == FB_OK, "the good call: %s", g_error.c_str());
  CHECK(check_describe_at(nullptr, LAST, W, H, "test", &bytes) == FB_ERR_ARG, "null arguments");
  CHECK(rc(ok, 0) == FB_ERR_ARG && g_error.find("not extracted") != std::string::npos, "never extracted: %s", g_error.c_str());
  { fb_orb_describe_args a = ok; a.batch = 3; CHECK(rc(a) == FB_ERR_ARG && g_error.find("last extract call had 2") != std::string::npos, "batch 3 of 2: %s", g_error.c_str()); }
  { fb_orb_describe_args a = ok; a.images = nullptr; CHECK(rc(a) == FB_ERR_ARG && g_error.find("needs the images") != std::string::npos, "IC without images: %s", g_error.c_str()); }
  { fb_orb_describe_args a = ok; a.images = nullptr; a.angle_mode = FB_DESCRIBE_KEEP_ANGLE; CHECK(rc(a) == FB_OK, "KEEP needs no images: %s", g_error.c_str()); }
  { fb_orb_describe_args a = ok; a.stride = W - 1; CHECK(rc(a) == FB_ERR_ARG, "a stride below the width"); }
  { fb_orb_describe_args a = ok; a.image_stride = (size_t)W * H - 1; CHECK(rc(a) == FB_ERR_ARG, "overlapping images"); }
  { fb_orb_describe_args a = ok; a.batch = 1; a.image_stride = 0; CHECK(rc(a) == FB_OK, "one image needs no image stride: %s", g_error.c_str()); }
  { fb_orb_describe_args a = ok; a.batch = -1; CHECK(rc(a) == FB_ERR_ARG, "negative batch"); }
  { fb_orb_describe_args a = ok; a.batch = 65536; CHECK(rc(a, 70000) == FB_ERR_ARG, "batch beyond the grid"); }
  { fb_orb_describe_args a = ok; a.kp_stride = -1; CHECK(rc(a) == FB_ERR_ARG, "negative stride"); }
  { fb_orb_describe_args a = ok; a.angle_mode = 2; CHECK(rc(a) == FB_ERR_ARG, "an angle mode that is neither"); }
  for (int drop = 0; drop < 3; drop++) {
    fb_orb_describe_args a = ok;
    if (drop == 0) a.n = nullptr;
    if (drop == 1) a.kps = nullptr;
    if (drop == 2) a.desc = nullptr;
    CHECK(rc(a) == FB_ERR_ARG, "required array %d missing", drop);
    a.kp_stride = 0;
    CHECK(rc(a) == FB_OK, "an empty call needs no arrays: %s", g_error.c_str());
  }
  { fb_orb_describe_args a = ok; a.status = nullptr; CHECK(rc(a) == FB_OK, "status is optional: %s", g_error.c_str()); }
  // the staged bytes: each array copied in and out at exactly that size
  for (int mode : {FB_DESCRIBE_KEEP_ANGLE, FB_DESCRIBE_IC_ANGLE}) {
    fb_orb_describe_args a = ok;
    a.angle_mode = mode;
    const DescAtStage z = describe_at_stage(a, H);
    CHECK(z.n == 8 && z.kps == 2 * 8 * sizeof(fb_keypoint) && z.desc == 2 * 8 * 32 && z.status == 2 * 8, "mode %d: array bytes", mode);
    CHECK(z.images == (mode == FB_DESCRIBE_IC_ANGLE ? (size_t)W * H + 1 + (size_t)W * H : 0), "mode %d: %zu image bytes", mode, z.images);
    CHECK(z.images <= img.size(), "the staged images lie inside the caller's buffer");
    const struct { const void *p; size_t bytes; } arr[] = {{a.images, z.images}, {a.n, z.n}, {a.kps, z.kps}, {a.desc, z.desc}, {a.status, z.status}};
    unsigned sum = 0;
    for (const auto &r : arr) {
      std::vector<uint8_t> stage(r.bytes);
      if (r.bytes) memcpy(stage.data(), r.p, r.bytes);
      for (uint8_t v : stage) sum += v;
    }
    CHECK(sum == 5, "the staged bytes are n[0] + n[1] and zeros (%u)", sum);  // n[2] lies past the batch
  }
  std::printf("cases=%ld failures=%ld\n", g_cases, g_failures);
  return g_failures ? 1 : 0;
}
