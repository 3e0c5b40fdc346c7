/*
 * fb_common.h -- shared host/device plumbing of the HIP library (gfx950 only).
 */
#ifndef FB_COMMON_H_
#define FB_COMMON_H_

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <climits>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/fishbird.h"

#define FB_HD __host__ __device__
#include "fb_detmath.h"

namespace fb {

void set_error(const char *fmt, ...);
int check_device();  // FB_OK or FB_ERR_NODEVICE (sets error)

#define FB_HIP(expr)                                                                   \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) {                                                            \
      fb::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
      (void)hipGetLastError(); /* the runtime also remembers it: a later hipGetLastError() must not report it again */ \
      return FB_ERR_HIP;                                                               \
    }                                                                                  \
  } while (0)

#define FB_ARG(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      fb::set_error("%s:%d: bad argument: %s", __FILE__, __LINE__, #cond); \
      return FB_ERR_ARG;                                                    \
    }                                                                       \
  } while (0)

#define FB_TRY(expr)           \
  do {                         \
    int rc_ = (expr);          \
    if (rc_ != FB_OK) return rc_; \
  } while (0)

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// ---- per-kernel timing (fb_prof_* in include/fishbird.h) ----
enum ProfId {
  P_RESIZE, P_FAST, P_OCTREE, P_DESCRIBE, P_GRID, P_BIRDCAM, P_HAMMING, P_PROJ_FRAME, P_PROJ_POINTS, P_BIRD_MP,
  P_BIRDVIEW, P_BOW, P_TRIANG, P_POSE, P_GATHER, P_BA_LINEARIZE, P_BA_SCHUR, P_BA_SOLVE, P_BA_UPDATE, P_BA_MISC,
  P_PROJ_KF, P_BOW_KF, P_FRUSTUM, P_UNDISTORT, P_BLUR, P_FUSE, P_DISTINCT, P_BOWT, P_FAST56, P_FAST72, P_TRACK_GLUE,
  P_NP_PREP, P_NP_M7, P_NP_CLAIM, P_NP_EMIT, P_KFDB, P_SIM3_PREP, P_SIM3_HYP, P_SIM3_ACCEPT, P_TAIL_FRONT,
  P_TAIL_BIRD, P_OPT_SIM3, P_DESCRIBE_AT, P_DET_FAST, P_DET_SELECT, P_DET_EMIT, P_COUNT
};
extern bool g_prof_on;
extern int g_prof_only;  // -1 = every kernel, else only this ProfId is bracketed
hipEvent_t prof_begin(int id, hipStream_t s);  // records the start event, returns the end event of this bracket
void prof_end(hipEvent_t end, hipStream_t s);
struct ProfScope {  // (the record list is mutex-protected and a scope closes its OWN bracket: launches from several host threads)
  hipStream_t s;
  bool on;
  hipEvent_t end = nullptr;
  ProfScope(int id, hipStream_t st) : s(st), on(g_prof_on && (g_prof_only < 0 || g_prof_only == id)) { if (on) end = prof_begin(id, s); }
  ~ProfScope() { if (on) prof_end(end, s); }
};

// Device scratch that lives for one host-pointer call.
// hipMalloc/hipFree cost tens of microseconds each and the host-pointer entry points need dozens of scratch
// buffers per call, so freed blocks are kept in a per-device pool of power-of-two size classes (runtime.hip).
// exact: a long-lived block (a handle's arena) is granted its size rounded up to 256 bytes instead of a power of two
void *pool_take(size_t bytes, size_t *granted, bool exact = false);  // nullptr on failure (error set)
void pool_give(void *p, size_t granted);
void pool_release();  // frees every idle block (fb_shutdown)
void ba_release_thread();  // ba.hip: the calling thread's per-device stream, event and pinned control block (fb_shutdown)

struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0, granted = 0;
  DevBuf() {}
  DevBuf(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes), granted(o.granted) { o.p = nullptr; }
  DevBuf &operator=(DevBuf &&o) noexcept {  // the block held before goes back to the pool with `o`
    std::swap(p, o.p); std::swap(bytes, o.bytes); std::swap(granted, o.granted);
    return *this;
  }
  ~DevBuf() { if (p) pool_give(p, granted); }
  int alloc(size_t n, bool exact = false) {
    if (p) { pool_give(p, granted); p = nullptr; }
    bytes = n ? n : 1;
    p = pool_take(bytes, &granted, exact);
    if (!p) return FB_ERR_HIP;
    return FB_OK;
  }
  int upload(const void *src, size_t n) {
    FB_TRY(alloc(n));
    if (n && src) FB_HIP(hipMemcpy(p, src, n, hipMemcpyHostToDevice));
    return FB_OK;
  }
  int download(void *dst, size_t n) const {
    if (n) FB_HIP(hipMemcpy(dst, p, n, hipMemcpyDeviceToHost));
    return FB_OK;
  }
  template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// One staged transfer per host-pointer call.  The drop-in entry points used to upload every argument array with its own
// synchronous hipMemcpy (16 of them for SearchByProjection: ~0.2 ms of a 0.33 ms call, `host_abi` in bench.py): the arrays of a
// call are now packed into one page-locked block (per host thread, grows on demand), travel with ONE copy into one device
// block, and the outputs come back with one copy.  The shape of every host drop-in:
//   fb_x_args D = *H;                  // every pointer field of D still holds the caller's host address
//   fb::Stager st;
//   st.in(D.n, B * 4);                 // input only
//   st.out(D.match, B * s * 4, true);  // in/out: uploaded first, entries the kernel skips keep the caller's contents
//   st.out(D.count, B * 4, false);     // output only
//   FB_TRY(st.commit(nullptr));        // re-points each staged field at its slice of the device block
//   FB_TRY(fb_x_dev(&D, nullptr));
//   return st.fetch(nullptr);          // one stream synchronisation, then the outputs land in the caller's arrays
// A field whose host pointer is null stays null.  A required array is checked (FB_ARG) before commit.
// Invariants:
//  - at most one live Stager (or other pinned_scratch user) per host thread: a host wrapper does not call another host
//    wrapper while its own Stager is live (calling one after the other is fine);
//  - after staging, no pointer field of D holds a host address: each one is staged or explicitly set to nullptr.
// If commit enqueued work and fetch did not wait for it (an error in between), the destructor synchronises the stream
// before the device block goes back to the pool and the pinned block can be refilled by the thread's next call.
void *pinned_scratch(size_t bytes);  // per-thread page-locked block of at least `bytes` (nullptr on failure, error set)
struct Stager {
  struct Item { void **field; const void *src; void *dst; size_t bytes, off; };
  std::vector<Item> ins, outs;
  DevBuf dev;
  uint8_t *pin = nullptr;
  size_t inBytes = 0, total = 0;
  hipStream_t stream = nullptr;
  bool pending = false;  // work that reads the blocks may be in flight on `stream`
  Stager() {}
  Stager(const Stager &) = delete;
  Stager &operator=(const Stager &) = delete;
  ~Stager() {
    if (pending) { (void)hipStreamSynchronize(stream); (void)hipGetLastError(); }
  }
  static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
  template <typename T> void in(const T *&field, size_t bytes) {
    if (field) ins.push_back({reinterpret_cast<void **>(const_cast<T **>(&field)), field, nullptr, bytes, 0});
  }
  template <typename T> void out(T *&field, size_t bytes, bool copy_in) {
    if (field) outs.push_back({reinterpret_cast<void **>(&field), copy_in ? field : nullptr, field, bytes, 0});
  }
  int commit(hipStream_t s) {
    size_t off = 0;
    for (auto &it : ins) { it.off = off; off += up256(it.bytes ? it.bytes : 1); }
    inBytes = off;
    for (auto &it : outs) { it.off = off; off += up256(it.bytes ? it.bytes : 1); }
    total = off ? off : 256;
    pin = static_cast<uint8_t *>(pinned_scratch(total));
    if (!pin) return FB_ERR_HIP;
    FB_TRY(dev.alloc(total));
    bool anyOutIn = false;
    for (auto &it : ins) if (it.bytes) memcpy(pin + it.off, it.src, it.bytes);
    for (auto &it : outs) if (it.src && it.bytes) { memcpy(pin + it.off, it.src, it.bytes); anyOutIn = true; }
    const size_t upBytes = anyOutIn ? total : inBytes;
    stream = s;
    pending = true;
    if (upBytes) FB_HIP(hipMemcpyAsync(dev.p, pin, upBytes, hipMemcpyHostToDevice, s));
    for (auto &it : ins) *it.field = dev.as<uint8_t>() + it.off;
    for (auto &it : outs) *it.field = dev.as<uint8_t>() + it.off;
    return FB_OK;
  }
  int fetch(hipStream_t s) {  // waits for the stream, then hands the outputs to the caller's arrays
    if (total > inBytes) FB_HIP(hipMemcpyAsync(pin + inBytes, dev.as<uint8_t>() + inBytes, total - inBytes, hipMemcpyDeviceToHost, s));
    FB_HIP(hipStreamSynchronize(s));
    pending = false;
    for (auto &it : outs) if (it.bytes) memcpy(it.dst, pin + it.off, it.bytes);
    return FB_OK;
  }
};

// a DBoW2::FeatureVector's four arrays (n problems) join the call's staged upload
inline void stage(Stager &st, fb_feature_vector &d, size_t n) {
  st.in(d.n_nodes, n * 4);
  st.in(d.node_ids, n * (size_t)d.node_stride * 4);
  st.in(d.node_start, n * (size_t)(d.node_stride + 1) * 4);
  st.in(d.items, n * (size_t)d.item_stride * 4);
}

// The key-frame pair of the two Sim3 stages (fb_sim3_solver_args / fb_optimize_sim3_args: pKF1 with batch 1, C candidates
// pKF2) joins the call's staged upload: what the kernels read of kf1 / kf2 / mp1 / mp2, T1w / T2w and kf2_index.  The unread
// pointer fields are set to nullptr, so that none holds a host address.
template <typename Args>
inline void stage_sim3_pair(Stager &st, Args &D, size_t C) {
  const size_t s1 = D.kf1.kf_stride, s2 = D.kf2.kf_stride;
  st.in(D.kf1.n_kf, 4); st.in(D.kf1.kf_kps, s1 * sizeof(fb_keypoint));
  st.in(D.kf2.kf_kps, C * s2 * sizeof(fb_keypoint));
  D.kf2.n_kf = nullptr;
  for (fb_kf_target *k : {&D.kf1, &D.kf2}) { k->kf_desc = nullptr; k->kf_cell_start = nullptr; k->kf_cell_items = nullptr; }
  st.in(D.mp1.mp_valid, s1); st.in(D.mp1.mp_xw, s1 * 12);
  st.in(D.mp2.mp_valid, C * s2); st.in(D.mp2.mp_xw, C * s2 * 12);
  for (fb_mp_list *m : {&D.mp1, &D.mp2}) {
    m->n_mp = nullptr; m->mp_normal = nullptr; m->mp_max_dist = nullptr; m->mp_min_dist = nullptr; m->mp_desc = nullptr;
  }
  st.in(D.T1w, 48); st.in(D.T2w, C * 48);
  st.in(D.kf2_index, C * s2 * 4);
}

// v of the lane selected by the DPP control, +0.0 where there is none
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

// fp64 reciprocal from the hardware seed (v_rcp_f64) and two Newton steps: 6 instead of the ~35 dependent instructions of
// the IEEE division sequence, relative error < 2^-50.  Only where the result is held to a tolerance (the LM evaluations of
// the pose optimisation, the pivots of the BA's reduced pose system: 1e-4), never where a decision needs the true quotient.
// Written with explicit fma so that the text means the same under every -ffp-contract setting.
__device__ __forceinline__ double rcp_f64_newton(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  r = fma(fma(-x, r, 1.0), r, r);
  return r;
}

// Column sums of up to 32 per-lane values over the 64 lanes as a reduce-scatter butterfly: at the step with mask m a
// lane sends one half of its values to lane^m, keeps the other half and adds what it receives, so the value count halves
// every step (16 + 8 + 4 + 2 + 1 + 1 = 32 fp64 exchanges instead of 6 per value).  On return v[0] of lane L is the sum
// over all lanes of column L >> 1.  (28 accumulators through plain butterflies were most of an LM evaluation: 168
// dependent cross-lane exchanges per wave.)
// c ? a : b on the two halves of a double, in assembly: written as a C++ select between two array elements the compiler
// turns the pair into ONE load with a computed index, which forces the whole array out of registers into scratch memory
__device__ __forceinline__ double select_f64(bool c, double a, double b) {
  const unsigned long long ua = __builtin_bit_cast(unsigned long long, a), ub = __builtin_bit_cast(unsigned long long, b);
  unsigned lo, hi;
  const unsigned long long m = __builtin_amdgcn_ballot_w64(c);
  asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(lo) : "v"((unsigned)ub), "v"((unsigned)ua), "s"(m));
  asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(hi) : "v"((unsigned)(ub >> 32)), "v"((unsigned)(ua >> 32)), "s"(m));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ double wave_column_sums32(double (&v)[32], int lane) {
#pragma unroll
  for (int half = 16, m = 32; half >= 1; half >>= 1, m >>= 1) {
    const bool up = (lane & m) != 0;
#pragma unroll
    for (int i = 0; i < half; i++) {
      const double send = select_f64(up, v[i], v[i + half]);
      const double keep = select_f64(up, v[i + half], v[i]);
      v[i] = keep + __shfl_xor(send, m, 64);
    }
  }
  return v[0] + __shfl_xor(v[0], 1, 64);
}

// a 32-byte descriptor row (16-byte aligned) as 8 dwords
__device__ __forceinline__ void load_desc(const uint8_t *p, uint32_t d[8]) {
  const uint4 *q = reinterpret_cast<const uint4 *>(p);
  const uint4 a = q[0], b = q[1];
  d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
}

// 256-bit Hamming distance of two 32-byte rows given as 8 dwords each
// (DescriptorDistance, ORBmatcher.cc:1951-1967; v_bcnt_u32_b32 instead of the SWAR bithack)
__device__ __forceinline__ int hamming256(const uint32_t a[8], const uint4 *__restrict__ b) {
  const uint4 b0 = b[0], b1 = b[1];
  return __popc(a[0] ^ b0.x) + __popc(a[1] ^ b0.y) + __popc(a[2] ^ b0.z) + __popc(a[3] ^ b0.w) +
         __popc(a[4] ^ b1.x) + __popc(a[5] ^ b1.y) + __popc(a[6] ^ b1.z) + __popc(a[7] ^ b1.w);
}

}  // namespace fb
#endif
