// frame.hip -- Frame geometry that sits either side of the matchers, on gfx950.
//
// Replaces (reference file:line):
//   Frame::isInFrustum            src/Frame.cc:435-491 (loop: Tracking::SearchLocalPoints, src/Tracking.cc:1071-1091)
//   Frame::UndistortKeyPoints     src/Frame.cc:636-669 (cv::fisheye::undistortPoints, R = I, P = K)
//   Frame::ComputeImageBounds     src/Frame.cc:741-795
//   Frame::GuidenceKeyBirdPts     src/Frame.cc:671-684 with nearEdges :717-739 and genEdgesPC :686-715 (bird key point filter)
//   cv::cornerSubPix              src/Frame.cc:345-352 on the bird key points (k_corner_subpix below; LDS plan: subpix_plan.h)
//
// The frustum and undistort kernels are one-lane-per-element streaming maps (28-44 B in, 1-21 B out per element): HBM-bound by
// construction, no LDS needed.  Per-problem constants (pose, camera centre) sit in SGPRs via uniform loads.
#include "fb_common.h"
#include "fb_frame_geom.h"
#include "fb_primitives.h"
#include "subpix_plan.h"

#include <cmath>

namespace {

constexpr int FRAME_THREADS = 256;

__global__ __launch_bounds__(FRAME_THREADS) void k_in_frustum(fb_frustum_args A) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * FRAME_THREADS + threadIdx.x;
  if (i >= A.n_mp[b]) return;
  const size_t e = (size_t)b * A.mp_stride + i;
  A.in_view[e] = 0;
  if (A.mp_valid && !A.mp_valid[e]) return;
  const float *T = A.Tcw + (size_t)b * 12, *Ow = A.Ow + (size_t)b * 3;
  fb::FrustumOut o;
  if (!fb::in_frustum(T, Ow, A.cam, A.mp_xw[e * 3], A.mp_xw[e * 3 + 1], A.mp_xw[e * 3 + 2], A.mp_normal[e * 3], A.mp_normal[e * 3 + 1],
                      A.mp_normal[e * 3 + 2], A.mp_max_dist[e], A.mp_min_dist[e], A.viewing_cos_limit, A.log_scale_factor, A.n_levels, o))
    return;
  const float u = o.u, v = o.v, invz = o.invz, viewCos = o.view_cos;
  const int lvl = o.level;
  A.in_view[e] = 1;
  A.proj[e * 2] = u;
  A.proj[e * 2 + 1] = v;
  if (A.proj_xr) A.proj_xr[e] = u - A.mbf * invz;
  A.level[e] = lvl;
  A.view_cos[e] = viewCos;
}

// Tracking::FilterBirdOutlierInFront geometric test: one workgroup per frame pair.  Pass 1 evaluates every match and
// lets the passing ones compete for their train slot with atomicMin on the match index (the serial rule "the first
// passing match takes the slot"); pass 2 writes the flags.
__global__ __launch_bounds__(256) void k_bird_filter(fb_bird_filter_args A) {
  extern __shared__ int s_first[];  // [kp2_stride] smallest passing match index per train slot
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const size_t mo = (size_t)b * A.match_stride, o1 = (size_t)b * A.kp1_stride, o2 = (size_t)b * A.kp2_stride;
  const int nm = A.n_matches[b];
  __shared__ float s_Twc1[12], s_T2[12];
  if (tid == 0) {
    fb::inv_T(A.Tcw1 + (size_t)b * 12, s_Twc1);
    for (int i = 0; i < 12; i++) s_T2[i] = A.Tcw2[(size_t)b * 12 + i];
  }
  for (int i = tid; i < A.kp2_stride; i += nt) s_first[i] = 0x7fffffff;
  __syncthreads();
  for (int i = tid; i < nm; i += nt) {
    const int qi = A.query_idx[mo + i], ti = A.train_idx[mo + i];
    bool pass = false;
    float ptw[3] = {0.f, 0.f, 0.f};
    if (!A.occupied2[o2 + ti]) {
      pass = fb::bird_filter_test(s_Twc1, s_T2, A.cam_xyz1 + (o1 + qi) * 3, A.cam_xyz2 + (o2 + ti) * 3, A.window_size, ptw);
    }
    if (pass) {
      atomicMin(&s_first[ti], i);
#pragma unroll
      for (int k = 0; k < 3; k++) A.pt_world[(mo + i) * 3 + k] = ptw[k];
    }
    A.keep[mo + i] = pass ? 2 : 0;  // 2 = passed the test, resolved below
  }
  __syncthreads();
  for (int i = tid; i < nm; i += nt)
    if (A.keep[mo + i] == 2) A.keep[mo + i] = (s_first[A.train_idx[mo + i]] == i) ? 1 : 0;
}

struct CamKD { float K[4], D[4]; };

__global__ __launch_bounds__(FRAME_THREADS) void k_undistort(const fb_keypoint *kps, const int32_t *n, int stride, CamKD C,
                                                             fb_keypoint *out) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * FRAME_THREADS + threadIdx.x;
  if (i >= n[b]) return;
  const size_t e = (size_t)b * stride + i;
  fb_keypoint kp = kps[e];
  if (C.D[0] != 0.0f) fb_fisheye_undistort(kp.x, kp.y, C.K, C.D, &kp.x, &kp.y);
  out[e] = kp;
}


// ---- Frame::GuidenceKeyBirdPts (Frame.cc:671-739) ------------------------------------------------------------------
constexpr int GUIDE_THREADS = 1024;


// One workgroup per bird image.  Phase A: 32 lanes per key point, one lane per contour ROW of its box (the box has at
// most 21 rows: trunc(x-10) .. ceil(x+10)-1), each lane walks its <= 21 contiguous bytes; the verdict is the OR over the
// half wave.  Phase B: stable compaction (push_back order) with one block scan; descriptors move as two 16-byte words.
__global__ __launch_bounds__(GUIDE_THREADS) void k_bird_guidance(fb_bird_guidance_args A) {
  extern __shared__ uint8_t s_keep[];  // [kp_stride]
  __shared__ int s_w[GUIDE_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(A.n_in[b], 0), A.kp_stride);  // the LDS flag array and the output rows hold kp_stride entries
  const size_t ko = (size_t)b * A.kp_stride;
  const uint8_t *icp = A.contour + (size_t)b * A.rows * A.pitch;
  const uint8_t *mask = A.mask ? A.mask + (size_t)b * A.rows * A.pitch : nullptr;
  const int sub = tid & 31;
  for (int base = 0; base < n; base += GUIDE_THREADS / 32) {
    const int i = base + (tid >> 5);
    bool hit = false, ok = true;
    if (i < n) {
      const fb_keypoint kpt = A.kps_in[ko + i];
      const int r = 10;
      const float pt1x = (kpt.x - r) > 0 ? (kpt.x - r) : 0;
      const float pt1y = (kpt.y - r) > 0 ? (kpt.y - r) : 0;
      const float pt2x = (kpt.x + r) < A.cols ? (kpt.x + r) : A.cols;
      const float pt2y = (kpt.y + r) < A.rows ? (kpt.y + r) : A.rows;
      const size_t row = (size_t)pt1x + sub;       // size_t row = pt1x; row < pt2x; row++
      if ((float)row < pt2x && row < (size_t)A.rows) {
        const uint8_t *src = icp + row * (size_t)A.pitch;
        for (size_t col = (size_t)pt1y; (float)col < pt2y && col < (size_t)A.cols; col++)
          if (src[col] >= 10) { hit = true; break; }
      }
      if (mask) {
        const int my = (int)(kpt.y + 0.5f), mx = (int)(kpt.x + 0.5f);
        ok = my >= 0 && my < A.rows && mx >= 0 && mx < A.cols && mask[(size_t)my * A.pitch + mx] != 0;
      }
    }
    const unsigned long long bal = __ballot(hit);
    const unsigned int mine = (unsigned int)(bal >> (tid & 32));
    if (sub == 0 && i < n) {
      const uint8_t k = (ok && mine != 0u) ? 1 : 0;
      s_keep[i] = k;
      if (A.keep) A.keep[ko + i] = k;
    }
  }
  __syncthreads();
  const int per = (n + GUIDE_THREADS - 1) / GUIDE_THREADS;
  const int i0 = tid * per, i1 = min(n, i0 + per);
  int cnt = 0;
  for (int i = i0; i < i1; i++) cnt += s_keep[i];
  int total;
  int o = fb::block_excl_scan<GUIDE_THREADS>(cnt, s_w, &total);
  for (int i = i0; i < i1; i++) {
    if (!s_keep[i]) continue;
    A.kps_out[ko + o] = A.kps_in[ko + i];
    if (A.desc_in) {
      const uint4 *src = reinterpret_cast<const uint4 *>(A.desc_in + (ko + i) * 32);
      uint4 *dst = reinterpret_cast<uint4 *>(A.desc_out + (ko + o) * 32);
      dst[0] = src[0]; dst[1] = src[1];
    }
    o++;
  }
  if (tid == 0) A.n_out[b] = total;
}

// The same in two launches, taken when the caller passes a `keep` array (it doubles as the flag store): the verdicts by
// 8 key points per 256-thread workgroup -- thousands of independent row walks in flight instead of 32 at a time inside
// one workgroup, whose serialised byte loads made the one-kernel version 0.29 ms per frame at batch 1 (rocprof, round 3)
// -- and the stable compaction by one workgroup per image.
__global__ __launch_bounds__(256) void k_bird_flags(fb_bird_guidance_args A, int aligned4) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = min(max(A.n_in[b], 0), A.kp_stride);
  const int i = blockIdx.x * 8 + (tid >> 5), sub = tid & 31;
  if (blockIdx.x * 8 >= n) return;
  const size_t ko = (size_t)b * A.kp_stride;
  const uint8_t *icp = A.contour + (size_t)b * A.rows * A.pitch;
  const uint8_t *mask = A.mask ? A.mask + (size_t)b * A.rows * A.pitch : nullptr;
  bool hit = false, ok = true;
  if (i < n) {
    const fb_keypoint kpt = A.kps_in[ko + i];
    const int r = 10;
    const float pt1x = (kpt.x - r) > 0 ? (kpt.x - r) : 0;
    const float pt1y = (kpt.y - r) > 0 ? (kpt.y - r) : 0;
    const float pt2x = (kpt.x + r) < A.cols ? (kpt.x + r) : A.cols;
    const float pt2y = (kpt.y + r) < A.rows ? (kpt.y + r) : A.rows;
    const size_t row = (size_t)pt1x + sub;       // size_t row = pt1x; row < pt2x; row++
    if ((float)row < pt2x && row < (size_t)A.rows) {
      const uint8_t *src = icp + row * (size_t)A.pitch;
      // columns [c0, c1): size_t col = pt1y; col < pt2y && col < cols (at most 21 of them)
      const size_t c0 = (size_t)pt1y;
      size_t c1 = (size_t)pt2y;
      if ((float)c1 < pt2y) c1++;                 // first integer >= pt2y
      if (c1 > (size_t)A.cols) c1 = (size_t)A.cols;
      if (aligned4) {
        // the <= 21 bytes as <= 6 aligned dwords requested together (a byte loop costs one dependent round trip per
        // column); a byte b is >= 10  <=>  ((b & 0x7f) + 0x76) | b  has bit 7 set
        const size_t d0 = c0 >> 2;
        uint32_t any = 0;
#pragma unroll
        for (int k = 0; k < 6; k++) {
          const size_t d = d0 + k;
          if (d * 4 >= c1) break;
          const uint32_t v = reinterpret_cast<const uint32_t *>(src)[d];
          uint32_t m = (((v & 0x7f7f7f7fu) + 0x76767676u) | v) & 0x80808080u;
          const long long lo = (long long)c0 - (long long)(d * 4), hi = (long long)c1 - (long long)(d * 4);  // valid bytes [lo, hi)
          if (lo > 0) m &= 0xffffffffu << (8 * (int)lo);
          if (hi < 4) m &= 0xffffffffu >> (8 * (int)(4 - hi));
          any |= m;
        }
        hit = any != 0u;
      } else {
        for (size_t col = c0; col < c1; col++)
          if (src[col] >= 10) { hit = true; break; }
      }
    }
    if (mask) {
      const int my = (int)(kpt.y + 0.5f), mx = (int)(kpt.x + 0.5f);
      ok = my >= 0 && my < A.rows && mx >= 0 && mx < A.cols && mask[(size_t)my * A.pitch + mx] != 0;
    }
  }
  const unsigned long long bal = __ballot(hit);
  const unsigned int mine = (unsigned int)(bal >> (tid & 32));
  if (sub == 0 && i < n) A.keep[ko + i] = (ok && mine != 0u) ? 1 : 0;
}

__global__ __launch_bounds__(GUIDE_THREADS) void k_bird_compact(fb_bird_guidance_args A) {
  __shared__ int s_w[GUIDE_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(A.n_in[b], 0), A.kp_stride);
  const size_t ko = (size_t)b * A.kp_stride;
  const int per = (n + GUIDE_THREADS - 1) / GUIDE_THREADS;
  const int i0 = min(n, tid * per), i1 = min(n, i0 + per);
  int cnt = 0;
  for (int i = i0; i < i1; i++) cnt += A.keep[ko + i];
  int total;
  int o = fb::block_excl_scan<GUIDE_THREADS>(cnt, s_w, &total);
  for (int i = i0; i < i1; i++) {
    if (!A.keep[ko + i]) continue;
    A.kps_out[ko + o] = A.kps_in[ko + i];
    if (A.desc_in) {
      const uint4 *src = reinterpret_cast<const uint4 *>(A.desc_in + (ko + i) * 32);
      uint4 *dst = reinterpret_cast<uint4 *>(A.desc_out + (ko + o) * 32);
      dst[0] = src[0]; dst[1] = src[1];
    }
    o++;
  }
  if (tid == 0) A.n_out[b] = total;
}

// genEdgesPC: raster-order compaction of the contour pixels into the "sign" ([10,150)) and "free" (>= 150) point lists.
// A thread owns a contiguous run of the raster, two block scans give its output offsets.
__global__ __launch_bounds__(GUIDE_THREADS) void k_bird_edges(fb_bird_guidance_args A) {
  __shared__ int s_w[GUIDE_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const uint8_t *icp = A.contour + (size_t)b * A.rows * A.pitch;
  const int total = A.rows * A.cols;
  const int per = (total + GUIDE_THREADS - 1) / GUIDE_THREADS;
  const int p0 = min(total, tid * per), p1 = min(total, p0 + per);
  int ns = 0, nf = 0;
  {
    int row = p0 / A.cols, col = p0 - row * A.cols;
    for (int p = p0; p < p1; p++) {
      const uint8_t v = icp[(size_t)row * A.pitch + col];
      ns += v >= 10 && v < 150;
      nf += v >= 150;
      if (++col == A.cols) { col = 0; row++; }
    }
  }
  int ts, tf;
  int os = fb::block_excl_scan<GUIDE_THREADS>(ns, s_w, &ts);
  int of = fb::block_excl_scan<GUIDE_THREADS>(nf, s_w, &tf);
  float *es = A.edge_sign + (size_t)b * A.edge_cap * 2, *ef = A.edge_free + (size_t)b * A.edge_cap * 2;
  {
    int row = p0 / A.cols, col = p0 - row * A.cols;
    for (int p = p0; p < p1; p++) {
      const uint8_t v = icp[(size_t)row * A.pitch + col];
      if (v >= 150) { if (of < A.edge_cap) { ef[of * 2] = (float)col; ef[of * 2 + 1] = (float)row; } of++; }
      else if (v >= 10) { if (os < A.edge_cap) { es[os * 2] = (float)col; es[os * 2 + 1] = (float)row; } os++; }
      if (++col == A.cols) { col = 0; row++; }
    }
  }
  if (tid == 0) { A.n_edge_sign[b] = ts; A.n_edge_free[b] = tf; }
}

// ---- cv::cornerSubPix on the bird key points (Frame.cc:345-352; the rules are restated at fb_corner_subpix_args) -----------
// One wave per key point, SUBPIX_WAVES of them in a workgroup, no workgroup barrier: a wave whose point has ended leaves.
// Every lane carries the same centre, so the loop is wave-uniform.  A round: the (2w+3) x (2h+3) patch, pixel p = lane,
// lane + 64, ... (4 byte loads and 3-4 float operations each), goes to the wave's LDS slice; window term k = lane, lane + 64,
// ... reads its four neighbours from there and adds its five fp64 products to the lane's partial sums in ascending k; five
// butterfly sums (fb::wave_sum) give every lane the same totals, bit for bit, and every lane does the 2 x 2 solve.  The
// separable weights come as two host-computed tables in the kernel arguments and are multiplied out into LDS once.
struct SubpixK {
  fb_corner_subpix_args A;
  float wx[2 * SUBPIX_MAX_HALF + 1], wy[2 * SUBPIX_MAX_HALF + 1];
  double eps2;
};

__device__ __forceinline__ void wave_lds_sync() {  // LDS written by the wave's lanes is visible to all of them
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(SUBPIX_THREADS) void k_corner_subpix(SubpixK K) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const fb_corner_subpix_args &A = K.A;
  const int b = blockIdx.y, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * SUBPIX_WAVES + wv;
  if (i >= min(max(A.n[b], 0), A.kp_stride)) return;
  SubpixLds L;
  subpix_layout(L, A.half_win_x, A.half_win_y);
  float *patch = reinterpret_cast<float *>(smem + (size_t)wv * L.slice + L.patch);
  float *weight = reinterpret_cast<float *>(smem + (size_t)wv * L.slice + L.weight);
  const int pw = L.pw, ph = L.ph, ww = L.ww, wh = L.wh, cols = A.cols, rows = A.rows;
  const uint8_t *img = A.image + (size_t)b * A.image_stride;
  const size_t e = (size_t)b * A.kp_stride + i;
  for (int k = lane; k < ww * wh; k += 64) {
    const int r = k / ww, c = k - r * ww;
    float vx = 0.f, vy = 0.f;
#pragma unroll
    for (int t = 0; t < 2 * SUBPIX_MAX_HALF + 1; t++) {  // the tables are kernel arguments: selected, not indexed
      if (c == t) vx = K.wx[t];
      if (r == t) vy = K.wy[t];
    }
    weight[k] = vy * vx;
  }
  const float tx = A.kps[e].x, ty = A.kps[e].y;
  float cx = tx, cy = ty;
  int iter = 0, code = FB_SUBPIX_EXIT_EPS;
  double err = 0.0;
  do {
    // getRectSubPix: the patch's top-left corner, its floor and fraction
    const float ox = cx - (float)(pw - 1) * 0.5f, oy = cy - (float)(ph - 1) * 0.5f;
    const float fx = floorf(ox), fy = floorf(oy);
    const float ax = ox - fx, ay = oy - fy;
    // (a corner further out than this sees the replicated border only: the clamp keeps the integer sums below in range)
    const int ipx = (int)fminf(fmaxf(fx, -1048576.f), 1048576.f), ipy = (int)fminf(fmaxf(fy, -1048576.f), 1048576.f);
    const float a11 = (1.f - ax) * (1.f - ay), a12 = ax * (1.f - ay), a21 = (1.f - ax) * ay, a22 = ax * ay;
    const float b1 = 1.f - ay, b2 = ay;
    for (int p = lane; p < pw * ph; p += 64) {
      const int r = p / pw, c = p - r * pw;
      const int sx = ipx + c, sy = ipy + r;
      const int x0 = min(max(sx, 0), cols - 1), x1 = min(max(sx + 1, 0), cols - 1);
      const int y0 = min(max(sy, 0), rows - 1), y1 = min(max(sy + 1, 0), rows - 1);
      const uint8_t *r0 = img + (size_t)y0 * A.pitch, *r1 = img + (size_t)y1 * A.pitch;
      const float p00 = (float)r0[x0], p01 = (float)r0[x1], p10 = (float)r1[x0], p11 = (float)r1[x1];
      patch[p] = (sx < 0 || sx >= cols - 1) ? p00 * b1 + p10 * b2 : p00 * a11 + p01 * a12 + p10 * a21 + p11 * a22;
    }
    wave_lds_sync();
    double sa = 0.0, sb = 0.0, sc = 0.0, s1 = 0.0, s2 = 0.0;
    for (int k = lane; k < ww * wh; k += 64) {
      const int r = k / ww, c = k - r * ww;
      const float *q = patch + (r + 1) * pw + (c + 1);
      const double m = (double)weight[k];
      const double tgx = (double)(q[1] - q[-1]), tgy = (double)(q[pw] - q[-pw]);
      const double gxx = tgx * tgx * m, gxy = tgx * tgy * m, gyy = tgy * tgy * m;
      const double px = (double)(c - A.half_win_x), py = (double)(r - A.half_win_y);
      sa += gxx; sb += gxy; sc += gyy;
      s1 += gxx * px + gxy * py;
      s2 += gxy * px + gyy * py;
    }
    sa = fb::wave_sum(sa); sb = fb::wave_sum(sb); sc = fb::wave_sum(sc); s1 = fb::wave_sum(s1); s2 = fb::wave_sum(s2);
    wave_lds_sync();  // every lane has read the patch before the next round overwrites it
    const double det = sa * sc - sb * sb;
    if (fabs(det) <= 2.220446049250313e-16 * 2.220446049250313e-16) { code = FB_SUBPIX_EXIT_DET; break; }
    const double scale = 1.0 / det;
    const float nx = (float)((double)cx + sc * scale * s1 - sb * scale * s2);
    const float ny = (float)((double)cy - sb * scale * s1 + sa * scale * s2);
    const float dx = nx - cx, dy = ny - cy;
    err = (double)(dx * dx + dy * dy);
    cx = nx; cy = ny;
    if (cx < 0.f || cx >= (float)cols || cy < 0.f || cy >= (float)rows) { code = FB_SUBPIX_EXIT_OUT; break; }
    if (++iter >= A.max_iter) { code = FB_SUBPIX_EXIT_ITER; break; }
  } while (err > K.eps2);
  if (fabsf(cx - tx) > (float)A.half_win_x || fabsf(cy - ty) > (float)A.half_win_y) { cx = tx; cy = ty; code |= FB_SUBPIX_REVERTED; }
  if (lane == 0) {
    A.kps[e].x = cx; A.kps[e].y = cy;
    if (A.iters) A.iters[e] = iter;
    if (A.exit_code) A.exit_code[e] = (uint8_t)code;
  }
}

int subpix_check(const fb_corner_subpix_args *A, const char *what, SubpixLds *L, size_t *bytes) {
  FB_ARG(A && A->batch >= 0 && A->batch <= 65535 && A->kp_stride >= 0 && A->cols > 0 && A->rows > 0 && A->pitch >= A->cols);
  FB_TRY(plan_subpix(A->half_win_x, A->half_win_y, what, L, bytes));
  FB_ARG(A->max_iter >= 1 && A->max_iter <= SUBPIX_MAX_ITERS && A->eps >= 0.0);
  FB_ARG(A->batch <= 1 || A->image_stride >= (size_t)A->rows * A->pitch);
  if (A->batch == 0 || A->kp_stride == 0) return FB_OK;
  FB_ARG(A->image && A->n && A->kps);
  return FB_OK;
}

}  // namespace

extern "C" {

int fb_bird_guidance_dev(const fb_bird_guidance_args *A, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(A && A->batch >= 0 && A->kp_stride >= 0 && A->cols > 0 && A->rows > 0 && A->pitch >= A->cols && A->edge_cap >= 0);
  if (A->batch == 0) return FB_OK;
  FB_ARG(A->contour && A->n_in && A->n_out && (A->kp_stride == 0 || (A->kps_in && A->kps_out)));
  FB_ARG(!A->desc_in || (A->desc_out && ((uintptr_t)A->desc_in % 16 == 0) && ((uintptr_t)A->desc_out % 16 == 0)));
  FB_ARG(A->kps_out != A->kps_in && (!A->desc_in || A->desc_out != A->desc_in));
  FB_ARG(A->edge_cap == 0 || (A->n_edge_sign && A->n_edge_free && A->edge_sign && A->edge_free));
  FB_ARG((size_t)A->rows * A->cols < (size_t)INT_MAX);
  const size_t lds = (size_t)A->kp_stride + 16;
  if (lds > 150 * 1024) { fb::set_error("fb_bird_guidance: kp_stride %d beyond the LDS flag array", A->kp_stride); return FB_ERR_CAPACITY; }
  FB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_bird_guidance), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  fb::ProfScope prof_(fb::P_BIRDCAM, fb::as_stream(stream));
  if (A->keep && A->kp_stride > 0 && A->batch <= 65535) {
    const int aligned4 = (A->pitch % 4 == 0) && ((uintptr_t)A->contour % 4 == 0) ? 1 : 0;
    k_bird_flags<<<dim3((A->kp_stride + 7) / 8, A->batch), 256, 0, fb::as_stream(stream)>>>(*A, aligned4);
    k_bird_compact<<<A->batch, GUIDE_THREADS, 0, fb::as_stream(stream)>>>(*A);
  } else {
    k_bird_guidance<<<A->batch, GUIDE_THREADS, lds, fb::as_stream(stream)>>>(*A);
  }
  FB_HIP(hipGetLastError());
  if (A->edge_cap > 0) {
    k_bird_edges<<<A->batch, GUIDE_THREADS, 0, fb::as_stream(stream)>>>(*A);
    FB_HIP(hipGetLastError());
  }
  return FB_OK;
}

int fb_bird_guidance(const fb_bird_guidance_args *H) {
  FB_TRY(fb::check_device());
  FB_ARG(H && H->batch >= 0 && H->kp_stride >= 0 && H->cols > 0 && H->rows > 0 && H->pitch >= H->cols && H->edge_cap >= 0);
  if (H->batch == 0) return FB_OK;
  FB_ARG(H->contour && H->n_in && H->n_out && (H->kp_stride == 0 || (H->kps_in && H->kps_out)));
  FB_ARG(!H->desc_in || H->desc_out);
  for (int b = 0; b < H->batch; b++) FB_ARG(H->n_in[b] >= 0 && H->n_in[b] <= H->kp_stride);
  fb_bird_guidance_args D = *H;
  const size_t B = H->batch, ks = H->kp_stride, img = (size_t)H->rows * H->pitch, ec = H->edge_cap;
  fb::Stager st;
  st.in(D.contour, B * img); st.in(D.mask, B * img); st.in(D.n_in, B * 4); st.in(D.kps_in, B * ks * sizeof(fb_keypoint));
  st.out(D.n_out, B * 4, false);
  // outputs are in/out: entries past n_out keep their previous content
  st.out(D.kps_out, B * ks * sizeof(fb_keypoint), true);
  st.out(D.keep, B * ks, true);
  if (H->desc_in) {
    st.in(D.desc_in, B * ks * 32);
    st.out(D.desc_out, B * ks * 32, true);
  } else {
    D.desc_out = nullptr;
  }
  if (ec) {
    FB_ARG(H->n_edge_sign && H->n_edge_free && H->edge_sign && H->edge_free);
    st.out(D.n_edge_sign, B * 4, false); st.out(D.n_edge_free, B * 4, false);
    st.out(D.edge_sign, B * ec * 8, true); st.out(D.edge_free, B * ec * 8, true);
  } else {
    D.n_edge_sign = D.n_edge_free = nullptr;
    D.edge_sign = D.edge_free = nullptr;
  }
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_bird_guidance_dev(&D, nullptr));
  return st.fetch(nullptr);
}

int fb_corner_subpix_dev(const fb_corner_subpix_args *A, void *stream) {
  FB_TRY(fb::check_device());
  SubpixLds L;
  size_t lds = 0;
  FB_TRY(subpix_check(A, "fb_corner_subpix", &L, &lds));
  if (A->batch == 0 || A->kp_stride == 0) return FB_OK;
  SubpixK K;
  memset(&K, 0, sizeof(K));
  K.A = *A;
  // the separable weights exp(-x*x), x = (j - w) / w in float; std::exp(float) of OpenCV, taken through the double exp so that
  // every host gives the same table
  for (int j = 0; j < L.ww; j++) { const float x = (float)(j - A->half_win_x) / (float)A->half_win_x; K.wx[j] = (float)std::exp((double)(-x * x)); }
  for (int i = 0; i < L.wh; i++) { const float y = (float)(i - A->half_win_y) / (float)A->half_win_y; K.wy[i] = (float)std::exp((double)(-y * y)); }
  K.eps2 = A->eps * A->eps;
  fb::ProfScope prof_(fb::P_BIRDCAM, fb::as_stream(stream));
  const dim3 grid((A->kp_stride + SUBPIX_WAVES - 1) / SUBPIX_WAVES, A->batch);
  k_corner_subpix<<<grid, SUBPIX_THREADS, lds, fb::as_stream(stream)>>>(K);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_corner_subpix(const fb_corner_subpix_args *H) {
  FB_TRY(fb::check_device());
  SubpixLds L;
  size_t lds = 0;
  FB_TRY(subpix_check(H, "fb_corner_subpix", &L, &lds));
  if (H->batch == 0 || H->kp_stride == 0) return FB_OK;
  for (int b = 0; b < H->batch; b++) FB_ARG(H->n[b] >= 0 && H->n[b] <= H->kp_stride);
  fb_corner_subpix_args D = *H;
  const size_t B = H->batch, ks = H->kp_stride;
  fb::Stager st;
  st.in(D.image, (B - 1) * H->image_stride + (size_t)H->rows * H->pitch); st.in(D.n, B * 4);
  // in/out: only x / y of the first n entries are written
  st.out(D.kps, B * ks * sizeof(fb_keypoint), true);
  st.out(D.iters, B * ks * 4, true); st.out(D.exit_code, B * ks, true);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_corner_subpix_dev(&D, nullptr));
  return st.fetch(nullptr);
}

int fb_in_frustum_dev(const fb_frustum_args *A, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(A && A->batch >= 0 && A->mp_stride >= 0 && A->n_levels > 0);
  if (A->batch == 0 || A->mp_stride == 0) return FB_OK;
  FB_ARG(A->Tcw && A->Ow && A->n_mp && A->mp_xw && A->mp_normal && A->mp_max_dist && A->mp_min_dist);
  FB_ARG(A->in_view && A->proj && A->level && A->view_cos);
  FB_ARG(A->batch <= 65535);
  fb::ProfScope prof_(fb::P_FRUSTUM, fb::as_stream(stream));
  const dim3 grid((A->mp_stride + FRAME_THREADS - 1) / FRAME_THREADS, A->batch);
  k_in_frustum<<<grid, FRAME_THREADS, 0, fb::as_stream(stream)>>>(*A);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_in_frustum(const fb_frustum_args *H) {
  FB_TRY(fb::check_device());
  FB_ARG(H && H->batch >= 0 && H->mp_stride >= 0);
  fb_frustum_args D = *H;
  const size_t B = H->batch, ms = H->mp_stride;
  if (B == 0 || ms == 0) return FB_OK;
  FB_ARG(H->in_view && H->proj && H->level && H->view_cos);
  fb::Stager st;  // one staged upload / download
  st.in(D.Tcw, B * 48); st.in(D.Ow, B * 12); st.in(D.n_mp, B * 4);
  st.in(D.mp_valid, B * ms); st.in(D.mp_xw, B * ms * 12);
  st.in(D.mp_normal, B * ms * 12); st.in(D.mp_max_dist, B * ms * 4);
  st.in(D.mp_min_dist, B * ms * 4);
  // outputs are in/out (entries that are not in view keep their previous content)
  st.out(D.in_view, B * ms, true); st.out(D.proj, B * ms * 8, true);
  st.out(D.proj_xr, B * ms * 4, true); st.out(D.level, B * ms * 4, true);
  st.out(D.view_cos, B * ms * 4, true);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_in_frustum_dev(&D, nullptr));
  return st.fetch(nullptr);
}

int fb_bird_filter_matches_dev(const fb_bird_filter_args *A, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(A && A->batch >= 0 && A->match_stride >= 0 && A->kp1_stride > 0 && A->kp2_stride > 0 && A->kp2_stride <= 40000);
  if (A->batch == 0 || A->match_stride == 0) return FB_OK;
  FB_ARG(A->n_matches && A->query_idx && A->train_idx && A->cam_xyz1 && A->cam_xyz2 && A->Tcw1 && A->Tcw2 && A->occupied2 && A->keep && A->pt_world);
  const size_t lds = (size_t)A->kp2_stride * 4;
  FB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_bird_filter), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  fb::ProfScope prof_(fb::P_FRUSTUM, fb::as_stream(stream));
  k_bird_filter<<<A->batch, 256, lds, fb::as_stream(stream)>>>(*A);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_bird_filter_matches(const fb_bird_filter_args *H) {
  FB_TRY(fb::check_device());
  FB_ARG(H && H->batch >= 0 && H->match_stride >= 0);
  fb_bird_filter_args D = *H;
  const size_t B = H->batch, ms = H->match_stride, s1 = H->kp1_stride, s2 = H->kp2_stride;
  if (B == 0 || ms == 0) return FB_OK;
  FB_ARG(H->keep && H->pt_world);
  fb::Stager st;
  st.in(D.n_matches, B * 4); st.in(D.query_idx, B * ms * 4);
  st.in(D.train_idx, B * ms * 4); st.in(D.cam_xyz1, B * s1 * 12);
  st.in(D.cam_xyz2, B * s2 * 12); st.in(D.Tcw1, B * 48); st.in(D.Tcw2, B * 48);
  st.in(D.occupied2, B * s2);
  st.out(D.keep, B * ms, true); st.out(D.pt_world, B * ms * 12, true);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_bird_filter_matches_dev(&D, nullptr));
  return st.fetch(nullptr);
}

int fb_undistort_keypoints_dev(const fb_keypoint *d_kps, const int32_t *d_n, int batch, int kp_stride, const float *K4,
                               const float *D4, fb_keypoint *d_kps_un, void *stream) {
  FB_TRY(fb::check_device());
  FB_ARG(batch >= 0 && kp_stride >= 0 && K4 && D4 && batch <= 65535);
  if (batch == 0 || kp_stride == 0) return FB_OK;
  FB_ARG(d_kps && d_n && d_kps_un);
  CamKD C;
  for (int i = 0; i < 4; i++) { C.K[i] = K4[i]; C.D[i] = D4[i]; }
  fb::ProfScope prof_(fb::P_UNDISTORT, fb::as_stream(stream));
  const dim3 grid((kp_stride + FRAME_THREADS - 1) / FRAME_THREADS, batch);
  k_undistort<<<grid, FRAME_THREADS, 0, fb::as_stream(stream)>>>(d_kps, d_n, kp_stride, C, d_kps_un);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_undistort_keypoints(const fb_keypoint *kps, int n, const float *K4, const float *D4, fb_keypoint *kps_un) {
  FB_TRY(fb::check_device());
  FB_ARG(n >= 0 && K4 && D4);
  if (n == 0) return FB_OK;
  FB_ARG(kps && kps_un);
  const int32_t n32 = n;
  const int32_t *cnt = &n32;
  fb::Stager st;
  st.in(kps, (size_t)n * sizeof(fb_keypoint)); st.in(cnt, 4);
  st.out(kps_un, (size_t)n * sizeof(fb_keypoint), false);
  FB_TRY(st.commit(nullptr));
  FB_TRY(fb_undistort_keypoints_dev(kps, cnt, 1, n, K4, D4, kps_un, nullptr));
  return st.fetch(nullptr);
}

int fb_image_bounds(int cols, int rows, const float *K4, const float *D4, float *bounds) {
  FB_ARG(cols > 0 && rows > 0 && K4 && D4 && bounds);
  if (D4[0] == 0.0f) {  // Frame.cc:787-793
    bounds[0] = 0.0f; bounds[1] = (float)cols; bounds[2] = 0.0f; bounds[3] = (float)rows;
    return FB_OK;
  }
  fb_keypoint c[4] = {}, u[4];
  c[1].x = (float)cols; c[2].y = (float)rows; c[3].x = (float)cols; c[3].y = (float)rows;
  FB_TRY(fb_undistort_keypoints(c, 4, K4, D4, u));
  // sic: the running maxima start from numeric_limits<float>::min(), the smallest POSITIVE float (Frame.cc:758-761)
  float mnMinX = 3.402823466e+38f, mnMaxX = 1.175494351e-38f, mnMinY = 3.402823466e+38f, mnMaxY = 1.175494351e-38f;
  for (int i = 0; i < 4; i++) {
    if (u[i].x < mnMinX) mnMinX = u[i].x;
    if (u[i].x > mnMaxX) mnMaxX = u[i].x;
    if (u[i].y < mnMinY) mnMinY = u[i].y;
    if (u[i].y > mnMaxY) mnMaxY = u[i].y;
  }
  bounds[0] = mnMinX; bounds[1] = mnMaxX; bounds[2] = mnMinY; bounds[3] = mnMaxY;
  return FB_OK;
}

}  // extern "C"
