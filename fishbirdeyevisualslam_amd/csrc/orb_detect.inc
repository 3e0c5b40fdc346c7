// orb_detect.inc -- cv::ORB's detector (OpenCV 3 features2d/src/orb.cpp computeKeyPoints, restated at fb_orb_detect_args in
// fishbird.h) on the handle's raw pyramid: k_det_mask, k_det_fast, k_det_select, k_det_emit (included by orb.hip).  The
// argument block, the tile grid, the workspace and the LDS of k_det_select are orb_detect_plan.h.
//
// Nothing returns to the host between the kernels: the first cut is read off a 256-bin histogram, the second is an exact
// radix select on the float bits, and every list is compacted in raster order by prefix scans, so the output order does
// not depend on how the workgroups are scheduled.

namespace {

// ---- the mask pyramid: THRESH_TOZERO at 254 on a freshly resized level (levels >= 1), in place ----------------------------
__global__ __launch_bounds__(256) void k_det_mask(uint8_t *level, long long imgStride, int dwords) {  // grid.y: the mask pyramids
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= dwords) return;
  uint32_t *p = reinterpret_cast<uint32_t *>(level + (long long)blockIdx.y * imgStride) + i;
  const uint32_t v = *p;
  uint32_t o = 0;
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (((v >> (8 * k)) & 0xFFu) == 0xFFu) o |= 0xFFu << (8 * k);
  *p = o;
}

__device__ __forceinline__ const uint8_t *det_raw_level(const DetK &K, int b, int l, int *pitch) {
  *pitch = l == 0 ? K.pitch0 : K.L[l].pitch;
  return l == 0 ? K.img0 + (long long)b * K.img_stride : K.pyr + (long long)b * K.pyr_stride + K.L[l].off;
}

// ---- cv::FAST(level, threshold, true) + runByImageBorder(31) + runByPixelsMask -> map, hist ------------------------------
// One workgroup per 64 x 16 tile of one level (the level from the tile index, like k_fast's waves).  Raw pixels are staged
// with their coordinates clamped into the level: a clamped pixel is only ever read by a score that is forced to 0 (its
// centre lies in the 3-px rim of the level).
__global__ __launch_bounds__(DET_FAST_THREADS) void k_det_fast(DetK K) {
  __shared__ __attribute__((aligned(4))) uint8_t s_raw[DET_RAW_H * DET_RAW_W];
  __shared__ __attribute__((aligned(4))) uint8_t s_sc[DET_SC_H * DET_SC_PITCH];
  __shared__ int s_hist[256];
  const int tid = threadIdx.x, b = blockIdx.y;
  int l = 0;
  while (l + 1 < K.nlevels && (int)blockIdx.x >= K.tileBase[l + 1]) l++;
  const DetLevel &Lv = K.L[l];
  const int t = blockIdx.x - K.tileBase[l];
  const int x0 = (t % Lv.tilesX) * DET_TW, y0 = (t / Lv.tilesX) * DET_TH;
  const int w = Lv.w, h = Lv.h;
  int rpitch;
  const uint8_t *raw = det_raw_level(K, b, l, &rpitch);
  s_hist[tid] = 0;
  for (int i = tid; i < DET_RAW_H * DET_RAW_W; i += DET_FAST_THREADS) {
    const int ry = i / DET_RAW_W, rx = i - ry * DET_RAW_W;
    const int gx = min(max(x0 - 4 + rx, 0), w - 1), gy = min(max(y0 - 4 + ry, 0), h - 1);
    s_raw[i] = raw[(long long)gy * rpitch + gx];
  }
  __syncthreads();
  for (int i = tid; i < DET_SC_H * DET_SC_W; i += DET_FAST_THREADS) {
    const int sy = i / DET_SC_W, sx = i - sy * DET_SC_W;
    const int gx = x0 - 1 + sx, gy = y0 - 1 + sy;
    int s = 0;
    if (gx >= 3 && gx < w - 3 && gy >= 3 && gy < h - 3) {
      const uint8_t *c = s_raw + (sy + 3) * DET_RAW_W + sx + 3;
      const int v = c[0];
      int d[16];
#pragma unroll
      for (int k = 0; k < 16; k++) d[k] = fbscore::IntOps::sub(v, c[fbscore::ring_offset(k, DET_RAW_W)]);
      s = fbscore::score_network<fbscore::IntOps>(d);
      if (s < K.thr) s = 0;  // passes at threshold t iff its score, the largest passing threshold, is >= t
    }
    s_sc[sy * DET_SC_PITCH + sx] = (uint8_t)s;
  }
  __syncthreads();
  const int oy = tid >> 4, ox4 = (tid & 15) * 4, gy = y0 + oy;
  uint32_t packed = 0;
  if (gy >= DET_EDGE && gy < h - DET_EDGE) {
    const uint8_t *mrow = nullptr;
    if (K.mask0)
      mrow = l == 0 ? K.mask0 + (long long)b * K.mask_img_stride + (long long)gy * K.mask_pitch0
                    : K.maskpyr + (long long)b * K.maskpyr_stride + Lv.off + (long long)gy * Lv.pitch;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int gx = x0 + ox4 + k;
      const uint8_t *p = s_sc + (oy + 1) * DET_SC_PITCH + ox4 + k + 1;
      const int s = p[0];
      bool keep = s > 0 && gx >= DET_EDGE && gx < w - DET_EDGE;
      keep = keep && s > p[-1] && s > p[1] && s > p[-DET_SC_PITCH - 1] && s > p[-DET_SC_PITCH] && s > p[-DET_SC_PITCH + 1] &&
             s > p[DET_SC_PITCH - 1] && s > p[DET_SC_PITCH] && s > p[DET_SC_PITCH + 1];
      if (keep && mrow) keep = mrow[gx] != 0;
      if (keep) {
        packed |= (uint32_t)s << (8 * k);
        atomicAdd(&s_hist[s], 1);
      }
    }
  }
  // the tile's 64 columns lie inside the level's pitch (a multiple of 64): the padding columns are written too, as 0
  if (gy < h) *reinterpret_cast<uint32_t *>(K.map + (long long)b * K.map_stride + Lv.moff + (long long)gy * Lv.pitch + x0 + ox4) = packed;
  __syncthreads();
  if (s_hist[tid]) atomicAdd(&K.hist[((size_t)b * K.nlevels + l) * 256 + tid], (unsigned)s_hist[tid]);
}

// HarrisResponses (blockSize 7, k = 0.04) at (px, py): integer sums of the 3x3 Sobel products over the 7 x 7 block, then
// the float expression with every operation rounded on its own
__device__ __forceinline__ float det_harris(const uint8_t *raw, int pitch, int px, int py) {
  int a = 0, bb = 0, c = 0;
  int r0[9], r1[9], r2[9];
  const uint8_t *p = raw + (long long)(py - 4) * pitch + px - 4;
#pragma unroll
  for (int j = 0; j < 9; j++) { r0[j] = p[j]; r1[j] = p[pitch + j]; }
  for (int i = 0; i < 7; i++) {
    const uint8_t *q = p + (long long)(i + 2) * pitch;
#pragma unroll
    for (int j = 0; j < 9; j++) r2[j] = q[j];
#pragma unroll
    for (int j = 1; j < 8; j++) {
      const int Ix = (r1[j + 1] - r1[j - 1]) * 2 + (r0[j + 1] - r0[j - 1]) + (r2[j + 1] - r2[j - 1]);
      const int Iy = (r2[j] - r0[j]) * 2 + (r2[j - 1] - r0[j - 1]) + (r2[j + 1] - r0[j + 1]);
      a += Ix * Ix;
      bb += Iy * Iy;
      c += Ix * Iy;
    }
#pragma unroll
    for (int j = 0; j < 9; j++) { r0[j] = r1[j]; r1[j] = r2[j]; }
  }
  const float fa = (float)a, fb_ = (float)bb, fc = (float)c;
  const float det = __fsub_rn(__fmul_rn(fa, fb_), __fmul_rn(fc, fc));
  const float tr = __fadd_rn(fa, fb_);
  return __fmul_rn(__fsub_rn(det, __fmul_rn(__fmul_rn(DET_HARRIS_K, tr), tr)), DET_S4);
}

// the order-preserving integer image of a float (-0.0 counts as 0.0; a NaN cannot occur)
__device__ __forceinline__ uint32_t det_key(float f) {
  uint32_t u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The largest bin d of a 256-bin histogram with count(bins >= d) >= want, found by the first wave: lane j owns the bins
// 255 - 4 j .. 252 - 4 j, an inclusive scan over the lanes finds the one lane whose bins hold the cut, and that lane walks its
// four.  out[0] = the total, out[1] = d, out[2] = want - count(bins > d), the rank left inside bin d.  With total < want,
// out[1] = 0 and out[2] is meaningless.  Ends with a barrier.
__device__ __forceinline__ void det_find_cut(const int *s_hist, int want, int *out) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x, top = 255 - 4 * lane;
    const int h0 = s_hist[top], h1 = s_hist[top - 1], h2 = s_hist[top - 2], h3 = s_hist[top - 3];
    const int c = h0 + h1 + h2 + h3, inc = fb::wave_incl_scan(c), above = inc - c;
    if (lane == 63) { out[0] = inc; if (inc < want) out[1] = 0; }
    if (above < want && want <= inc) {
      int d = top, acc = above;
      if (acc + h0 < want) { acc += h0; d--; if (acc + h1 < want) { acc += h1; d--; if (acc + h2 < want) { acc += h2; d--; } } }
      out[1] = d;
      out[2] = want - acc;
    }
  }
  __syncthreads();
}

// ---- retainBest #1 -> Harris -> retainBest #2 of one (image, level): cnt, and the level's final list in pos / resp --------
__global__ __launch_bounds__(DET_SEL_THREADS) void k_det_select(DetK K) {
  extern __shared__ __attribute__((aligned(16))) uint8_t det_smem[];
  DetSelLds S;
  det_select_layout(S);
  int *s_hist = reinterpret_cast<int *>(det_smem + S.hist), *s_wv = reinterpret_cast<int *>(det_smem + S.wv);
  int *s_misc = reinterpret_cast<int *>(det_smem + S.misc);
  const int tid = threadIdx.x, l = blockIdx.x, b = blockIdx.y;
  const DetLevel &Lv = K.L[l];
  int32_t *cnt = K.cnt + (size_t)b * K.nlevels + l;
  if (Lv.tilesX == 0 || Lv.K2 <= 0) {  // a level that holds no key point; retainBest(0) clears the list
    if (tid == 0) *cnt = 0;
    return;
  }
  // the first cut: the smallest score that is kept
  if (tid < 256) s_hist[tid] = (int)K.hist[((size_t)b * K.nlevels + l) * 256 + tid];
  __syncthreads();
  det_find_cut(s_hist, Lv.K1, s_misc);
  const int T1 = s_misc[0] > Lv.K1 ? s_misc[1] : 1;  // (bin 0 is empty: with more than K1 survivors the cut is a score >= 1)
  uint32_t *pos = K.pos + (size_t)b * K.cand_stride + Lv.candBase;
  float *resp = K.resp + (size_t)b * K.cand_stride + Lv.candBase;
  // the survivors in raster order: the rows [31, h - 31) of the map as one run of 16-byte chunks (pitch % 64 == 0)
  const uint4 *map = reinterpret_cast<const uint4 *>(K.map + (long long)b * K.map_stride + Lv.moff);
  const int cpr = Lv.pitch >> 4, chunk0 = DET_EDGE * cpr, chunk1 = (Lv.h - DET_EDGE) * cpr;
  int n1 = 0;
  for (int base = chunk0; base < chunk1; base += DET_SEL_THREADS) {
    const int ch = base + tid;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (ch < chunk1) v = map[ch];
    const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
    int c = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) c += (int)((wd[k >> 2] >> (8 * (k & 3))) & 0xFFu) >= T1;
    int tot;
    int o = n1 + fb::block_excl_scan<DET_SEL_THREADS>(c, s_wv, &tot);
    if (c) {
      const int py = ch / cpr, pxb = (ch - py * cpr) * 16;
#pragma unroll
      for (int k = 0; k < 16; k++) {
        const uint32_t s = (wd[k >> 2] >> (8 * (k & 3))) & 0xFFu;
        if ((int)s >= T1) {
          if (o < Lv.candCap) pos[o] = (uint32_t)(pxb + k) | ((uint32_t)py << 12) | (s << 24);
          o++;
        }
      }
    }
    n1 += tot;
  }
  n1 = min(n1, Lv.candCap);  // (the suppression bounds it; the clamp only keeps a broken map inside the list)
  __syncthreads();
  // the Harris response of each
  int rpitch;
  const uint8_t *raw = det_raw_level(K, b, l, &rpitch);
  for (int i = tid; i < n1; i += DET_SEL_THREADS) {
    const uint32_t p = pos[i];
    resp[i] = det_harris(raw, rpitch, (int)(p & 0xFFFu), (int)((p >> 12) & 0xFFFu));
  }
  __syncthreads();
  // the second cut: the key of the K2-th largest response, digit by digit from the top
  uint32_t Tk = 0;
  if (n1 > Lv.K2) {
    uint32_t prefix = 0, known = 0;
    int want = Lv.K2;  // its rank among the keys that share `prefix`
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) s_hist[tid] = 0;
      __syncthreads();
      for (int i = tid; i < n1; i += DET_SEL_THREADS) {
        const uint32_t k = det_key(resp[i]);
        if ((k & known) == prefix) atomicAdd(&s_hist[(k >> shift) & 0xFFu], 1);
      }
      __syncthreads();
      det_find_cut(s_hist, want, s_misc);  // (the keys that share `prefix` are at least `want`: the cut exists)
      prefix |= (uint32_t)s_misc[1] << shift;
      known |= 0xFFu << shift;
      want = s_misc[2];
      __syncthreads();
    }
    Tk = prefix;
  }
  // the kept ones, still in raster order, in place: an entry moves to an index at or below its own, and every entry of a
  // round is read before the scan's barriers and written behind them
  int n2 = 0;
  for (int base = 0; base < n1; base += DET_SEL_THREADS) {
    const int i = base + tid;
    uint32_t p = 0;
    float r = 0.f;
    bool keep = false;
    if (i < n1) { p = pos[i]; r = resp[i]; keep = det_key(r) >= Tk; }
    int tot;
    const int o = n2 + fb::block_excl_scan<DET_SEL_THREADS>(keep ? 1 : 0, s_wv, &tot);
    if (keep) { pos[o] = p; resp[o] = r; }
    n2 += tot;
    __syncthreads();
  }
  if (tid == 0) *cnt = n2;
}

// ---- IC_Angle and the key-point record of output slot i: one wave each, levels ascending, raster order within a level ------
__global__ __launch_bounds__(DET_EMIT_WAVES * 64) void k_det_emit(DetK K) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int i = blockIdx.x * DET_EMIT_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int32_t *cnt = K.cnt + (size_t)b * K.nlevels;
  int total = 0, l = -1, first = 0;
  for (int k = 0; k < K.nlevels; k++) {
    const int c = cnt[k];
    if (i >= total && i < total + c) { l = k; first = total; }
    total += c;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    K.n[b] = min(total, K.kp_stride);
    if (K.n_true) K.n_true[b] = total;
  }
  if (l < 0 || i >= K.kp_stride) return;
  const DetLevel &Lv = K.L[l];
  const size_t e = (size_t)b * K.cand_stride + Lv.candBase + (i - first);
  const uint32_t p = K.pos[e];
  const int px = (int)(p & 0xFFFu), py = (int)((p >> 12) & 0xFFFu);
  int rpitch;
  const uint8_t *raw = det_raw_level(K, b, l, &rpitch);
  // IC_Angle as k_describe_at computes it: lanes 2 (v + 15) and 2 (v + 15) + 1 sum the left (u < 0) and the right (u >= 0)
  // part of row v with the weights and the circular mask of plan_angle_table; 31 <= px < w - 31 keeps every byte inside
  int m10 = 0, m01 = 0;
  if (lane < 62) {
    const uint4 T = reinterpret_cast<const uint4 *>(K.ang_tab)[lane];
    const uint32_t tw[4] = {T.x, T.y, T.z, T.w};
    const int v = (lane >> 1) - HALF_PATCH, half = lane & 1;
    const uint8_t *row = raw + (long long)(py + v) * rpitch + px - HALF_PATCH + (half ? HALF_PATCH : 0);
    int a10 = 0, rs = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int wgt = (int)((tw[j >> 2] >> (8 * (j & 3))) & 0xFFu), val = row[j];
      a10 += val * (wgt & 0xF);
      rs += val * ((wgt >> 4) & 1);
    }
    m10 = half ? a10 : -a10;
    m01 = v * rs;
  }
  m10 = fb::wave_sum(m10);
  m01 = fb::wave_sum(m01);
  if (lane == 0) {
    fb_keypoint kp;
    kp.x = __fmul_rn((float)px, Lv.scale);
    kp.y = __fmul_rn((float)py, Lv.scale);
    kp.size = __fmul_rn(DET_PATCH, Lv.scale);
    kp.angle = fb_fast_atan2((float)m01, (float)m10);
    kp.response = K.resp[e];
    kp.octave = l;
    K.kps[(size_t)b * K.kp_stride + i] = kp;
  }
}

}  // namespace
