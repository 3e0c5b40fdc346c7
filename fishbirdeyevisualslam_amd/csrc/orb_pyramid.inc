// orb_pyramid.inc -- ComputePyramid: the three cv::resize kernels of the ORB extractor (included by orb.hip; the tables
// they read and the choice between them are planned in orb_plan.h).

namespace {

// ------------------------------------------------------------------------------------------
// cv::resize INTER_LINEAR, 8U, 11-bit fixed point (oracle: resize_linear_u8). 4 px per lane.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int win_byte(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, int k) {  // byte k of a 16-byte window
  const uint32_t lo = k & 8 ? w2 : w0, hi = k & 8 ? w3 : w1;
  const uint32_t w = k & 4 ? hi : lo;
  return (w >> (8 * (k & 3))) & 0xFF;
}

__global__ __launch_bounds__(256) void k_resize(const uint8_t *__restrict__ src0, long long srcImgStride, int sw,
                                                int sh, int spitch, uint8_t *__restrict__ dst0, long long dstImgStride,
                                                int dw, int dh, int dpitch, ResizeTabs tb) {
  const int b = blockIdx.z;
  const int dy = blockIdx.y * blockDim.y + threadIdx.y;
  const int dx4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (dy >= dh || dx4 >= dpitch) return;
  const uint8_t *src = src0 + (long long)b * srcImgStride;
  uint8_t *dst = dst0 + (long long)b * dstImgStride;
  int sy0 = tb.yofs[dy], sy1 = sy0 + 1;
  sy0 = sy0 >= 0 ? (sy0 < sh ? sy0 : sh - 1) : 0;
  sy1 = sy1 >= 0 ? (sy1 < sh ? sy1 : sh - 1) : 0;
  const int b0 = tb.ibeta[dy * 2], b1 = tb.ibeta[dy * 2 + 1];
  const uint8_t *r0p = src + (long long)sy0 * spitch, *r1p = src + (long long)sy1 * spitch;
  uint32_t packed = 0;
  // the 4 destination pixels of this lane read source columns [sxa, sxb+1]; when that span fits a 16-byte
  // window that is 4-byte aligned and inside the row, fetch it with 4 dword loads per row instead of 16 byte loads
  const int dxl = min(dx4 + 3, dw - 1);
  const int sxa = dx4 < dw ? tb.xofs[dx4] : 0, sxb = dx4 < dw ? min(tb.xofs[dxl] + 1, sw - 1) : 0;
  const int a = sxa & ~3;
  const bool wide = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)spitch) & 3) == 0 && (sxb - a) < 16 && a + 16 <= spitch;
  if (wide) {
    const uint32_t *p0 = reinterpret_cast<const uint32_t *>(r0p + a), *p1 = reinterpret_cast<const uint32_t *>(r1p + a);
    const uint32_t u0 = p0[0], u1 = p0[1], u2 = p0[2], u3 = p0[3], v0 = p1[0], v1 = p1[1], v2 = p1[2], v3 = p1[3];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int dx = dx4 + k;
      int v = 0;
      if (dx < dw) {
        const int sx = tb.xofs[dx];
        const int sx1 = min(sx + 1, sw - 1);
        const int a0 = tb.ialpha[dx * 2], a1 = tb.ialpha[dx * 2 + 1];
        const int r0 = win_byte(u0, u1, u2, u3, sx - a) * a0 + win_byte(u0, u1, u2, u3, sx1 - a) * a1;
        const int r1 = win_byte(v0, v1, v2, v3, sx - a) * a0 + win_byte(v0, v1, v2, v3, sx1 - a) * a1;
        v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
        v = min(max(v, 0), 255);
      }
      packed |= (uint32_t)v << (8 * k);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int dx = dx4 + k;
      int v = 0;
      if (dx < dw) {
        const int sx = tb.xofs[dx];
        const int sx1 = min(sx + 1, sw - 1);
        const int a0 = tb.ialpha[dx * 2], a1 = tb.ialpha[dx * 2 + 1];
        const int r0 = r0p[sx] * a0 + r0p[sx1] * a1;
        const int r1 = r1p[sx] * a0 + r1p[sx1] * a1;
        v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
        v = min(max(v, 0), 255);
      }
      packed |= (uint32_t)v << (8 * k);
    }
  }
  *reinterpret_cast<uint32_t *>(dst + (long long)dy * dpitch + dx4) = packed;
}

// Same arithmetic, restructured for throughput (used when the source is dword aligned and the scale is <= 2, i.e.
// always for the ORB pyramid): a lane owns 4 adjacent destination pixels and walks RR destination rows.  The column
// constants (window offset, byte offsets, packed weights) live in registers for the whole walk; per source row the
// lane fetches one 12-byte window (3 dword loads) and does the horizontal pass with v_alignbyte + v_perm + v_dot2;
// a source row shared by two successive destination rows (4 of 5 at scale 1.2) is filtered once.

__global__ __launch_bounds__(256) void k_resize_rows(const uint8_t *__restrict__ src0, long long srcImgStride, int sw,
                                                     int sh, int spitch, uint8_t *__restrict__ dst0,
                                                     long long dstImgStride, int dw, int dh, int dpitch, ResizeTabs tb) {
  const int b = blockIdx.z;
  const int dyBase = __builtin_amdgcn_readfirstlane((blockIdx.y * blockDim.y + threadIdx.y) * RESIZE_ROWS);
  const int dx4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (dyBase >= dh || dx4 >= dpitch) return;
  const uint8_t *src = src0 + (long long)b * srcImgStride;
  uint8_t *dst = dst0 + (long long)b * dstImgStride;
  // column constants
  const int dxf = min(dx4, dw - 1);
  const int a = tb.xofs[dxf] & ~3;
  const int aw = min(a, spitch - 12);  // keep the 12-byte window inside the row (only the zero-padded tail moves)
  // The taps of the lane's 4 pixels lie within 8 bytes of the first tap (scale <= 2): two v_alignbyte bring those 8
  // bytes to a fixed place, one v_perm per pixel spreads its two taps for v_dot2.
  uint32_t selw[4];                    // v_perm selector: tap0 -> bits 0..7, tap1 -> bits 16..23 of the shifted pair
  uint32_t wgt[4];                     // a0 | a1 << 16
  uint32_t liveMask = 0;               // bytes of the packed result that are destination pixels
  const int o0 = tb.xofs[dxf] - aw;    // byte offset of the first tap inside the 12-byte window, 0..10
  const uint32_t sh0 = (uint32_t)o0 & 3u;
  const int q0 = o0 >> 2;              // 0, except in the clamped window of the row's tail
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int dx = dx4 + k;
    if (dx < dw) liveMask |= 0xffu << (8 * k);
    const int dxc = min(dx, dw - 1);
    const int sx = tb.xofs[dxc];
    int a0 = tb.ialpha[dxc * 2], a1 = tb.ialpha[dxc * 2 + 1];
    if (sx + 1 > sw - 1) { a0 += a1; a1 = 0; }  // right border: both taps read sx
    const uint32_t ob = (uint32_t)(sx - aw - o0);  // 0..6
    selw[k] = ob | (0x0cu << 8) | ((ob + 1u) << 16) | (0x0cu << 24);
    wgt[k] = (uint32_t)(a0 & 0xffff) | ((uint32_t)a1 << 16);
  }
  const bool anyTail = __ballot(q0 != 0) != 0ull;  // wave-uniform
  const uint32_t mq1 = q0 == 1 ? ~0u : 0u, mq2 = q0 >= 2 ? ~0u : 0u, mq12 = mq1 | mq2;
  auto loadWin = [&](int sy, uint32_t (&wv)[3]) {
    sy = sy >= 0 ? (sy < sh ? sy : sh - 1) : 0;
    const uint32_t *p = reinterpret_cast<const uint32_t *>(src + ((uint32_t)__mul24(sy, spitch) + (uint32_t)aw));
    wv[0] = p[0]; wv[1] = p[1]; wv[2] = p[2];
  };
  auto hpass = [&](const uint32_t (&wv)[3], int h[4]) {
    uint32_t x0 = wv[0], x1 = wv[1], x2 = wv[2];
    if (anyTail) {  // the first tap sits in dword q0 of the window (bit selects: no divergent branches)
      x0 = (wv[0] & ~mq12) | (wv[1] & mq1) | (wv[2] & mq2);
      x1 = (wv[1] & ~mq12) | (wv[2] & mq12);
    }
    const uint32_t e0 = __builtin_amdgcn_alignbyte(x1, x0, sh0), e1 = __builtin_amdgcn_alignbyte(x2, x1, sh0);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t spread = __builtin_amdgcn_perm(e1, e0, selw[k]);  // tap0 | tap1 << 16
      int d;
      asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(d) : "v"(spread), "v"(wgt[k]));
      h[k] = d >> 4;
    }
  };
  int h0[4], h1[4];
  int prevS1 = -0x40000000;
  const int dyEnd = min(dyBase + RESIZE_ROWS, dh);
  // every source window of the RESIZE_ROWS destination rows is requested before the first one is used (a row that two
  // destination rows share is simply requested twice): load -> wait -> use per row serialises the memory latency
  int sy0s[RESIZE_ROWS], b0s[RESIZE_ROWS], b1s[RESIZE_ROWS];
  uint32_t wa[RESIZE_ROWS][3], wb[RESIZE_ROWS][3];
#pragma unroll
  for (int j = 0; j < RESIZE_ROWS; j++) {
    const int dyc = min(dyBase + j, dh - 1);
    sy0s[j] = tb.yofs[dyc];
    b0s[j] = tb.ibeta[dyc * 2];
    b1s[j] = tb.ibeta[dyc * 2 + 1];
    loadWin(sy0s[j], wa[j]);
    loadWin(sy0s[j] + 1, wb[j]);
  }
#pragma unroll
  for (int j = 0; j < RESIZE_ROWS; j++) {
    const int dy = dyBase + j;
    if (dy >= dyEnd) break;
    const int sy0 = sy0s[j];
    const int b0 = b0s[j], b1 = b1s[j];
    if (sy0 == prevS1) {
#pragma unroll
      for (int k = 0; k < 4; k++) h0[k] = h1[k];
    } else {
      hpass(wa[j], h0);
    }
    hpass(wb[j], h1);
    prevS1 = sy0 + 1;
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      // |b| <= 2048, h <= 255 * 2048 >> 4, b0 + b1 = 2048, no negative weight: 0 <= v <= 255 without a clamp
      const int v = ((__mul24(b0, h0[k]) >> 16) + (__mul24(b1, h1[k]) >> 16) + 2) >> 2;
      packed |= (uint32_t)v << (8 * k);
    }
    *reinterpret_cast<uint32_t *>(dst + (long long)dy * dpitch + dx4) = packed & liveMask;
  }
}

// k_resize_rows loads BOTH source rows of every destination row although neighbours share one (at scale 1.2 eight rows ask
// for 16 windows but need 10 or 11 different ones), and the kernel is bound by the bytes it has in flight per wave.  This one
// walks the SOURCE rows of a run of RM_ROWS destination rows once: all RM_SRC windows are requested up front, every source row
// is filtered horizontally once, and a destination row is written when its second source row has been filtered (each source
// row closes at most one destination row because the scale is >= 1).  Same arithmetic as k_resize_rows; used when every run of
// RM_ROWS destination rows spans at most RM_SRC source rows (scale factors up to 1.25), k_resize_rows otherwise.

__global__ __launch_bounds__(256) void k_resize_merge(const uint8_t *__restrict__ src0, long long srcImgStride, int sw,
                                                      int sh, int spitch, uint8_t *__restrict__ dst0,
                                                      long long dstImgStride, int dw, int dh, int dpitch, ResizeTabs tb) {
  const int b = blockIdx.z;
  const int dyBase = __builtin_amdgcn_readfirstlane((blockIdx.y * blockDim.y + threadIdx.y) * RM_ROWS);
  const int dx4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (dyBase >= dh || dx4 >= dpitch) return;
  const int lane = threadIdx.x;  // blockDim.x = 64: a wave is one row of the block
  const uint8_t *src = src0 + (long long)b * srcImgStride;
  uint8_t *dst = dst0 + (long long)b * dstImgStride;
  // column constants (as in k_resize_rows)
  const int dxf = min(dx4, dw - 1);
  const int a = tb.xofs[dxf] & ~3;
  const int aw = min(a, spitch - 12);
  uint32_t selw[4], wgt[4], liveMask = 0;
  const int o0 = tb.xofs[dxf] - aw;
  const uint32_t sh0 = (uint32_t)o0 & 3u;
  const int q0 = o0 >> 2;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int dx = dx4 + k;
    if (dx < dw) liveMask |= 0xffu << (8 * k);
    const int dxc = min(dx, dw - 1);
    const int sx = tb.xofs[dxc];
    int a0 = tb.ialpha[dxc * 2], a1 = tb.ialpha[dxc * 2 + 1];
    if (sx + 1 > sw - 1) { a0 += a1; a1 = 0; }
    const uint32_t ob = (uint32_t)(sx - aw - o0);
    selw[k] = ob | (0x0cu << 8) | ((ob + 1u) << 16) | (0x0cu << 24);
    wgt[k] = (uint32_t)(a0 & 0xffff) | ((uint32_t)a1 << 16);
  }
  const bool anyTail = __ballot(q0 != 0) != 0ull;
  const uint32_t mq1 = q0 == 1 ? ~0u : 0u, mq2 = q0 >= 2 ? ~0u : 0u, mq12 = mq1 | mq2;
  // row constants: lane j of the wave holds the first source row and the two weights of destination row dyBase + j
  const int nrows = min(RM_ROWS, dh - dyBase);
  const int dyl = min(dyBase + min(lane, RM_ROWS - 1), dh - 1);
  const int syLane = tb.yofs[dyl];
  const int betaLane = (int)((uint32_t)(uint16_t)tb.ibeta[dyl * 2] | ((uint32_t)(uint16_t)tb.ibeta[dyl * 2 + 1] << 16));
  const int base = __builtin_amdgcn_readfirstlane(syLane);  // first source row of the run
  uint32_t w[RM_SRC][3];
#pragma unroll
  for (int r = 0; r < RM_SRC; r++) {
    int sy = base + r;
    sy = sy >= 0 ? (sy < sh ? sy : sh - 1) : 0;
    const uint32_t *p = reinterpret_cast<const uint32_t *>(src + ((uint32_t)__mul24(sy, spitch) + (uint32_t)aw));
    w[r][0] = p[0]; w[r][1] = p[1]; w[r][2] = p[2];
  }
  int hp[4] = {0, 0, 0, 0}, hc[4];
  int j = 0;
#pragma unroll
  for (int r = 0; r < RM_SRC; r++) {
    {  // horizontal pass of source row base + r
      uint32_t x0 = w[r][0], x1 = w[r][1];
      const uint32_t x2 = w[r][2];
      if (anyTail) {
        x0 = (w[r][0] & ~mq12) | (w[r][1] & mq1) | (w[r][2] & mq2);
        x1 = (w[r][1] & ~mq12) | (w[r][2] & mq12);
      }
      const uint32_t e0 = __builtin_amdgcn_alignbyte(x1, x0, sh0), e1 = __builtin_amdgcn_alignbyte(x2, x1, sh0);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t spread = __builtin_amdgcn_perm(e1, e0, selw[k]);
        int d;
        asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(d) : "v"(spread), "v"(wgt[k]));
        hc[k] = d >> 4;
      }
    }
    if (r >= 1 && j < nrows) {
      const int sy0 = __builtin_amdgcn_readlane(syLane, j);
      if (sy0 == base + r - 1) {  // wave-uniform: this source row is the second row of destination row j
        const int bw = __builtin_amdgcn_readlane(betaLane, j);
        const int b0 = (int)(short)(bw & 0xffff), b1 = bw >> 16;
        uint32_t packed = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int v = ((__mul24(b0, hp[k]) >> 16) + (__mul24(b1, hc[k]) >> 16) + 2) >> 2;
          packed |= (uint32_t)v << (8 * k);
        }
        *reinterpret_cast<uint32_t *>(dst + (long long)(dyBase + j) * dpitch + dx4) = packed & liveMask;
        j++;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) hp[k] = hc[k];
  }
}

}  // namespace
