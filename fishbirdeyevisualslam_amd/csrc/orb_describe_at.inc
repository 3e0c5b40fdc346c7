// orb_describe_at.inc -- computeOrbDescriptor (and IC_Angle, on request) at key points the CALLER supplies: k_describe_at
// (included by orb.hip).  The rules are restated at fb_orb_describe_args in fishbird.h; the LDS plan and the argument block
// are orb_describe_at_plan.h.

namespace {

// One wave per key point, DESCAT_WAVES of them in a workgroup, no workgroup barrier (the shape of k_corner_subpix): a wave
// whose slot is empty, or whose key point is refused, leaves.  Unlike k_describe, which takes the level from blockIdx and
// packed integer level coordinates from the quadtree's runs, everything here comes from the key point's own record: every
// lane loads the same 24 bytes, the octave is made wave-uniform with readfirstlane and selects the level's geometry in the
// kernel arguments, and the position is cvRound(pt * mvInvScaleFactor[octave]) -- tested against the level's 19-px border
// as a float, before the conversion, so that NaN and +-inf end as FB_DESCRIBE_BORDER by the form of the comparison.
// The radius-18 blurred patch (and in IC-angle mode the radius-15 raw patch) is then staged into the wave's LDS slice with
// dword loads, all issued before the first is used; the orientation moments and the 256 steered tests read LDS, for the
// reason recorded at k_describe (scattered byte loads are bound by the L1 tag rate).  Each wave reads back only what it
// wrote itself, so a wave-level fence is all the synchronisation there is.
__global__ __launch_bounds__(DESCAT_THREADS) void k_describe_at(DescAtK K) {
  extern __shared__ __attribute__((aligned(16))) uint8_t descat_smem[];
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = blockIdx.x * DESCAT_WAVES + wv;
  if (i >= min(max(K.n[b], 0), K.kp_stride)) return;
  const size_t e = (size_t)b * K.kp_stride + i;
  const fb_keypoint kp = K.kps[e];
  const int l = __builtin_amdgcn_readfirstlane(kp.octave);
  if (l < 0 || l >= K.nlevels) {
    if (lane == 0 && K.status) K.status[e] = FB_DESCRIBE_LEVEL;
    return;
  }
  const DescAtLevel &Lv = K.L[l];
  // cvRound(kpt.pt.x * scale): the product in float, to nearest with halves to even (the default rounding mode)
  const float rx = rintf(kp.x * Lv.inv_scale), ry = rintf(kp.y * Lv.inv_scale);
  const bool inside = rx >= (float)DESCAT_EDGE && rx <= (float)(Lv.w - DESCAT_EDGE - 1) && ry >= (float)DESCAT_EDGE && ry <= (float)(Lv.h - DESCAT_EDGE - 1);
  if (!inside) {  // (false for NaN: every comparison with it is)
    if (lane == 0 && K.status) K.status[e] = FB_DESCRIBE_BORDER;
    return;
  }
  const int px = __builtin_amdgcn_readfirstlane((int)rx), py = __builtin_amdgcn_readfirstlane((int)ry);
  const int pitch = Lv.pitch;
  const bool ic = K.angle_mode == FB_DESCRIBE_IC_ANGLE;
  DescAtLds S;
  describe_at_layout(S, K.angle_mode);
  uint32_t *blp = reinterpret_cast<uint32_t *>(descat_smem + (size_t)wv * S.slice + S.blur);
  uint32_t *rawp = reinterpret_cast<uint32_t *>(descat_smem + (size_t)wv * S.slice + S.raw);
  // Sources.  The blurred level is the handle's own buffer: base, level offset and pitch are multiples of 64.  The raw
  // level is the handle's pyramid above level 0 (aligned likewise) and the caller's image at level 0, which may start and
  // stride anywhere: dword loads only where pointer and pitch allow them, byte loads otherwise.
  const uint8_t *bsrc = K.blur + (long long)b * K.blur_stride + Lv.boff;
  const uint8_t *rsrc = l == 0 ? K.img0 + (long long)b * K.img_stride : K.pyr + (long long)b * K.pyr_stride + Lv.off;
  const int rpitch = l == 0 ? K.pitch0 : pitch;
  const bool rawAligned = ((reinterpret_cast<uintptr_t>(rsrc) | (uintptr_t)rpitch) & 3) == 0;
  const int bxa = (px - DESCAT_BL_R) & ~3, box = (px - DESCAT_BL_R) - bxa;
  const int rxa = (px - DESCAT_RAW_R) & ~3, rox = rawAligned ? (px - DESCAT_RAW_R) - rxa : 0;
  // Dword t = lane + 64 it of a patch is (row t / DW, dword t % DW).  19 <= px <= w - 20 and the same in y keep every row
  // inside the level; a row's last dword may reach up to 3 bytes past column w - 1, which is the row's padding or the
  // start of the next row (the patches end >= 1 / 4 rows above the level's last row), never past the buffer.
  constexpr int NB = DESCAT_BL_ROWS * DESCAT_BL_DW, NR = DESCAT_RAW_ROWS * DESCAT_RAW_DW;
  constexpr int NB_IT = (NB + 63) / 64, NR_IT = (NR + 63) / 64;
  uint32_t vb[NB_IT], vr[NR_IT];
#pragma unroll
  for (int it = 0; it < NB_IT; it++) {
    const int t = min(lane + 64 * it, NB - 1), r = t / DESCAT_BL_DW, d = t - r * DESCAT_BL_DW;
    vb[it] = *reinterpret_cast<const uint32_t *>(bsrc + (uint32_t)(__mul24(py - DESCAT_BL_R + r, pitch) + bxa + 4 * d));
  }
  if (ic && rawAligned) {
#pragma unroll
    for (int it = 0; it < NR_IT; it++) {
      const int t = min(lane + 64 * it, NR - 1), r = t / DESCAT_RAW_DW, d = t - r * DESCAT_RAW_DW;
      vr[it] = *reinterpret_cast<const uint32_t *>(rsrc + (uint32_t)(__mul24(py - DESCAT_RAW_R + r, rpitch) + rxa + 4 * d));
    }
  }
#pragma unroll
  for (int it = 0; it < NB_IT; it++)
    if (lane + 64 * it < NB) blp[lane + 64 * it] = vb[it];
  if (ic) {
    if (rawAligned) {
#pragma unroll
      for (int it = 0; it < NR_IT; it++)
        if (lane + 64 * it < NR) rawp[lane + 64 * it] = vr[it];
    } else {
      uint8_t *rb = reinterpret_cast<uint8_t *>(rawp);
      for (int t = lane; t < DESCAT_RAW_ROWS * DESCAT_RAW_ROWS; t += 64) {
        const int yy = t / DESCAT_RAW_ROWS, xx = t - yy * DESCAT_RAW_ROWS;
        rb[yy * (DESCAT_RAW_DW * 4) + xx] = rsrc[(long long)(py - DESCAT_RAW_R + yy) * rpitch + px - DESCAT_RAW_R + xx];
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float angle = kp.angle;
  if (ic) {
    // IC_Angle (ORBextractor.cc:77-104): lanes 2 (v + 15) and 2 (v + 15) + 1 sum the left (u < 0) and the right (u >= 0)
    // part of row v of the circular patch: 16 bytes each, weighted with |u| and masked with |u| <= umax[|v|] by the
    // per-lane table of the handle's workspace (plan_angle_table: weight in the low nibble, mask in bit 4)
    const uint4 T = reinterpret_cast<const uint4 *>(K.ang_tab)[lane < 62 ? lane : 0];
    int m10 = 0, m01 = 0;
    if (lane < 62) {
      const int r = lane >> 1, half = lane & 1;
      const int sb = rox + (half ? DESCAT_RAW_R : 0);
      const uint32_t *rowd = rawp + r * DESCAT_RAW_DW + (sb >> 2);
      const uint32_t sh = (uint32_t)(sb & 3);
      const uint32_t d0 = rowd[0], d1 = rowd[1], d2 = rowd[2], d3 = rowd[3], d4 = rowd[4];
      const uint32_t q[4] = {__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh),
                             __builtin_amdgcn_alignbyte(d3, d2, sh), __builtin_amdgcn_alignbyte(d4, d3, sh)};
      const uint32_t tw[4] = {T.x, T.y, T.z, T.w};
      uint32_t a10 = 0u, rs = 0u;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        a10 = __builtin_amdgcn_udot4(q[k], tw[k] & 0x0f0f0f0fu, a10, false);
        rs = __builtin_amdgcn_udot4(q[k], (tw[k] >> 4) & 0x01010101u, rs, false);
      }
      m10 = half ? (int)a10 : -(int)a10;
      m01 = __mul24(r - DESCAT_RAW_R, (int)rs);
    }
    m10 = fb::wave_sum(m10);
    m01 = fb::wave_sum(m01);
    angle = fb_fast_atan2((float)m01, (float)m10);
  }
  // computeOrbDescriptor (ORBextractor.cc:107-147): the lane computes the tests 4 lane .. 4 lane + 3.  A finite angle keeps
  // every rotated sample within 18 px of the centre; the clamp only keeps a non-finite angle handed in by the caller
  // (FB_DESCRIBE_KEEP_ANGLE) inside the wave's slice.
  const uint4 pq = reinterpret_cast<const uint4 *>(c_pattern.test)[lane];
  const float factorPI = 0x1.1df46ap-6f;
  float sa, ca;
  fb_sincos_f(angle * factorPI, &sa, &ca);
  const uint8_t *centre = reinterpret_cast<const uint8_t *>(blp) + DESCAT_BL_R * (DESCAT_BL_DW * 4) + box + DESCAT_BL_R;
  auto sample = [&](float x, float y) {
    const int rr = min(max(fb_cvround(x * sa + y * ca), -DESCAT_BL_R), DESCAT_BL_R);
    const int cc = min(max(fb_cvround(x * ca - y * sa), -DESCAT_BL_R), DESCAT_BL_R);
    return (int)centre[__mul24(rr, DESCAT_BL_DW * 4) + cc];
  };
  int nib = 0;
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const uint32_t p = t == 0 ? pq.x : t == 1 ? pq.y : t == 2 ? pq.z : pq.w;
    const float x0 = (float)(p & 0xFFu) - (float)PAT_BIAS, y0 = (float)((p >> 8) & 0xFFu) - (float)PAT_BIAS;
    const float x1 = (float)((p >> 16) & 0xFFu) - (float)PAT_BIAS, y1 = (float)(p >> 24) - (float)PAT_BIAS;
    nib |= (sample(x0, y0) < sample(x1, y1)) << t;
  }
  // lane 2 j holds the low nibble of descriptor byte j, lane 2 j + 1 the high nibble; the lanes 8 j assemble dword j
  const int byteVal = nib | (__shfl_down(nib, 1, 64) << 4);
  const int b1 = __shfl_down(byteVal, 2, 64), b2 = __shfl_down(byteVal, 4, 64), b3 = __shfl_down(byteVal, 6, 64);
  const uint32_t dw = (uint32_t)byteVal | ((uint32_t)b1 << 8) | ((uint32_t)b2 << 16) | ((uint32_t)b3 << 24);
  if ((lane & 7) == 0) reinterpret_cast<uint32_t *>(K.desc + e * 32)[lane >> 3] = dw;
  if (lane == 0) {
    if (ic) K.kps[e].angle = angle;
    if (K.status) K.status[e] = FB_DESCRIBE_OK;
  }
}

}  // namespace
