// orb_describe.inc -- GaussianBlur, IC_Angle and computeOrbDescriptor: k_blur and k_describe (included by orb.hip).

namespace {

// ------------------------------------------------------------------------------------------
// GaussianBlur(level, 7x7, sigma 2, BORDER_REFLECT_101) of every pyramid level (ORBextractor.cc:1080), integer
// kernel {18,34,49,55,49,34,18}/256 per pass, (sum + 2^15) >> 16 (oracle gaussian_blur7).  A wave owns a strip of
// 256 columns x BLUR_ROWS rows: a lane filters 4 adjacent pixels and walks down the rows with the last seven
// horizontal results in registers.  Horizontal pass = 2 x v_dot4_u32_u8 per pixel on a 12-byte window.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect101(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  return i;
}

// One launch blurs the levels [l0, l1): its grid covers the strips blurStrips[l0] .. blurStrips[l1] (the whole pyramid is
// [0, nlevels)), so that a level can be blurred as soon as the resize that writes it has run (FB_ORB_BLUR_CUTS).
__global__ __launch_bounds__(256) void k_blur(OrbK K, int l0, int l1, const uint8_t *__restrict__ img0, long long imgStride, int pitch0,
                                              const uint8_t *__restrict__ pyr, uint8_t *__restrict__ blur) {
  const int b = blockIdx.y;
  const int strip = __builtin_amdgcn_readfirstlane(K.blurStrips[l0] + blockIdx.x * 4 + (threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  if (strip >= K.blurStrips[l1]) return;
  int l = l0;
  while (strip >= K.blurStrips[l + 1]) l++;
  const LevelInfo &L = K.L[l];
  const int w = L.w, h = L.h;
  const int sidx = strip - K.blurStrips[l];
  const int nsx = (w + 255) >> 8;
  const int sy = sidx / nsx, sx = sidx - sy * nsx;
  const int x0 = sx * 256 + lane * 4;
  const int y0 = sy * BLUR_ROWS;
  if (x0 >= w) return;
  const uint8_t *img;
  int pitch;
  if (l == 0) { img = img0 + (long long)b * imgStride; pitch = pitch0; }
  else { img = pyr + (long long)b * K.pyrStride + L.off; pitch = L.pitch; }
  uint8_t *out = blur + (long long)b * K.blurStride + L.boff;
  // Column groups whose 12-byte window leaves the row (x0 == 0 and the last one or two groups): the window is loaded
  // from a clamped start instead and its bytes are rearranged with two v_perm per dword so that every out-of-row
  // column holds its BORDER_REFLECT_101 partner (which always lies inside the same 12 bytes).
  const bool edge = x0 < 4 || x0 + 8 > w;
  const int base = edge ? max(min(x0 - 4, w - 12), 0) : x0 - 4;
  uint32_t m1[3] = {0, 0, 0}, m2[3] = {0, 0, 0};
  if (edge) {
#pragma unroll
    for (int i = 0; i < 12; i++) {
      const int c = reflect101(min(x0 - 4 + i, w + 2), w);
      const int sidx8 = min(max(c - base, 0), 11);
      const uint32_t lo = sidx8 < 8 ? (uint32_t)sidx8 : 0x0cu, hi = sidx8 < 8 ? 0x0cu : (uint32_t)(sidx8 - 8);
      m1[i >> 2] |= lo << (8 * (i & 3));
      m2[i >> 2] |= hi << (8 * (i & 3));
    }
  }
  const bool anyEdge = __ballot(edge) != 0ull;
  // horizontal pass: the taps of pixel j are the window bytes 1+j .. 7+j.  The weights are shifted to the bytes, not the
  // bytes to the weights: W<j><d> weighs dword d of the window for pixel j (2 + 3 + 3 + 2 dots per row and no v_alignbyte;
  // 6 v_alignbyte + 8 dots before).  The constants live in scalar registers.
  constexpr uint32_t W0A = (18u << 8) | (34u << 16) | (49u << 24), W0B = 55u | (49u << 8) | (34u << 16) | (18u << 24);
  constexpr uint32_t W1A = (18u << 16) | (34u << 24), W1B = 49u | (55u << 8) | (49u << 16) | (34u << 24), W1C = 18u;
  constexpr uint32_t W2A = 18u << 24, W2B = 34u | (49u << 8) | (55u << 16) | (49u << 24), W2C = 34u | (18u << 8);
  constexpr uint32_t W3B = 18u | (34u << 8) | (49u << 16) | (55u << 24), W3C = 49u | (34u << 8) | (18u << 16);
  // vertical pass: the horizontal sums are 16-bit (<= 255 * 256), so two successive rows of a pixel share a register and
  // v_dot2_u32_u16 takes two taps at once: pairs[r % 6][k] = row r-1 | row r << 16 of pixel k
  uint32_t pairs[6][4];
  uint32_t prevh[4] = {0u, 0u, 0u, 0u};
  uint32_t rnd = 1u << 15;         // the rounding term of the vertical pass, pinned to a scalar register: as a literal it is
  asm volatile("" : "+s"(rnd));    // moved into a vector register again for every row
  // The source rows run BLUR_PF rows ahead of the arithmetic: a load -> wait -> use per row would serialise one memory
  // latency per row (22 per wave).  Row indices past the image are reflected, so every prefetch address is valid.
  constexpr int BLUR_PF = 4;
  uint32_t q[BLUR_PF][3];
  auto loadRow = [&](int r, uint32_t (&dst)[3]) {
    const int ys = reflect101(min(y0 + r - 3, h + 2), h);
    const uint8_t *row = img + (uint32_t)__mul24(ys, pitch);  // 32-bit offset: 64-bit multiplies are quarter rate
    const uint32_t *pw = reinterpret_cast<const uint32_t *>(row + base);
    dst[0] = pw[0]; dst[1] = pw[1]; dst[2] = pw[2];
  };
#pragma unroll
  for (int r = 0; r < BLUR_PF; r++) loadRow(r, q[r]);
#pragma unroll
  for (int r = 0; r < BLUR_ROWS + 6; r++) {
    const int yo = y0 + r - 6;  // destination row completed by this source row
    if (r >= 6 && yo >= h) break;
    uint32_t w0 = q[r % BLUR_PF][0], w1 = q[r % BLUR_PF][1], w2 = q[r % BLUR_PF][2];
    if (r + BLUR_PF < BLUR_ROWS + 6) loadRow(r + BLUR_PF, q[r % BLUR_PF]);
    if (anyEdge) {
      const uint32_t e0 = __builtin_amdgcn_perm(w1, w0, m1[0]) | __builtin_amdgcn_perm(w2, w2, m2[0]);
      const uint32_t e1 = __builtin_amdgcn_perm(w1, w0, m1[1]) | __builtin_amdgcn_perm(w2, w2, m2[1]);
      const uint32_t e2 = __builtin_amdgcn_perm(w1, w0, m1[2]) | __builtin_amdgcn_perm(w2, w2, m2[2]);
      if (edge) { w0 = e0; w1 = e1; w2 = e2; }
    }
    uint32_t hr[4];
    // taps of pixel j are window bytes 1+j .. 7+j
    hr[0] = __builtin_amdgcn_udot4(w1, W0B, __builtin_amdgcn_udot4(w0, W0A, 0u, false), false);
    hr[1] = __builtin_amdgcn_udot4(w2, W1C, __builtin_amdgcn_udot4(w1, W1B, __builtin_amdgcn_udot4(w0, W1A, 0u, false), false), false);
    hr[2] = __builtin_amdgcn_udot4(w2, W2C, __builtin_amdgcn_udot4(w1, W2B, __builtin_amdgcn_udot4(w0, W2A, 0u, false), false), false);
    hr[3] = __builtin_amdgcn_udot4(w2, W3C, __builtin_amdgcn_udot4(w1, W3B, 0u, false), false);
    if (r >= 6) {
      typedef unsigned short u16x2b __attribute__((ext_vector_type(2)));
      const u16x2b W01 = {18, 34}, W23 = {49, 55}, W45 = {49, 34};
      uint32_t sum[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        // rows r-6 .. r with weights 18 34 49 55 49 34 18: three two-tap dots on the row pairs + the new row
        sum[k] = (uint32_t)__mul24(18, (int)hr[k]) + rnd;
        sum[k] = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2b, pairs[(r + 1) % 6][k]), W01, sum[k], false);  // rows r-6, r-5
        sum[k] = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2b, pairs[(r + 3) % 6][k]), W23, sum[k], false);  // rows r-4, r-3
        sum[k] = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2b, pairs[(r + 5) % 6][k]), W45, sum[k], false);  // rows r-2, r-1
      }
      // min(sum >> 16, 255) of four pixels -> four bytes: the high halves of two sums share a register (sum <= 257 * 65535
      // + 2^15, so a high half is <= 257), one packed 16-bit min clamps both, and a last v_perm gathers the low bytes
      const u16x2b C255 = {255, 255};
      const u16x2b h01 = __builtin_elementwise_min(__builtin_bit_cast(u16x2b, __builtin_amdgcn_perm(sum[1], sum[0], 0x07060302u)), C255);
      const u16x2b h23 = __builtin_elementwise_min(__builtin_bit_cast(u16x2b, __builtin_amdgcn_perm(sum[3], sum[2], 0x07060302u)), C255);
      const uint32_t packed = __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, h23), __builtin_bit_cast(uint32_t, h01), 0x06040200u);
      *reinterpret_cast<uint32_t *>(out + (uint32_t)(__mul24(yo, L.pitch) + x0)) = packed;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) { pairs[r % 6][k] = prevh[k] | (hr[k] << 16); prevh[k] = hr[k]; }
  }
}

// ------------------------------------------------------------------------------------------
// Orientation (IC_Angle on the raw level), 256 steered BRIEF tests on the blurred level, and the final cv::KeyPoint
// record.  Key points sit >= 19 px inside the level (EDGE_THRESHOLD), so the radius-15 orientation patch and the
// radius-18 test footprint never leave the image.
// ------------------------------------------------------------------------------------------
// The radius-15 raw patch (orientation) and the radius-18 blurred patch (BRIEF tests) are staged into LDS with
// coalesced dword loads: the 512 rotated sample positions are then LDS gathers instead of scattered byte loads that
// would each cost a cache-line lookup in the vector L1 (measured: the L1 tag rate, not ALU or HBM, bounded the
// direct-gather version).
constexpr int DP_RAW_DW = 9, DP_RAW_ROWS = 31;    // 31 rows x 36 B  (x-15 .. x+15 after dword alignment)
constexpr int DP_BL_DW = 10, DP_BL_ROWS = 37;     // 37 rows x 40 B  (x-18 .. x+18 after dword alignment)

// A wave owns DESC_KPW consecutive slots of ONE level's run of lvlOut (never of two levels: the last wave of a level
// with an odd count has one key point).  The workgroups of a level are K.descBase[l] .. K.descBase[l + 1]), sized for the
// run's capacity, so the level and the address of the wave's records follow from blockIdx alone: the records, the level
// counts and the level's geometry are requested together, and one wait later the wave knows whether its slots are
// occupied (slot < cnts[l]), where its key points go (sum of the counts below l, + slot: level-major, quadtree order
// within a level) and what to fetch.  (Before, a wave owned a global key-point index: counts -> record -> level geometry
// -> patches were four dependent round trips.)  The sampling pattern is 16 B and the orientation table 16 B per lane
// (64 B and 32 B as float4 / separate weight and mask dwords before).
// The kernel is bound by the latency of its ~70 scattered cache lines per key point, not by arithmetic.  Measured at
// B=256 (single stream, front / bird image): 698 / 416 us per launch with global key-point indices and float tables,
// 651 / 392 us with this mapping (minima 527 / 393 -> 468 / 365 us); the overlapped step 3.466 -> 3.387 ms.  The
// prologue-only ablation (K.dbg == 11) does NOT fall with it, 25 -> 42 us at B=64: it now contains the level geometry
// and waits for the scalar tables of all FB_MAX_LEVELS levels, which the full kernel hides behind the record fetch.
// DESC_KPW 3 and 4 with the freed registers (88 / 95 VGPRs against 75, scratch 0) give the same step within the
// run-to-run spread (3.375 / 3.384 against 3.387 ms): 2 stays.  Older measurements, with global indices (per step, both
// images): one key point per wave 0.97 ms; 8 per wave with the NEXT patch prefetched during the tests 1.47 ms (the
// tests are far too short to cover a patch); 2 per wave with both patches requested together 0.93 ms.  More resident
// waves did not help the overlapped step (amdgpu_waves_per_eu 6: same time; 7: spills, 1.12 ms), so the occupancy is
// pinned at the 5 waves per SIMD it had at 85 VGPRs.
__global__ __launch_bounds__(64 * DESC_WPB) __attribute__((amdgpu_waves_per_eu(5, 5)))
void k_describe(OrbK K, const uint8_t *__restrict__ img0, long long imgStride,
                                                 int pitch0, const uint8_t *__restrict__ pyr,
                                                 const uint8_t *__restrict__ blur, const uint4 *__restrict__ angTab,
                                                 const uint32_t *__restrict__ lvlOut, const int *__restrict__ lvlCount,
                                                 fb_keypoint *__restrict__ kps, uint8_t *__restrict__ desc,
                                                 int32_t *__restrict__ nOut) {
  __shared__ __attribute__((aligned(16))) uint32_t rawp_all[DESC_WPB][DP_RAW_ROWS * DP_RAW_DW + 4];
  __shared__ __attribute__((aligned(16))) uint32_t blp_all[DESC_WPB][DP_BL_ROWS * DP_BL_DW + 2];
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t *rawp = rawp_all[wv], *blp = blp_all[wv];
  // per-lane tables: tests 4*lane .. 4*lane+3 and the IC_Angle weights of this lane's half row
  const uint4 pq = reinterpret_cast<const uint4 *>(c_pattern.test)[lane];
  const uint4 angT = angTab[lane < 62 ? lane : 0];
  // XCD-aware mapping (as in k_fast): consecutive workgroups go to different XCDs; give each XCD a contiguous run of
  // slots (neighbours in the quadtree order overlap in the image) so that their patches share lines in one L2.  The
  // grid is a multiple of 8 workgroups; those past the last level's run find their slot past every count and leave.
  const int wg = (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
  int l = 0, runBase = K.runBase[0], runCap = K.runCap[0];
#pragma unroll
  for (int i = 1; i < FB_MAX_LEVELS; i++)
    if (i < K.nlevels && wg >= K.descBase[i]) { l = i; runBase = K.runBase[i]; runCap = K.runCap[i]; }
  const int slot = ((wg - K.descBase[l]) * DESC_WPB + wv) * DESC_KPW;
  // three independent fetches: the records (an empty slot reads the run's last entry and drops it) ...
  const uint32_t *run = lvlOut + (long long)b * K.outStride + runBase;
  uint32_t rec[DESC_KPW];
#pragma unroll
  for (int j = 0; j < DESC_KPW; j++) rec[j] = run[min(slot + j, runCap - 1)];
  // ... the level counts ...
  const int *cnts = lvlCount + b * K.nlevels;
  int below = 0, total = 0, mine = 0;
#pragma unroll
  for (int i = 0; i < FB_MAX_LEVELS; i++) {
    const int ci = cnts[i];  // (the buffer has FB_MAX_LEVELS entries of slack: an unconditional load, all of them together)
    const int c = i < K.nlevels ? ci : 0;
    total += c; below += i < l ? c : 0; mine = i == l ? c : mine;
  }
  // ... and the level's geometry
  const LevelInfo &Lv = K.L[l];
  const int lvPitch = Lv.pitch, lvPatch = Lv.patchSize;
  const long long lvOff = Lv.off, lvBoff = Lv.boff;
  const float lvScale = Lv.scale;
  const int nk = min(total, K.capOut);
  if (wg == 0 && threadIdx.x == 0) nOut[b] = nk;  // wg == 0 is blockIdx.x == 0: once per image
  const int first = below + slot;  // output index of the wave's first key point; past capOut it is dropped
  const int nmine = min(DESC_KPW, min(mine - slot, nk - first));
  if (K.dbg == 11) { if ((int)(pq.x + pq.w) + (int)angT.x + (int)rec[0] + (int)rec[DESC_KPW - 1] + nmine + lvPitch + lvPatch + (int)lvOff + (int)lvBoff + (int)lvScale == 1234567) nOut[0] = 1; return; }
  if (nmine <= 0) return;
  const uint4 angW = make_uint4(angT.x & 0x0f0f0f0fu, angT.y & 0x0f0f0f0fu, angT.z & 0x0f0f0f0fu, angT.w & 0x0f0f0f0fu);
  const uint4 angK = make_uint4((angT.x >> 4) & 0x01010101u, (angT.y >> 4) & 0x01010101u, (angT.z >> 4) & 0x01010101u, (angT.w >> 4) & 0x01010101u);
  // the wave's level: source of the raw patch (level 0 is the caller's image) and of the blurred patch
  const uint8_t *lvImg = l == 0 ? img0 + (long long)b * imgStride : pyr + (long long)b * K.pyrStride + lvOff;
  const int rawPitch = l == 0 ? pitch0 : lvPitch;
  const uint8_t *lvBlur = blur + (long long)b * K.blurStride + lvBoff;
  const bool rawAligned = ((reinterpret_cast<uintptr_t>(lvImg) | (uintptr_t)rawPitch) & 3) == 0;
  // fixed lane -> (row within a group, dword) mapping: 6 rows x 10 dwords (7 x 9 for the raw patch) per pass, so the
  // global offsets and the LDS indices are constants per lane (32-bit offsets from wave-uniform bases, 24-bit
  // multiplies: 64/32-bit integer multiplies are quarter rate)
  constexpr int NB_IT = (DP_BL_ROWS + 5) / 6, NR_IT = (DP_RAW_ROWS + 6) / 7;
  const int rb0 = (lane * 205) >> 11, dwb = lane - rb0 * DP_BL_DW;   // lane / 10
  const int rr0 = (lane * 57) >> 9, dwr = lane - rr0 * DP_RAW_DW;    // lane / 9
  struct KP {  // wave-uniform description of one key point
    int cx, cy, resp, pitch, bpitch, bxa, box, rxa, rox;
    const uint8_t *img, *bbase;
    bool rawAligned;
  };
  auto decode = [&](int j) {
    KP k;
    const uint32_t r = rec[j];
    k.cx = r & 0xFFF; k.cy = (r >> 12) & 0xFFF; k.resp = r >> 24;
    k.img = lvImg; k.pitch = rawPitch; k.bbase = lvBlur; k.bpitch = lvPitch; k.rawAligned = rawAligned;
    k.bxa = (k.cx - 18) & ~3; k.box = (k.cx - 18) - k.bxa;
    k.rxa = (k.cx - 15) & ~3;
    k.rox = k.rawAligned ? (k.cx - 15) - k.rxa : 0;
    return k;
  };
  uint32_t vb[DESC_KPW][NB_IT], vr[DESC_KPW][NR_IT];
  // All global loads of both patches are issued together (rows past a patch are clamped and their data dropped; key
  // points sit >= 19 px inside the level, so neither patch leaves the image)
  auto issue = [&](const KP &k, uint32_t (&vb)[NB_IT], uint32_t (&vr)[NR_IT]) {
    {  // row offsets advance by a constant; only the last group can run past the patch and is clamped
      uint32_t off = (uint32_t)(__mul24(k.cy - 18 + rb0, k.bpitch) + k.bxa + min(dwb, DP_BL_DW - 1) * 4);
      const uint32_t step = 6u * (uint32_t)k.bpitch;
#pragma unroll
      for (int it = 0; it < NB_IT - 1; it++, off += step) vb[it] = *reinterpret_cast<const uint32_t *>(k.bbase + off);
      vb[NB_IT - 1] = *reinterpret_cast<const uint32_t *>(k.bbase + (uint32_t)(__mul24(k.cy - 18 + min((NB_IT - 1) * 6 + rb0, DP_BL_ROWS - 1), k.bpitch) + k.bxa + min(dwb, DP_BL_DW - 1) * 4));
    }
    if (k.rawAligned) {
      uint32_t off = (uint32_t)(__mul24(k.cy - 15 + rr0, k.pitch) + k.rxa + min(dwr, DP_RAW_DW - 1) * 4);
      const uint32_t step = 7u * (uint32_t)k.pitch;
#pragma unroll
      for (int it = 0; it < NR_IT - 1; it++, off += step) vr[it] = *reinterpret_cast<const uint32_t *>(k.img + off);
      vr[NR_IT - 1] = *reinterpret_cast<const uint32_t *>(k.img + (uint32_t)(__mul24(k.cy - 15 + min((NR_IT - 1) * 7 + rr0, DP_RAW_ROWS - 1), k.pitch) + k.rxa + min(dwr, DP_RAW_DW - 1) * 4));
    }
  };
  auto stage = [&](const KP &k, const uint32_t (&vb)[NB_IT], const uint32_t (&vr)[NR_IT]) {
    if (lane < 6 * DP_BL_DW) {
#pragma unroll
      for (int it = 0; it < NB_IT; it++)
        if (it * 6 + rb0 < DP_BL_ROWS) blp[it * 6 * DP_BL_DW + lane] = vb[it];
    }
    if (k.rawAligned) {
      if (lane < 7 * DP_RAW_DW) {
#pragma unroll
        for (int it = 0; it < NR_IT; it++)
          if (it * 7 + rr0 < DP_RAW_ROWS) rawp[it * 7 * DP_RAW_DW + lane] = vr[it];
      }
    } else {  // caller's level-0 image with an odd stride: byte loads
      uint8_t *rb = reinterpret_cast<uint8_t *>(rawp);
      for (int i = lane; i < DP_RAW_ROWS * 31; i += 64) {
        const int yy = i / 31, xx = i - yy * 31;
        rb[yy * (DP_RAW_DW * 4) + xx] = k.img[(long long)(k.cy - 15 + yy) * k.pitch + k.cx - 15 + xx];
      }
    }
    // each wave reads back only what it wrote itself: LDS operations of one wave complete in order, so a wave-level
    // fence (no s_barrier across the workgroup) is all that is needed
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  // the patch loads of ALL of the wave's key points are requested before the first patch is used
  KP kpv[DESC_KPW];
#pragma unroll
  for (int j = 0; j < DESC_KPW; j++) {
    kpv[j] = decode(j);
    if (j < nmine) issue(kpv[j], vb[j], vr[j]);
  }
#pragma unroll
  for (int j = 0; j < DESC_KPW; j++) {
    if (j >= nmine) break;
    const KP &cur = kpv[j];
    stage(cur, vb[j], vr[j]);
    // IC_Angle (ORBextractor.cc:77-104): lanes 2*(v+15) and 2*(v+15)+1 sum the left (u < 0) and right (u >= 0) part
    // of row v of the circular patch.  Each half row is 16 bytes read as dwords; |u| weights and the circular mask
    // (|u| <= umax[|v|]) come from a per-lane table (angTab[lane] = 4 dwords, unpacked above into angW / angK) and the sums
    // are v_dot4_u32_u8.
    int m10 = 0, m01 = 0;
    if (lane < 62) {
      const int r = lane >> 1, half = lane & 1;
      const int sb = cur.rox + (half ? 15 : 0);  // left half: u = -15..0 at bytes rox..rox+15, right half: u = 0..15 at rox+15..
      const uint32_t *rowd = rawp + r * DP_RAW_DW + (sb >> 2);
      const uint32_t sh = (uint32_t)(sb & 3);
      const uint32_t d0 = rowd[0], d1 = rowd[1], d2 = rowd[2], d3 = rowd[3], d4 = rowd[4];
      const uint32_t q0 = __builtin_amdgcn_alignbyte(d1, d0, sh), q1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
      const uint32_t q2 = __builtin_amdgcn_alignbyte(d3, d2, sh), q3 = __builtin_amdgcn_alignbyte(d4, d3, sh);
      const uint4 W = angW, Km = angK;
      const uint32_t a10 = __builtin_amdgcn_udot4(q0, W.x, __builtin_amdgcn_udot4(q1, W.y, __builtin_amdgcn_udot4(q2, W.z, __builtin_amdgcn_udot4(q3, W.w, 0u, false), false), false), false);
      const uint32_t rs = __builtin_amdgcn_udot4(q0, Km.x, __builtin_amdgcn_udot4(q1, Km.y, __builtin_amdgcn_udot4(q2, Km.z, __builtin_amdgcn_udot4(q3, Km.w, 0u, false), false), false), false);
      m10 = half ? (int)a10 : -(int)a10;
      m01 = __mul24(r - 15, (int)rs);
    }
    m10 = fb::wave_sum(m10);
    m01 = fb::wave_sum(m01);
    if (K.dbg == 12) { if (m10 + m01 == 12345678 && (int)(pq.x + pq.w) == 77777) nOut[0] = 1; continue; }
    const float angle = fb_fast_atan2((float)m01, (float)m10);
    // computeOrbDescriptor (ORBextractor.cc:107-147): lane computes tests 4*lane .. 4*lane+3
    const float factorPI = 0x1.1df46ap-6f;
    float sa, ca;
    fb_sincos_f(angle * factorPI, &sa, &ca);
    const float a = ca, bb = sa;
    const uint8_t *centre = reinterpret_cast<const uint8_t *>(blp) + 18 * (DP_BL_DW * 4) + cur.box + 18;
    int nib = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const uint32_t p = t == 0 ? pq.x : t == 1 ? pq.y : t == 2 ? pq.z : pq.w;
      const float x0 = (float)(p & 0xFFu) - (float)PAT_BIAS, y0 = (float)((p >> 8) & 0xFFu) - (float)PAT_BIAS;
      const float x1 = (float)((p >> 16) & 0xFFu) - (float)PAT_BIAS, y1 = (float)(p >> 24) - (float)PAT_BIAS;
      const int t0 = centre[__mul24(fb_cvround(x0 * bb + y0 * a), DP_BL_DW * 4) + fb_cvround(x0 * a - y0 * bb)];
      const int t1 = centre[__mul24(fb_cvround(x1 * bb + y1 * a), DP_BL_DW * 4) + fb_cvround(x1 * a - y1 * bb)];
      nib |= (t0 < t1) << t;
    }
    // lane 2j holds the low nibble of descriptor byte j, lane 2j+1 the high nibble; lanes 8j assemble dword j
    const int hi = __shfl_down(nib, 1, 64);
    const int byteVal = nib | (hi << 4);
    const int b1 = __shfl_down(byteVal, 2, 64), b2 = __shfl_down(byteVal, 4, 64), b3 = __shfl_down(byteVal, 6, 64);
    const uint32_t dw = (uint32_t)byteVal | ((uint32_t)b1 << 8) | ((uint32_t)b2 << 16) | ((uint32_t)b3 << 24);
    const long long o = (long long)b * K.kpStride + first + j;
    if ((lane & 7) == 0) reinterpret_cast<uint32_t *>(desc + o * 32)[lane >> 3] = dw;
    if (lane == 0) {
      fb_keypoint kp;
      kp.x = (float)cur.cx;
      kp.y = (float)cur.cy;
      if (l != 0) { kp.x *= lvScale; kp.y *= lvScale; }  // ORBextractor.cc:1095-1101
      kp.size = (float)lvPatch;
      kp.angle = angle;
      kp.response = (float)cur.resp;
      kp.octave = l;
      kps[o] = kp;
    }
    // the LDS reads of this key point are ordered before the writes of the next one (same wave, in-order LDS)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace
