// orb_fast.inc -- the FAST cell loop of ComputeKeyPointsOctTree: k_fast (included by orb.hip; its LDS carve and grid bases
// are planned in orb_plan.h).

namespace {

// ------------------------------------------------------------------------------------------
// FAST-9-16 score = max over the 16 arcs of 9 of min(d) (and of min(-d)), minus 1
// (cv::cornerScore<16>); the pixel is a corner at threshold t iff score >= t.
// ------------------------------------------------------------------------------------------
// `corner` points 3 rows above and 3 columns left of the pixel: every tap is corner + a non-negative constant, i.e. one LDS
// read with an immediate offset (taps at negative offsets from the pixel cost a vector add each).
template <int TP>
__device__ __forceinline__ int fast_score16(const uint8_t *__restrict__ corner) {
  const uint8_t *c = corner + 3 * TP + 3;
  const int v = c[0];
  int d[16];
#pragma unroll
  for (int i = 0; i < 16; i++) d[i] = fbscore::IntOps::sub(v, c[fbscore::ring_offset(i, TP)]);
  return fbscore::score_network<fbscore::IntOps>(d);  // already clamped at 0
}

// min3 / max3 of the packed form of fb_fast_score.h: the three-operand packed binary16 instructions of gfx950 (no packed
// INTEGER min3 / max3 exists: two pixels in v_pk_min_i16 form cost what two scalar trips cost).
struct PkF16MinMax {
  static __device__ __forceinline__ uint32_t min3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
  }
  static __device__ __forceinline__ uint32_t max3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
  }
};

// Scores of TWO pixels (corners c0 and c1, as for fast_score16): byte 0 of the result is the clamped score of the
// first, byte 2 that of the second, bytes 1 and 3 are zero.  Per ring position: two LDS byte reads, one v_lshl_or_b32
// to pair them and one v_pk_sub_u16 (the d16 forms of the LDS byte loads, which would pair for free, clear the other
// half on this ECC part).
template <int TP>
__device__ __forceinline__ uint32_t fast_score16x2(const uint8_t *__restrict__ c0, const uint8_t *__restrict__ c1) {
  typedef fbscore::PackedOps<PkF16MinMax> Ops;
  constexpr int ctr = 3 * TP + 3;
  const uint32_t v = fbscore::pk_centre(c0[ctr], c1[ctr]);
  uint32_t d[16];
#pragma unroll
  for (int i = 0; i < 16; i++) d[i] = Ops::sub(v, fbscore::pk_pair(c0[ctr + fbscore::ring_offset(i, TP)], c1[ctr + fbscore::ring_offset(i, TP)]));
  return fbscore::score_network<Ops>(d);
}

// inclusive scan over the 64 lanes in the VALU (DPP row shifts, then the row broadcasts of gfx9)
__device__ __forceinline__ int wave_incl_scan_dpp(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);  // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1 and 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2 and 3
  return v;
}


// One WAVE per run of FAST_CPW consecutive cells (64-thread workgroups, no cross-wave barriers, up to 31 waves per CU).
// Per cell:
//  1. the cell window is staged in LDS with 4-byte loads, all issued before the first LDS write; the window of the
//     NEXT cell is requested before this one is processed;
//  2. per 128 pixels: a necessary corner test on the 4 compass pixels (any 9-arc holds two consecutive compass
//     points), two pixels per lane in packed 16-bit arithmetic, ballot-compaction of the survivors into an
//     iniThFAST list and a minThFAST list; full score only for listed pixels;
//  3. 3x3 strict NMS over the thresholded score tile, survivors staged in LDS (over the image tile);
//  4. if none survived at iniThFAST the cell is redone at minThFAST (ORBextractor.cc:809-816);
//  5. the survivors go to the cell's own run of output slots + a per-cell count (no atomics; k_octree packs the runs).
//     Candidate order is irrelevant downstream (the quadtree breaks response ties with an order key derived from x,y).
// TP = tile pitch in bytes, a compile-time constant so that every LDS access of the sweep / score / NMS is
// base + immediate offset (44 covers cells up to 35 px wide, i.e. every level of the usual image sizes).
#ifndef FB_FAST_PACK_MIN
#define FB_FAST_PACK_MIN 64  // list entries left from which a score trip runs in the packed two-per-lane form (0: always; 1 << 30: never)
#endif
#ifndef FB_FAST_WPE44
#define FB_FAST_WPE44 6  // register budget of the 44-byte instantiation, in waves per SIMD
#endif
template <int TP, bool TIMED>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(TP == 44 ? FB_FAST_WPE44 : 4, 8))) void k_fast(OrbK K, const uint8_t *__restrict__ img0, long long imgStride, int pitch0,
                                             const uint8_t *__restrict__ pyr, uint32_t *__restrict__ cand,
                                             int *__restrict__ cellCount) {
  // LDS carve (sized on the host for the largest cell of this image size): tile (later: survivors) | sc | list
  extern __shared__ __attribute__((aligned(16))) uint8_t fsm[];
  uint8_t *tile = fsm;
  uint8_t *sc = fsm + K.fastTileBytes;
  // the NMS survivors overlay the image tile: the first survivor is written only after the last read of the tile
  // (a pass that keeps anything is the final pass; 4 * fastMaxOut <= fastTileBytes)
  uint32_t *s_out = reinterpret_cast<uint32_t *>(fsm);
  unsigned short *s_list = reinterpret_cast<unsigned short *>(fsm + 2 * K.fastTileBytes);  // [fastMaxPix]
  const int b = blockIdx.y, lane = threadIdx.x;
  // FB_FAST_DBG=20: one workgroup in 16 accumulates its phase times in registers and adds them once, at the end
  const bool timed = TIMED && (blockIdx.x & 15) == 0;  // the TIMED instantiation is launched for FB_FAST_DBG=20 only
  uint32_t t_mark = 0, t_acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // shader clock, low 32 bits
  if (timed) { __builtin_amdgcn_sched_barrier(0); t_mark = (uint32_t)__builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); }
  const uint32_t t_start = t_mark;
#define FAST_TICK(slot_) if (TIMED && timed) { __builtin_amdgcn_sched_barrier(0); const uint32_t t_ = (uint32_t)__builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); t_acc[slot_] += t_ - t_mark; t_mark = t_; }
  // XCD-aware mapping: workgroups are dealt round-robin over the 8 XCDs (blocks b and b+8 share one), so give each
  // XCD a contiguous run of cell groups -- neighbouring cells overlap by 6 px and share lines in that XCD's L2
  int grp, l = 0;
  {
    const int nb = gridDim.x, per = (nb + 7) >> 3;
    grp = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (grp >= K.totalGroups) return;  // grid is padded to a multiple of 8
  }
#pragma unroll
  for (int i = 1; i < FB_MAX_LEVELS; i++) l += (i < K.nlevels && grp >= K.grpBase[i]) ? 1 : 0;
  const LevelInfo &Lv = K.L[l];
  const int cFirst = (grp - K.grpBase[l]) * FAST_CPW, cEnd = min(cFirst + FAST_CPW, Lv.nCols * Lv.nRows);
  const int maxBX = Lv.w - BORDER, maxBY = Lv.h - BORDER;
  const uint8_t *img;
  int pitch;
  if (l == 0) { img = img0 + (long long)b * imgStride; pitch = pitch0; }
  else { img = pyr + (long long)b * K.pyrStride + Lv.off; pitch = Lv.pitch; }
  // the window is staged with tile column 0 = image column xa (4-byte aligned when the image allows it)
  const bool aligned = ((reinterpret_cast<uintptr_t>(img) | (uintptr_t)pitch) & 3) == 0;
  constexpr int tp = TP;  // tile pitch
  // fixed lane -> (row within a group, dword) mapping: the global offsets and the LDS indices are constants per lane.
  // ALL loads of a tile are issued together (rows past the window are clamped, their data is dropped): a load -> wait
  // -> write loop serialises one memory latency per RPI rows.
  constexpr int DW = TP / 4, RPI = 64 / DW;  // dwords per tile row, rows per iteration
  constexpr int NIT1 = (40 + RPI - 1) / RPI, NIT2 = (FAST_MAX_TILE + RPI - 1) / RPI - NIT1;  // usual windows: <= 40 rows
  const int r0 = lane / DW, dwc = lane - r0 * DW;
  struct Geo { int x0, y0, x1, y1, cw, ch, xa, ox, wpr; bool ok; };  // wave-uniform
  auto geo = [&](int ci, int cj) {  // cell (row ci, column cj) of the level
    Geo g;
    g.x0 = BORDER + cj * Lv.wCell; g.y0 = BORDER + ci * Lv.hCell;
    g.x1 = min(g.x0 + Lv.wCell + 6, maxBX); g.y1 = min(g.y0 + Lv.hCell + 6, maxBY);
    g.cw = g.x1 - g.x0; g.ch = g.y1 - g.y0;
    g.ok = !(g.y0 >= maxBY - 3 || g.x0 >= maxBX - 6) && g.cw >= 7 && g.ch >= 7;  // ORBextractor.cc:794,802
    g.xa = aligned ? (g.x0 & ~3) : g.x0;
    g.ox = g.x0 - g.xa;
    g.wpr = ((g.x1 - g.xa) + 3) >> 2;  // dwords per window row (<= DW)
    return g;
  };
  uint32_t v[NIT1];
  auto issue = [&](const Geo &g) {  // the first NIT1 * RPI rows of the window -> registers
    if (r0 < RPI && dwc < g.wpr) {
      const uint8_t *src = img + (long long)g.y0 * pitch + g.xa;  // wave-uniform base + 32-bit lane offsets
      const uint32_t lo = (uint32_t)dwc * 4u;
      int r0v = r0;
      asm volatile("" : "+v"(r0v));  // keeps the NIT1 row numbers from being hoisted out of the cell loop into NIT1 registers
#pragma unroll
      for (int it = 0; it < NIT1; it++)
        v[it] = *reinterpret_cast<const uint32_t *>(src + ((uint32_t)__mul24(min(r0v + it * RPI, g.ch - 1), pitch) + lo));
    }
  };
  auto stage = [&](const Geo &g) {  // registers (+ the rows of a tall window) -> LDS tile, score tile cleared
    if (aligned) {
      if (r0 < RPI && dwc < g.wpr) {
        uint32_t *dst = reinterpret_cast<uint32_t *>(&tile[dwc * 4]);
#pragma unroll
        for (int it = 0; it < NIT1; it++) dst[(r0 + it * RPI) * DW] = v[it];  // rows >= ch: copies of the last row, masked later
        // (NIT1 * RPI rows always fit tile + score tile -- the host sizes fastTileBytes for it -- and the score tile is cleared
        // below, after these writes; unconditional stores also let the compiler count the loads it has consumed)
        if (g.ch > NIT1 * RPI) {  // tall cells of small levels
          const uint8_t *src = img + (long long)g.y0 * pitch + g.xa;
          int r0t = r0, dwct = dwc;
          asm volatile("" : "+v"(r0t), "+v"(dwct));  // nothing of this rare path is precomputed (and spilled) outside the cell loop
          const uint32_t lo = (uint32_t)dwct * 4u;
          uint32_t w[NIT2];
#pragma unroll
          for (int it = 0; it < NIT2; it++) w[it] = *reinterpret_cast<const uint32_t *>(src + ((uint32_t)__mul24(min(r0t + (NIT1 + it) * RPI, g.ch - 1), pitch) + lo));
          uint32_t *dstt = reinterpret_cast<uint32_t *>(&tile[dwct * 4]);
#pragma unroll
          for (int it = 0; it < NIT2; it++)
            if (r0t + (NIT1 + it) * RPI < g.ch) dstt[(r0t + (NIT1 + it) * RPI) * DW] = w[it];
        }
      }
    } else {
      for (int i = lane; i < g.cw * g.ch; i += 64) {
        const int yy = i / g.cw, xx = i - yy * g.cw;
        tile[yy * tp + xx] = img[(long long)(g.y0 + yy) * pitch + g.x0 + xx];
      }
    }
    {  // score tile <- 0, 16 bytes per lane and store (the tile sizes are multiples of 16, the carve is 16-byte aligned)
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
      const u32x4 z = {0u, 0u, 0u, 0u};
      const int n16 = (tp * g.ch + 15) / 16;
      if (lane < n16) reinterpret_cast<u32x4 *>(sc)[lane] = z;  // the usual 44 x <= 46 bytes: two stores, no loop
      if (lane + 64 < n16) reinterpret_cast<u32x4 *>(sc)[lane + 64] = z;
      if (n16 > 128)
        for (int i = lane + 128; i < n16; i += 64) reinterpret_cast<u32x4 *>(sc)[i] = z;
    }
    __syncthreads();
  };
  uint32_t validKept = 0u;  // the sweep's valid-pixel mask of the last cell size seen (process)
  int validKey = -1;
  auto process = [&](const Geo &g, int cell) {
    const int x0 = g.x0, y0 = g.y0, cw = g.cw, ch = g.ch, ox = g.ox;
    if (K.dbg == 1) { if (tile[lane] == 255 && sc[lane] == 7) cand[0] = 1; return; }
    const int dwid = cw - 6, dhei = ch - 6, npix = dwid * dhei;
    // ---- ONE sweep over the cell: every pixel that can be a corner (necessary compass test) becomes a bit of a
    //      per-lane mask, one mask for iniThFAST (A) and one for minThFAST only (B); the A masks are expanded into a
    //      list of tile offsets (front of s_list), the B masks only if the cell has to be redone at minThFAST (back of
    //      s_list, growing down).  No cross-lane work and no scalar bookkeeping inside the sweep.
    const int cap = K.fastMaxPix;
    // Lanes map to (row-pair, column): 32 columns x 2 row pairs per iteration for the usual <= 32 px wide cells, 64 x 1
    // otherwise, so the LDS offset advances by a constant and no index division is needed.  A lane tests TWO vertically
    // adjacent pixels at once in packed 16-bit arithmetic.  With the compass pixels n0 (below), n4 (right), n8 (above),
    // n12 (left) of centre v, "two ADJACENT compass points brighter than v + T" is "one of {n0, n8} AND one of {n4, n12}"
    // (every such pair is adjacent), i.e. v + T < B with B = min(max(n0, n8), max(n4, n12)); likewise two darker ones are
    // v - T > A with A = max(min(n0, n8), min(n4, n12)).  strength = max(v - A, B - v) > T is the test for ANY threshold:
    // 9 packed operations for two pixels; the sign bits of T - strength shift into the masks (3 operations per threshold).
    (void)npix;
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    typedef short s16x2 __attribute__((ext_vector_type(2)));
    typedef __attribute__((address_space(3))) unsigned short lds_u16;
    const bool two = dwid <= 32;  // two row pairs per iteration
    const int G = two ? 32 : 64, ppi = two ? 2 : 1;
    const int sxx = lane & (G - 1);
    const bool hiHalf = two && lane >= 32, colok = sxx < dwid;
    const int tp3 = 3 * tp, sstep = __builtin_amdgcn_readfirstlane(2 * ppi * tp);  // scalar: products with it stay off the quarter-rate 32-bit vector multiply
    const int rLane = hiHalf ? 2 : 0;                        // first row of the lane
    const int off = (3 + rLane) * tp + ox + 3 + sxx;         // its upper pixel
    const uint32_t listBase = (uint32_t)(uintptr_t)s_list;  // LDS byte address
    uint32_t baseA = listBase, baseB = listBase + 2u * (uint32_t)(cap - 1);  // next free slot: A grows up, B down
    const u16x2 iniV = {(unsigned short)K.iniTh, (unsigned short)K.iniTh}, minV = {(unsigned short)K.minTh, (unsigned short)K.minTh};
    constexpr int Cc = 3 * TP + 3;  // the centre (upper pixel of the pair) seen from the lane's lowest tap
    // a mask word: bit p of the low half = upper pixel of chunk iteration p - (16 - n), high half = lower pixel
    auto expand = [&](uint32_t W, uint32_t &base, const bool up, int cj) {
      const int cnt = __popc(W);
      const int incl = wave_incl_scan_dpp(cnt);
      const int total = __builtin_amdgcn_readlane(incl, 63);
      if (total == 0) return;  // wave-uniform
      const uint32_t e = 2u * (uint32_t)(incl - cnt);
      uint32_t a = up ? base + e : base - e;
      while (W != 0u) {  // one listed pixel per lane and trip
        const int bpos = __builtin_ctz(W);
        W &= W - 1u;
        // bit p of the low half = iteration p (rows advance by sstep), high half = the lower pixel of the pair (+ tp):
        // cj + (p & 15) * sstep + (p >> 4) * tp as two multiply-adds
        int offp;  // (in assembly: the compiler turns the 24-bit products into quarter-rate 32-bit multiplies here)
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(offp) : "v"(bpos), "s"(sstep), "v"(cj));
        asm("v_mad_i32_i24 %0, %1, %2, %0" : "+v"(offp) : "v"(bpos >> 4), "s"(__builtin_amdgcn_readfirstlane(tp - 16 * sstep)));
        *reinterpret_cast<lds_u16 *>((uintptr_t)a) = (unsigned short)offp;
        a = up ? a + 2u : a - 2u;
      }
      base = up ? base + 2u * (uint32_t)total : base - 2u * (uint32_t)total;
    };
    // all ten taps at non-negative constant distances from the lane's lowest tap (3 rows up, 3 columns left is the
    // corner of that box), so that every LDS read is base + immediate
    typedef __attribute__((address_space(3))) const uint8_t lds_cu8;
    const uint32_t tileAddr = (uint32_t)(uintptr_t)tile;
    uint32_t lo = tileAddr + (uint32_t)(off - tp3 - 3);  // LDS byte address of the lane's lowest tap
    const int nIt = __builtin_amdgcn_readfirstlane((dhei + 2 * ppi - 1) >> ppi);  // 2 * ppi = 1 << ppi rows per iteration
    uint32_t WB[2] = {0u, 0u};  // the minThFAST-only masks of the (at most two) chunks of 16 iterations
    for (int it0 = 0, ck = 0; it0 < nIt; it0 += 16, ck++) {
      const int n = __builtin_amdgcn_readfirstlane(min(16, nIt - it0));
      uint32_t accA = 0u, accB = 0u;
      const int cj = (int)(lo - tileAddr) + Cc - (16 - n) * sstep;  // tile offset of bit 0
      for (int j = 0; j < n; j++, lo += (uint32_t)sstep) {
        // rows beyond the cell read inside the LDS tile + score tile; their bits are masked below
        asm volatile("" : "+v"(lo));
        lds_cu8 *c = reinterpret_cast<lds_cu8 *>((uintptr_t)lo);
        const uint32_t b0 = c[Cc], b1 = c[Cc + TP], b2 = c[Cc + 3 * TP], b3 = c[Cc + 4 * TP], b4 = c[Cc - 3 * TP], b5 = c[Cc - 2 * TP];
        const uint32_t b6 = c[Cc + 3], b7 = c[Cc + TP + 3], b8 = c[Cc - 3], b9 = c[Cc + TP - 3];
        __builtin_amdgcn_sched_group_barrier(0x100, 10, 0);  // the ten LDS reads back to back, then the arithmetic
        auto pair = [&](uint32_t x, uint32_t yv) { return __builtin_bit_cast(u16x2, x | (yv << 16)); };
        const u16x2 v = pair(b0, b1), n0 = pair(b2, b3), n8 = pair(b4, b5), n4 = pair(b6, b7), n12 = pair(b8, b9);
  #define PMIN(a, b) __builtin_elementwise_min(a, b)
  #define PMAX(a, b) __builtin_elementwise_max(a, b)
        const u16x2 A = PMAX(PMIN(n0, n8), PMIN(n4, n12)), Bv = PMIN(PMAX(n0, n8), PMAX(n4, n12));
        const s16x2 st = PMAX(__builtin_bit_cast(s16x2, (u16x2)(v - A)), __builtin_bit_cast(s16x2, (u16x2)(Bv - v)));
  #undef PMIN
  #undef PMAX
        const u16x2 stu = __builtin_bit_cast(u16x2, st);
        const uint32_t sA = __builtin_bit_cast(uint32_t, (u16x2)(iniV - stu)), sB = __builtin_bit_cast(uint32_t, (u16x2)(minV - stu));
        accA = (accA >> 1) | (sA & 0x80008000u);  // T - strength < 0  <=>  strength > T
        accB = (accB >> 1) | (sB & 0x80008000u);
      }
      // valid bits of this lane: its column inside the cell, its rows inside the cell (kept from the previous cell of the
      // wave when that had the same size, i.e. nearly always)
      uint32_t valid;
      const int key = (dwid << 8) | dhei;
      if (it0 == 0 && key == validKey) {
        valid = validKept;
      } else {
        const int avail = dhei - (it0 * 2 * ppi + rLane);  // rows from the lane's first upper pixel of the chunk to the cell's end
        const int nU = min(max((avail + 2 * ppi - 1) >> ppi, 0), n), nL = min(max((avail + 2 * ppi - 2) >> ppi, 0), n);
        const uint32_t sh = (uint32_t)(16 - n);
        valid = colok ? ((((1u << nU) - 1u) << sh) | (((1u << nL) - 1u) << (sh + 16u))) : 0u;
        if (it0 == 0) { validKept = valid; validKey = key; }
      }
      accA &= valid;
      WB[ck] = accB & valid & ~accA;
      expand(accA, baseA, true, cj);
    }
    const int nlA = (int)((baseA - listBase) >> 1);
    int nlB = 0;
#ifdef FB_FAST_LISTHIST  // probe build: list lengths in 64 bins of 8 (bin k: 8k-7 .. 8k entries, bin 0: empty list)
    if (lane == 0) atomicAdd(&K.timers[16 + min((nlA + 7) >> 3, 63)], 1ull);
#endif
    __syncthreads();
    FAST_TICK(2)  // sweep
      if (K.dbg == 4) { if (nlA + (int)WB[0] == 123456) cand[0] = 1; return; }
    for (int pass = 0; pass < 2; pass++) {
      const int T = pass == 0 ? K.iniTh : K.minTh;
      // ---- scores, stored RAW (the score does not depend on the threshold; clamped at 0): pass 0 scores list A, pass 1
      //      (cells without a corner at iniThFAST) only list B.  The NMS asks "score >= T" of the centre only: a neighbour
      //      below T loses against the centre whether it is stored raw or as the 0 cv::FAST keeps for non-corners, and
      //      a pixel in neither list (score < minThFAST) holds 0
      if (pass == 1) {  // the cell is redone at minThFAST: now its B masks become the B list
        // tile offset of bit 0 of a chunk (as in the sweep): the lane's first tap + the centre - (16 - n) iterations
        const int lo0 = off - tp3 - 3 + Cc;
        expand(WB[0], baseB, false, lo0 - (16 - min(16, nIt)) * sstep);
        if (nIt > 16) expand(WB[1], baseB, false, lo0 + 16 * sstep - (16 - min(16, nIt - 16)) * sstep);
        nlB = (int)((listBase + 2u * (uint32_t)(cap - 1) - baseB) >> 1);
#ifdef FB_FAST_LISTHIST
        if (lane == 0) atomicAdd(&K.timers[16 + 64 + min((nlB + 7) >> 3, 63)], 1ull);  // cells redone at minThFAST
#endif
        __syncthreads();
      }
      const int nl = pass == 0 ? nlA : nlA + nlB;  // the NMS of pass 1 visits A then B
      auto listed = [&](int i) { return (int)(i < nlA ? s_list[i] : s_list[cap - nlB + (i - nlA)]); };
      for (int base = pass == 0 ? 0 : nlA; base < nl;) {
        const int i = base + lane;
        if (nl - base > FB_FAST_PACK_MIN) {  // wave-uniform: lane i scores entries i and i + 64 of a 128-entry trip
          if (i < nl) {
            const int o0 = listed(i);
            const int o1 = i + 64 < nl ? listed(i + 64) : o0;  // absent second half: the first pixel again (reads stay inside the carve)
            int oc0 = o0 - 3 * TP - 3, oc1 = o1 - 3 * TP - 3;
            asm volatile("" : "+v"(oc0), "+v"(oc1));  // keeps the compiler from re-basing the taps on the pixels
            const uint32_t r = fast_score16x2<TP>(&tile[oc0], &tile[oc1]);
            sc[o0] = (uint8_t)r;
            sc[o1] = (uint8_t)(r >> 16);  // o1 == o0: the same byte again
          }
          base += 128;
        } else {
          if (i < nl) {
            const int o = listed(i);
            int oc = o - 3 * TP - 3;
            asm volatile("" : "+v"(oc));  // keeps the compiler from re-basing the taps on the pixel
            sc[o] = (uint8_t)fast_score16<TP>(&tile[oc]);
          }
          base += 64;
        }
      }
      const int Tk = max(T, 1);  // a corner has score >= T and score != 0
      __syncthreads();
      if (pass == 0) { FAST_TICK(3) } else { FAST_TICK(6) }  // score
      if (K.dbg == 2) { if (sc[lane] == 255) cand[0] = 1; return; }
      // ---- 3x3 strict non-max suppression over the candidate list (only listed pixels can hold a score >= T);
      //      the rim holds 0
      int total = 0;
      for (int base = 0; base < nl; base += 64) {
        const int i = base + lane;
        bool keep = false;
        uint32_t rec = 0;
        if (i < nl) {
          const int o = i < nlA ? s_list[i] : s_list[cap - nlB + (i - nlA)];
          int oq = o - TP - 1;  // the upper left neighbour: all nine reads at immediate offsets
          asm volatile("" : "+v"(oq));
          const uint8_t *q = &sc[oq] + TP + 1;
          const int sv = q[0];
          if (sv >= Tk) {
            const int mx = max(max(max(max((int)q[-1], (int)q[1]), (int)q[-tp - 1]), max((int)q[-tp], (int)q[-tp + 1])),
                               max(max((int)q[tp - 1], (int)q[tp]), (int)q[tp + 1]));
            keep = sv > mx;
            const int yy = o / tp, xx = o - yy * tp - ox;
            rec = (uint32_t)(x0 + xx) | ((uint32_t)(y0 + yy) << 12) | ((uint32_t)sv << 24);
          }
        }
        const unsigned long long m = __ballot(keep);
        if (keep) s_out[total + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = rec;
        total += __popcll(m);
      }
      if (pass == 0) { FAST_TICK(4) } else { FAST_TICK(7) }  // NMS
      if (K.dbg == 3) { if (total == 12345) cand[0] = 1; return; }
      if (total == 0) continue;  // wave-uniform: retry with minThFAST
      __syncthreads();
      // Every cell owns a fixed run of slotCap candidate slots and a count (pre-zeroed by the host); k_octree packs the
      // runs of a level.  (One returning atomic per cell on a per-level counter was a third of a wave's life time: the
      // ~900 cells of a level queue up on one address.)
      uint32_t *out = cand + (long long)b * K.candStride + Lv.candBase + (long long)cell * Lv.slotCap;
#pragma unroll 1
      for (int i = lane; i < total; i += 64) out[i] = s_out[i];
      if (lane == 0) cellCount[(long long)b * K.totalCells + Lv.cellBase + cell] = total;
      if (pass == 0) { FAST_TICK(5) } else { FAST_TICK(8) }  // emission
      break;
    }
  };
  // the one division of the wave (its quotient comes out of the vector ALU: readfirstlane keeps what follows scalar)
  int ci = __builtin_amdgcn_readfirstlane(cFirst / Lv.nCols), cj = cFirst - ci * Lv.nCols;
  Geo g = geo(ci, cj);
  if (timed) { if (g.cw + g.ch + g.x0 + g.y0 == 123456789) cand[0] = 1; }  // forces the kernel-argument loads to have landed
  FAST_TICK(9)  // group decode (scalar loads of the level tables)
  if (g.ok && aligned) issue(g);
  for (int cell = cFirst; cell < cEnd; cell++) {
    const bool haveNext = cell + 1 < cEnd;
    if (haveNext) { cj++; if (cj == Lv.nCols) { cj = 0; ci++; } }
    const Geo gn = geo(ci, cj);
    if (g.ok) {
      stage(g);
      if (timed) { if (tile[lane] == 255 && sc[lane] == 7) cand[0] = 1; }  // forces the wait for the staged tile
      FAST_TICK(0)  // wait for the tile + LDS writes
      // Nothing is outstanding here (the tile has landed), but the compiler cannot see that for the lanes that skipped a
      // row: without this explicit vmcnt(0) it protects their registers with vmcnt(0) waits AFTER the prefetch below,
      // i.e. the wave would sit out the next tile's latency before it starts on this one.
      __builtin_amdgcn_s_waitcnt(0x0F70);
      if (haveNext && gn.ok && aligned) issue(gn);  // in flight while this cell is processed
      FAST_TICK(1)  // prefetch issue
      process(g, cell);
      __syncthreads();  // the next tile overwrites the survivors / lists
    } else if (haveNext && gn.ok && aligned) {
      issue(gn);
    }
    g = gn;
  }
  if (TIMED && timed && lane == 0) {
#pragma unroll
    for (int i = 0; i < 10; i++) atomicAdd(&K.timers[i], (unsigned long long)t_acc[i]);
    atomicAdd(&K.timers[10], (unsigned long long)(t_mark - t_start));
    atomicAdd(&K.timers[11], 1ull);
  }
#undef FAST_TICK
}

}  // namespace
