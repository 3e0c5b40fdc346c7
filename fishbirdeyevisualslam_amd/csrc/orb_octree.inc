// orb_octree.inc -- DistributeOctTree: k_octree, one workgroup per image level (included by orb.hip; ONode and the LDS size
// are in orb_plan.h).

namespace {

// ------------------------------------------------------------------------------------------
// DistributeOctTree.  The std::list of the reference is an ordered array here: every node is
// pushed to the FRONT when created, so list order == descending creation order (initial nodes
// last), which is also the "pointer" order used to break ties in the (size,pointer) sort
// (modelled as creation sequence in the oracle).  Each round: count keypoints per child
// quadrant (LDS atomics), rebuild the list with block scans, remap the keypoints.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int quadrant(const ONode &n, int rx, int ry) {
  const int halfX = (int)ceilf((float)(n.x1 - n.x0) / 2), halfY = (int)ceilf((float)(n.y1 - n.y0) / 2);
  const int mx = n.x0 + halfX, my = n.y0 + halfY;
  return (rx < mx ? 0 : 1) + (ry < my ? 0 : 2);  // n1=0 (UL), n2=1 (UR), n3=2 (BL), n4=3 (BR)
}

__device__ __forceinline__ ONode child_of(const ONode &n, int q, int cnt) {
  const int halfX = (int)ceilf((float)(n.x1 - n.x0) / 2), halfY = (int)ceilf((float)(n.y1 - n.y0) / 2);
  const int mx = n.x0 + halfX, my = n.y0 + halfY;
  ONode c;
  c.x0 = (q & 1) ? mx : n.x0;
  c.x1 = (q & 1) ? n.x1 : mx;
  c.y0 = (q & 2) ? my : n.y0;
  c.y1 = (q & 2) ? n.y1 : my;
  c.cnt = cnt;
  return c;
}

// NT threads: 256 when many (image, level) workgroups share the GPU, 1024 for a small batch, where the workgroup of level 0
// (tens of thousands of candidates, ~10 rounds of three passes over them) is the latency of the whole front chain.
template <int NT>
__global__ __launch_bounds__(NT) void k_octree(OrbK K, const uint32_t *__restrict__ cellCand, const int *__restrict__ cellCount,
                                                uint32_t *__restrict__ cand, int *__restrict__ candCount, uint16_t *__restrict__ nodeOf,
                                                uint32_t *__restrict__ lvlOut, int *__restrict__ lvlCount, int maxNodes) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  // level-major grid: the workgroups of level 0, the longest by far, are dispatched first and the short ones fill in behind
  const int l = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
  const LevelInfo &Lv = K.L[l];
  const int M = maxNodes;
  ONode *listA = reinterpret_cast<ONode *>(smem);        // [M]
  ONode *listB = listA + M;                              // [M]
  int *ccnt = reinterpret_cast<int *>(listB + M);        // [M][4] child counts
  unsigned short *cpos = reinterpret_cast<unsigned short *>(ccnt + 4 * M);  // [M][4] new position of child
  unsigned short *npos = cpos + 4 * M;                   // [M] new position of a surviving node
  unsigned short *order = npos + M;                      // [M] final phase: rank -> position
  unsigned char *split = reinterpret_cast<unsigned char *>(order + M);  // [M] node is split this round
  unsigned long long *best = reinterpret_cast<unsigned long long *>(smem + (((size_t)(split + M - smem)) + 7 & ~(size_t)7));
  __shared__ int s_w[NT / 64], s_S, s_nexp, s_jstar;
  // ---- pack the per-cell candidate runs of k_fast into one dense list (order is irrelevant downstream: the quadtree
  //      breaks response ties with an order key derived from x, y).  offs[] aliases the node lists, not yet in use.
  uint32_t *cdw = cand + (long long)b * K.candStride + Lv.candBase;
  int n;
  {
    int *offs = reinterpret_cast<int *>(smem);  // [ncell + 1]
    const int ncell = Lv.nCols * Lv.nRows;
    const int *cc = cellCount + (long long)b * K.totalCells + Lv.cellBase;
    const uint32_t *sp = cellCand + (long long)b * K.candStride + Lv.candBase;
    int run = 0;
    for (int c0 = 0; c0 < ncell; c0 += NT) {
      const int c = c0 + tid;
      const int v = c < ncell ? cc[c] : 0;
      int tot;
      const int ex = fb::block_excl_scan<NT>(v, s_w, &tot);
      if (c < ncell) offs[c] = run + ex;
      run += tot;
      __syncthreads();  // s_w is reused by the next chunk
    }
    n = run;
    if (tid == 0) { offs[ncell] = n; candCount[b * K.nlevels + l] = n; }
    __syncthreads();
    // dense index -> cell by binary search over the offsets; 4 independent copies per thread and step so that the
    // loads are in flight together
    for (int k0 = tid; k0 < n; k0 += NT * 4) {
      uint32_t val[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int k = min(k0 + u * NT, n - 1);
        int lo = 0, hi = ncell;  // offs[lo] <= k < offs[hi]
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (offs[mid] <= k) lo = mid; else hi = mid;
        }
        val[u] = sp[(long long)lo * Lv.slotCap + (k - offs[lo])];
      }
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (k0 + u * NT < n) cdw[k0 + u * NT] = val[u];
    }
    __threadfence_block();
    __syncthreads();  // the lists below overwrite offs[]; the dense list is read back by this block only
  }
  const uint32_t *cd = cdw;
  uint16_t *nof = nodeOf + (long long)b * K.candStride + Lv.candBase;
  int *outCount = lvlCount + b * K.nlevels + l;
  uint32_t *out = lvlOut + (long long)b * K.outStride + Lv.outBase;
  if (n == 0 || Lv.nIni < 1) { if (tid == 0) *outCount = 0; return; }
  const int N = Lv.N;
  const int Hh = Lv.h - 2 * BORDER;
  // ---- initial nodes (ORBextractor.cc:543-593)
  for (int i = tid; i < Lv.nIni; i += NT) {
    ONode nd;
    nd.x0 = (short)(int)(Lv.hX * (float)i);
    nd.x1 = (short)(int)(Lv.hX * (float)(i + 1));
    nd.y0 = 0; nd.y1 = (short)Hh; nd.cnt = 0;
    listB[i] = nd;
  }
  __syncthreads();
  for (int k = tid; k < n; k += NT) {
    const int rx = (int)(cd[k] & 0xFFF) - BORDER;
    int idx = (int)((float)rx / Lv.hX);
    idx = min(idx, Lv.nIni - 1);
    nof[k] = (uint16_t)idx;
    atomicAdd(&listB[idx].cnt, 1);
  }
  __syncthreads();
  if (tid == 0) {  // drop empty initial nodes, keep order
    int S = 0;
    for (int i = 0; i < Lv.nIni; i++) {
      npos[i] = (unsigned short)S;
      if (listB[i].cnt > 0) listA[S++] = listB[i];
    }
    s_S = S;
  }
  __syncthreads();
  for (int k = tid; k < n; k += NT) nof[k] = npos[nof[k]];
  __syncthreads();
  ONode *cur = listA, *nxt = listB;
  int S = s_S;
  bool finalPhase = false;
  for (int guard = 0; guard < 64; guard++) {
    const int prevSize = S;
    // ---- count children of every expandable node
    for (int i = tid; i < 4 * S; i += NT) ccnt[i] = 0;
    __syncthreads();
    // candidate passes: 4 candidates per thread and step, all their global loads requested before the first use
    for (int k0 = tid; k0 < n; k0 += NT * 4) {
      int pk[4];
      uint32_t ck[4];
#pragma unroll
      for (int u = 0; u < 4; u++) { const int kk = min(k0 + u * NT, n - 1); pk[u] = nof[kk]; ck[u] = cd[kk]; }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        if (k0 + u * NT >= n) break;
        const int p = pk[u];
        const ONode nd = cur[p];
        if (nd.cnt > 1) {
          const uint32_t c = ck[u];
          atomicAdd(&ccnt[4 * p + quadrant(nd, (int)(c & 0xFFF) - BORDER, (int)((c >> 12) & 0xFFF) - BORDER)], 1);
        }
      }
    }
    __syncthreads();
    // ---- choose the nodes to split
    if (!finalPhase) {
      for (int p = tid; p < S; p += NT) split[p] = cur[p].cnt > 1;
    } else {
      // sort expandable nodes by (count desc, list position asc) == (size, pointer) sort walked
      // from the back (ORBextractor.cc:684-686); split in that order until the list holds N
      for (int p = tid; p < S; p += NT) {
        split[p] = 0;
        const int c = cur[p].cnt;
        if (c > 1) {
          int rank = 0;
          for (int j = 0; j < S; j++) {
            const int cj = cur[j].cnt;
            if (cj > 1 && (cj > c || (cj == c && j < p))) rank++;
          }
          order[rank] = (unsigned short)p;
        }
      }
      __syncthreads();
      if (tid == 0) {
        int sz = S, j = 0;
        const int C = s_nexp;
        for (; j < C; j++) {
          const int p = order[j];
          const int kk = (ccnt[4 * p] > 0) + (ccnt[4 * p + 1] > 0) + (ccnt[4 * p + 2] > 0) + (ccnt[4 * p + 3] > 0);
          sz += kk - 1;
          split[p] = 1;
          if (sz >= N) { j++; break; }
        }
        s_jstar = j;  // number of nodes split
      }
    }
    __syncthreads();
    // ---- new list: children of split nodes go to the front, most recently created first
    // phase 1 : creation order = list order of parents, q = 0..3  -> position = reverse of it
    // final   : creation order = rank order of parents,  q = 0..3
    const int per = (S + NT - 1) / NT;
    const int a0 = min(tid * per, S), a1 = min(a0 + per, S);
    int myKids = 0, myKeep = 0;
    if (!finalPhase) {
      for (int p = a0; p < a1; p++) {
        if (split[p]) myKids += (ccnt[4 * p] > 0) + (ccnt[4 * p + 1] > 0) + (ccnt[4 * p + 2] > 0) + (ccnt[4 * p + 3] > 0);
        else myKeep++;
      }
    } else {
      const int J = s_jstar;
      const int perj = (J + NT - 1) / NT;
      const int r0 = min(tid * perj, J), r1 = min(r0 + perj, J);
      for (int r = r0; r < r1; r++) {
        const int p = order[r];
        myKids += (ccnt[4 * p] > 0) + (ccnt[4 * p + 1] > 0) + (ccnt[4 * p + 2] > 0) + (ccnt[4 * p + 3] > 0);
      }
      for (int p = a0; p < a1; p++) if (!split[p]) myKeep++;
    }
    int totalKids, totalKeep;
    const int kidsBefore = fb::block_excl_scan<NT>(myKids, s_w, &totalKids);
    const int keepBefore = fb::block_excl_scan<NT>(myKeep, s_w, &totalKeep);
    // children created before mine: kidsBefore -> my first child has creation index kidsBefore,
    // list position = totalKids-1-creationIndex
    {
      int ci = kidsBefore, kp = totalKids + keepBefore;
      if (!finalPhase) {
        for (int p = a0; p < a1; p++) {
          if (split[p]) {
            for (int q = 0; q < 4; q++)
              if (ccnt[4 * p + q] > 0) {
                const int pos = totalKids - 1 - ci++;
                cpos[4 * p + q] = (unsigned short)pos;
                nxt[pos] = child_of(cur[p], q, ccnt[4 * p + q]);
              }
          } else {
            npos[p] = (unsigned short)kp;
            nxt[kp++] = cur[p];
          }
        }
      } else {
        const int J = s_jstar;
        const int perj = (J + NT - 1) / NT;
        const int r0 = min(tid * perj, J), r1 = min(r0 + perj, J);
        for (int r = r0; r < r1; r++) {
          const int p = order[r];
          for (int q = 0; q < 4; q++)
            if (ccnt[4 * p + q] > 0) {
              const int pos = totalKids - 1 - ci++;
              cpos[4 * p + q] = (unsigned short)pos;
              nxt[pos] = child_of(cur[p], q, ccnt[4 * p + q]);
            }
        }
        for (int p = a0; p < a1; p++)
          if (!split[p]) { npos[p] = (unsigned short)kp; nxt[kp++] = cur[p]; }
      }
    }
    const int Snew = totalKids + totalKeep;
    __syncthreads();
    // ---- remap keypoints
    for (int k0 = tid; k0 < n; k0 += NT * 4) {
      int pk[4];
      uint32_t ck[4];
#pragma unroll
      for (int u = 0; u < 4; u++) { const int kk = min(k0 + u * NT, n - 1); pk[u] = nof[kk]; ck[u] = cd[kk]; }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int k = k0 + u * NT;
        if (k >= n) break;
        const int p = pk[u];
        if (split[p]) {
          const uint32_t c = ck[u];
          nof[k] = cpos[4 * p + quadrant(cur[p], (int)(c & 0xFFF) - BORDER, (int)((c >> 12) & 0xFFF) - BORDER)];
        } else nof[k] = npos[p];
      }
    }
    // nToExpand of the new list = children with more than one keypoint
    int myExp = 0;
    {
      const int pern = (Snew + NT - 1) / NT;
      const int n0 = min(tid * pern, Snew), n1 = min(n0 + pern, Snew);
      for (int p = n0; p < n1; p++) myExp += (p < totalKids && nxt[p].cnt > 1);
    }
    int nToExpand;
    fb::block_excl_scan<NT>(myExp, s_w, &nToExpand);
    if (tid == 0) s_nexp = nToExpand;
    __syncthreads();
    ONode *t = cur; cur = nxt; nxt = t;
    S = Snew;
    // ---- termination (ORBextractor.cc:669-739)
    if (S >= N || S == prevSize) break;
    if (!finalPhase) {
      if (S + nToExpand * 3 > N) finalPhase = true;
    }
  }
  // ---- best keypoint per node: max response, first in vToDistributeKeys order on ties
  for (int p = tid; p < S; p += NT) best[p] = 0ull;
  __syncthreads();
  for (int k0 = tid; k0 < n; k0 += NT * 4) {
    int pk[4];
    uint32_t ck[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { const int kk = min(k0 + u * NT, n - 1); pk[u] = nof[kk]; ck[u] = cd[kk]; }
#pragma unroll
    for (int u = 0; u < 4; u++) {
    const int k = k0 + u * NT;
    if (k >= n) break;
    const uint32_t c = ck[u];
    const int x = c & 0xFFF, y = (c >> 12) & 0xFFF, r = c >> 24;
    const int cellI = (y - EDGE_THRESHOLD) / Lv.hCell, cellJ = (x - EDGE_THRESHOLD) / Lv.wCell;
    const int dwid = min(Lv.wCell, Lv.w - 2 * EDGE_THRESHOLD - cellJ * Lv.wCell);
    const int inCell = (y - EDGE_THRESHOLD - cellI * Lv.hCell) * dwid + (x - EDGE_THRESHOLD - cellJ * Lv.wCell);
    const unsigned orderKey = (unsigned)(cellI * Lv.nCols + cellJ) * 4096u + (unsigned)inCell;  // < 2^32 (cells < 2^20)
    // response (8 bits) | inverted order key (32 bits) | candidate index (24 bits)
    const unsigned long long key = ((unsigned long long)r << 56) | ((unsigned long long)(0xFFFFFFFFu - orderKey) << 24) | (unsigned)k;
    atomicMax(&best[pk[u]], key);
    }
  }
  __syncthreads();
  for (int p = tid; p < S; p += NT) out[p] = cd[(unsigned)(best[p] & 0xFFFFFFull)];
  if (tid == 0) *outCount = S;
}

}  // namespace
