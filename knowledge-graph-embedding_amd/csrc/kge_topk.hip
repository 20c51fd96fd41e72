// Top-k link prediction for gfx950: for each query (h, r, ?) / (?, r, t) the k
// best-scoring entities that are not known positives, best first, ties by
// ascending entity id. The scoring is kge_rank's (kge_rank_impl.h: the same
// ops in the same order, so a returned score has the bits kge_rank writes for
// that entity as pos_score_out); this file adds the selection:
//
//   topk_lane_kernel   workgroup = a group of 8 (or, for wide rows / large k,
//   topk_tile_kernel   2) queries, or a tile of 64, x one slab of candidates.
//                      It loops over the slab -- 256 candidates, one per lane,
//                      through rank_scores, or 64 x 64 register tiles through
//                      rank_tile_scores -- and keeps per query, in LDS, a
//                      threshold (its current k-th best key) and a buffer of
//                      cap >= 2k keys. A candidate that beats the threshold is
//                      appended through an LDS counter; when an append finds
//                      a buffer full the workgroup sorts every buffer (one
//                      batched bitonic network), keeps the best k of each and
//                      raises the thresholds, and the refused lanes try again.
//                      At slab end each query's best k keys go to the
//                      workspace [n, nslab, k].
//   topk_merge_kernel  workgroup per query: streams its nslab lists through
//                      an LDS buffer (carry the best k, sort, repeat), decodes
//                      the keys to ids and scores and pads the unused slots.
//
// A key is 64 bits and orders like the answer under plain unsigned >: the high
// word is the score under the usual order-preserving map of its bits (-0
// mapped to +0's word, a NaN to 0, below -inf), the low word (2^31 - 1 - id)
// << 1, plus one bit that remembers a -0 so the decoded score keeps its sign.
// Ids are unique per query, hence so are keys, and the result cannot depend on
// the order the atomics append in. Key 0 is "no candidate" (no valid key is 0
// while id < 2^31 - 1: kge_topk refuses larger tables).
#include <algorithm>

#include "kge_rank_impl.h"

namespace kge {

using u64 = unsigned long long;

__device__ __forceinline__ u64 topk_key(float s, int64_t e) {
  const uint32_t b = __float_as_uint(s);
  uint32_t hi, nz = 0u;
  if (s != s) hi = 0u;
  else if (b == 0x80000000u) { hi = 0x80000000u; nz = 1u; }
  else hi = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  const uint32_t lo = ((0x7fffffffu - (uint32_t)e) << 1) | nz;
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ int64_t topk_key_id(u64 key) { return (int64_t)(0x7fffffffu - ((uint32_t)key >> 1)); }
__device__ __forceinline__ float topk_key_score(u64 key) {
  const uint32_t hi = (uint32_t)(key >> 32);
  if (hi == 0u) return __uint_as_float(0x7fc00000u);
  if (hi == 0x80000000u) return __uint_as_float(((uint32_t)key & 1u) ? 0x80000000u : 0u);
  return __uint_as_float((hi & 0x80000000u) ? (hi & 0x7fffffffu) : ~hi);
}

// nseg segments of cap keys (cap a power of two) laid end to end, each sorted
// descending by the whole workgroup: one bitonic network over all segments.
// Ends with a barrier; the caller synchronises before.
__device__ __forceinline__ void topk_sort_desc(u64* buf, int nseg, int cap) {
  const int half = nseg * (cap >> 1);
  for (int kk = 2; kk <= cap; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < half; t += blockDim.x) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const bool desc = ((i & (cap - 1)) & kk) == 0;
        const u64 a = buf[i], b = buf[i | j];
        if ((a < b) == desc) { buf[i] = b; buf[i | j] = a; }
      }
      __syncthreads();
    }
  }
}

// A workgroup's selection state in LDS: per query a buffer of cap keys, the
// number appended (it may run past cap: the appends that were refused) and the
// threshold, 0 until the query has seen k candidates.
struct TopkSel {
  u64* buf; u64* thr; int* cnt;
  int nq, cap, k;
};
__host__ __device__ inline uint32_t topk_sel_bytes(int nq, int cap) { return (uint32_t)nq * ((uint32_t)cap * 8u + 16u); }

__device__ __forceinline__ TopkSel topk_sel_init(void* mem, int nq, int cap, int k) {
  TopkSel S;
  S.buf = (u64*)mem;
  S.thr = S.buf + (size_t)nq * cap;
  S.cnt = (int*)(S.thr + nq);
  S.nq = nq; S.cap = cap; S.k = k;
  for (int q = threadIdx.x; q < nq; q += blockDim.x) { S.thr[q] = 0ull; S.cnt[q] = 0; }
  return S;
}

// Every buffer down to its best k, sorted, and the thresholds raised. All
// threads call it, after a barrier; it ends with one.
__device__ __forceinline__ void topk_sel_compact(const TopkSel& S) {
  const int tot = S.nq * S.cap;
  for (int i = threadIdx.x; i < tot; i += blockDim.x)
    if ((i & (S.cap - 1)) >= S.cnt[i / S.cap]) S.buf[i] = 0ull;
  __syncthreads();
  topk_sort_desc(S.buf, S.nq, S.cap);
  for (int q = threadIdx.x; q < S.nq; q += blockDim.x) {
    const int c = min(min(S.cnt[q], S.cap), S.k);
    S.cnt[q] = c;
    if (c == S.k) S.thr[q] = S.buf[q * S.cap + S.k - 1];
  }
  __syncthreads();
}

// Offer this thread's NI (query, key) items (key 0: none). All threads call
// it; it ends with a barrier.
template <int NI>
__device__ __forceinline__ void topk_sel_push(const TopkSel& S, const int (&qi)[NI], const u64 (&key)[NI]) {
  uint32_t pend = 0u;
#pragma unroll
  for (int i = 0; i < NI; ++i) pend |= key[i] > S.thr[qi[i]] ? 1u << i : 0u;
  for (;;) {
    int full = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      if (!((pend >> i) & 1u)) continue;
      if (key[i] > S.thr[qi[i]]) {   // (again: a compaction may have raised it)
        const int slot = atomicAdd(&S.cnt[qi[i]], 1);
        if (slot < S.cap) { S.buf[qi[i] * S.cap + slot] = key[i]; pend &= ~(1u << i); }
        else full = 1;
      } else {
        pend &= ~(1u << i);
      }
    }
    if (!__syncthreads_or(full)) break;
    topk_sel_compact(S);   // frees cap - k >= k slots of every buffer: the retry makes progress
  }
}

// Slab end: the best k keys of each query of the group, zeros after the last.
__device__ __forceinline__ void topk_sel_flush(const TopkSel& S, const TopkArgs& T, int64_t q0i, int nq, int64_t nslab,
                                               int64_t slab) {
  topk_sel_compact(S);
  for (int i = threadIdx.x; i < nq * S.k; i += blockDim.x) {
    const int q = i / S.k, j = i % S.k;
    T.lists[((q0i + q) * nslab + slab) * S.k + j] = S.buf[q * S.cap + j];
  }
}

template <int MODE, int PJ, int SK, int NQ>
__global__ __launch_bounds__(kRankThreads) void topk_lane_kernel(RankArgs A, TopkArgs T, TopkPlan P, int64_t g0) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  // x: query group (consecutive workgroups stream the same slab: its rows are
  // reused from L2), y: slab
  const int64_t q0i = (g0 + blockIdx.x) * NQ, slab = blockIdx.y;
  const int nq = (int)min<int64_t>(NQ, A.n - q0i);
  const int LQ = (A.dim + 3) & ~3;
  float* s0 = smem;
  float* s1 = smem + NQ * LQ;
  float* sw = smem + 2 * NQ * LQ;
  rank_stage_queries<NQ>(A, q0i, nq, smem);
  const TopkSel S = topk_sel_init(smem + 3 * NQ * LQ, NQ, P.cap, T.k);
  __syncthreads();
  const int64_t e_end = min<int64_t>(A.E, (slab + 1) * P.slab);
  for (int64_t eb = slab * P.slab; eb < e_end; eb += kRankThreads) {
    const int64_t e = eb + threadIdx.x;
    const bool in = e < e_end;
    const int64_t ee = in ? e : 0;
    float s[NQ];
    rank_scores<MODE, PJ, SK, NQ>(A, ee, s0, s1, sw, LQ, s);
    int qi[NQ];
    u64 key[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      bool keep = in && q < nq;
      if (keep && A.fbits) keep = !((A.fbits[(q0i + q) * A.fw + (ee >> 5)] >> (uint32_t)(ee & 31)) & 1u);
      qi[q] = q;
      key[q] = keep ? topk_key(s[q], ee) : 0ull;
    }
    topk_sel_push<NQ>(S, qi, key);
  }
  topk_sel_flush(S, T, q0i, nq, P.nslab, slab);
}

template <int MODE, int SK, bool HS>
__global__ __launch_bounds__(256) void topk_tile_kernel(RankArgs A, TopkArgs T, TopkPlan P, int64_t qt0) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tq = threadIdx.x >> 4, tc = threadIdx.x & 15;
  const int64_t q0i = (qt0 + blockIdx.x) * kRT, slab = blockIdx.y;
  const int nq = (int)min<int64_t>(kRT, A.n - q0i);
  const TopkSel S = topk_sel_init(smem, kRT, P.cap, T.k);
  __syncthreads();
  const int64_t e_end = min<int64_t>(A.E, (slab + 1) * P.slab);
  for (int64_t c0 = slab * P.slab; c0 < e_end; c0 += kRT) {
    uint32_t fmask[4];
    rank_tile_fmask(A, q0i, c0, fmask);
    float sc[4][4];
    rank_tile_scores<MODE, SK, HS>(A, q0i, c0, sc);
    int qi[16];
    u64 key[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t e = c0 + 4 * tc + j;
        const bool keep = 4 * tq + i < nq && e < e_end && !((fmask[i] >> j) & 1u);
        qi[4 * i + j] = 4 * tq + i;
        key[4 * i + j] = keep ? topk_key(sc[i][j], e) : 0ull;
      }
    }
    topk_sel_push<16>(S, qi, key);
  }
  topk_sel_flush(S, T, q0i, nq, P.nslab, slab);
}

// M: keys of LDS, a power of two >= 2k.
__global__ __launch_bounds__(256) void topk_merge_kernel(TopkArgs T, int64_t nslab, int M, int64_t qb) {
  extern __shared__ __attribute__((aligned(16))) u64 mbuf[];
  const int64_t q = qb + blockIdx.x;
  const int k = T.k;
  const int64_t total = nslab * k;
  const u64* src = T.lists + q * total;
  int carry = 0;   // the best so far sit in mbuf[0, carry)
  for (int64_t pos = 0; pos < total;) {
    const int room = M - carry;
    const int take = (int)min<int64_t>(room, total - pos);
    for (int i = threadIdx.x; i < room; i += blockDim.x) mbuf[carry + i] = i < take ? src[pos + i] : 0ull;
    __syncthreads();
    topk_sort_desc(mbuf, 1, M);
    pos += take;
    carry = k;
  }
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    const u64 key = mbuf[i];
    const int64_t id = key ? topk_key_id(key) : -1;
    if (T.out64) ((int64_t*)T.ids)[q * k + i] = id;
    else ((int32_t*)T.ids)[q * k + i] = (int32_t)id;
    T.scores[q * k + i] = key ? topk_key_score(key) : -INFINITY;
    // the written entries are a prefix: the last of them knows the count
    if (T.count) {
      if (key && (i == k - 1 || mbuf[i + 1] == 0ull)) T.count[q] = i + 1;
      if (!key && i == 0) T.count[q] = 0;
    }
  }
}

static int pow2_ceil(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

TopkPlan topk_plan(int mode, int proj, int dim, int64_t n, int64_t E, int k, int flags) {
  TopkPlan P{};
  const int kp = pow2_ceil(k);
  const bool elementwise = (mode == KGE_RANK_TRANS && proj == KGE_RPROJ_NONE) || mode == KGE_RANK_MUL || mode == KGE_RANK_DOT;
  // the tile's 64 buffers of 2k keys beside its 12 KB of staged rows: k <= 32
  P.tiled = elementwise && !(flags & KGE_TOPK_FLAG_LANE_PASS) && 2 * kp <= 64;
  if (P.tiled) {
    P.nq = kRT;
    P.cap = std::max(2 * kp, 32);
    P.lds_bytes = topk_sel_bytes(kRT, P.cap);
  } else {
    P.cap = std::max(2 * kp, 128);
    const uint32_t row = 3u * (uint32_t)((dim + 3) & ~3) * 4u;   // one query's staged rows
    P.nq = kRankQ * row + topk_sel_bytes(kRankQ, P.cap) <= 64u * 1024u ? kRankQ : 2;
    P.lds_bytes = P.nq * row + topk_sel_bytes(P.nq, P.cap);
  }
  // enough workgroups to fill the device, slabs of at least 2048 candidates
  const int64_t groups = (n + P.nq - 1) / P.nq;
  int64_t ns = 1;
  if (flags & KGE_TOPK_FLAG_DEBUG_SLAB) {
    P.slab = 256;
  } else {
    ns = std::max<int64_t>(1, std::min<int64_t>((2048 + groups - 1) / std::max<int64_t>(groups, 1), (E + 2047) / 2048));
    P.slab = (((E + ns - 1) / ns) + 255) / 256 * 256;
  }
  P.nslab = (E + P.slab - 1) / P.slab;
  if (P.nslab > 65535) {   // grid y
    P.slab = (((E + 65534) / 65535) + 255) / 256 * 256;
    P.nslab = (E + P.slab - 1) / P.slab;
  }
  return P;
}

constexpr int64_t kTopkMaxX = (int64_t)1 << 22;   // x * 256 work-items < 2^32 per launch

template <int MODE, int PJ, int SK>
static void topk_launch(const RankArgs& A, const TopkArgs& T, const TopkPlan& P, hipStream_t st) {
  if constexpr ((MODE == KGE_RANK_TRANS && PJ == KGE_RPROJ_NONE) || MODE == KGE_RANK_MUL || MODE == KGE_RANK_DOT) {
    if (P.tiled) {
      const int64_t nqt = (A.n + kRT - 1) / kRT;
      for (int64_t t0 = 0; t0 < nqt; t0 += kTopkMaxX) {
        const dim3 grid((unsigned)std::min(nqt - t0, kTopkMaxX), (unsigned)P.nslab);
        if (A.hside) hipLaunchKernelGGL((topk_tile_kernel<MODE, SK, true>), grid, dim3(256), P.lds_bytes, st, A, T, P, t0);
        else hipLaunchKernelGGL((topk_tile_kernel<MODE, SK, false>), grid, dim3(256), P.lds_bytes, st, A, T, P, t0);
      }
      return;
    }
  }
  const int64_t ng = (A.n + P.nq - 1) / P.nq;
  for (int64_t g0 = 0; g0 < ng; g0 += kTopkMaxX) {
    const dim3 grid((unsigned)std::min(ng - g0, kTopkMaxX), (unsigned)P.nslab);
    if (P.nq == kRankQ)
      hipLaunchKernelGGL((topk_lane_kernel<MODE, PJ, SK, kRankQ>), grid, dim3(kRankThreads), P.lds_bytes, st, A, T, P, g0);
    else
      hipLaunchKernelGGL((topk_lane_kernel<MODE, PJ, SK, 2>), grid, dim3(kRankThreads), P.lds_bytes, st, A, T, P, g0);
  }
}

template <int MODE, int PJ>
static void topk_by_sk(const RankArgs& A, const TopkArgs& T, const TopkPlan& P, int sk, hipStream_t st) {
  switch (sk) {
    case SK_P1: topk_launch<MODE, PJ, SK_P1>(A, T, P, st); break;
    case SK_P2: topk_launch<MODE, PJ, SK_P2>(A, T, P, st); break;
    case SK_PINF: topk_launch<MODE, PJ, SK_PINF>(A, T, P, st); break;
    case SK_PGEN: topk_launch<MODE, PJ, SK_PGEN>(A, T, P, st); break;
    default: topk_launch<MODE, PJ, SK_DOT>(A, T, P, st); break;
  }
}

kge_status launch_topk(const RankArgs& A, const TopkArgs& T, const TopkPlan& P, int mode, int proj, int sk,
                       hipStream_t st) {
  if (mode == KGE_RANK_ROT && sk == SK_DOT) return KGE_EUNSUPPORTED;
  if (A.fbits && launch_rank_bits(A, st) != KGE_OK) return KGE_EHIP;   // before the producers that read it
  switch (mode) {
    case KGE_RANK_TRANS:
      if (proj == KGE_RPROJ_HYPER) topk_by_sk<KGE_RANK_TRANS, KGE_RPROJ_HYPER>(A, T, P, sk, st);
      else if (proj == KGE_RPROJ_RANK1) topk_by_sk<KGE_RANK_TRANS, KGE_RPROJ_RANK1>(A, T, P, sk, st);
      else topk_by_sk<KGE_RANK_TRANS, KGE_RPROJ_NONE>(A, T, P, sk, st);
      break;
    case KGE_RANK_ROT: topk_by_sk<KGE_RANK_ROT, KGE_RPROJ_NONE>(A, T, P, sk, st); break;
    case KGE_RANK_MUL: topk_launch<KGE_RANK_MUL, KGE_RPROJ_NONE, SK_DOT>(A, T, P, st); break;
    case KGE_RANK_DOT: topk_launch<KGE_RANK_DOT, KGE_RPROJ_NONE, SK_DOT>(A, T, P, st); break;
    default: return KGE_EUNSUPPORTED;
  }
  const int M = std::max(2 * pow2_ceil(T.k), 1024);
  for (int64_t qb = 0; qb < A.n; qb += kTopkMaxX)
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)std::min(A.n - qb, kTopkMaxX)), dim3(256), (size_t)M * 8, st, T,
                       P.nslab, M, qb);
  return KGE_OK;
}

}  // namespace kge
