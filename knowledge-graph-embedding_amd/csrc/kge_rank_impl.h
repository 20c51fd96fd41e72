// Candidate scoring shared by kge_rank.hip (filtered ranks) and kge_topk.hip
// (top-k link prediction): both evaluate every score with these functions, op
// by op (no contraction) in one fixed element order, so a candidate's score
// has the same bits in every pass of either entry point.
#pragma once

#include "kge_step.h"

namespace kge {

// Scores of candidate entity `e` against NQ queries whose rows sit at
// q0 + j * qs, q1 + j * qs, w + j * qs (any address space). The candidate's
// elements are loaded once and used by every query; each query's sum runs in
// the same element order for any NQ, so NQ = 1 (pos / filter passes) and
// NQ = 8 (count pass) give identical bits. MODE: KGE_RANK_*; PJ: KGE_RPROJ_*.
template <int MODE, int PJ, int SK, int NQ>
__device__ __forceinline__ void rank_scores(const RankArgs& A, int64_t e, const float* q0, const float* q1,
                                            const float* w, int qs, float (&out)[NQ]) {
#pragma clang fp contract(off)
  const float* x = A.cand + e * A.cand_ld;
  const int D = A.dim;
  float acc[NQ];
#pragma unroll
  for (int j = 0; j < NQ; ++j) acc[j] = 0.f;
  auto lp = [&](float& ac, float a) {
    const float m = fabsf(a);
    if (SK == SK_P2) ac = ac + m * m;
    else if (SK == SK_P1) ac = ac + m;
    else if (SK == SK_PGEN) ac = ac + powf(m, A.p);
    else ac = fmaxf(ac, m);
  };
  if (MODE == KGE_RANK_ROT) {
    // complex pairs; t-side a = q0 - e, h-side a = e o q0 - q1
    for (int c = 0; c < D; c += 2) {
      const float er = x[c], ei = x[c + 1];
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        const float* a0 = q0 + j * qs;
        float ar, ai;
        if (A.hside) {
          const float* a1 = q1 + j * qs;
          const float xr = er * a0[c] - ei * a0[c + 1];
          const float xi = er * a0[c + 1] + ei * a0[c];
          ar = xr - a1[c];
          ai = xi - a1[c + 1];
        } else {
          ar = a0[c] - er;
          ai = a0[c + 1] - ei;
        }
        if (SK == SK_P2) acc[j] = acc[j] + (ar * ar + ai * ai);
        else {
          const float m = sqrtf(ar * ar + ai * ai);
          acc[j] = SK == SK_P1 ? acc[j] + m : SK == SK_PGEN ? acc[j] + powf(m, A.p) : fmaxf(acc[j], m);
        }
      }
    }
  } else if (MODE == KGE_RANK_MUL || MODE == KGE_RANK_DOT) {
    // DistMult sum(h * r * t): t-side q0 = h * r, h-side (e * r) * t;
    // RESCAL: q0 = R^T h (t-side) or R t (h-side)
    for (int c = 0; c < D; ++c) {
      const float xe = x[c];
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        const float* a0 = q0 + j * qs;
        acc[j] = acc[j] + ((MODE == KGE_RANK_MUL && A.hside) ? (xe * a0[c]) * q1[j * qs + c] : a0[c] * xe);
      }
    }
  } else {
    // translating: P(e) then t-side a = q0 - P(e), h-side a = (P(e) + q0) - q1
    float dt[NQ], sc[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) { dt[j] = 0.f; sc[j] = 1.f; }
    if (PJ == KGE_RPROJ_HYPER) {
      for (int c = 0; c < D; ++c) {
        const float xe = x[c];
#pragma unroll
        for (int j = 0; j < NQ; ++j) dt[j] = dt[j] + w[j * qs + c] * xe;
      }
    } else if (PJ == KGE_RPROJ_RANK1) {
      // e_p . e is the candidate's own; the clip norm depends on the query's r_p
      const float* ep = A.caux + e * A.caux_ld;
      float de = 0.f;
      for (int c = 0; c < A.ecols; ++c) de = de + ep[c] * x[c];
#pragma unroll
      for (int j = 0; j < NQ; ++j) dt[j] = de;
      if (A.clip) {
        float n2[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) n2[j] = 0.f;
        for (int c = 0; c < D; ++c) {
          const float xe = c < A.kmin ? x[c] : 0.f;
#pragma unroll
          for (int j = 0; j < NQ; ++j) {
            const float p = w[j * qs + c] * de + xe;
            n2[j] = n2[j] + p * p;
          }
        }
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
          const float n = sqrtf(n2[j]);
          if (!(n < 1.f)) sc[j] = fmaxf(n, 1e-9f);
        }
      }
    }
    for (int c = 0; c < D; ++c) {
      const float xe = (PJ != KGE_RPROJ_RANK1 || c < A.kmin) ? x[c] : 0.f;
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        const float* a0 = q0 + j * qs;
        float p;
        if (PJ == KGE_RPROJ_HYPER) p = xe - dt[j] * w[j * qs + c];
        else if (PJ == KGE_RPROJ_RANK1) p = (w[j * qs + c] * dt[j] + xe) / sc[j];
        else p = xe;
        if (SK == SK_DOT) acc[j] = acc[j] + (A.hside ? (p + a0[c]) * q1[j * qs + c] : a0[c] * p);
        else lp(acc[j], A.hside ? (p + a0[c]) - q1[j * qs + c] : a0[c] - p);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    if (SK == SK_DOT || MODE == KGE_RANK_MUL || MODE == KGE_RANK_DOT) {
      out[j] = acc[j];
    } else {
      float lpv;
      out[j] = score_value<SK>(acc[j], A.pw, &lpv, A.p);
    }
  }
}

// The lane-per-candidate passes' query rows: a group of NQ queries' q0 / q1 /
// qw rows staged in LDS at s0 / s1 / sw = qs + {0, 1, 2} * NQ * LQ floats,
// LQ = dim rounded up to 4 (rows past the set: zeros, results discarded).
template <int NQ>
__device__ __forceinline__ void rank_stage_queries(const RankArgs& A, int64_t q0i, int nq, float* qs) {
  const int LQ = (A.dim + 3) & ~3;
  float* s0 = qs;
  float* s1 = qs + NQ * LQ;
  float* sw = qs + 2 * NQ * LQ;
  for (int t = threadIdx.x; t < NQ * A.dim; t += blockDim.x) {
    const int q = t / A.dim, c = t % A.dim;
    const bool v = q < nq;
    s0[q * LQ + c] = v ? A.q0[(q0i + q) * A.ldq + c] : 0.f;
    s1[q * LQ + c] = (v && A.q1) ? A.q1[(q0i + q) * A.ldq + c] : 0.f;
    sw[q * LQ + c] = (v && A.qw) ? A.qw[(q0i + q) * A.ldq + c] : 0.f;
  }
}

// Register-tiled scoring for the element-wise scores (translating without a
// projection: TransE, TransR's pre-projected candidates; DistMult; RESCAL): a
// 256-thread workgroup scores the 64-query x 64-candidate tile at (q0i, c0),
// each thread the 4 x 4 pairs (4 tq + i, 4 tc + j) held in registers, over
// 16-element chunks staged transposed in LDS ([element][row]: a thread's four
// queries and four candidates are one ds_read_b128 each). Candidate rows are
// read once per 64 queries and with whole-row float4 loads. Every pair's sum
// runs over the elements in ascending order with the same ops as rank_scores,
// so the scores are bit for bit those of the lane-per-candidate passes. Rows
// past n / E score as rows of zeros (the caller discards them). May be called
// in a loop over tiles: it synchronises before it overwrites the staged rows.
constexpr int kRT = 64;    // queries / candidates per tile
constexpr int kRC = 16;    // elements per staged chunk

template <int MODE, int SK, bool HS>
__device__ __forceinline__ void rank_tile_scores(const RankArgs& A, int64_t q0i, int64_t c0, float (&sc)[4][4]) {
#pragma clang fp contract(off)
  using f2 = __attribute__((ext_vector_type(2))) float;
  __shared__ __attribute__((aligned(16))) float sq0[kRC][kRT];
  __shared__ __attribute__((aligned(16))) float sq1[kRC][kRT];
  __shared__ __attribute__((aligned(16))) float sx[kRC][kRT];
  const int tid = threadIdx.x, tq = tid >> 4, tc = tid & 15;
  constexpr bool two = (MODE == KGE_RANK_TRANS || MODE == KGE_RANK_MUL) && HS;   // h-side: q1 too
  const int D = A.dim;
  // pairs (i, 2jp) and (i, 2jp + 1) side by side: the element ops run as
  // packed f32 (v_pk_add / v_pk_mul), each lane of a pair in the scalar order
  f2 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = f2{0.f, 0.f};
  // staging: thread t loads row (t >> 2) elements 4 (t & 3) .. +3 of each tile
  const int sr = tid >> 2, se = (tid & 3) * 4;
  const int64_t qr = q0i + sr, er = c0 + sr;
  const bool qv = qr < A.n, ev = er < A.E;
  for (int e0 = 0; e0 < D; e0 += kRC) {
    const int ne = min(kRC, D - e0);
    float a[4], b[4], x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = e0 + se + u;
      const bool in = se + u < ne;
      a[u] = (qv && in) ? A.q0[qr * A.ldq + c] : 0.f;
      b[u] = (two && qv && in) ? A.q1[qr * A.ldq + c] : 0.f;
      x[u] = (ev && in) ? A.cand[er * A.cand_ld + c] : 0.f;
    }
    __syncthreads();   // the previous chunk is consumed
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      sq0[se + u][sr] = a[u];
      if (two) sq1[se + u][sr] = b[u];
      sx[se + u][sr] = x[u];
    }
    __syncthreads();
    for (int c = 0; c < ne; ++c) {
      const float4 qa = *reinterpret_cast<const float4*>(&sq0[c][4 * tq]);
      const float4 xa = *reinterpret_cast<const float4*>(&sx[c][4 * tc]);
      float4 qb = make_float4(0.f, 0.f, 0.f, 0.f);
      if (two) qb = *reinterpret_cast<const float4*>(&sq1[c][4 * tq]);
      const float qv0[4] = {qa.x, qa.y, qa.z, qa.w}, qv1[4] = {qb.x, qb.y, qb.z, qb.w};
      const f2 xp[2] = {f2{xa.x, xa.y}, f2{xa.z, xa.w}};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f2 a0 = f2{qv0[i], qv0[i]}, a1 = f2{qv1[i], qv1[i]};
#pragma unroll
        for (int jp = 0; jp < 2; ++jp) {
          const f2 xe = xp[jp];
          f2& ac = acc[i][jp];
          if (MODE == KGE_RANK_MUL) {
            ac = ac + (HS ? (xe * a0) * a1 : a0 * xe);
          } else if (MODE == KGE_RANK_DOT) {
            ac = ac + a0 * xe;
          } else if (SK == SK_DOT) {
            ac = ac + (HS ? (xe + a0) * a1 : a0 * xe);
          } else {
            const f2 d = HS ? (xe + a0) - a1 : a0 - xe;
            if (SK == SK_P2) {
              ac = ac + d * d;   // |d| |d| == d d bit for bit
            } else {
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                const float m = fabsf(d[h]);
                if (SK == SK_P1) ac[h] = ac[h] + m;
                else if (SK == SK_PGEN) ac[h] = ac[h] + powf(m, A.p);
                else ac[h] = fmaxf(ac[h], m);
              }
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float av = acc[i][j >> 1][j & 1];
      if (SK == SK_DOT || MODE == KGE_RANK_MUL || MODE == KGE_RANK_DOT) {
        sc[i][j] = av;
      } else {
        float lpv;
        sc[i][j] = score_value<SK>(av, A.pw, &lpv, A.p);
      }
    }
  }
}

// The filter words of the tile thread's four candidates 4 tc .. 4 tc + 3 (c0
// is a multiple of 64, so they share one word), per query of its four: bit j
// of fmask[i] marks candidate 4 tc + j as a known positive of query 4 tq + i.
__device__ __forceinline__ void rank_tile_fmask(const RankArgs& A, int64_t q0i, int64_t c0, uint32_t (&fmask)[4]) {
  const int tq = threadIdx.x >> 4, tc = threadIdx.x & 15;
#pragma unroll
  for (int i = 0; i < 4; ++i) fmask[i] = 0u;
  if (A.fbits && c0 + 4 * tc < A.E) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t q = q0i + 4 * tq + i;
      if (q < A.n) fmask[i] = A.fbits[q * A.fw + ((c0 + 4 * tc) >> 5)] >> (uint32_t)((4 * tc) & 31);
    }
  }
}

}  // namespace kge
