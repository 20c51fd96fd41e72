// TransR fused training step for gfx950 (TransR.py:154-211): the host side
// (launch_step_transr), the materialised update launch and the rel_proj apply
// pass. The score / gradient kernel is transr2_kernel (kge_transr2.h),
// instantiated per score kind by kge_transr2_*.hip.
//
// TransR projects every entity row of a triple through its relation's
// matrix M_r [d, k] before scoring:  s = score(clip(h M_r) + r, clip(t M_r)).
// All triples of a positive share M_r, so the projection work of one
// positive is three small fp32 MFMA GEMMs, done by ONE workgroup (8 waves):
//
//   X  [K, d]     the K negatives' entity rows, gathered into LDS (h and t
//                 ride along on the VALU)
//   P  = X M_r    GEMM1 -> projected rows, kept in MFMA accumulator layout
//   scores / loss / dL/dP per triple; the per-triple gradients wrt every
//   projected row (slices), back through the clip
//   Y  = S M_r^T  GEMM2 -> entity-row gradients (h, t to the positive-gradient
//                 rows, negatives to gneg[code]) and the entity slice norms
//   dM = X^T S'   GEMM3 -> this positive's rel_proj gradient (a per-positive
//                 partial; the apply pass sums a relation's partials in
//                 positive order)
//
// The update pass is the shared destination-major kernel in its
// materialised mode (gradient rows summed in code order); rel_proj is
// updated by transr_proj_apply.
#include "kge_transr2.h"

namespace kge {

// (defined by the kge_transr2_*.hip units, one score kind each)
extern template void launch_transr2<SK_P1>(const StepArgs&, const TrArgs&, hipStream_t);
extern template void launch_transr2<SK_P2>(const StepArgs&, const TrArgs&, hipStream_t);
extern template void launch_transr2<SK_PINF>(const StepArgs&, const TrArgs&, hipStream_t);
extern template void launch_transr2<SK_DOT>(const StepArgs&, const TrArgs&, hipStream_t);
extern template void launch_transr2<SK_PGEN>(const StepArgs&, const TrArgs&, hipStream_t);

// rel_proj update: per relation, the positives' dM partials summed in
// sorted (positive) order, clip scale, SGD -- or the dense gradient in
// KGE_OPT_GRAD mode. 1024 elements of M_r per workgroup.
__global__ __launch_bounds__(256) void transr_proj_apply(StepArgs A, TrArgs T) {
  if (ws_refused(A.ctl, A.sig, A.status, A.loss_out)) return;
  const int64_t dk = (int64_t)T.d * T.k;
  const int64_t chunks = (dk + 1023) / 1024;
  const int64_t r = blockIdx.x / chunks, ch = blockIdx.x % chunks;
  const int64_t beg = T.rel_beg[r], end = beg + T.rel_cnt[r];
  if (beg == end) return;
  const float sc = A.ctl->scale[2];
  const int64_t e1 = min(dk, (ch + 1) * 1024);
  const bool v4 = dk % 4 == 0 && T.proj.ld % 4 == 0 && ((uintptr_t)T.proj.p % 16) == 0 &&
                  ((uintptr_t)T.dmpart % 16) == 0 && (!T.gproj_out || ((uintptr_t)T.gproj_out % 16) == 0);
  if (v4) {
    // a float4 of M_r per thread; the relation's partials four positives at
    // a time, every load issued before the adds (same ascending order)
    const int64_t e = ch * 1024 + 4 * (int64_t)threadIdx.x;
    if (e >= e1) return;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    auto add = [&](const float4& x) { g.x += x.x; g.y += x.y; g.z += x.z; g.w += x.w; };
    const float* base = T.dmpart + e;
    int64_t p = beg;
    for (; p + 4 <= end; p += 4) {
      float4 x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) x[u] = *reinterpret_cast<const float4*>(base + (int64_t)T.sorted[p + u] * dk);
#pragma unroll
      for (int u = 0; u < 4; ++u) add(x[u]);
    }
    for (; p < end; ++p) add(*reinterpret_cast<const float4*>(base + (int64_t)T.sorted[p] * dk));
    if (T.gproj_out) *reinterpret_cast<float4*>(T.gproj_out + r * dk + e) = g;
    else {
      float4* w = reinterpret_cast<float4*>(T.proj.p + r * T.proj.ld + e);
      float4 m = *w;
      m.x = m.x + g.x * sc; m.y = m.y + g.y * sc; m.z = m.z + g.z * sc; m.w = m.w + g.w * sc;
      *w = m;
    }
    return;
  }
  for (int64_t e = ch * 1024 + threadIdx.x; e < e1; e += 256) {
    float g = 0.f;
    for (int64_t p = beg; p < end; ++p) g += T.dmpart[(int64_t)T.sorted[p] * dk + e];
    if (T.gproj_out) T.gproj_out[r * dk + e] = g;
    else {
      float* w = T.proj.p + r * T.proj.ld + e;
      *w = *w + g * sc;
    }
  }
}

static void launch_update_mat(const StepArgs& A, const StepGeom& G, hipStream_t st) {
#define KGE_UPD(V, N)                                                                                            \
  do {                                                                                                           \
    if (A.compact)                                                                                               \
      hipLaunchKernelGGL((update_kernel<Materialised, V, N, SK_DOT, 1, true>), dim3(G.gridU), dim3(kUpdThreads), 0, \
                         st, A);                                                                                 \
    else                                                                                                         \
      hipLaunchKernelGGL((update_kernel<Materialised, V, N, SK_DOT>), dim3(G.gridU), dim3(kUpdThreads), 0, st, A); \
  } while (0)
  if (G.vec == 4) {
    if (G.nc == 1) KGE_UPD(4, 1); else if (G.nc == 2) KGE_UPD(4, 2); else KGE_UPD(4, 4);
  } else {
    if (G.nc == 1) KGE_UPD(1, 1); else if (G.nc == 2) KGE_UPD(1, 2); else KGE_UPD(1, 4);
  }
#undef KGE_UPD
}

template <int SK>
static void launch_tr(const StepArgs& A, const StepGeom& G, const TrArgs& T, const RelArgs& P, hipStream_t st,
                      hipEvent_t const* ev) {
  if (A.train) launch_rel_rank(P, st);
  launch_transr2<SK>(A, T, st);
  if (ev) (void)hipEventRecord(ev[2], st);
  if (A.train) {
    launch_update_mat(A, G, st);
    const int64_t chunks = ((int64_t)T.d * T.k + 1023) / 1024;
    hipLaunchKernelGGL(transr_proj_apply, dim3((unsigned)(T.proj.rows * chunks)), dim3(256), 0, st, A, T);
  }
}

kge_status launch_step_transr(const StepArgs& A, const StepGeom& G, const TrArgs& T, const RelArgs& P, int sk,
                              hipStream_t st, hipEvent_t const* ev) {
  switch (sk) {
    case SK_P1: launch_tr<SK_P1>(A, G, T, P, st, ev); break;
    case SK_P2: launch_tr<SK_P2>(A, G, T, P, st, ev); break;
    case SK_PINF: launch_tr<SK_PINF>(A, G, T, P, st, ev); break;
    case SK_PGEN: launch_tr<SK_PGEN>(A, G, T, P, st, ev); break;
    default: launch_tr<SK_DOT>(A, G, T, P, st, ev); break;
  }
  return KGE_OK;
}

}  // namespace kge
