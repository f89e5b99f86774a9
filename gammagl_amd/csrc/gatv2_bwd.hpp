// gammagl_amd/csrc/gatv2_bwd.hpp — what GATv2's logit adds to the backward of the edge-softmax aggregate.  Included by
// gat.hip alone (so the host builds compile it too: no lane talks to another).
//
//   z[e,h] = sum_c att[h,c] * LeakyReLU(xl[src(e),h,c] + xr[dst(e),h,c])
// With gz = dL/dz from ggl_edge_softmax_agg_bwd_dst, the logit's part of the node gradients is
//   g_xr[i,h,c] = att[h,c] * sum_{e -> i} gz[e,h] * lrelu'(s_e),    s_e = xl[src(e),h,c] + xr[i,h,c]
//   g_xl[j,h,c] = the same over the edges that LEAVE j (transposed plan), plus the value part gv
//   g_att[h,c]  = sum_e gz[e,h] * lrelu(s_e) = column sums of R[i,h,c] = sum_{e -> i} gz[e,h] * lrelu(s_e)
// bspmm cannot carry this: the LeakyReLU mask is per (edge, head, channel).  One kernel serves both plans: for row r of
// the plan it is given, head h, channel c, positions p ascending in [rowptr[r], rowptr[r+1]), e_p = perm ? perm[p] : p:
//   s    = __fadd_rn(other[col[p],h,c], self[r,h,c])
//   w    = gz[e_p,h]
//   accD = __fadd_rn(accD, s > 0 ? w : __fmul_rn(w, slope))
//   accA = __fadd_rn(accA, __fmul_rn(w, s > 0 ? s : __fmul_rn(s, slope)))          (only with att_rows)
//   g_self[r,h,c]   = add ? __fadd_rn(add[r,h,c], __fmul_rn(att[h,c], accD)) : __fmul_rn(att[h,c], accD)
//   att_rows[r,h,c] = accA
// A row with more than plan->chunk positions is walked in consecutive pieces of `chunk` positions (gat_bwd_src_kernel's
// rule): one wavefront per piece, each summing from 0.0f; gatv2_logit_bwd_final_kernel adds the partials in ascending
// chunk order from 0.0f, and the att multiply and `add` follow the merge.  A lane owns VEC channels of one (row, head):
// 4 where C % 4 == 0 and the pointers are 16-byte aligned, 1 otherwise; no sum's order depends on VEC.
#pragma once
#include "gat_common.hpp"

namespace ggl {

template <int VEC, bool ATT>
__device__ __forceinline__ void gatv2_logit_walk(const int32_t *__restrict__ col, const int32_t *__restrict__ perm,
                                                 const float *__restrict__ other, const float (&sv)[VEC],
                                                 const float *__restrict__ gz, float slope, int64_t H, int64_t K,
                                                 int64_t h, int64_t kk, int64_t beg, int64_t end, float (&accD)[VEC],
                                                 float (&accA)[VEC]) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) accD[i] = accA[i] = 0.0f;
  auto absorb = [&](float w, const float (&o)[VEC]) {
    const float ws = __fmul_rn(w, slope);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const float s = __fadd_rn(o[i], sv[i]);
      accD[i] = __fadd_rn(accD[i], s > 0.0f ? w : ws);
      if (ATT) accA[i] = __fadd_rn(accA[i], __fmul_rn(w, s > 0.0f ? s : __fmul_rn(s, slope)));
    }
  };
  int64_t p = beg;
  for (; p + 4 <= end; p += 4) {  // four rows in flight; absorbed in position order
    int64_t c[4], e[4];
    float o[4][VEC], w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { c[u] = col[p + u]; e[u] = Logit<kLogitEdge>::rec(perm, col, p + u, c[u]); }
#pragma unroll
    for (int u = 0; u < 4; ++u) F32V<VEC>::load(other + c[u] * K + kk, o[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) w[u] = gz[e[u] * H + h];
#pragma unroll
    for (int u = 0; u < 4; ++u) absorb(w[u], o[u]);
  }
  for (; p < end; ++p) {
    const int64_t c0 = col[p], e0 = Logit<kLogitEdge>::rec(perm, col, p, c0);
    float o0[VEC];
    F32V<VEC>::load(other + c0 * K + kk, o0);
    absorb(gz[e0 * H + h], o0);
  }
}

// what follows the sums of a (row, head, channel group): the att multiply, the optional add, the two stores
template <int VEC, bool ATT>
__device__ __forceinline__ void gatv2_logit_store(const float *__restrict__ att, const float *__restrict__ add,
                                                  float *__restrict__ g_self, float *__restrict__ att_rows, int64_t at,
                                                  int64_t kk, const float (&accD)[VEC], const float (&accA)[VEC]) {
  float a[VEC], r[VEC];
  F32V<VEC>::load(att + kk, a);
#pragma unroll
  for (int i = 0; i < VEC; ++i) r[i] = __fmul_rn(a[i], accD[i]);
  if (add) {
    float b[VEC];
    F32V<VEC>::load(add + at, b);
#pragma unroll
    for (int i = 0; i < VEC; ++i) r[i] = __fadd_rn(b[i], r[i]);
  }
  F32V<VEC>::store(g_self + at, r);
  if (ATT) F32V<VEC>::store(att_rows + at, accA);
}

template <int VEC, bool ATT>
__global__ __launch_bounds__(kBlock) void gatv2_logit_bwd_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int32_t *__restrict__ perm,
    const int32_t *__restrict__ row_order, const int32_t *__restrict__ long_rows,
    const int64_t *__restrict__ chunk_ptr, const float *__restrict__ other, const float *__restrict__ self,
    const float *__restrict__ gz, const float *__restrict__ att, const float *__restrict__ add,
    float *__restrict__ g_self, float *__restrict__ att_rows, float *__restrict__ pD, float *__restrict__ pA,
    const GatDims d) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int64_t H = d.H, K = d.K;
  if (block_id() < d.chunk_blocks) {  // one wavefront per chunk of a long row
    const int64_t cid = block_id() * kWavesPerBlock + wave;
    if (cid >= d.n_chunks) return;
    const HubChunk hc = hub_chunk(rowptr, long_rows, chunk_ptr, d.n_long, d.chunk, cid);
    for (int64_t kk = (int64_t)lane * VEC; kk < K; kk += (int64_t)kWave * VEC) {
      float sv[VEC], accD[VEC], accA[VEC];
      F32V<VEC>::load(self + hc.row * K + kk, sv);
      gatv2_logit_walk<VEC, ATT>(col, perm, other, sv, gz, d.slope, H, K, kk / d.C, kk, hc.beg, hc.end, accD, accA);
      F32V<VEC>::store(pD + cid * K + kk, accD);
      if (ATT) F32V<VEC>::store(pA + cid * K + kk, accA);
    }
    return;
  }
  const int L = 1 << d.logL;
  const int64_t slot = ((block_id() - d.chunk_blocks) * kWavesPerBlock + wave) * (kWave >> d.logL) +
                       (lane >> d.logL);
  if (slot >= d.N) return;
  const int64_t row = row_order ? (int64_t)row_order[slot] : slot;
  const int li = lane & (L - 1);
  const int64_t beg = rowptr[row], end = rowptr[row + 1];
  if (end - beg > d.chunk) return;
  for (int64_t kk = (int64_t)li * VEC; kk < K; kk += (int64_t)L * VEC) {
    float sv[VEC], accD[VEC], accA[VEC];
    F32V<VEC>::load(self + row * K + kk, sv);
    gatv2_logit_walk<VEC, ATT>(col, perm, other, sv, gz, d.slope, H, K, kk / d.C, kk, beg, end, accD, accA);
    gatv2_logit_store<VEC, ATT>(att, add, g_self, att_rows, row * K + kk, kk, accD, accA);
  }
}

// long rows: the partials of a row's chunks added in chunk order from 0.0f (deterministic), then the att multiply and add
template <bool ATT>
__global__ __launch_bounds__(kBlock) void gatv2_logit_bwd_final_kernel(
    const int32_t *__restrict__ long_rows, const int64_t *__restrict__ chunk_ptr, const float *__restrict__ pD,
    const float *__restrict__ pA, const float *__restrict__ att, const float *__restrict__ add,
    float *__restrict__ g_self, float *__restrict__ att_rows, const GatDims d) {
  const int64_t j = block_id();
  if (j >= d.n_long) return;
  const int64_t row = long_rows[j];
  const int64_t c0 = chunk_ptr[j], c1 = chunk_ptr[j + 1];
  for (int64_t k = threadIdx.x; k < d.K; k += kBlock) {
    float accD[1] = {0.0f}, accA[1] = {0.0f};
    for (int64_t c = c0; c < c1; ++c) {
      accD[0] = __fadd_rn(accD[0], pD[c * d.K + k]);
      if (ATT) accA[0] = __fadd_rn(accA[0], pA[c * d.K + k]);
    }
    gatv2_logit_store<1, ATT>(att, add, g_self, att_rows, row * d.K + k, k, accD, accA);
  }
}

}  // namespace ggl

// plan->partial of ggl_gatv2_logit_bwd for a plan with long rows: [n_chunks, H * C] sums of the derivative terms and, with
// att_rows, as many of the activation terms
extern "C" size_t ggl_gatv2_logit_bwd_partial_bytes(int64_t n_chunks, int64_t H, int64_t C, int with_att_rows) {
  if (n_chunks <= 0 || H <= 0 || C <= 0) return 0;
  return (size_t)n_chunks * (size_t)(H * C) * (with_att_rows ? 2 : 1) * sizeof(float) + 64;
}

extern "C" int ggl_gatv2_logit_bwd(const ggl_segplan_t *plan, const int32_t *col, const float *other, const float *self,
                                   const float *gz, const float *att, float slope, int64_t H, int64_t C,
                                   const float *add, float *g_self, float *att_rows, void *stream) {
  using namespace ggl;
  WalkPlan p;
  if (int rc = walk_plan(plan, "plan", "plan is NULL", "H, C and chunk must be positive",
                         ggl_gatv2_logit_bwd_partial_bytes(hub_chunks(plan), H, C, att_rows != nullptr), p))
    return rc;
  GGL_REQUIRE(H > 0 && C > 0, GGL_EINVAL, "H, C and chunk must be positive");
  const int64_t N = p.N;
  if (N == 0) return GGL_OK;
  GGL_REQUIRE(self && att && g_self, GGL_EINVAL, "NULL pointer");
  GGL_REQUIRE((col && other && gz) || p.E == 0, GGL_EINVAL, "NULL pointer");
  GatDims d{};
  d.slope = slope; d.N = N; d.H = H; d.C = C; d.K = H * C; d.E = p.E;
  d.chunk = p.chunk; d.n_long = p.n_long; d.n_chunks = p.n_chunks;
  float *pD = p.partial, *pA = nullptr;
  if (p.n_long > 0) {
    pA = pD + p.n_chunks * d.K;
    d.chunk_blocks = ceil_div(p.n_chunks, kWavesPerBlock);
  }
  const bool vec4 = (C % 4 == 0) && gat_aligned<float>(other, 4) && gat_aligned<float>(self, 4) &&
                    gat_aligned<float>(att, 4) && gat_aligned<float>(add, 4) && gat_aligned<float>(g_self, 4) &&
                    gat_aligned<float>(att_rows, 4) && gat_aligned<float>(pD, 4) && !options().force_generic;
  d.logL = pow2_log2(ceil_div(d.K, vec4 ? 4 : 1));
  d.nblocks = ceil_div(N, (int64_t)kWavesPerBlock * (kWave >> d.logL));
  const int64_t grid = d.chunk_blocks + d.nblocks;
  GGL_REQUIRE(grid < ((int64_t)1 << 31), GGL_EINVAL, "too many rows for one launch");
  hipStream_t s = as_stream(stream);
#define GGL_GATV2_BWD(V, AT)                                                                                        \
  GGL_LAUNCH((gatv2_logit_bwd_kernel<V, AT>), grid, kBlock, s, plan->rowptr, col, plan->perm, p.order, plan->long_rows, \
             plan->chunk_ptr, other, self, gz, att, add, g_self, att_rows, pD, pA, d)
  if (vec4 && att_rows) GGL_GATV2_BWD(4, true);
  else if (vec4) GGL_GATV2_BWD(4, false);
  else if (att_rows) GGL_GATV2_BWD(1, true);
  else GGL_GATV2_BWD(1, false);
#undef GGL_GATV2_BWD
  GGL_LAUNCH_CHECK();
  if (p.n_long > 0) {
    if (att_rows)
      GGL_LAUNCH((gatv2_logit_bwd_final_kernel<true>), p.n_long, kBlock, s, plan->long_rows, plan->chunk_ptr,
                 (const float *)pD, (const float *)pA, att, add, g_self, att_rows, d);
    else
      GGL_LAUNCH((gatv2_logit_bwd_final_kernel<false>), p.n_long, kBlock, s, plan->long_rows, plan->chunk_ptr,
                 (const float *)pD, (const float *)pA, att, add, g_self, att_rows, d);
    GGL_LAUNCH_CHECK();
  }
  return GGL_OK;
}
