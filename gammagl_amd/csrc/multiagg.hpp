// gammagl_amd/csrc/multiagg.hpp — several statistics of the same message rows in ONE row walk: ggl_segment_multi_fwd / _bwd.
// Included by reduce.hip alone (no lane talks to another: the host builds compile it too).
//
// PNA (pna_conv.py:159-201) wants mean, min, max and std of one [E, K] message tensor per destination; composed from the
// segment ops that is four to five walks that each gather the same rows through perm, plus an [E, K] tensor of squares.
// Here a lane keeps its columns' running sum, sum of squares, minimum, maximum and both witnesses in registers and reads
// every message row once.
//
// FORWARD.  out [N, K / C, A, C]: column k of statistic number a (the order of `aggs`) lands at (k / C) * A * C + a * C + k % C.
// For row i with n elements, per column, positions p ascending in [rowptr[i], rowptr[i+1]), e = perm ? perm[p] : p,
// v = x[e, k]; every step one rounded f32 operation, never contracted:
//   S = __fadd_rn(S, v)                         from 0.0f
//   Q = __fadd_rn(Q, __fmul_rn(v, v))           from 0.0f
//   if (mx < v) { mx = v; amax = e; }           from -FLT_MAX, E      (strict <: the first element wins ties, NaN never wins)
//   if (v < mn) { mn = v; amin = e; }           from +FLT_MAX, E
//   nf   = (float)min(n, 2^24)                  (TT<float>::count: ggl_segment_mean's divisor)
//   mean = n > 1 ? __fdiv_rn(S, nf) : S;   msq = n > 1 ? __fdiv_rn(Q, nf) : Q
//   var  = __fsub_rn(msq, __fmul_rn(mean, mean))
//   std  = sqrtf(__fadd_rn(fmaxf(var, 0.0f), 1e-5f))                 (correctly rounded; pna_conv.py:174-178, cancellation included)
// An empty row: sum = mean = var = 0, std = sqrt(1e-5f), min / max their start values — or 0.0f with empty_zero — and
// witnesses E.  Only the accumulators the requested aggs need exist (SUM, SQ, MN, MX are template parameters).
// A row of more than plan->chunk positions is cut into pieces of `chunk` positions (gat_bwd_src_kernel's rule); each piece
// is reduced from the start values by its own wavefront into a partial (S, Q, mn, mx, amin, amax) — the panels the aggs
// need, [n_chunks, K] each, in that order — and multi_merge_kernel combines a row's partials in ascending piece order:
// sums restart from 0.0f (tot = __fadd_rn(tot, part)), min / max compare with the same strict rule, so the earliest piece
// keeps ties.  The serial hub pipeline of hubf32.hip is not used.
//
// BACKWARD.  One walk, no reduction: no partials, no merge.  g [N, A * K] in out's layout.  Per (row, column), once, with
// n' = max(n, 1), nf = (float)min(n', 2^24), s0 = sqrtf(1e-5f):
//   gv = g_var                                                        (0.0f without var)
//   with std:  t = std > s0 ? __fdiv_rn(g_std, __fmul_rn(2.0f, std)) : 0.0f;   gv = var requested ? __fadd_rn(gv, t) : t
//   c1 = __fdiv_rn(__fmul_rn(2.0f, gv), nf)
//   c0 = 0.0f;  sum: c0 = __fadd_rn(c0, g_sum);  mean: c0 = __fadd_rn(c0, __fdiv_rn(g_mean, nf));
//               var or std: c0 = __fsub_rn(c0, __fmul_rn(c1, mean))
// "var > 0" is re-derived from the stored std as std > s0 (var is not stored): sqrt is monotone, so var == 0 gives exactly
// s0 and no gradient through std, and a one-element row (x == mean) gets none either way.
// Then for each position p of the row, e = perm ? perm[p] : p:
//   t = var or std ? __fadd_rn(c0, __fmul_rn(c1, x[e, k])) : c0
//   if (argmax[i, k] == e) t = __fadd_rn(t, g_max);   if (argmin[i, k] == e) t = __fadd_rn(t, g_min);   gx[e, k] = t
// Every element of gx [E, K] is written (each e lies in exactly one row).  x is read only with var / std, the witnesses only
// with min / max, mean only with var / std, out only with std.  A hub row's pieces each recompute the coefficients.
//
// A lane owns VEC columns: 4 with 16-byte accesses where C % 4 == 0 and every pointer is 16-byte aligned (its four columns
// never straddle a group), 1 otherwise; no result depends on VEC.
#pragma once

namespace ggl {

// sqrtf, not __fsqrt_rn: HIP's __fsqrt_rn is the native v_sqrt_f32 (1 ulp) unless OCML_BASIC_ROUNDED_OPERATIONS is defined,
// while sqrtf is lowered correctly rounded (measured on the MI355X: __fsqrt_rn was one ulp off the host's result for 24 of
// 192 values).  The subtraction is a plain rounded one on both builds (-ffp-contract=off: never contracted).
__device__ __forceinline__ float multi_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ float multi_sub(float a, float b) { return a - b; }

struct MultiDims {
  int64_t N, K, E, C;
  int64_t chunk, n_long, n_chunks, chunk_blocks, nblocks;
  int logL, swizzle;
  int A;
  int codes[6];      // the aggs, in output order
  int at[6];         // at[code] = position of that statistic in aggs, or -1
  int empty_zero;
};

// the partial panels of a plan with long rows, [n_chunks, K] each, in the order S, Q, mn, mx, amin, amax
struct MultiPart {
  float *S, *Q, *mn, *mx;
  int32_t *amin, *amax;
};

template <int VEC> struct MultiAcc {
  float S[VEC], Q[VEC], mn[VEC], mx[VEC];
  int32_t amin[VEC], amax[VEC];
};

template <int VEC, bool SUM, bool SQ, bool MN, bool MX>
__device__ __forceinline__ void multi_init(MultiAcc<VEC> &a, int32_t fill) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    if (SUM) a.S[i] = 0.0f;
    if (SQ) a.Q[i] = 0.0f;
    if (MN) { a.mn[i] = FLT_MAX; a.amin[i] = fill; }
    if (MX) { a.mx[i] = -FLT_MAX; a.amax[i] = fill; }
  }
}

template <int VEC, bool SUM, bool SQ, bool MN, bool MX>
__device__ __forceinline__ void multi_absorb(MultiAcc<VEC> &a, const float (&v)[VEC], int32_t e) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    if (SUM) a.S[i] = __fadd_rn(a.S[i], v[i]);
    if (SQ) a.Q[i] = __fadd_rn(a.Q[i], __fmul_rn(v[i], v[i]));
    if (MX) {
      if (a.mx[i] < v[i]) { a.mx[i] = v[i]; a.amax[i] = e; }
    }
    if (MN) {
      if (v[i] < a.mn[i]) { a.mn[i] = v[i]; a.amin[i] = e; }
    }
  }
}

// positions [beg, end) of one row for the VEC columns from kk on: U positions' indices first, then their rows, then the adds
template <int VEC, bool SUM, bool SQ, bool MN, bool MX, bool PERM, int U>
__device__ __forceinline__ void multi_walk(const float *__restrict__ x, const int32_t *__restrict__ perm, int64_t K,
                                           int64_t kk, int64_t beg, int64_t end, MultiAcc<VEC> &a) {
  int64_t p = beg;
  for (; p + U <= end; p += U) {
    int32_t e[U];
    float v[U][VEC];
#pragma unroll
    for (int u = 0; u < U; ++u) e[u] = PERM ? perm[p + u] : (int32_t)(p + u);
#pragma unroll
    for (int u = 0; u < U; ++u) VecIO<float, VEC>::load(x + (int64_t)e[u] * K + kk, v[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) multi_absorb<VEC, SUM, SQ, MN, MX>(a, v[u], e[u]);
  }
  const int rem = (int)(end - p);   // < U: the loads issued together, consumed in order
  if (rem > 0) {
    int32_t e[U];
    float v[U][VEC];
#pragma unroll
    for (int u = 0; u < U - 1; ++u)
      if (u < rem) e[u] = PERM ? perm[p + u] : (int32_t)(p + u);
#pragma unroll
    for (int u = 0; u < U - 1; ++u)
      if (u < rem) VecIO<float, VEC>::load(x + (int64_t)e[u] * K + kk, v[u]);
#pragma unroll
    for (int u = 0; u < U - 1; ++u)
      if (u < rem) multi_absorb<VEC, SUM, SQ, MN, MX>(a, v[u], e[u]);
  }
}

// the statistics of a finished (row, VEC columns) and their stores
template <int VEC, bool SUM, bool SQ, bool MN, bool MX>
__device__ __forceinline__ void multi_finish(const MultiDims &d, int64_t row, int64_t n, int64_t kk, const MultiAcc<VEC> &a,
                                             float *__restrict__ out, float *__restrict__ mean_out,
                                             int32_t *__restrict__ argmin, int32_t *__restrict__ argmax) {
  float mean[VEC], var[VEC], sd[VEC], mn[VEC], mx[VEC];
  const float nf = TT<float>::count(n);
  const bool div = TT<float>::gt1(nf);
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    if (SUM) mean[i] = div ? __fdiv_rn(a.S[i], nf) : a.S[i];
    if (SQ) {
      const float msq = div ? __fdiv_rn(a.Q[i], nf) : a.Q[i];
      var[i] = multi_sub(msq, __fmul_rn(mean[i], mean[i]));
      sd[i] = multi_sqrt(__fadd_rn(fmaxf(var[i], 0.0f), 1e-5f));
    }
    if (MN) mn[i] = (n == 0 && d.empty_zero) ? 0.0f : a.mn[i];
    if (MX) mx[i] = (n == 0 && d.empty_zero) ? 0.0f : a.mx[i];
  }
  float *o = out + row * (d.A * d.K) + (kk / d.C) * (d.A * d.C) + kk % d.C;
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    if (s >= d.A) break;
    const int code = d.codes[s];
    float *os = o + (int64_t)s * d.C;
    if (SUM && code == GGL_AGG_SUM) VecIO<float, VEC>::store(os, a.S);
    if (SUM && code == GGL_AGG_MEAN) VecIO<float, VEC>::store(os, mean);
    if (MN && code == GGL_AGG_MIN) VecIO<float, VEC>::store(os, mn);
    if (MX && code == GGL_AGG_MAX) VecIO<float, VEC>::store(os, mx);
    if (SQ && code == GGL_AGG_VAR) VecIO<float, VEC>::store(os, var);
    if (SQ && code == GGL_AGG_STD) VecIO<float, VEC>::store(os, sd);
  }
  if (SUM && mean_out) VecIO<float, VEC>::store(mean_out + row * d.K + kk, mean);
  if (MN && argmin) VecIO<int32_t, VEC>::store(argmin + row * d.K + kk, a.amin);
  if (MX && argmax) VecIO<int32_t, VEC>::store(argmax + row * d.K + kk, a.amax);
}

template <int VEC, bool SUM, bool SQ, bool MN, bool MX, bool PERM, int U>
__global__ __launch_bounds__(kBlock) void multi_fwd_kernel(const float *__restrict__ x, const int32_t *__restrict__ perm,
                                                           const int64_t *__restrict__ rowptr,
                                                           const int32_t *__restrict__ row_order,
                                                           const int32_t *__restrict__ long_rows,
                                                           const int64_t *__restrict__ chunk_ptr, const MultiPart part,
                                                           float *__restrict__ out, float *__restrict__ mean_out,
                                                           int32_t *__restrict__ argmin, int32_t *__restrict__ argmax,
                                                           const MultiDims d) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int64_t K = d.K;
  if (block_id() < d.chunk_blocks) {   // one wavefront per piece of a long row; chunk blocks lead the grid
    const int64_t cid = block_id() * kWavesPerBlock + wave;
    if (cid >= d.n_chunks) return;
    const HubChunk hc = hub_chunk(rowptr, long_rows, chunk_ptr, d.n_long, d.chunk, cid);
    for (int64_t kk = (int64_t)lane * VEC; kk < K; kk += (int64_t)kWave * VEC) {
      MultiAcc<VEC> a;
      multi_init<VEC, SUM, SQ, MN, MX>(a, (int32_t)d.E);
      multi_walk<VEC, SUM, SQ, MN, MX, PERM, U>(x, perm, K, kk, hc.beg, hc.end, a);
      const int64_t at = cid * K + kk;
      if (SUM) VecIO<float, VEC>::store(part.S + at, a.S);
      if (SQ) VecIO<float, VEC>::store(part.Q + at, a.Q);
      if (MN) { VecIO<float, VEC>::store(part.mn + at, a.mn); VecIO<int32_t, VEC>::store(part.amin + at, a.amin); }
      if (MX) { VecIO<float, VEC>::store(part.mx + at, a.mx); VecIO<int32_t, VEC>::store(part.amax + at, a.amax); }
    }
    return;
  }
  if (block_id() - d.chunk_blocks >= d.nblocks) return;   // padding blocks of a folded (2-D) grid
  const int64_t blk = xcd_remap(block_id() - d.chunk_blocks, d.nblocks, d.swizzle);
  const int L = 1 << d.logL;
  const int64_t slot = (blk * kWavesPerBlock + wave) * (kWave >> d.logL) + (lane >> d.logL);
  if (slot >= d.N) return;
  const int64_t row = row_order ? (int64_t)row_order[slot] : slot;
  const int li = lane & (L - 1);
  const int64_t beg = rowptr[row], end = rowptr[row + 1];
  if (end - beg > d.chunk) return;   // long row: the chunk blocks above + multi_merge_kernel
  for (int64_t kk = (int64_t)li * VEC; kk < K; kk += (int64_t)L * VEC) {
    MultiAcc<VEC> a;
    multi_init<VEC, SUM, SQ, MN, MX>(a, (int32_t)d.E);
    multi_walk<VEC, SUM, SQ, MN, MX, PERM, U>(x, perm, K, kk, beg, end, a);
    multi_finish<VEC, SUM, SQ, MN, MX>(d, row, end - beg, kk, a, out, mean_out, argmin, argmax);
  }
}

// long rows: a row's partials combined in ascending piece order, then the statistics
template <bool SUM, bool SQ, bool MN, bool MX>
__global__ __launch_bounds__(kBlock) void multi_merge_kernel(const int64_t *__restrict__ rowptr,
                                                             const int32_t *__restrict__ long_rows,
                                                             const int64_t *__restrict__ chunk_ptr, const MultiPart part,
                                                             float *__restrict__ out, float *__restrict__ mean_out,
                                                             int32_t *__restrict__ argmin, int32_t *__restrict__ argmax,
                                                             const MultiDims d) {
  const int64_t j = block_id();
  if (j >= d.n_long) return;
  const int64_t row = long_rows[j];
  const int64_t c0 = chunk_ptr[j], c1 = chunk_ptr[j + 1];
  for (int64_t k = threadIdx.x; k < d.K; k += kBlock) {
    MultiAcc<1> a;
    multi_init<1, SUM, SQ, MN, MX>(a, (int32_t)d.E);
    for (int64_t c = c0; c < c1; ++c) {
      const int64_t at = c * d.K + k;
      if (SUM) a.S[0] = __fadd_rn(a.S[0], part.S[at]);
      if (SQ) a.Q[0] = __fadd_rn(a.Q[0], part.Q[at]);
      if (MX) {
        const float v = part.mx[at];
        if (a.mx[0] < v) { a.mx[0] = v; a.amax[0] = part.amax[at]; }
      }
      if (MN) {
        const float v = part.mn[at];
        if (v < a.mn[0]) { a.mn[0] = v; a.amin[0] = part.amin[at]; }
      }
    }
    multi_finish<1, SUM, SQ, MN, MX>(d, row, rowptr[row + 1] - rowptr[row], k, a, out, mean_out, argmin, argmax);
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------
template <int VEC> struct MultiCoef {
  float c0[VEC], c1[VEC], gmx[VEC], gmn[VEC];
  int32_t amin[VEC], amax[VEC];
};

template <int VEC, bool SQ, bool MN, bool MX>
__device__ __forceinline__ void multi_coef(const MultiDims &d, int64_t row, int64_t n, int64_t kk,
                                           const float *__restrict__ g, const float *__restrict__ out,
                                           const float *__restrict__ mean, const int32_t *__restrict__ argmin,
                                           const int32_t *__restrict__ argmax, MultiCoef<VEC> &c) {
  const int64_t base = row * (d.A * d.K) + (kk / d.C) * (d.A * d.C) + kk % d.C;
  const float nf = TT<float>::count(n > 1 ? n : 1);
  float gs[VEC], gm[VEC], gvar[VEC], gstd[VEC], sd[VEC], mu[VEC];
  if (d.at[GGL_AGG_SUM] >= 0) VecIO<float, VEC>::load(g + base + d.at[GGL_AGG_SUM] * d.C, gs);
  if (d.at[GGL_AGG_MEAN] >= 0) VecIO<float, VEC>::load(g + base + d.at[GGL_AGG_MEAN] * d.C, gm);
  if (SQ && d.at[GGL_AGG_VAR] >= 0) VecIO<float, VEC>::load(g + base + d.at[GGL_AGG_VAR] * d.C, gvar);
  if (SQ && d.at[GGL_AGG_STD] >= 0) {
    VecIO<float, VEC>::load(g + base + d.at[GGL_AGG_STD] * d.C, gstd);
    VecIO<float, VEC>::load(out + base + d.at[GGL_AGG_STD] * d.C, sd);
  }
  if (SQ) VecIO<float, VEC>::load(mean + row * d.K + kk, mu);
  if (MX) {
    VecIO<float, VEC>::load(g + base + d.at[GGL_AGG_MAX] * d.C, c.gmx);
    VecIO<int32_t, VEC>::load(argmax + row * d.K + kk, c.amax);
  }
  if (MN) {
    VecIO<float, VEC>::load(g + base + d.at[GGL_AGG_MIN] * d.C, c.gmn);
    VecIO<int32_t, VEC>::load(argmin + row * d.K + kk, c.amin);
  }
  const float s0 = multi_sqrt(1e-5f);
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    float gv = 0.0f;
    if (SQ && d.at[GGL_AGG_VAR] >= 0) gv = gvar[i];
    if (SQ && d.at[GGL_AGG_STD] >= 0) {
      const float t = sd[i] > s0 ? __fdiv_rn(gstd[i], __fmul_rn(2.0f, sd[i])) : 0.0f;
      gv = d.at[GGL_AGG_VAR] >= 0 ? __fadd_rn(gv, t) : t;
    }
    c.c1[i] = SQ ? __fdiv_rn(__fmul_rn(2.0f, gv), nf) : 0.0f;
    float c0 = 0.0f;
    if (d.at[GGL_AGG_SUM] >= 0) c0 = __fadd_rn(c0, gs[i]);
    if (d.at[GGL_AGG_MEAN] >= 0) c0 = __fadd_rn(c0, __fdiv_rn(gm[i], nf));
    if (SQ) c0 = multi_sub(c0, __fmul_rn(c.c1[i], mu[i]));
    c.c0[i] = c0;
  }
}

template <int VEC, bool SQ, bool MN, bool MX, bool PERM>
__device__ __forceinline__ void multi_bwd_walk(const float *__restrict__ x, const int32_t *__restrict__ perm, int64_t K,
                                               int64_t kk, int64_t beg, int64_t end, const MultiCoef<VEC> &c,
                                               float *__restrict__ gx) {
  auto emit = [&](int32_t e, const float (&v)[VEC]) {
    float t[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      t[i] = SQ ? __fadd_rn(c.c0[i], __fmul_rn(c.c1[i], v[i])) : c.c0[i];
      if (MX) {
        if (c.amax[i] == e) t[i] = __fadd_rn(t[i], c.gmx[i]);
      }
      if (MN) {
        if (c.amin[i] == e) t[i] = __fadd_rn(t[i], c.gmn[i]);
      }
    }
    VecIO<float, VEC>::store(gx + (int64_t)e * K + kk, t);
  };
  int64_t p = beg;
  for (; p + 4 <= end; p += 4) {
    int32_t e[4];
    float v[4][VEC];
#pragma unroll
    for (int u = 0; u < 4; ++u) e[u] = PERM ? perm[p + u] : (int32_t)(p + u);
    if (SQ) {
#pragma unroll
      for (int u = 0; u < 4; ++u) VecIO<float, VEC>::load(x + (int64_t)e[u] * K + kk, v[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) emit(e[u], v[u]);
  }
  for (; p < end; ++p) {
    const int32_t e = PERM ? perm[p] : (int32_t)p;
    float v[VEC];
    if (SQ) VecIO<float, VEC>::load(x + (int64_t)e * K + kk, v);
    emit(e, v);
  }
}

template <int VEC, bool SQ, bool MN, bool MX, bool PERM>
__global__ __launch_bounds__(kBlock) void multi_bwd_kernel(const float *__restrict__ g, const float *__restrict__ x,
                                                           const float *__restrict__ out, const float *__restrict__ mean,
                                                           const int32_t *__restrict__ argmin,
                                                           const int32_t *__restrict__ argmax,
                                                           const int32_t *__restrict__ perm,
                                                           const int64_t *__restrict__ rowptr,
                                                           const int32_t *__restrict__ row_order,
                                                           const int32_t *__restrict__ long_rows,
                                                           const int64_t *__restrict__ chunk_ptr, float *__restrict__ gx,
                                                           const MultiDims d) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int64_t K = d.K;
  if (block_id() < d.chunk_blocks) {   // a piece of a long row: its own coefficients, its own positions
    const int64_t cid = block_id() * kWavesPerBlock + wave;
    if (cid >= d.n_chunks) return;
    const HubChunk hc = hub_chunk(rowptr, long_rows, chunk_ptr, d.n_long, d.chunk, cid);
    const int64_t n = rowptr[hc.row + 1] - rowptr[hc.row];
    for (int64_t kk = (int64_t)lane * VEC; kk < K; kk += (int64_t)kWave * VEC) {
      MultiCoef<VEC> c;
      multi_coef<VEC, SQ, MN, MX>(d, hc.row, n, kk, g, out, mean, argmin, argmax, c);
      multi_bwd_walk<VEC, SQ, MN, MX, PERM>(x, perm, K, kk, hc.beg, hc.end, c, gx);
    }
    return;
  }
  if (block_id() - d.chunk_blocks >= d.nblocks) return;
  const int64_t blk = xcd_remap(block_id() - d.chunk_blocks, d.nblocks, d.swizzle);
  const int L = 1 << d.logL;
  const int64_t slot = (blk * kWavesPerBlock + wave) * (kWave >> d.logL) + (lane >> d.logL);
  if (slot >= d.N) return;
  const int64_t row = row_order ? (int64_t)row_order[slot] : slot;
  const int li = lane & (L - 1);
  const int64_t beg = rowptr[row], end = rowptr[row + 1];
  if (end - beg > d.chunk || end == beg) return;
  for (int64_t kk = (int64_t)li * VEC; kk < K; kk += (int64_t)L * VEC) {
    MultiCoef<VEC> c;
    multi_coef<VEC, SQ, MN, MX>(d, row, end - beg, kk, g, out, mean, argmin, argmax, c);
    multi_bwd_walk<VEC, SQ, MN, MX, PERM>(x, perm, K, kk, beg, end, c, gx);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
struct MultiNeed { bool sum, sq, mn, mx; };

// aggs -> dims (codes, at) and what the walk must carry; refuses unknown and duplicate codes
static int multi_parse(const int *aggs, int n_aggs, MultiDims &d, MultiNeed &need) {
  GGL_REQUIRE(aggs != nullptr, GGL_EINVAL, "segment_multi: aggs is NULL");
  GGL_REQUIRE(n_aggs >= 1 && n_aggs <= 6, GGL_EINVAL, "segment_multi: n_aggs must be in [1, 6], got %d", n_aggs);
  for (int c = 0; c < 6; ++c) d.at[c] = -1;
  for (int s = 0; s < 6; ++s) d.codes[s] = -1;
  for (int s = 0; s < n_aggs; ++s) {
    GGL_REQUIRE(aggs[s] >= GGL_AGG_SUM && aggs[s] <= GGL_AGG_STD, GGL_EINVAL, "segment_multi: unknown aggregate code %d", aggs[s]);
    GGL_REQUIRE(d.at[aggs[s]] < 0, GGL_EINVAL, "segment_multi: duplicate aggregate code %d", aggs[s]);
    d.at[aggs[s]] = s;
    d.codes[s] = aggs[s];
  }
  d.A = n_aggs;
  need.sq = d.at[GGL_AGG_VAR] >= 0 || d.at[GGL_AGG_STD] >= 0;
  need.sum = need.sq || d.at[GGL_AGG_SUM] >= 0 || d.at[GGL_AGG_MEAN] >= 0;
  need.mn = d.at[GGL_AGG_MIN] >= 0;
  need.mx = d.at[GGL_AGG_MAX] >= 0;
  return GGL_OK;
}

static int multi_plan(const ggl_segplan_t *plan, int64_t K, int64_t C, bool vec4, MultiDims &d) {
  GGL_REQUIRE(plan && plan->rowptr, GGL_EINVAL, "segment_multi: plan / rowptr is NULL");
  GGL_REQUIRE(plan->chunk > 0, GGL_EINVAL, "segment_multi: plan->chunk must be > 0");
  GGL_REQUIRE(K >= 0 && plan->N >= 0 && plan->E >= 0, GGL_EINVAL, "segment_multi: negative size");
  GGL_REQUIRE(C > 0 && (K % C) == 0, GGL_EINVAL, "segment_multi: C = %lld does not divide K = %lld", (long long)C, (long long)K);
  GGL_REQUIRE(plan->E < ((int64_t)1 << 31), GGL_EINVAL, "segment_multi: 2^31 or more elements in one plan");
  d.N = plan->N; d.K = K; d.E = plan->E; d.C = C;
  d.chunk = plan->chunk;
  d.n_long = plan->n_long > 0 ? plan->n_long : 0;
  d.n_chunks = d.n_long > 0 ? plan->n_chunks : 0;
  if (d.n_long > 0)
    GGL_REQUIRE(plan->long_rows && plan->chunk_ptr, GGL_EINVAL, "segment_multi: plan has long rows but long_rows / chunk_ptr is NULL");
  d.chunk_blocks = d.n_long > 0 ? ceil_div(d.n_chunks, kWavesPerBlock) : 0;
  const int64_t kv = ceil_div(K, vec4 ? 4 : 1);
  d.logL = pow2_ceil_log2(kv < kWave ? kv : kWave);
  d.nblocks = ceil_div(d.N, (int64_t)kWavesPerBlock * (kWave >> d.logL));
  d.swizzle = (int)options().xcd_swizzle;
  GGL_REQUIRE(d.chunk_blocks + d.nblocks < ((int64_t)1 << 31), GGL_EINVAL, "segment_multi: too many rows for one launch");
  return GGL_OK;
}

static int multi_panels(const MultiNeed &need) {
  return (need.sum ? 1 : 0) + (need.sq ? 1 : 0) + (need.mn ? 2 : 0) + (need.mx ? 2 : 0);
}

template <int VEC, bool SUM, bool SQ, bool MN, bool MX>
static int multi_fwd_launch(const float *x, const ggl_segplan_t *plan, const int32_t *order, const MultiPart &part, float *out,
                            float *mean_out, int32_t *argmin, int32_t *argmax, const MultiDims &d, hipStream_t s) {
  const int64_t grid = d.chunk_blocks + d.nblocks;
  // (the full set carries 16 accumulators + 8 witnesses per 4-column lane: U = 4 row registers beside them, see
  //  profiles/segment_multi.txt)
  if (plan->perm)
    GGL_LAUNCH((multi_fwd_kernel<VEC, SUM, SQ, MN, MX, true, 4>), grid, kBlock, s, x, plan->perm, plan->rowptr, order,
               plan->long_rows, plan->chunk_ptr, part, out, mean_out, argmin, argmax, d);
  else
    GGL_LAUNCH((multi_fwd_kernel<VEC, SUM, SQ, MN, MX, false, 4>), grid, kBlock, s, x, plan->perm, plan->rowptr, order,
               plan->long_rows, plan->chunk_ptr, part, out, mean_out, argmin, argmax, d);
  GGL_LAUNCH_CHECK();
  if (d.n_long > 0) {
    GGL_LAUNCH((multi_merge_kernel<SUM, SQ, MN, MX>), d.n_long, kBlock, s, plan->rowptr, plan->long_rows, plan->chunk_ptr, part,
               out, mean_out, argmin, argmax, d);
    GGL_LAUNCH_CHECK();
  }
  return GGL_OK;
}

template <int VEC, bool SQ, bool MN, bool MX>
static int multi_bwd_launch(const float *g, const float *x, const float *out, const float *mean, const int32_t *argmin,
                            const int32_t *argmax, const ggl_segplan_t *plan, const int32_t *order, float *gx,
                            const MultiDims &d, hipStream_t s) {
  const int64_t grid = d.chunk_blocks + d.nblocks;
  if (plan->perm)
    GGL_LAUNCH((multi_bwd_kernel<VEC, SQ, MN, MX, true>), grid, kBlock, s, g, x, out, mean, argmin, argmax, plan->perm,
               plan->rowptr, order, plan->long_rows, plan->chunk_ptr, gx, d);
  else
    GGL_LAUNCH((multi_bwd_kernel<VEC, SQ, MN, MX, false>), grid, kBlock, s, g, x, out, mean, argmin, argmax, plan->perm,
               plan->rowptr, order, plan->long_rows, plan->chunk_ptr, gx, d);
  GGL_LAUNCH_CHECK();
  return GGL_OK;
}

}  // namespace ggl

// plan->partial of ggl_segment_multi_fwd for a plan with long rows: one [n_chunks, K] panel of 4-byte words per carried
// quantity — S (any of sum / mean / var / std), Q (var / std), mn + amin (min), mx + amax (max)
extern "C" size_t ggl_segment_multi_partial_bytes(int64_t n_chunks, int64_t K, const int *aggs, int n_aggs) {
  using namespace ggl;
  MultiDims d{};
  MultiNeed need{};
  if (n_chunks <= 0 || K <= 0 || multi_parse(aggs, n_aggs, d, need)) return 0;
  return (size_t)n_chunks * (size_t)K * 4 * (size_t)multi_panels(need) + 64;
}

extern "C" int ggl_segment_multi_fwd(const float *x, const ggl_segplan_t *plan, int64_t K, int64_t C, const int *aggs,
                                     int n_aggs, int empty_zero, float *out, float *mean, int32_t *argmin, int32_t *argmax,
                                     void *stream) {
  using namespace ggl;
  MultiDims d{};
  MultiNeed need{};
  if (int rc = multi_parse(aggs, n_aggs, d, need)) return rc;
  const bool vec4 = !options().force_generic && C > 0 && (C % 4 == 0) && aligned16(x) && aligned16(out) && aligned16(mean) &&
                    aligned16(argmin) && aligned16(argmax) && (!plan || aligned16(plan->partial));
  if (int rc = multi_plan(plan, K, C, vec4, d)) return rc;
  d.empty_zero = empty_zero ? 1 : 0;
  if (d.N == 0 || K == 0) return GGL_OK;
  GGL_REQUIRE(out != nullptr, GGL_EINVAL, "segment_multi_fwd: out is NULL");
  GGL_REQUIRE(x != nullptr || d.E == 0, GGL_EINVAL, "segment_multi_fwd: x is NULL");
  GGL_REQUIRE(mean == nullptr || need.sum, GGL_EINVAL, "segment_multi_fwd: mean is given but no sum / mean / var / std is carried");
  MultiPart part{};
  if (d.n_long > 0) {
    GGL_REQUIRE(plan->partial != nullptr, GGL_EINVAL, "segment_multi_fwd: plan has long rows but plan->partial is NULL");
    if (int rc = partial_fits(plan, "plan", ggl_segment_multi_partial_bytes(d.n_chunks, K, aggs, n_aggs))) return rc;
    float *w = static_cast<float *>(plan->partial);
    const int64_t panel = d.n_chunks * K;
    if (need.sum) { part.S = w; w += panel; }
    if (need.sq) { part.Q = w; w += panel; }
    if (need.mn) { part.mn = w; w += panel; }
    if (need.mx) { part.mx = w; w += panel; }
    if (need.mn) { part.amin = reinterpret_cast<int32_t *>(w); w += panel; }
    if (need.mx) { part.amax = reinterpret_cast<int32_t *>(w); w += panel; }
  }
  const int32_t *order = options().row_order ? plan->row_order : nullptr;
  hipStream_t s = as_stream(stream);
#define GGL_MULTI_FWD(SUM, SQ, MN, MX)                                                                                   \
  return vec4 ? multi_fwd_launch<4, SUM, SQ, MN, MX>(x, plan, order, part, out, mean, argmin, argmax, d, s)              \
              : multi_fwd_launch<1, SUM, SQ, MN, MX>(x, plan, order, part, out, mean, argmin, argmax, d, s)
  const int key = (need.sum ? 1 : 0) | (need.sq ? 2 : 0) | (need.mn ? 4 : 0) | (need.mx ? 8 : 0);
  switch (key) {
    case 1: GGL_MULTI_FWD(true, false, false, false);
    case 3: GGL_MULTI_FWD(true, true, false, false);
    case 4: GGL_MULTI_FWD(false, false, true, false);
    case 5: GGL_MULTI_FWD(true, false, true, false);
    case 7: GGL_MULTI_FWD(true, true, true, false);
    case 8: GGL_MULTI_FWD(false, false, false, true);
    case 9: GGL_MULTI_FWD(true, false, false, true);
    case 11: GGL_MULTI_FWD(true, true, false, true);
    case 12: GGL_MULTI_FWD(false, false, true, true);
    case 13: GGL_MULTI_FWD(true, false, true, true);
    case 15: GGL_MULTI_FWD(true, true, true, true);
  }
#undef GGL_MULTI_FWD
  set_error("segment_multi_fwd: no kernel for this set of aggregates");
  return GGL_EINVAL;
}

extern "C" int ggl_segment_multi_bwd(const float *g, const float *x, const float *out, const float *mean,
                                     const int32_t *argmin, const int32_t *argmax, const ggl_segplan_t *plan, int64_t K,
                                     int64_t C, const int *aggs, int n_aggs, float *gx, void *stream) {
  using namespace ggl;
  MultiDims d{};
  MultiNeed need{};
  if (int rc = multi_parse(aggs, n_aggs, d, need)) return rc;
  const bool vec4 = !options().force_generic && C > 0 && (C % 4 == 0) && aligned16(g) && aligned16(gx) &&
                    (!need.sq || (aligned16(x) && aligned16(mean) && aligned16(out))) && (!need.mn || aligned16(argmin)) &&
                    (!need.mx || aligned16(argmax));
  if (int rc = multi_plan(plan, K, C, vec4, d)) return rc;
  if (d.E == 0 || K == 0) return GGL_OK;
  GGL_REQUIRE(g != nullptr, GGL_EINVAL, "segment_multi_bwd: g is NULL");
  GGL_REQUIRE(gx != nullptr, GGL_EINVAL, "segment_multi_bwd: gx is NULL");
  GGL_REQUIRE(!need.sq || x != nullptr, GGL_EINVAL, "segment_multi_bwd: x is NULL (var / std read it)");
  GGL_REQUIRE(!need.sq || mean != nullptr, GGL_EINVAL, "segment_multi_bwd: mean is NULL (var / std read it)");
  GGL_REQUIRE(d.at[GGL_AGG_STD] < 0 || out != nullptr, GGL_EINVAL, "segment_multi_bwd: out is NULL (std reads it)");
  GGL_REQUIRE(!need.mn || argmin != nullptr, GGL_EINVAL, "segment_multi_bwd: argmin is NULL (min reads it)");
  GGL_REQUIRE(!need.mx || argmax != nullptr, GGL_EINVAL, "segment_multi_bwd: argmax is NULL (max reads it)");
  const int32_t *order = options().row_order ? plan->row_order : nullptr;
  hipStream_t s = as_stream(stream);
#define GGL_MULTI_BWD(SQ, MN, MX)                                                                                 \
  return vec4 ? multi_bwd_launch<4, SQ, MN, MX>(g, x, out, mean, argmin, argmax, plan, order, gx, d, s)           \
              : multi_bwd_launch<1, SQ, MN, MX>(g, x, out, mean, argmin, argmax, plan, order, gx, d, s)
  switch ((need.sq ? 1 : 0) | (need.mn ? 2 : 0) | (need.mx ? 4 : 0)) {
    case 0: GGL_MULTI_BWD(false, false, false);
    case 1: GGL_MULTI_BWD(true, false, false);
    case 2: GGL_MULTI_BWD(false, true, false);
    case 3: GGL_MULTI_BWD(true, true, false);
    case 4: GGL_MULTI_BWD(false, false, true);
    case 5: GGL_MULTI_BWD(true, false, true);
    case 6: GGL_MULTI_BWD(false, true, true);
    default: GGL_MULTI_BWD(true, true, true);
  }
#undef GGL_MULTI_BWD
}
