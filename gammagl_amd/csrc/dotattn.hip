// gammagl_amd/csrc/dotattn.hip — fused scaled dot-product graph attention, forward, GPU build only.
//
//   z[e,h]     = scale * <q[dst(e),h,:], k[src(e),h,:]>
//   out[i,h,:] = sum_{e -> i} drop(softmax_i(z[:,h]))[e] * v[src(e),h,:]
// (hgt_conv.py:115-153: reduce_sum(k_j * q_i, -1) -> segment_softmax -> v_j * alpha, and every graph-transformer layer.)
// Composed from the library's ops that is an edge-dot walk (ggl_bspmm_grad_w*) that writes z [E, H] and the edge-softmax
// aggregate (ggl_edge_softmax_agg_fwd) that reads it back through perm: two passes over col.  Here the dot is formed inside
// the aggregate's walk, so col is read once, k and v rows of an edge are requested together, and z is stored only when the
// caller wants it (a backward will read it) — in inference no [E, H] array exists.
//
// Everything behind the logit is gat_fwd_kernel's code (gat.hip): lane layout (2^logL lanes per short row, one wavefront
// per hub chunk, a lane owns VEC = 4 channels of one head), the online softmax of gat_online statement by statement, the
// same dropout word, the same partial layout merged by gat_long_final_kernel.  So out / rowmax / rowden are
// ggl_edge_softmax_agg_fwd's bits on the z stored here.
//
// The dot: the g = C / 4 lanes of a head each multiply their four q and k values (q sits in registers for the whole row,
// channels ascending, __fmul_rn / __fadd_rn) and the partial sums are added across the group with a BUTTERFLY of wave
// shuffles: step o adds lane l's and lane l ^ o's value — the same pair in either order, and a + b == b + a in IEEE
// arithmetic — so after log2(g) steps EVERY lane of the group holds the SAME bits.  The per-lane copies of (m, den), which
// the lanes of a head keep redundantly as in gat_online, therefore stay in step and no broadcast is needed.  (A reduction
// to one lane followed by a broadcast would do as well; a reduction that leaves different roundings in different lanes
// would let the copies of m drift apart and split a head's channels over different reference points.)
// This order differs from the composed route's (edgedot.hip sums the C channels serially), hence z carries an error bound,
// |z - z64| <= gamma_{C+1} |scale| sum_c |q_c k_c|, not the other route's bits.
//
// Shuffle partners: the group of lane l is the aligned block of g lanes around it, g a power of two <= 2^logL, so all its
// lanes belong to the same row (or chunk) and the same head, see the same [beg, end) and the same kk < K test (K = H * C is
// a multiple of 4 g): they run the same trip counts and are active together; a lane with kk >= K never runs a shuffle.
#include "gat_common.hpp"

namespace ggl {

template <int LOGG> __device__ __forceinline__ float dot_group_sum(float s) {
#pragma unroll
  for (int o = (1 << LOGG) >> 1; o > 0; o >>= 1) s = __fadd_rn(s, __shfl_xor(s, o, kWave));
  return s;
}

// gat_online with the logit formed in place.  qv: the lane's four q values of (row, head); first: the head's first lane
// (stores z).  ZOUT = false: no perm load, no store.
template <int LOGG, bool DROP, bool ZOUT>
__device__ __forceinline__ void dot_online(const int32_t *__restrict__ col, const int32_t *__restrict__ perm,
                                           const float (&qv)[4], const float *__restrict__ k,
                                           const float *__restrict__ v, float scale, int64_t H, int64_t K, int64_t h,
                                           int64_t kk, bool first, int64_t beg, int64_t end, const GatDims &d,
                                           const int64_t *__restrict__ rng, float *__restrict__ z_out, float &m,
                                           float &den, float (&acc)[4]) {
  m = -FLT_MAX;
  den = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = 0.0f;
  const uint64_t seed = DROP ? (uint64_t)rng[0] : 0, offset = DROP ? (uint64_t)rng[1] : 0;
  auto absorb = [&](uint32_t word, float s, const float (&x)[4]) {  // gat_online's, unchanged
    if (m < s) {
      const float sc = GGL_EXPF(__fadd_rn(m, -s));
      den = __fmul_rn(den, sc);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = __fmul_rn(acc[i], sc);
      m = s;
    }
    const float e = GGL_EXPF(__fadd_rn(s, -m));
    den = __fadd_rn(den, e);
    float ek = e;
    if (DROP) ek = (word >= d.drop_thresh) ? __fmul_rn(e, d.drop_scale) : 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = __fadd_rn(acc[i], __fmul_rn(x[i], ek));
  };
  auto logit = [&](const float (&kv)[4]) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s = __fadd_rn(s, __fmul_rn(qv[i], kv[i]));
    return __fmul_rn(scale, dot_group_sum<LOGG>(s));
  };
  using LP = Logit<kLogitEdge>;
  auto single = [&](int64_t p) {
    const int64_t c0 = col[p];
    const int64_t e0 = ZOUT ? LP::rec(perm, col, p, c0) : 0;
    float k0[4], v0[4];
    F32V<4>::load(k + c0 * K + kk, k0);
    F32V<4>::load(v + c0 * K + kk, v0);
    const float s = logit(k0);
    if (ZOUT && first) z_out[e0 * H + h] = s;
    absorb(DROP ? drop_word(p, H, h, offset, seed) : 0u, s, v0);
  };
  int64_t p = beg;
  if (DROP) {
    for (; p < end && (p & 3) != 0; ++p) single(p);
  }
  for (; p + 4 <= end; p += 4) {
    int64_t c[4], e[4];
    float kr[4][4], vr[4][4], s[4];
    U4 rw{0u, 0u, 0u, 0u};
    if (DROP) rw = drop_words4(p >> 2, H, h, offset, seed);
#pragma unroll
    for (int u = 0; u < 4; ++u) { c[u] = col[p + u]; e[u] = ZOUT ? LP::rec(perm, col, p + u, c[u]) : 0; }
#pragma unroll
    for (int u = 0; u < 4; ++u) F32V<4>::load(k + c[u] * K + kk, kr[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) F32V<4>::load(v + c[u] * K + kk, vr[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) s[u] = logit(kr[u]);
    if (ZOUT && first) {
#pragma unroll
      for (int u = 0; u < 4; ++u) z_out[e[u] * H + h] = s[u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) absorb(pick_word(rw, u), s[u], vr[u]);
  }
  for (; p < end; ++p) single(p);
}

// gat_fwd_kernel<float, float, 4, DROP, kLogitEdge> with dot_online in place of gat_online; C = 4 << LOGG.
template <int LOGG, bool DROP, bool ZOUT>
__global__ __launch_bounds__(kBlock) void dot_attn_fwd_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int32_t *__restrict__ row_order,
    const int32_t *__restrict__ long_rows, const int64_t *__restrict__ chunk_ptr, const int32_t *__restrict__ perm,
    const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v, float scale,
    float *__restrict__ y, float *__restrict__ rowmax, float *__restrict__ rowden, float *__restrict__ pacc,
    float *__restrict__ pm, float *__restrict__ pd, const int64_t *__restrict__ rng, float *__restrict__ z_out,
    const GatDims d) {
  constexpr int64_t C = (int64_t)4 << LOGG;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int64_t H = d.H, K = d.K;
  if (block_id() < d.chunk_blocks) {  // one wavefront per chunk of a long row
    const int64_t cid = block_id() * kWavesPerBlock + wave;
    if (cid >= d.n_chunks) return;
    int64_t lo = 0, hi = d.n_long - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (chunk_ptr[mid] <= cid) lo = mid; else hi = mid - 1;
    }
    const int64_t row = long_rows[lo];
    const int64_t beg = rowptr[row] + (cid - chunk_ptr[lo]) * d.chunk;
    const int64_t rend = rowptr[row + 1];
    const int64_t end = (beg + d.chunk < rend) ? beg + d.chunk : rend;
    for (int64_t kk = (int64_t)lane * 4; kk < K; kk += (int64_t)kWave * 4) {  // whole heads per pass: 256 % C == 0
      const int64_t h = kk / C;
      float qv[4], m, dsum, acc[4];
      F32V<4>::load(q + row * K + kk, qv);
      dot_online<LOGG, DROP, ZOUT>(col, perm, qv, k, v, scale, H, K, h, kk, kk == h * C, beg, end, d, rng, z_out, m,
                                   dsum, acc);
      F32V<4>::store(pacc + cid * K + kk, acc);
      if (kk == h * C) {
        pm[cid * H + h] = m;
        pd[cid * H + h] = dsum;
      }
    }
    return;
  }
  const int L = 1 << d.logL;
  const int64_t slot = ((block_id() - d.chunk_blocks) * kWavesPerBlock + wave) * (kWave >> d.logL) + (lane >> d.logL);
  if (slot >= d.N) return;
  const int64_t row = row_order ? (int64_t)row_order[slot] : slot;
  const int li = lane & (L - 1);
  const int64_t beg = rowptr[row], end = rowptr[row + 1];
  if (end - beg > d.chunk) return;
  for (int64_t kk = (int64_t)li * 4; kk < K; kk += (int64_t)L * 4) {  // L < 64 only when one pass covers K
    const int64_t h = kk / C;
    float qv[4], m, dsum, acc[4];
    F32V<4>::load(q + row * K + kk, qv);
    dot_online<LOGG, DROP, ZOUT>(col, perm, qv, k, v, scale, H, K, h, kk, kk == h * C, beg, end, d, rng, z_out, m, dsum,
                                 acc);
    const float inv = __fadd_rn(dsum, 1e-16f);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = __fdiv_rn(acc[i], inv);
    F32V<4>::store(y + row * K + kk, acc);
    if (kk == h * C) {
      rowmax[row * H + h] = m;
      rowden[row * H + h] = dsum;
    }
  }
}

}  // namespace ggl

using namespace ggl;

// C = 4 g with g = 2, 4, 8 or 16 lanes per head, any H: the shapes instantiated and tested
extern "C" int ggl_dot_attn_supported(int64_t H, int64_t C) {
  return (H > 0 && (C == 8 || C == 16 || C == 32 || C == 64)) ? 1 : 0;
}

// Whether the fused forward is the default for a supported shape.  The rule: it is, unless it was measured slower than the
// composed route (sorted edge dot + ggl_edge_softmax_agg_fwd) by more than the run-to-run spread.  profiles/dot_attention.txt:
// 1 x 64, 8 x 8 and 4 x 32 on the Reddit- and products-sized graphs are 1.5-2.1x FASTER fused (spread below 2 %), so no
// shape is excluded; C = 16 was not timed.
extern "C" int ggl_policy_dot_attn_fused(int64_t H, int64_t C, int64_t E, int64_t N_in) {
  (void)E; (void)N_in;
  return ggl_dot_attn_supported(H, C);
}

extern "C" int ggl_dot_attn_fwd(const ggl_segplan_t *plan, const int32_t *col, const float *q, const float *k,
                                const float *v, float scale, int64_t H, int64_t C, float p_drop, int64_t *rng_state,
                                float *out, float *rowmax, float *rowden, float *z_out, void *stream) {
  WalkPlan p;
  if (int rc = walk_plan(plan, "plan", "plan is NULL", "H, C and chunk must be positive", p)) return rc;
  GGL_REQUIRE(H > 0 && C > 0, GGL_EINVAL, "H, C and chunk must be positive");
  GGL_REQUIRE(ggl_dot_attn_supported(H, C), GGL_EINVAL, "ggl_dot_attn_fwd: C must be 8, 16, 32 or 64 (ggl_dot_attn_supported)");
  const int64_t N = p.N;
  if (N == 0) return GGL_OK;
  GGL_REQUIRE(q && out && rowmax && rowden, GGL_EINVAL, "NULL pointer");
  GGL_REQUIRE((col && k && v) || p.E == 0, GGL_EINVAL, "NULL pointer");
  GatDims d{};
  d.slope = 1.0f; d.N = N; d.H = H; d.C = C; d.K = H * C; d.E = p.E;
  d.chunk = p.chunk; d.n_long = p.n_long; d.n_chunks = p.n_chunks;
  if (int rc = set_dropout(d, p_drop, rng_state)) return rc;
  float *pacc = p.partial, *pm = nullptr, *pd = nullptr;
  if (p.n_long > 0) {
    pm = pacc + p.n_chunks * d.K;
    pd = pm + p.n_chunks * H;
    d.chunk_blocks = ceil_div(p.n_chunks, kWavesPerBlock);
  }
  GGL_REQUIRE(gat_aligned<float>(q, 4) && gat_aligned<float>(k, 4) && gat_aligned<float>(v, 4) &&
                  gat_aligned<float>(out, 4) && gat_aligned<float>(pacc, 4),
              GGL_EINVAL, "ggl_dot_attn_fwd: q, k, v, out and plan->partial must be 16-byte aligned");
  d.logL = pow2_log2(d.K / 4);  // >= log2(C / 4): a head's lane group never straddles two rows
  d.nblocks = ceil_div(N, (int64_t)kWavesPerBlock * (kWave >> d.logL));
  const int64_t grid = d.chunk_blocks + d.nblocks;
  GGL_REQUIRE(grid < ((int64_t)1 << 31), GGL_EINVAL, "too many rows for one launch");
  hipStream_t s = as_stream(stream);
  const int32_t *perm = plan->perm;
#define GGL_DOT_FWD(LG, DR, ZO)                                                                                    \
  GGL_LAUNCH((dot_attn_fwd_kernel<LG, DR, ZO>), grid, kBlock, s, plan->rowptr, col, p.order, plan->long_rows,       \
             plan->chunk_ptr, perm, q, k, v, scale, out, rowmax, rowden, pacc, pm, pd, (const int64_t *)rng_state, \
             z_out, d)
#define GGL_DOT_FWD_C(LG)                                    \
  do {                                                       \
    if (d.drop_thresh && z_out) GGL_DOT_FWD(LG, true, true); \
    else if (d.drop_thresh) GGL_DOT_FWD(LG, true, false);    \
    else if (z_out) GGL_DOT_FWD(LG, false, true);            \
    else GGL_DOT_FWD(LG, false, false);                      \
  } while (0)
  if (C == 8) GGL_DOT_FWD_C(1);
  else if (C == 16) GGL_DOT_FWD_C(2);
  else if (C == 32) GGL_DOT_FWD_C(3);
  else GGL_DOT_FWD_C(4);
#undef GGL_DOT_FWD_C
#undef GGL_DOT_FWD
  GGL_LAUNCH_CHECK();
  if (plan->n_long > 0) {
    GGL_LAUNCH((gat_long_final_kernel), plan->n_long, kBlock, s, plan->long_rows, plan->chunk_ptr, (const float *)pacc,
               (const float *)pm, (const float *)pd, out, rowmax, rowden, d);
    GGL_LAUNCH_CHECK();
  }
  if (d.drop_thresh) return rng_advance(rng_state, stream);
  return GGL_OK;
}
