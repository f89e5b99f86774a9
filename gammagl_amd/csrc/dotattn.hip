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
// Everything behind the logit is the shared forward walk (gat_common.hpp: gat_fwd_kernel<float, float, 4, DROP, LS> and
// gat_online), instantiated with the policy below: `el` is k, `x` is v, `slope` is scale.  So out / rowmax / rowden are
// ggl_edge_softmax_agg_fwd's bits on the z stored here by construction.
//
// The dot: the g = C / 4 lanes of a head each multiply their four q and k values (q sits in registers for the whole row,
// channels ascending, __fmul_rn / __fadd_rn) and the partial sums are added across the group with a BUTTERFLY of wave
// shuffles (group_sum), after which EVERY lane of the group holds the SAME bits.  The per-lane copies of (m, den), which
// the lanes of a head keep redundantly in gat_online, therefore stay in step and no broadcast is needed.  (A reduction
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

struct DotAux {
  const float *__restrict__ q;      // [N, H, C]
  const int32_t *__restrict__ perm;  // plan->perm or NULL
  float *__restrict__ z;             // [E, H] in the caller's edge order; not touched unless ZOUT
};
struct F4 { float v[4]; };
// C = 4 << LOGG.  ZOUT = false: no perm load, no z store.
template <int LOGG, bool ZOUT> struct DotLogit {
  using Aux = DotAux;
  using Row = F4;   // the lane's four q values of (row, head)
  using Opnd = F4;  // ... and of k[col[p], head]
  static constexpr int64_t kC = (int64_t)4 << LOGG;
  static __device__ __forceinline__ F4 row(const Aux &a, int64_t, int64_t i, int64_t K, int64_t kk) {
    return load(a.q, 0, i * K + kk);
  }
  static __device__ __forceinline__ int64_t rec(const Aux &a, const int32_t *__restrict__ col, int64_t p, int64_t c) {
    return ZOUT ? Logit<kLogitEdge>::rec(a.perm, col, p, c) : 0;
  }
  static __device__ __forceinline__ F4 load(const float *__restrict__ k, int64_t, int64_t ck) {
    F4 r;
    F32V<4>::load(k + ck, r.v);
    return r;
  }
  static __device__ __forceinline__ float raw(const F4 &kv, const F4 &qv) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s = __fadd_rn(s, __fmul_rn(qv.v[i], kv.v[i]));
    return group_sum<LOGG>(s);
  }
  static __device__ __forceinline__ float act(float raw, float scale) { return __fmul_rn(scale, raw); }
  static __device__ __forceinline__ void put(const Aux &a, int64_t eh, bool first, float s) {
    if (ZOUT && first) a.z[eh] = s;
  }
};
#define GGL_DOT_LOGIT(LG)                                                               \
  template <> struct Logit<kLogitDot + 2 * LG> : DotLogit<LG, false> {};                \
  template <> struct Logit<kLogitDot + 2 * LG + 1> : DotLogit<LG, true> {};
GGL_DOT_LOGIT(1) GGL_DOT_LOGIT(2) GGL_DOT_LOGIT(3) GGL_DOT_LOGIT(4)
#undef GGL_DOT_LOGIT

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
  if (int rc = walk_plan(plan, "plan", "plan is NULL", "H, C and chunk must be positive",
                         gat_fwd_partial_bytes(hub_chunks(plan), H, C), p))
    return rc;
  GGL_REQUIRE(H > 0 && C > 0, GGL_EINVAL, "H, C and chunk must be positive");
  GGL_REQUIRE(ggl_dot_attn_supported(H, C), GGL_EINVAL, "ggl_dot_attn_fwd: C must be 8, 16, 32 or 64 (ggl_dot_attn_supported)");
  const int64_t N = p.N;
  if (N == 0) return GGL_OK;
  GGL_REQUIRE(q && out && rowmax && rowden, GGL_EINVAL, "NULL pointer");
  GGL_REQUIRE((col && k && v) || p.E == 0, GGL_EINVAL, "NULL pointer");
  GatFwd f;
  if (int rc = gat_fwd_setup(p, scale, H, C, p_drop, rng_state, f)) return rc;
  GGL_REQUIRE(gat_aligned<float>(q, 4) && gat_aligned<float>(k, 4) && gat_aligned<float>(v, 4) &&
                  gat_aligned<float>(out, 4) && gat_aligned<float>(f.pacc, 4),
              GGL_EINVAL, "ggl_dot_attn_fwd: q, k, v, out and plan->partial must be 16-byte aligned");
  if (int rc = gat_fwd_grid(f, 4)) return rc;  // logL >= log2(C / 4): a head's lane group never straddles two rows
  const DotAux aux{q, plan->perm, z_out};
#define GGL_DOT_FWD(LG, DR, ZO)                                                                                     \
  GGL_LAUNCH((gat_fwd_kernel<float, float, 4, DR, kLogitDot + 2 * LG + ZO>), f.grid, kBlock, as_stream(stream),     \
             plan->rowptr, col, p.order, plan->long_rows, plan->chunk_ptr, k, aux, v, out, rowmax, rowden, f.pacc,  \
             f.pm, f.pd, (const int64_t *)rng_state, f.d)
#define GGL_DOT_FWD_C(LG)                                     \
  do {                                                        \
    if (f.d.drop_thresh && z_out) GGL_DOT_FWD(LG, true, 1);   \
    else if (f.d.drop_thresh) GGL_DOT_FWD(LG, true, 0);       \
    else if (z_out) GGL_DOT_FWD(LG, false, 1);                \
    else GGL_DOT_FWD(LG, false, 0);                           \
  } while (0)
  if (C == 8) GGL_DOT_FWD_C(1);
  else if (C == 16) GGL_DOT_FWD_C(2);
  else if (C == 32) GGL_DOT_FWD_C(3);
  else GGL_DOT_FWD_C(4);
#undef GGL_DOT_FWD_C
#undef GGL_DOT_FWD
  return gat_fwd_finish<float>(plan, f, out, rowmax, rowden, rng_state, stream);
}
