// gammagl_amd/csrc/gatv2.hip — fused GATv2 (additive) graph attention, forward, GPU build only.
//
//   z[e,h]     = sum_c att[h,c] * LeakyReLU(xl[src(e),h,c] + xr[dst(e),h,c])
//   out[i,h,:] = sum_{e -> i} drop(softmax_i(z[:,h]))[e] * xl[src(e),h,:]
// ("How Attentive are Graph Attention Networks?": the LeakyReLU sits inside the channel sum, so the logit neither separates
// into el[src] + er[dst] nor reduces to a dot product.)  Composed from the library's ops that needs xl[src] + xr[dst] as an
// [E, H, C] tensor in front of ggl_edge_softmax_agg_fwd.  Here the logit is formed inside the aggregate's walk from the VALUE
// row xl[col[p]] the walk gathers anyway (LogitOnValue: no second request for it), and z is stored only when the caller
// wants it (a backward will read it) — in inference no [E, H] array exists, and no route needs an [E, H, C] one.
//
// Everything behind the logit is the shared forward walk (gat_common.hpp: gat_fwd_kernel<float, float, 4, DROP, LS> and
// gat_online) with the policy below: `x` is xl, `el` is not read.  So out / rowmax / rowden are ggl_edge_softmax_agg_fwd's
// bits on the z stored here by construction.
//
// The logit: the g = C / 4 lanes of a head keep their four xr[i,h,·] and att[h,·] values in registers for the whole row; per
// edge each forms its four terms __fmul_rn(att, lrelu(__fadd_rn(xl, xr))), adds them in ascending channel order from 0.0f,
// and the partial sums are added across the group with the butterfly of dotattn.hip (group_sum), after which EVERY lane of
// the group holds the SAME bits: the per-lane copies of (m, den) stay in step.  The composed route sums the C terms in
// torch's order, hence z carries an error bound, |z - z64| <= gamma_{C+2} sum_c |att_c| |lrelu(xl_c + xr_c)|, not bits.
//
// Shuffle partners: dotattn.hip's rules unchanged — the group of lane l is the aligned block of g lanes around it, g a
// power of two <= 2^logL, so its lanes share the row (or chunk), the head, [beg, end) and the kk < K test (K = H * C is a
// multiple of 4 g); a lane with kk >= K never runs a shuffle.
#include "gat_common.hpp"

namespace ggl {

struct Gatv2Aux {
  const float *__restrict__ xr;      // [N_dst, H, C]
  const float *__restrict__ att;     // [H, C]
  float slope;                       // LeakyReLU's, inside the channel sum (the walk's own `slope` argument goes unused)
  const int32_t *__restrict__ perm;  // plan->perm or NULL
  float *__restrict__ z;             // [E, H] in the caller's edge order; not touched unless ZOUT
};
struct Gatv2Row { float r[4], a[4], slope; };  // the lane's four xr and att values of (row, head)
struct Gatv2Opnd { float v[4]; };              // ... and of xl[col[p], head]: the walk's value row
// C = 4 << LOGG.  ZOUT = false: no perm load, no z store.
template <int LOGG, bool ZOUT> struct Gatv2Logit {
  using Aux = Gatv2Aux;
  using Row = Gatv2Row;
  using Opnd = Gatv2Opnd;
  static constexpr int64_t kC = (int64_t)4 << LOGG;
  static __device__ __forceinline__ Row row(const Aux &a, int64_t, int64_t i, int64_t K, int64_t kk) {
    Row r;
    F32V<4>::load(a.xr + i * K + kk, r.r);
    F32V<4>::load(a.att + kk, r.a);  // att [H, C] flat: kk = h * C + c
    r.slope = a.slope;
    return r;
  }
  static __device__ __forceinline__ int64_t rec(const Aux &a, const int32_t *__restrict__ col, int64_t p, int64_t c) {
    return ZOUT ? Logit<kLogitEdge>::rec(a.perm, col, p, c) : 0;
  }
  static __device__ __forceinline__ Opnd of_value(const float (&v)[4]) { return Opnd{{v[0], v[1], v[2], v[3]}}; }
  static __device__ __forceinline__ float raw(const Opnd &x, const Row &ri) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s = __fadd_rn(s, __fmul_rn(ri.a[i], lrelu(__fadd_rn(x.v[i], ri.r[i]), ri.slope)));
    return group_sum<LOGG>(s);
  }
  static __device__ __forceinline__ float act(float raw, float) { return raw; }
  static __device__ __forceinline__ void put(const Aux &a, int64_t eh, bool first, float s) {
    if (ZOUT && first) a.z[eh] = s;
  }
};
#define GGL_GATV2_LOGIT(LG)                                                                  \
  template <> struct Logit<kLogitGatv2 + 2 * LG> : Gatv2Logit<LG, false> {};                 \
  template <> struct Logit<kLogitGatv2 + 2 * LG + 1> : Gatv2Logit<LG, true> {};              \
  template <> struct LogitOnValue<kLogitGatv2 + 2 * LG> { static constexpr bool value = true; }; \
  template <> struct LogitOnValue<kLogitGatv2 + 2 * LG + 1> { static constexpr bool value = true; };
GGL_GATV2_LOGIT(1) GGL_GATV2_LOGIT(2) GGL_GATV2_LOGIT(3) GGL_GATV2_LOGIT(4)
#undef GGL_GATV2_LOGIT

}  // namespace ggl

using namespace ggl;

// C = 4 g with g = 2, 4, 8 or 16 lanes per head, any H: the shapes instantiated and tested
extern "C" int ggl_gatv2_supported(int64_t H, int64_t C) {
  return (H > 0 && (C == 8 || C == 16 || C == 32 || C == 64)) ? 1 : 0;
}

// Whether the fused forward is the default for a supported shape.  The rule is dot_attention's: it is, unless it was
// measured slower than the composed route (z formed by torch in edge blocks + ggl_edge_softmax_agg_fwd) by more than the
// run-to-run spread.  profiles/gatv2_attention.txt: 8 x 8, 1 x 64 and 4 x 32 on the Reddit- and products-sized graphs are
// 22-26x FASTER fused (5.5-9.0 ms against 121-220 ms, spread at most 3.1 %), so no shape is excluded; C = 16 was not timed.
extern "C" int ggl_policy_gatv2_fused(int64_t H, int64_t C, int64_t E, int64_t N_in) {
  (void)E; (void)N_in;
  return ggl_gatv2_supported(H, C);
}

extern "C" int ggl_gatv2_fwd(const ggl_segplan_t *plan, const int32_t *col, const float *xl, const float *xr,
                             const float *att, float slope, int64_t H, int64_t C, float p_drop, int64_t *rng_state,
                             float *out, float *rowmax, float *rowden, float *z_out, void *stream) {
  WalkPlan p;
  if (int rc = walk_plan(plan, "plan", "plan is NULL", "H, C and chunk must be positive",
                         gat_fwd_partial_bytes(hub_chunks(plan), H, C), p))
    return rc;
  GGL_REQUIRE(H > 0 && C > 0, GGL_EINVAL, "H, C and chunk must be positive");
  GGL_REQUIRE(ggl_gatv2_supported(H, C), GGL_EINVAL, "ggl_gatv2_fwd: C must be 8, 16, 32 or 64 (ggl_gatv2_supported)");
  const int64_t N = p.N;
  if (N == 0) return GGL_OK;
  GGL_REQUIRE(xr && att && out && rowmax && rowden, GGL_EINVAL, "NULL pointer");
  GGL_REQUIRE((col && xl) || p.E == 0, GGL_EINVAL, "NULL pointer");
  GatFwd f;
  if (int rc = gat_fwd_setup(p, slope, H, C, p_drop, rng_state, f)) return rc;
  GGL_REQUIRE(gat_aligned<float>(xl, 4) && gat_aligned<float>(xr, 4) && gat_aligned<float>(att, 4) &&
                  gat_aligned<float>(out, 4) && gat_aligned<float>(f.pacc, 4),
              GGL_EINVAL, "ggl_gatv2_fwd: xl, xr, att, out and plan->partial must be 16-byte aligned");
  if (int rc = gat_fwd_grid(f, 4)) return rc;  // logL >= log2(C / 4): a head's lane group never straddles two rows
  const Gatv2Aux aux{xr, att, slope, plan->perm, z_out};
#define GGL_GATV2_FWD(LG, DR, ZO)                                                                                    \
  GGL_LAUNCH((gat_fwd_kernel<float, float, 4, DR, kLogitGatv2 + 2 * LG + ZO>), f.grid, kBlock, as_stream(stream),    \
             plan->rowptr, col, p.order, plan->long_rows, plan->chunk_ptr, xl, aux, xl, out, rowmax, rowden, f.pacc, \
             f.pm, f.pd, (const int64_t *)rng_state, f.d)
#define GGL_GATV2_FWD_C(LG)                                     \
  do {                                                          \
    if (f.d.drop_thresh && z_out) GGL_GATV2_FWD(LG, true, 1);   \
    else if (f.d.drop_thresh) GGL_GATV2_FWD(LG, true, 0);       \
    else if (z_out) GGL_GATV2_FWD(LG, false, 1);                \
    else GGL_GATV2_FWD(LG, false, 0);                           \
  } while (0)
  if (C == 8) GGL_GATV2_FWD_C(1);
  else if (C == 16) GGL_GATV2_FWD_C(2);
  else if (C == 32) GGL_GATV2_FWD_C(3);
  else GGL_GATV2_FWD_C(4);
#undef GGL_GATV2_FWD_C
#undef GGL_GATV2_FWD
  return gat_fwd_finish<float>(plan, f, out, rowmax, rowden, rng_state, stream);
}
