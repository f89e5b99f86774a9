// gammagl_amd/csrc/gat_common.hpp — what gat.hip (every head shape, also built for the host-emulated tests),
// gat_fast.hip (the GPU-only fast paths), dotattn.hip (dot-product attention, GPU only) and gatv2.hip (GATv2's additive
// attention, GPU only) share: launch dimensions, the logit policies, the attention-dropout word, small helpers, the
// declarations of the hub-chunk combine kernels defined in gat.hip, and the forward walk (gat_online, gat_fwd_kernel and
// its launch recipe) that gat.hip, dotattn.hip and gatv2.hip instantiate.
#pragma once
#include "common.hpp"

#ifndef GGL_EMULATE
#define GGL_EXPF(x) expf(x)
#else
#define GGL_EXPF(x) std::exp(x)
#endif

namespace ggl {

struct GatDims {
  float slope;
  int64_t N, H, C, K, E;
  int64_t chunk, n_long, n_chunks, chunk_blocks, nblocks;
  uint32_t drop_thresh;  // attention dropout (gat_conv.py:104, GATConvFuse's last argument): keep when
  float drop_scale;      // Philox(p * H + h).x >= drop_thresh, kept alphas scaled by 1 / (1 - p)
  int64_t es;  // element stride of alpha / de: 1 = two [E,H] arrays, 2 = interleaved [E,H,2] (one 64-byte line per edge)
  int logL;
  int vl;  // wide backward kernel on 16-bit rows: 1 = a lane's four channels are one aligned access, 0 = four single loads
};

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.0f ? v : __fmul_rn(v, slope); }

// Where the general walks take the logit s_p of sorted position p, head h, from.  The policy is a template parameter of
// gat_online and gat_fwd_kernel (below) and of gat_bwd_dst_kernel and gat_bwd_dst_wide_kernel (gat.hip), separable by
// default; everything behind s_p (online softmax, hub chunks and their merges, dropout words, row hand-out) is the same
// code for all of them.
//   kLogitSeparable  GAT: s_p = LeakyReLU(el[col[p], h] + er[i, h]).  The kernels' (el, er) are the two [N, H] terms.
//   kLogitEdge       any attention layer: s_p = z[e_p, h], e_p = perm ? perm[p] : p the CALLER's edge number, z [E, H] used
//                    as it is.  The kernels' `el` is z and their `er` slot carries plan->perm (int32, NULL for ids that
//                    arrived sorted); the backward's `de` is gz, stored at e_p — the caller's order — and may be NULL.
//   kLogitDot + ...  dot-product attention, forward only: s_p = slope * <q[i, h, :], k[col[p], h, :]>, formed by the lanes
//                    of the head together (dotattn.hip, GPU build only).  `el` is k, `er` carries q, plan->perm and z.
//   kLogitGatv2 + ... GATv2's additive attention, forward only: s_p = sum_c att[h, c] LeakyReLU(x[col[p], h, c] + xr[i, h, c]),
//                    formed by the lanes of the head together from the VALUE row the walk gathers anyway (gatv2.hip, GPU
//                    build only).  `el` is not read, `er` carries xr, att, the slope, plan->perm and z.
// A policy supplies
//   Aux          what travels in the kernels' `er` slot;
//   Row, row()   the per-(row, head) state a lane keeps in registers for the whole walk: er[i, h], nothing, the lane's q.
//                row(aux, i * H + h, i, K, kk): the [N, H] index the backward kernels pass alone, then what the dot policy
//                forms q's address i * K + kk from (formed in the kernel it would move row * K in front of the walk in
//                every instantiation: profiles/attn_walk_dedup.txt);
//   rec()        the record of `el` an edge reads: it is asked for next to col[p], so perm[p] -> z is in flight together with
//                col[p] -> x, not behind it.  The edge policy's load is UNCONDITIONAL — without a perm it re-reads col[p] (the
//                line is already on its way) and selects p: written as `perm ? perm[p] : p` the compiler branches around
//                every load and waits for each one (vmcnt(0) per element), which puts the four id / perm pairs of an
//                unrolled group in series;
//   Opnd, load() the per-position operand, requested in one statement group with the x rows: el[e, h], or the lane's k;
//   raw(), act(), dact()  the logit from (operand, row state), its activation and the activation's derivative;
//   put()        what the forward keeps of s_p: nothing, or the dot's z[e_p, h] (stored by the head's first lane);
//   kC           the head width where the policy fixes it at compile time, 0 = GatDims::C.
// A policy whose operand IS the lane's x row (LogitOnValue<LS>::value, false unless specialised) supplies of_value() in
// place of load(): the walk hands it the row it has loaded and requests nothing more.
enum { kLogitSeparable = 0, kLogitEdge = 1, kLogitDot = 2, kLogitGatv2 = 12 };
template <int LS> struct LogitOnValue { static constexpr bool value = false; };
template <int LS> struct Logit {
  using Aux = const float *__restrict__;  // er [N, H]
  using Row = float;
  using Opnd = float;
  static constexpr int64_t kC = 0;
  static __device__ __forceinline__ float row(Aux er, int64_t ih, int64_t = 0, int64_t = 0, int64_t = 0) {
    return er[ih];
  }
  static __device__ __forceinline__ int64_t rec(Aux, const int32_t *__restrict__, int64_t, int64_t c) { return c; }
  static __device__ __forceinline__ float load(const float *__restrict__ el, int64_t eh, int64_t) { return el[eh]; }
  static __device__ __forceinline__ float raw(float v, float er_i) { return __fadd_rn(v, er_i); }
  static __device__ __forceinline__ float act(float raw, float slope) { return raw > 0.0f ? raw : __fmul_rn(raw, slope); }
  static __device__ __forceinline__ float dact(float raw, float ds, float slope) {
    return raw > 0.0f ? ds : __fmul_rn(ds, slope);
  }
  static __device__ __forceinline__ void put(Aux, int64_t, bool, float) {}
};
template <> struct Logit<kLogitEdge> {
  using Aux = const int32_t *__restrict__;  // plan->perm [E] or NULL
  using Row = float;
  using Opnd = float;
  static constexpr int64_t kC = 0;
  static __device__ __forceinline__ float row(Aux, int64_t, int64_t = 0, int64_t = 0, int64_t = 0) {
    return 0.0f;
  }
  static __device__ __forceinline__ int64_t rec(Aux perm, const int32_t *__restrict__ col, int64_t p, int64_t) {
    const int64_t r = (perm ? perm : col)[p];
    return perm ? r : p;
  }
  static __device__ __forceinline__ float load(const float *__restrict__ z, int64_t eh, int64_t) { return z[eh]; }
  static __device__ __forceinline__ float raw(float v, float) { return v; }
  static __device__ __forceinline__ float act(float raw, float) { return raw; }
  static __device__ __forceinline__ float dact(float, float ds, float) { return ds; }
  static __device__ __forceinline__ void put(Aux, int64_t, bool, float) {}
};

__device__ __forceinline__ uint32_t pick_word(const U4 &u, int c) {
  return c == 0 ? u.x : (c == 1 ? u.y : (c == 2 ? u.z : u.w));
}
// Attention-dropout word of (sorted position p, head h): counter-based, ~15 VALU instructions per word.
// Round 1 drew these from Philox4x32-10 (one 4-word block per four positions); the backward's source walks meet forward
// positions in scattered order and had to run the full ten rounds per edge for one word — 2.6-3.2 ms of a 5-9 ms
// walk on the Reddit-sized graph.  Dropout masks need decorrelation, not cryptographic strength.  The (seed, offset)
// pair of a launch goes through splitmix64 ONCE (loop-invariant: the compiler keeps it in scalar registers) to give a
// 64-bit launch key; the word is a two-round keyed mix of the 64-bit index: multiply-xorshift with the key's low half,
// the index's high half and the key's high half folded in before the second multiply, xxHash32's avalanche as the
// finaliser.  Consecutive steps (offset + 1) get unrelated keys in BOTH rounds, so their masks are not related by a
// constant XOR of the pre-avalanche value (round 2's generator: advisor finding), and no index bit is dropped.
// The layer epilogue's dropout (epilogue.hip, reduce.hip) stays on Philox.  Host restatement + the statistical test
// (keep rate, step-to-step and neighbour correlation, bit balance): tests/parity_cases.py gat_drop_word /
// check_drop_word_statistics.
__device__ __forceinline__ uint64_t drop_key(uint64_t offset, uint64_t seed) {
  uint64_t z = seed + offset * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ uint32_t drop_word(int64_t p, int64_t H, int64_t h, uint64_t offset, uint64_t seed) {
  const uint64_t idx = (uint64_t)(p * H + h);
  const uint64_t key = drop_key(offset, seed);
  uint32_t x = ((uint32_t)idx ^ (uint32_t)key) * 0x9E3779B1u;
  x ^= x >> 15;
  x = (x ^ (uint32_t)(idx >> 32) ^ (uint32_t)(key >> 32)) * 0x85EBCA77u;
  x ^= x >> 13; x *= 0xC2B2AE3Du;
  x ^= x >> 16;
  return x;
}
// the words of positions 4b .. 4b+3 (the unrolled walks consume them four at a time)
__device__ __forceinline__ U4 drop_words4(int64_t b, int64_t H, int64_t h, uint64_t offset, uint64_t seed) {
  return U4{drop_word(4 * b, H, h, offset, seed), drop_word(4 * b + 1, H, h, offset, seed),
            drop_word(4 * b + 2, H, h, offset, seed), drop_word(4 * b + 3, H, h, offset, seed)};
}

// A lane's VEC consecutive channels of a row whose elements are stored as T: float, or the 16-bit STORAGE types
// mxbf16_t / mxf16_t (common.hpp), widened at the load (exact) and rounded once at the store.  One access of
// VEC * sizeof(element) bytes, at most 16 (float x 8: two), so a pointer handed to VEC > 1 is aligned to that many
// bytes (gat_aligned below); VEC = 1 reads single elements at any alignment.  The arithmetic between a load and a
// store is f32 whatever T is.
template <typename T, int VEC> struct RowV {
  using S = typename TT<T>::S;
  static __device__ __forceinline__ void load(const S *__restrict__ p, float (&v)[VEC]) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = TT<T>::load(p[i]);
  }
  static __device__ __forceinline__ void store(S *__restrict__ p, const float (&v)[VEC]) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) p[i] = TT<T>::store(v[i]);
  }
};
template <> struct RowV<float, 4> {
  static __device__ __forceinline__ void load(const float *__restrict__ p, float (&v)[4]) {
    const float4 t = *reinterpret_cast<const float4 *>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  static __device__ __forceinline__ void store(float *__restrict__ p, const float (&v)[4]) {
    float4 t;
    t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3];
    *reinterpret_cast<float4 *>(p) = t;
  }
};
template <> struct RowV<float, 8> {  // f32 beside 16-bit rows of 8 (an f32 out / g, the hub-chunk partials): two float4
  static __device__ __forceinline__ void load(const float *__restrict__ p, float (&v)[8]) {
    const float4 a = reinterpret_cast<const float4 *>(p)[0], b = reinterpret_cast<const float4 *>(p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
  static __device__ __forceinline__ void store(float *__restrict__ p, const float (&v)[8]) {
    float4 a, b;
    a.x = v[0]; a.y = v[1]; a.z = v[2]; a.w = v[3]; b.x = v[4]; b.y = v[5]; b.z = v[6]; b.w = v[7];
    reinterpret_cast<float4 *>(p)[0] = a;
    reinterpret_cast<float4 *>(p)[1] = b;
  }
};
// 16-bit rows: W 32-bit words = 2 W elements in one 8-byte (W = 2) or 16-byte (W = 4) access
template <int W> struct alignas(4 * W) HWords { uint32_t w[W]; };
template <typename T, int W> struct RowV16 {
  static __device__ __forceinline__ void load(const uint16_t *__restrict__ p, float (&v)[2 * W]) {
    const HWords<W> t = *reinterpret_cast<const HWords<W> *>(p);
#pragma unroll
    for (int i = 0; i < W; ++i) {  // little endian: the lower half-word is the lower channel
      v[2 * i] = TT<T>::load((uint16_t)(t.w[i] & 0xffffu));
      v[2 * i + 1] = TT<T>::load((uint16_t)(t.w[i] >> 16));
    }
  }
  static __device__ __forceinline__ void store(uint16_t *__restrict__ p, const float (&v)[2 * W]) {
    HWords<W> t;
#pragma unroll
    for (int i = 0; i < W; ++i) t.w[i] = (uint32_t)TT<T>::store(v[2 * i]) | ((uint32_t)TT<T>::store(v[2 * i + 1]) << 16);
    *reinterpret_cast<HWords<W> *>(p) = t;
  }
};
template <> struct RowV<mxbf16_t, 4> : RowV16<mxbf16_t, 2> {};
template <> struct RowV<mxbf16_t, 8> : RowV16<mxbf16_t, 4> {};
template <> struct RowV<mxf16_t, 4> : RowV16<mxf16_t, 2> {};
template <> struct RowV<mxf16_t, 8> : RowV16<mxf16_t, 4> {};
template <int VEC> using F32V = RowV<float, VEC>;

// Can p be read / written VEC elements of T at a time?  (NULL: nothing is accessed through it.)
template <typename T> static inline bool gat_aligned(const void *p, int vec) {
  size_t bytes = sizeof(typename TT<T>::S) * (size_t)vec;
  if (bytes > 16) bytes = 16;
  return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0;
}
// is T one of the 16-bit storage tags (the rows of ggl_gat_fused_*_x16)?
template <typename T> struct gat_is16 { static constexpr bool value = sizeof(typename TT<T>::S) == 2; };

static inline int pow2_log2(int64_t v) {
  int l = 0;
  while (l < 6 && ((int64_t)1 << l) < v) ++l;
  return l;
}

static inline int64_t gat_grid_for(int64_t n) {
  int64_t b = ceil_div(n, kBlock);
  if (b > 16384) b = 16384;
  return b < 1 ? 1 : b;
}

// D: GatDims, or the shared-row path's ShDims (gat_fast.hip)
template <typename D> static inline int set_dropout(D &d, float p_drop, const int64_t *rng) {
  GGL_REQUIRE(p_drop >= 0.0f && p_drop < 1.0f, GGL_EINVAL, "p_drop must be in [0, 1)");
  GGL_REQUIRE(p_drop == 0.0f || rng, GGL_EINVAL, "attention dropout needs an rng_state");
  dropout_params(p_drop, &d.drop_thresh, &d.drop_scale);
  return GGL_OK;
}

// hub-chunk combine kernels (defined in gat.hip)
__global__ void gat_long_final_kernel(const int32_t *__restrict__ long_rows, const int64_t *__restrict__ chunk_ptr,
                                      const float *__restrict__ pacc, const float *__restrict__ pm,
                                      const float *__restrict__ pd, float *__restrict__ y, float *__restrict__ rowmax,
                                      float *__restrict__ rowden, const GatDims d);
__global__ void gat_bwd_dst_final_kernel(const int32_t *__restrict__ long_rows, const int64_t *__restrict__ chunk_ptr,
                                         const float *__restrict__ pger, float *__restrict__ ger, int64_t n_long,
                                         int64_t H);
__global__ void gat_bwd_src_final_kernel(const int32_t *__restrict__ long_rows, const int64_t *__restrict__ chunk_ptr,
                                         const float *__restrict__ pacc, const float *__restrict__ pgel,
                                         float *__restrict__ gx, float *__restrict__ gel, const GatDims d);
template <typename OT>  // 16-bit out (defined and instantiated in gat.hip)
__global__ void gat_long_final16_kernel(const int32_t *__restrict__ long_rows, const int64_t *__restrict__ chunk_ptr,
                                        const float *__restrict__ pacc, const float *__restrict__ pm,
                                        const float *__restrict__ pd, uint16_t *__restrict__ y,
                                        float *__restrict__ rowmax, float *__restrict__ rowden, const GatDims d);

#ifndef GGL_EMULATE  // (the host emulation build cannot shuffle between its sequentially executed lanes)
// sum over the aligned group of 2^LOGG lanes, a butterfly of wave shuffles: step o adds lane l's and lane l ^ o's value —
// the same pair in either order — so every lane of the group ends with the SAME bits
template <int LOGG> __device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = (1 << LOGG) >> 1; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
  return v;
}
#endif

// the per-position operand of policy LS: its load(), or — LogitOnValue — what it makes of the x row v the walk holds
template <int LS, int VEC>
__device__ __forceinline__ typename Logit<LS>::Opnd logit_opnd(const float *__restrict__ el, int64_t eh, int64_t ck,
                                                               const float (&v)[VEC]) {
  if constexpr (LogitOnValue<LS>::value) return Logit<LS>::of_value(v);
  else return Logit<LS>::load(el, eh, ck);
}

// ---- the forward walk: the kernel of ggl_gat_fused_fwd(_x16), ggl_edge_softmax_agg_fwd (gat.hip), ggl_dot_attn_fwd
// (dotattn.hip) and ggl_gatv2_fwd (gatv2.hip) ----
// One walk over positions [beg, end) of a destination row for head h, channels [kk, kk+VEC):
//   m   = max_p s_p,   s_p = LeakyReLU(el[col[p],h] + er_i)   (or what the Logit policy LS makes of its operands)
//   den = sum_p exp(s_p - m)
//   acc = sum_p exp(s_p - m) * x[col[p], kk:kk+VEC]
// computed online: the running (den, acc) are rescaled by exp(m_old - m_new) whenever a new maximum
// appears (O(log len) times on average), so every feature row, el value and column index is read exactly
// once.  The in-tree chain (softmax.py:29-35) makes three passes (max, sum, weighted sum); the one-walk
// form differs from it only in rounding (a few ulp per rescale; the parity bar for float reductions is
// 1e-5 relative and is tested against the oracle's three-pass restatement).  Four feature rows in flight.
// DROP: attention dropout — the softmax statistics (m, den) see every edge, the weighted sum only the
// kept ones, scaled by 1/(1-p): out = sum_p keep_p alpha_p x_p / (1-p), alpha = softmax over ALL edges.
// Random word of (position p, head h): drop_word(p, h) above — a 15-instruction counter-based mix, so a draw per
// edge is affordable in every walk (with Philox4x32-10 a draw per edge doubled the forward: 4.1 -> 9.4 ms, and the
// walks were aligned to multiples of 4 to share one 4-word block; the alignment is kept for the 16-byte index loads).
// XT: how x is stored (float, or mxbf16_t / mxf16_t: 16-bit storage widened at the load; everything below is f32).
// ri: the policy's state of (row, head); C: the head width (the lane with kk == h * C leads the head).
template <typename XT, int VEC, bool DROP, int LS = kLogitSeparable>
__device__ __forceinline__ void gat_online(const int32_t *__restrict__ col, const float *__restrict__ el,
                                           typename Logit<LS>::Aux aux, const typename TT<XT>::S *__restrict__ x,
                                           typename Logit<LS>::Row ri, float slope, int64_t H, int64_t K,
                                           int64_t C, int64_t h, int64_t kk, int64_t beg, int64_t end,
                                           const GatDims &d, const int64_t *__restrict__ rng,
                                           float &m, float &den, float (&acc)[VEC]) {
  m = -FLT_MAX;  // unsorted_segment_max: lowest() fill, strict <
  den = 0.0f;
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
  const uint64_t seed = DROP ? (uint64_t)rng[0] : 0, offset = DROP ? (uint64_t)rng[1] : 0;
  auto absorb = [&](uint32_t word, float s, const float (&v)[VEC]) {
    if (m < s) {  // new maximum: bring the running sums to the new reference point
      const float sc = GGL_EXPF(__fadd_rn(m, -s));  // m = -FLT_MAX on the first element: exp(-inf) = 0
      den = __fmul_rn(den, sc);
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = __fmul_rn(acc[i], sc);
      m = s;
    }
    const float e = GGL_EXPF(__fadd_rn(s, -m));
    den = __fadd_rn(den, e);
    float ek = e;
    if (DROP) ek = (word >= d.drop_thresh) ? __fmul_rn(e, d.drop_scale) : 0.0f;
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = __fadd_rn(acc[i], __fmul_rn(v[i], ek));
  };
  using LP = Logit<LS>;
  auto single = [&](int64_t q) {
    const int64_t c0 = col[q];
    const int64_t e0 = LP::rec(aux, col, q, c0);
    float v0[VEC];
    RowV<XT, VEC>::load(x + c0 * K + kk, v0);
    const float s0 = LP::act(LP::raw(logit_opnd<LS, VEC>(el, e0 * H + h, c0 * K + kk, v0), ri), slope);
    LP::put(aux, e0 * H + h, kk == h * C, s0);
    absorb(DROP ? drop_word(q, H, h, offset, seed) : 0u, s0, v0);
  };
  int64_t p = beg;
  if (DROP) {  // walk up to a multiple of 4 so that each unrolled group shares one draw
    for (; p < end && (p & 3) != 0; ++p) single(p);
  }
  for (; p + 4 <= end; p += 4) {
    int64_t c[4], e[4];
    float v[4][VEC], s[4];
    U4 rw{0u, 0u, 0u, 0u};
    if (DROP) rw = drop_words4(p >> 2, H, h, offset, seed);
#pragma unroll
    for (int u = 0; u < 4; ++u) { c[u] = col[p + u]; e[u] = LP::rec(aux, col, p + u, c[u]); }
#pragma unroll
    for (int u = 0; u < 4; ++u) RowV<XT, VEC>::load(x + c[u] * K + kk, v[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      s[u] = LP::act(LP::raw(logit_opnd<LS, VEC>(el, e[u] * H + h, c[u] * K + kk, v[u]), ri), slope);
#pragma unroll
    for (int u = 0; u < 4; ++u) LP::put(aux, e[u] * H + h, kk == h * C, s[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) absorb(pick_word(rw, u), s[u], v[u]);
  }
  for (; p < end; ++p) single(p);
}

// Forward (ONE launch + gat_long_final_kernel for hub rows): a group of 2^logL lanes owns one short destination row, a
// whole wavefront one chunk of a long one; each lane VEC channels of one head.
// OT: how out is stored (XT, or float beside 16-bit rows: a last layer's logits).  The hub-chunk partials are f32.
// `el` and `er` are what the Logit policy LS says they are.
template <typename XT, typename OT, int VEC, bool DROP, int LS = kLogitSeparable>
__global__ __launch_bounds__(kBlock) void gat_fwd_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const int32_t *__restrict__ row_order, const int32_t *__restrict__ long_rows,
    const int64_t *__restrict__ chunk_ptr, const float *__restrict__ el, typename Logit<LS>::Aux er,
    const typename TT<XT>::S *__restrict__ x, typename TT<OT>::S *__restrict__ y, float *__restrict__ rowmax,
    float *__restrict__ rowden, float *__restrict__ pacc, float *__restrict__ pm,
    float *__restrict__ pd, const int64_t *__restrict__ rng, const GatDims d) {
  using LP = Logit<LS>;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int64_t H = d.H, K = d.K;
  const int64_t C = LP::kC > 0 ? LP::kC : d.C;
  if (block_id() < d.chunk_blocks) {  // one wavefront per chunk of a long row
    const int64_t cid = block_id() * kWavesPerBlock + wave;
    if (cid >= d.n_chunks) return;
    const HubChunk hc = hub_chunk(rowptr, long_rows, chunk_ptr, d.n_long, d.chunk, cid);
    for (int64_t kk = (int64_t)lane * VEC; kk < K; kk += (int64_t)kWave * VEC) {
      const int64_t h = kk / C;
      const typename LP::Row ri = LP::row(er, hc.row * H + h, hc.row, K, kk);
      float m, dsum, acc[VEC];
      gat_online<XT, VEC, DROP, LS>(col, el, er, x, ri, d.slope, H, K, C, h, kk, hc.beg, hc.end, d, rng, m, dsum, acc);
      F32V<VEC>::store(pacc + cid * K + kk, acc);
      if (kk == h * C) {
        pm[cid * H + h] = m;
        pd[cid * H + h] = dsum;
      }
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
    const int64_t h = kk / C;
    const typename LP::Row ri = LP::row(er, row * H + h, row, K, kk);
    float m, dsum, acc[VEC];
    gat_online<XT, VEC, DROP, LS>(col, el, er, x, ri, d.slope, H, K, C, h, kk, beg, end, d, rng, m, dsum, acc);
    const float inv = __fadd_rn(dsum, 1e-16f);  // softmax.py:35: exp / (sum + 1e-16)
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = __fdiv_rn(acc[i], inv);
    RowV<OT, VEC>::store(y + row * K + kk, acc);  // the one rounding of a 16-bit out
    if (kk == h * C) {  // first lane of the head records the softmax statistics
      rowmax[row * H + h] = m;
      rowden[row * H + h] = dsum;
    }
  }
}

// The launch recipe around gat_fwd_kernel, behind the entry point's own argument checks: dimensions, dropout and the
// carving of plan->partial; the grid once the lane width VEC is known; the merge of the hub chunks and the rng step.
struct GatFwd {
  GatDims d;
  float *pacc, *pm, *pd;  // hub-chunk partials: [n_chunks, K] sums, [n_chunks, H] maxima and denominators
  int64_t grid;
};
// what gat_fwd_setup carves (and ggl_gat_fast_fwd, which takes the same three panels), + 64 bytes: ggl_gat_partial_bytes
static inline size_t gat_fwd_partial_bytes(int64_t n_chunks, int64_t H, int64_t C) {
  if (n_chunks <= 0 || H <= 0 || C <= 0) return 0;
  return (size_t)n_chunks * (size_t)(H * C + 2 * H) * sizeof(float) + 64;
}
static inline int gat_fwd_setup(const WalkPlan &p, float slope, int64_t H, int64_t C, float p_drop,
                                const int64_t *rng_state, GatFwd &f) {
  GatDims &d = f.d;
  d = GatDims{};
  d.slope = slope; d.N = p.N; d.H = H; d.C = C; d.K = H * C; d.E = p.E;
  d.chunk = p.chunk; d.n_long = p.n_long; d.n_chunks = p.n_chunks;
  if (int rc = set_dropout(d, p_drop, rng_state)) return rc;
  f.pacc = p.partial; f.pm = nullptr; f.pd = nullptr;
  if (p.n_long > 0) {
    f.pm = f.pacc + p.n_chunks * d.K;
    f.pd = f.pm + p.n_chunks * H;
    d.chunk_blocks = ceil_div(p.n_chunks, kWavesPerBlock);
  }
  return GGL_OK;
}
static inline int gat_fwd_grid(GatFwd &f, int vec) {
  GatDims &d = f.d;
  d.logL = pow2_log2(ceil_div(d.K, vec));
  d.nblocks = ceil_div(d.N, (int64_t)kWavesPerBlock * (kWave >> d.logL));
  f.grid = d.chunk_blocks + d.nblocks;
  GGL_REQUIRE(f.grid < ((int64_t)1 << 31), GGL_EINVAL, "too many rows for one launch");
  return GGL_OK;
}
template <typename OT>
static inline int gat_fwd_finish(const ggl_segplan_t *plan, const GatFwd &f, typename TT<OT>::S *out, float *rowmax,
                                 float *rowden, int64_t *rng_state, void *stream) {
  GGL_LAUNCH_CHECK();  // the walk's launch
  if (plan->n_long > 0) {
    if constexpr (std::is_same<OT, float>::value)
      GGL_LAUNCH((gat_long_final_kernel), plan->n_long, kBlock, as_stream(stream), plan->long_rows, plan->chunk_ptr,
                 (const float *)f.pacc, (const float *)f.pm, (const float *)f.pd, out, rowmax, rowden, f.d);
    else
      GGL_LAUNCH((gat_long_final16_kernel<OT>), plan->n_long, kBlock, as_stream(stream), plan->long_rows,
                 plan->chunk_ptr, (const float *)f.pacc, (const float *)f.pm, (const float *)f.pd, out, rowmax, rowden,
                 f.d);
    GGL_LAUNCH_CHECK();
  }
  if (f.d.drop_thresh) return rng_advance(rng_state, stream);  // the next call draws a new mask
  return GGL_OK;
}

}  // namespace ggl
