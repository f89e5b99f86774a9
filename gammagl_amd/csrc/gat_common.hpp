// gammagl_amd/csrc/gat_common.hpp — what gat.hip (every head shape, also built for the host-emulated tests) and
// gat_fast.hip (the GPU-only fast paths) share: launch dimensions, the attention-dropout word, small helpers, and
// the declarations of the hub-chunk combine kernels defined in gat.hip.
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

// Where the general walks (gat.hip) take the logit s_p of sorted position p, head h, from.  The policy is a template parameter
// of gat_online, gat_fwd_kernel, gat_bwd_dst_kernel and gat_bwd_dst_wide_kernel, separable by default; everything behind
// s_p (online softmax, hub chunks and their merges, dropout words, row hand-out) is the same code for both.
//   kLogitSeparable  GAT: s_p = LeakyReLU(el[col[p], h] + er[i, h]).  The kernels' (el, er) are the two [N, H] terms.
//   kLogitEdge       any attention layer: s_p = z[e_p, h], e_p = perm ? perm[p] : p the CALLER's edge number, z [E, H] used
//                    as it is.  The kernels' `el` is z and their `er` slot carries plan->perm (int32, NULL for ids that
//                    arrived sorted); the backward's `de` is gz, stored at e_p — the caller's order — and may be NULL.
// rec() is the record of `el` an edge reads: it is asked for next to col[p], so perm[p] -> z is in flight together with
// col[p] -> x, not behind it.  The edge policy's load is UNCONDITIONAL — without a perm it re-reads col[p] (the line is
// already on its way) and selects p: written as `perm ? perm[p] : p` the compiler branches around every load and waits
// for each one (vmcnt(0) per element), which puts the four id / perm pairs of an unrolled group in series.
enum { kLogitSeparable = 0, kLogitEdge = 1 };
template <int LS> struct Logit {
  using Aux = const float *;  // er [N, H]
  static __device__ __forceinline__ float row(Aux er, int64_t i) { return er[i]; }
  static __device__ __forceinline__ int64_t rec(Aux, const int32_t *__restrict__, int64_t, int64_t c) { return c; }
  static __device__ __forceinline__ float raw(float v, float er_i) { return __fadd_rn(v, er_i); }
  static __device__ __forceinline__ float act(float raw, float slope) { return raw > 0.0f ? raw : __fmul_rn(raw, slope); }
  static __device__ __forceinline__ float dact(float raw, float ds, float slope) {
    return raw > 0.0f ? ds : __fmul_rn(ds, slope);
  }
};
template <> struct Logit<kLogitEdge> {
  using Aux = const int32_t *;  // plan->perm [E] or NULL
  static __device__ __forceinline__ float row(Aux, int64_t) { return 0.0f; }
  static __device__ __forceinline__ int64_t rec(Aux perm, const int32_t *__restrict__ col, int64_t p, int64_t) {
    const int64_t r = (perm ? perm : col)[p];
    return perm ? r : p;
  }
  static __device__ __forceinline__ float raw(float v, float) { return v; }
  static __device__ __forceinline__ float act(float raw, float) { return raw; }
  static __device__ __forceinline__ float dact(float, float ds, float) { return ds; }
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

}  // namespace ggl
