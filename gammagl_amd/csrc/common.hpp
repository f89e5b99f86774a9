// gammagl_amd/csrc/common.hpp — shared host/device helpers for libggl_mpops_hip.so (gfx950 only).
#pragma once
#ifdef GGL_EMULATE
// Host build of the SAME kernel sources, one "thread" at a time (csrc/host/host_shim.hpp): the CPU backend of the
// ops (libggl_mpops_host.so, CPU dispatch key) and the engine of the GPU-less container's kernel-logic tests.
#include "host/host_shim.hpp"
#else
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include <cfloat>
#include <climits>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "../../include/ggl_mpops.h"

namespace ggl {

constexpr int kWave = 64;        // CDNA wavefront
constexpr int kBlock = 256;      // 4 waves: one per SIMD of a CU
constexpr int kWavesPerBlock = kBlock / kWave;

enum Op { OP_SUM = 0, OP_MEAN = 1, OP_MAX = 2 };

// ---- error plumbing ---------------------------------------------------------------------------
void set_error(const char *fmt, ...);
#define GGL_HIP_CHECK(expr)                                                              \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      ::ggl::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,  \
                       __LINE__);                                                        \
      return GGL_EHIP;                                                                   \
    }                                                                                    \
  } while (0)
#define GGL_REQUIRE(cond, code, ...)                                                     \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      ::ggl::set_error(__VA_ARGS__);                                                     \
      return (code);                                                                     \
    }                                                                                    \
  } while (0)
#define GGL_LAUNCH_CHECK() GGL_HIP_CHECK(hipGetLastError())

// kernel launch: KERN is a parenthesised kernel name, e.g. (k<float, 4>).  A dispatch carries its grid as
// 32-bit WORK-ITEM counts per dimension, so gridDim.x * blockDim.x must stay below 2^32: a 256-thread
// block per 4 rows overflows that at 67 M rows (found on the papers100M-sized graph: the tail of the rows
// was silently not launched).  Grids wider than max_grid_x blocks are therefore folded into (x, y) and
// kernels that index by block use block_id(); every such kernel already returns for ids past its work.
int64_t max_grid_x();
static inline void fold_grid(int64_t grid, unsigned *gx, unsigned *gy) {
  const int64_t mx = max_grid_x();
  if (grid <= mx) { *gx = (unsigned)(grid > 0 ? grid : 1); *gy = 1; return; }
  *gx = (unsigned)mx;
  *gy = (unsigned)((grid + mx - 1) / mx);
}
#ifdef GGL_EMULATE
#define GGL_LAUNCH(KERN, GRID, BLOCK, STREAM, ...)                                       \
  do {                                                                                   \
    unsigned ggl_gx_, ggl_gy_;                                                           \
    ::ggl::fold_grid((GRID), &ggl_gx_, &ggl_gy_);                                        \
    ::ggl_emul::launch2d(ggl_gx_, ggl_gy_, (BLOCK), [&]() { KERN(__VA_ARGS__); });       \
  } while (0)
#else
#define GGL_LAUNCH(KERN, GRID, BLOCK, STREAM, ...)                                       \
  do {                                                                                   \
    unsigned ggl_gx_, ggl_gy_;                                                           \
    ::ggl::fold_grid((GRID), &ggl_gx_, &ggl_gy_);                                        \
    hipLaunchKernelGGL(KERN, dim3(ggl_gx_, ggl_gy_), dim3((unsigned)(BLOCK)), 0, (STREAM), __VA_ARGS__); \
  } while (0)
#endif
// linear block index of a (possibly folded) launch
__device__ __forceinline__ int64_t block_id() { return (int64_t)blockIdx.y * (int64_t)gridDim.x + (int64_t)blockIdx.x; }
__device__ __forceinline__ int64_t thread_id() { return block_id() * (int64_t)blockDim.x + (int64_t)threadIdx.x; }
__device__ __forceinline__ int64_t grid_threads() { return (int64_t)gridDim.x * (int64_t)gridDim.y * (int64_t)blockDim.x; }

// The library's options, declared ONCE: X(name, default) /* what it selects, and the measurement behind the default */.
// The Options fields, the environment read (GGL_ + the upper-cased name, once, at first use), ggl_set_option,
// ggl_get_option and ggl_option_name (plan.hip) are all generated from this list.  Forms that were measured, lost and
// removed in ABI 11 are recorded in DESIGN.md ("Forms removed in ABI 11"); they were last present in 992473a.
#define GGL_OPTIONS(X)                                                                                                      \
  X(unroll, 4)               /* neighbour loads in flight per lane in the f32 fast path (4 or 8) */                         \
  X(unroll_narrow, 16)       /* ... and where a row owns <= 4 lanes (K <= 16 floats): 4 or 16 */                            \
  X(unroll_narrow_max, 0)    /* ... for max too (lost with 64-bit argmax registers in round 1; re-measured in round 4) */   \
  /* 1 = give each XCD a contiguous range of row blocks (private-L2 locality).  OFF by default: measured on MI355X          \
     (profiles/kbench_r1.txt) it changes nothing on a randomly ordered graph and is 4x SLOWER on a degree-ordered one       \
     (one XCD inherits all the hub rows); round-robin is the load balancer. */                                              \
  X(xcd_swizzle, 0)                                                                                                         \
  X(force_generic, 0)        /* route f32 through the VEC=1 generic kernel (tests force the path) */                        \
  X(col_block, 64)           /* wide f32 SpMM-sum / mean: launches over column blocks of this width (0 = one launch) */     \
  X(col_block_min_degree, 24)     /* ... and only where a row averages at least this many edges (reuse to find) */          \
  X(col_block_min_edges, 8000000) /* below this many edges the blocks are twice as wide (launch-bound graphs) */            \
  X(ragged4, 1)              /* f32 rows that are not aligned float4s (K % 4 != 0): 4 floats per lane + ragged last lane */ \
  X(ragged_max, 1)           /* ... for segment_max as well (0 = the one-element-per-lane kernels of rounds 2-3) */         \
  /* 0 = natural row order; 1 = length-sorted rows where several rows share a wavefront (balances the lanes of a wave);     \
     2 = also for the wave-per-row kernels (heavy rows first) */                                                            \
  X(row_order, 1)                                                                                                           \
  X(max_grid_x, 1 << 22)     /* blocks per grid row before a launch is folded into 2-D (tests lower it; set clamps to >= 1) */ \
  /* f32 sums: rows longer than the plan's chunk are added up in the reference's serial order (hubf32.hip: bit-identical    \
     to the CPU extension on EVERY row) instead of chunk by chunk (within rounding of it); 0 = the chunked walk */          \
  X(exact_long_rows, 1)                                                                                                     \
  /* hosts: gspmm max backward (products-sized graph, forward + backward in ms, profiles/r5_max_backward.txt):              \
                 int64 witnesses   int32 witnesses   winner mask, forward-order records                                     \
       K =  64        16.8              12.7                        14.0                                                    \
       K = 128        32.4              25.0                        21.6                                                    \
       K = 256        67.1              53.0                        41.1                                                    \
     (removed in ABI 11: records assembled with selects instead of v_writelane, 44.4 ms at K = 256; records scattered to    \
      transposed positions, 41.7 ms; the masked walk in 64-column blocks, 46.8-54.6 ms) */                                  \
  X(maxbwd_arg32, 1)         /* witnesses from a compact int32 copy (ggl_spmm_max_bwd32) ... */                             \
  X(maxbwd_mask, 128)        /* ... and from this many columns up a 1-bit winner mask instead (0 = never) */                \
  /* ... up to this many columns (the mask is an E x K/8-byte transient; K = 602 measured slower AND 12 GiB on the          \
     Reddit-sized graph: ggl_policy_maxbwd_form; 0 = no upper bound: tests force the mask at any width) */                  \
  X(maxbwd_mask_kmax, 256)                                                                                                  \
  X(exact_long_max, (int64_t)1 << 21) /* exact_long_rows: unless the plan's longest row is longer than this (0 = no limit) */ \
  X(exact_side_stream, 1)    /* ... launched beside the walk over the other rows (0 = in front of it, same stream) */       \
  X(softmax_sublanes, 0)     /* edge softmax (gat.hip): lanes that share a (row, column), GPU build (0 = ggl_policy_softmax_sublanes) */ \
  /* hub walk once per aggregate over the full width: 1 = always, 0 = once per column block, 2 = where the long rows lead the ids */ \
  X(hub_one_launch, 2)                                                                                                      \
  /* wide 16-bit-storage SpMM-sum / mean (ggl_spmm_*_x16): column blocks of this width (0 = one launch).  128 columns of    \
     16 bits are the 256-byte slices the f32 launches gather at col_block = 64 (sweep: profiles/spmm16.txt, DESIGN.md       \
     "Mixed-precision aggregate") */                                                                                        \
  X(col_block16, 128)

struct Options {
#define GGL_OPTION_FIELD(name, dflt) int64_t name = (dflt);
  GGL_OPTIONS(GGL_OPTION_FIELD)
#undef GGL_OPTION_FIELD
};
Options &options();

// Philox4x32-10 keyed on (seed, offset); one 4-word draw per vector of 4 outputs (epilogue.hip, reduce.hip)
struct U4 { uint32_t x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(uint64_t index, uint64_t offset, uint64_t seed) {
  uint32_t c0 = (uint32_t)index, c1 = (uint32_t)(index >> 32), c2 = (uint32_t)offset, c3 = (uint32_t)(offset >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return U4{c0, c1, c2, c3};
}

int rng_advance(int64_t *rng_state, void *stream);  // offset += 1 on the stream (epilogue.hip)

// hubf32.hip: the long rows of an f32 sum in serial order, one partial row each (see the file's header)
struct HubF32Args {
  const float *x;
  int64_t x_ld;
  const int32_t *perm;      // segment mode: element of sorted position p; SpMM: weight index of p when !w_by_pos
  const int32_t *col;       // SpMM: source row of sorted position p (NULL = segment mode)
  const float *w;           // edge weights or NULL
  int w_by_pos;
  int64_t H, C;             // C > 0: multi-head weights w[wi * H + column / C]
  const int64_t *rowptr;
  const int32_t *long_rows;
  const int32_t *long_order;   // positions in long_rows, longest row first (or NULL)
  int64_t n_long;
  int64_t K;                // columns of this launch (a column block of a wider matrix: x points at its first column)
  float *partial;           // [n_long, K]
  int64_t avg_long_len;     // average length of the long rows (picks the stage size)
  int f64;                  // segment sums of doubles: x / x_ld / K / partial in 4-byte WORDS (2 per element), see hubf32.hip
  int x16;                  // 0, or GGL_BF16 / GGL_F16: x holds 16-bit elements (x_ld / K in elements), widened before the multiply;
                            // tile, consumer and partial stay f32 (SpMM modes without heads only)
};
#ifndef GGL_EMULATE   // (GPU build only: the host build walks every row in one piece)
int hub_f32_launch(const HubF32Args &a, hipStream_t stream, bool beside, int *forked);   // *forked: 0 or the join token
int hub_f32_join(hipStream_t stream, int token);
#endif

static inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }
static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- host-side recipes every entry point shares (plain C++: the host build compiles them too) ----------------------
// Dropout probability -> keep where the element's random word >= thresh (P(drop) = thresh / 2^32), kept values times scale
static inline void dropout_params(float p_drop, uint32_t *thresh, float *scale) {
  *thresh = p_drop > 0.0f ? (uint32_t)((double)p_drop * 4294967296.0) : 0u;
  *scale = p_drop > 0.0f ? 1.0f / (1.0f - p_drop) : 1.0f;
}

// What a launcher reads off a plan before it walks it.  n_chunks is 0 and partial NULL for a plan without long rows;
// how the partial buffer is carved up (pm = pacc + n_chunks * K, ...) belongs to the kernel and stays with the caller,
// next to the *_partial_bytes export that sizes it: the caller passes that export's answer for hub_chunks(plan) as `need`.
struct WalkPlan {
  int64_t N, E, chunk, n_long, n_chunks;
  const int32_t *order;   // the plan's length-sorted row order, or NULL (option row_order = 0)
  float *partial;
};
// the chunk count a walk's *_partial_bytes export is asked about: 0 for no plan (rejected next) and no long rows
static inline int64_t hub_chunks(const ggl_segplan_t *plan) { return (plan && plan->n_long > 0) ? plan->n_chunks : 0; }
// plan->partial_bytes against what the walk carves out of plan->partial (only asked for a plan with long rows)
static inline int partial_fits(const ggl_segplan_t *plan, const char *which, size_t need) {
  GGL_REQUIRE(plan->partial_bytes >= need, GGL_EWORKSPACE, "%s has long rows and a partial of %zu bytes: its walk needs %zu",
              which, plan->partial_bytes, need);
  return GGL_OK;
}
// The entry points word their rejections differently and the words are part of the ABI: null_text / chunk_text are the
// caller's, `which` ("plan", "transposed plan") names the plan in the workspace errors.
static inline int walk_plan(const ggl_segplan_t *plan, const char *which, const char *null_text, const char *chunk_text,
                            size_t need, WalkPlan &p) {
  GGL_REQUIRE(plan && plan->rowptr, GGL_EINVAL, "%s", null_text);
  GGL_REQUIRE(plan->chunk > 0, GGL_EINVAL, "%s", chunk_text);
  p.N = plan->N; p.E = plan->E; p.chunk = plan->chunk;
  p.n_long = plan->n_long > 0 ? plan->n_long : 0;
  p.n_chunks = p.n_long > 0 ? plan->n_chunks : 0;
  p.order = options().row_order ? plan->row_order : nullptr;
  p.partial = nullptr;
  if (p.n_long > 0) {
    GGL_REQUIRE(plan->long_rows && plan->chunk_ptr && plan->partial, GGL_EWORKSPACE,
                "%s has long rows but long_rows/chunk_ptr/partial is NULL", which);
    if (int rc = partial_fits(plan, which, need)) return rc;
    p.partial = static_cast<float *>(plan->partial);
  }
  return GGL_OK;
}

// ---- dtype semantics: "accumulate in the storage dtype" (segment_sum_cpu.cpp:56) ---------------
// S = storage type in memory, A = register type.  add() rounds to storage precision after every
// step, exactly like c10::Half / c10::BFloat16 operator+= (float add, then round-to-nearest-even).
struct bf16_t { uint16_t bits; };
struct f16_t { uint16_t bits; };

__device__ __forceinline__ float bf16_to_f32(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
  uint32_t x = __float_as_uint(f);
  if ((x & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;  // c10::BFloat16: NaN -> 0x7FC0
  return (uint16_t)((x + (((x >> 16) & 1u) + 0x7fffu)) >> 16);
}
__device__ __forceinline__ float f16_to_f32(uint16_t b) {
  _Float16 h;
  __builtin_memcpy(&h, &b, 2);
  return (float)h;
}
__device__ __forceinline__ uint16_t f32_to_f16(float f) {
  _Float16 h = (_Float16)f;  // v_cvt_f16_f32, round-to-nearest-even
  uint16_t b;
  __builtin_memcpy(&b, &h, 2);
  return b;
}

template <typename T> struct TT;

#define GGL_INT_TT(T, LOW)                                                               \
  template <> struct TT<T> {                                                             \
    using S = T;                                                                         \
    using A = T;                                                                         \
    static __device__ __forceinline__ A load(S v) { return v; }                          \
    static __device__ __forceinline__ S store(A v) { return v; }                         \
    static __device__ __forceinline__ A add(A a, A b) {                                  \
      using U = typename std::make_unsigned<T>::type;                                    \
      return (T)(U)((U)a + (U)b);                                                        \
    }                                                                                    \
    static __device__ __forceinline__ bool less(A a, A b) { return a < b; }              \
    static __device__ __forceinline__ A lowest() { return (T)(LOW); }                    \
    static __device__ __forceinline__ A zero() { return (T)0; }                          \
    static __device__ __forceinline__ A count(int64_t c) { return (T)c; }                \
    static __device__ __forceinline__ bool gt1(A c) { return c > (T)1; }                 \
    static __device__ __forceinline__ A div(A a, A c) { return (T)(a / c); }             \
  };
GGL_INT_TT(uint8_t, 0)
GGL_INT_TT(int8_t, INT8_MIN)
GGL_INT_TT(int16_t, INT16_MIN)
GGL_INT_TT(int32_t, INT32_MIN)
GGL_INT_TT(int64_t, INT64_MIN)

template <> struct TT<float> {
  using S = float;
  using A = float;
  static __device__ __forceinline__ A load(S v) { return v; }
  static __device__ __forceinline__ S store(A v) { return v; }
  static __device__ __forceinline__ A add(A a, A b) { return __fadd_rn(a, b); }
  static __device__ __forceinline__ bool less(A a, A b) { return a < b; }
  static __device__ __forceinline__ A lowest() { return -FLT_MAX; }
  static __device__ __forceinline__ A zero() { return 0.0f; }
  // the reference counts in x's dtype with += 1 (segment_mean_cpu.cpp:44,52): a float counter
  // stops growing at 2^24
  static __device__ __forceinline__ A count(int64_t c) { return (float)(c < 16777216 ? c : 16777216); }
  static __device__ __forceinline__ bool gt1(A c) { return c > 1.0f; }
  static __device__ __forceinline__ A div(A a, A c) { return __fdiv_rn(a, c); }
};
template <> struct TT<double> {
  using S = double;
  using A = double;
  static __device__ __forceinline__ A load(S v) { return v; }
  static __device__ __forceinline__ S store(A v) { return v; }
  static __device__ __forceinline__ A add(A a, A b) { return __dadd_rn(a, b); }
  static __device__ __forceinline__ bool less(A a, A b) { return a < b; }
  static __device__ __forceinline__ A lowest() { return -DBL_MAX; }
  static __device__ __forceinline__ A zero() { return 0.0; }
  static __device__ __forceinline__ A count(int64_t c) { return (double)c; }
  static __device__ __forceinline__ bool gt1(A c) { return c > 1.0; }
  static __device__ __forceinline__ A div(A a, A c) { return __ddiv_rn(a, c); }
};
template <> struct TT<f16_t> {
  using S = uint16_t;
  using A = float;  // always holds a value exactly representable in f16
  static __device__ __forceinline__ A load(S v) { return f16_to_f32(v); }
  static __device__ __forceinline__ S store(A v) { return f32_to_f16(v); }
  static __device__ __forceinline__ A add(A a, A b) { return f16_to_f32(f32_to_f16(__fadd_rn(a, b))); }
  static __device__ __forceinline__ bool less(A a, A b) { return a < b; }
  static __device__ __forceinline__ A lowest() { return -65504.0f; }
  static __device__ __forceinline__ A zero() { return 0.0f; }
  static __device__ __forceinline__ A count(int64_t c) { return (float)(c < 2048 ? c : 2048); }
  static __device__ __forceinline__ bool gt1(A c) { return c > 1.0f; }
  static __device__ __forceinline__ A div(A a, A c) { return f16_to_f32(f32_to_f16(__fdiv_rn(a, c))); }
};
template <> struct TT<bf16_t> {
  using S = uint16_t;
  using A = float;  // always holds a value exactly representable in bf16
  static __device__ __forceinline__ A load(S v) { return bf16_to_f32(v); }
  static __device__ __forceinline__ S store(A v) { return f32_to_bf16(v); }
  static __device__ __forceinline__ A add(A a, A b) { return bf16_to_f32(f32_to_bf16(__fadd_rn(a, b))); }
  static __device__ __forceinline__ bool less(A a, A b) { return a < b; }
  static __device__ __forceinline__ A lowest() { return bf16_to_f32(0xFF7Fu); }
  static __device__ __forceinline__ A zero() { return 0.0f; }
  static __device__ __forceinline__ A count(int64_t c) { return (float)(c < 256 ? c : 256); }
  static __device__ __forceinline__ bool gt1(A c) { return c > 1.0f; }
  static __device__ __forceinline__ A div(A a, A c) { return bf16_to_f32(f32_to_bf16(__fdiv_rn(a, c))); }
};

// ---- mixed precision: 16-bit STORAGE, f32 ARITHMETIC (ggl_spmm_*_x16) ---------------------------------------------------
// The element is widened at the load (exact), every product and add is the f32 one the float kernels make, in the same
// order, and the sum is rounded ONCE, at the store: out == f32_op(x.float()).to(x.dtype) bit for bit.  Not the traits
// above: the segment ops keep the reference's storage-type running sums (a bf16 sum of ones stalls at 256).
struct mxbf16_t {};
struct mxf16_t {};
template <typename T> struct f32out {};     // T's rows, result stored as f32 (no rounding at all)
#define GGL_MX_TT(T, LOAD, STORE)                                                        \
  template <> struct TT<T> {                                                             \
    using S = uint16_t;                                                                  \
    using A = float;                                                                     \
    static __device__ __forceinline__ A load(S v) { return LOAD(v); }                    \
    static __device__ __forceinline__ S store(A v) { return STORE(v); }                  \
    static __device__ __forceinline__ A add(A a, A b) { return __fadd_rn(a, b); }        \
    static __device__ __forceinline__ bool less(A a, A b) { return a < b; }              \
    static __device__ __forceinline__ A lowest() { return -FLT_MAX; }                    \
    static __device__ __forceinline__ A zero() { return 0.0f; }                          \
    static __device__ __forceinline__ A count(int64_t c) { return TT<float>::count(c); } \
    static __device__ __forceinline__ bool gt1(A c) { return c > 1.0f; }                 \
    static __device__ __forceinline__ A div(A a, A c) { return __fdiv_rn(a, c); }        \
  };
GGL_MX_TT(mxbf16_t, bf16_to_f32, f32_to_bf16)
GGL_MX_TT(mxf16_t, f16_to_f32, f32_to_f16)
#undef GGL_MX_TT
template <typename T> struct TT<f32out<T>> : TT<T> {};
template <typename T> struct mx_code { static constexpr int value = 0; };     // 0 = not a mixed-precision type
template <> struct mx_code<mxbf16_t> { static constexpr int value = GGL_BF16; };
template <> struct mx_code<mxf16_t> { static constexpr int value = GGL_F16; };
template <typename T> struct mx_code<f32out<T>> : mx_code<T> {};

// Where a row kernel's results go: O = element type of `out`, P = of the chunk partials.  The storage type itself for every
// type but the mixed-precision ones, whose partials are f32 (a 16-bit partial would round twice) and whose output is 16-bit
// or f32 (f32out<>).
template <typename T> struct TO {
  using O = typename TT<T>::S;
  using P = typename TT<T>::S;
  static __device__ __forceinline__ O ostore(typename TT<T>::A v) { return TT<T>::store(v); }
  static __device__ __forceinline__ typename TT<T>::A oload(O v) { return TT<T>::load(v); }
  static __device__ __forceinline__ P pstore(typename TT<T>::A v) { return TT<T>::store(v); }
  static __device__ __forceinline__ typename TT<T>::A pload(P v) { return TT<T>::load(v); }
};
template <typename T, typename OT> struct TOmx {
  using O = OT;
  using P = float;
  static __device__ __forceinline__ O ostore(float v) {
    if constexpr (std::is_same<OT, float>::value) return v; else return TT<T>::store(v);
  }
  static __device__ __forceinline__ float oload(O v) {
    if constexpr (std::is_same<OT, float>::value) return v; else return TT<T>::load(v);
  }
  static __device__ __forceinline__ P pstore(float v) { return v; }
  static __device__ __forceinline__ float pload(P v) { return v; }
};
template <> struct TO<mxbf16_t> : TOmx<mxbf16_t, uint16_t> {};
template <> struct TO<mxf16_t> : TOmx<mxf16_t, uint16_t> {};
template <typename T> struct TO<f32out<T>> : TOmx<T, float> {};

// eight 16-bit elements at a 2-byte aligned address as ONE 16-byte access (the backend emits global_load_dwordx4 for the
// packed struct: unaligned access mode) — rows of f16 / bf16 whose width is not a multiple of 8 (reduce.hip, hub16.hip)
struct __attribute__((packed, aligned(2))) H8U { uint16_t v[8]; };

static inline size_t dtype_size(int dtype) {
  switch (dtype) {
    case GGL_U8: case GGL_I8: return 1;
    case GGL_I16: case GGL_F16: case GGL_BF16: return 2;
    case GGL_I32: case GGL_F32: return 4;
    case GGL_I64: case GGL_F64: return 8;
    default: return 0;
  }
}

// block id -> logical block id so that the blocks one XCD executes (block b runs on XCD b % 8, observed) cover RUNS of
// consecutive row blocks: neighbouring rows of a locality-ordered graph then share one private 4 MiB L2 instead of
// being dealt round-robin to all eight.  swizzle = 1: one contiguous eighth of the launch per XCD (4x slower on a
// degree-ordered graph: one XCD inherits every heavy row); swizzle = B >= 2: runs of B consecutive blocks, the eight
// XCDs working on eight adjacent runs (balanced whatever the order).  Pure performance: any bijection is correct.
// (guide §5.5 T1)
__device__ __forceinline__ int64_t xcd_remap(int64_t b, int64_t nb, int swizzle) {
  if (!swizzle) return b;
  if (swizzle == 1) {
    const int64_t per = nb >> 3;
    const int64_t main_blocks = per << 3;
    if (b >= main_blocks) return b;  // ragged tail keeps identity
    return (b & 7) * per + (b >> 3);
  }
  const int64_t B = swizzle;
  const int64_t main_blocks = (nb / (8 * B)) * (8 * B);
  if (b >= main_blocks) return b;
  const int64_t xcd = b & 7, k = b >> 3;          // the k-th block this XCD executes
  return ((k / B) * 8 + xcd) * B + (k % B);
}

// Chunk `cid` of a plan's long rows: slot = the last j with chunk_ptr[j] <= cid (the long row that owns the chunk),
// row = long_rows[slot], [beg, end) = the chunk's sorted positions.
struct HubChunk { int64_t slot, row, beg, end; };
__device__ __forceinline__ HubChunk hub_chunk(const int64_t *rowptr, const int32_t *long_rows, const int64_t *chunk_ptr,
                                              int64_t n_long, int64_t chunk, int64_t cid) {
  int64_t lo = 0, hi = n_long - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (chunk_ptr[mid] <= cid) lo = mid; else hi = mid - 1;
  }
  const int64_t row = long_rows[lo];
  const int64_t beg = rowptr[row] + (cid - chunk_ptr[lo]) * chunk;
  const int64_t rend = rowptr[row + 1];
  return HubChunk{lo, row, beg, (beg + chunk < rend) ? beg + chunk : rend};
}

}  // namespace ggl
