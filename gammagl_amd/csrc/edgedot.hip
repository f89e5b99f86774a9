// gammagl_amd/csrc/edgedot.hip — bspmm's weight gradient on the destination-sorted plan:
//   ggl_bspmm_grad_w_sorted : gw[e,h] = sum_c x[src_e,h,c] * g[dst_e,h,c]   (cpu/bspmm_sum_cpu.cpp:95-107)
//
// The reference sums over c serially (rounded multiply, rounded add, c ascending) and the golden weight gradients pin
// that order bit for bit, so the dot of an (edge, head) item is one dependent chain: it has to live in ONE lane.  The
// thread-per-item kernel of backward.hip does exactly that and reads its two strips 16 bytes at a time — a wavefront
// then touches 64 different rows per load, C/4 times over, which thrashes the 32 KiB L1 of a CU for C > 16 (every
// 128-byte line is fetched up to 8 times from L2): products-sized graph, H = 1, C = 256: 69 ms where the forward
// SpMM — the same gather volume — takes 16.4 ms.
//
// Here the loads are coalesced and the transposition happens in LDS: a workgroup owns 256 consecutive items of the
// DESTINATION-SORTED order (so the g strips of a batch are a handful of rows: each lane reads its own straight from
// memory and L1 serves the lanes that share a row; only x[src] is a random gather, exactly as in the forward walk),
// stages 32-column slabs of the items' x strips into an LDS tile with 16-byte loads in which 8 consecutive lanes cover
// 128 contiguous bytes — the next slab's loads in flight while the current one is folded — and every lane folds ITS
// item's 32 products in order from LDS (row stride 36 floats: the 16-byte reads of a 16-lane pass fall into distinct
// banks).
// Results go to gw[perm[p], h], the caller's edge order.  A launch may cover a column range [c_lo, c_hi) only,
// taking the chain so far from `carry_in` and leaving it in `carry_out` (both in SORTED order: coalesced): the host
// runs wide heads as launches over 64-column blocks like the forward (launch_f32_cols, reduce.hip) — same serial
// order, and the 256-byte slices keep 4x as many hub rows in L2; only the last block scatters through perm.
//
//   ggl_spmm_grad_w : gw[e] = sum_k x[src_e,k] * g[dst_e,k]  — gspmm's (sum, mean) gradient with respect to its edge
// weights (an extension: gspmm.cpp:79 returns none).  It is the dot above with one head, so f32 x and f32 g RUN the
// kernels above (H = 1, C = K).  What is added here is the dot on rows STORED as bf16 / f16 (either operand, or both):
// every element is widened at the load (exact) and the products and adds are the f32 ones in the f32 order, so
// gw(x16, g16) == gw(widen(x16), widen(g16)) bit for bit.  The tile of such a kernel (dot16_kernel):
//   - a 16-byte piece of a 16-bit strip is 8 columns, so the unit of the walk is 8 columns (K % 8 == 0; the rest takes
//     the plain kernel) and a slab stays 32 columns — the g registers of a fold are those of the f32 kernel at most;
//   - a 16-bit x strip stays 16-bit in LDS and is widened in registers after the read: a slab is 4 pieces per item,
//     tile row stride 5 pieces (80 bytes, odd in 16-byte slots: the 16 lanes of a ds_read_b128 group fall into 16
//     distinct slots, as the f32 tile's 9-piece stride does), 20 KiB per workgroup instead of 36, and half the
//     global-load and LDS-store instructions per column of the f32 kernel;
//   - an f32 x strip (16-bit g only) keeps the f32 tile: 8 pieces per slab, stride 9.
// `mean` divides g by the destination row's edge count first — (g / count) * w, the order ggl_spmm_mean_bwd documents —
// once per row into an f32 [N_dst, K] panel in the scratch (a divide per edge and column inside the walk would be ten
// instructions beside the dot's two); the walk is then the sum form on that panel.
#include "common.hpp"

namespace ggl {

// float4s per strip per slab: 8 (32 columns; tile row stride 36 floats: the 16-byte reads of a 16-lane pass fall into
// distinct banks).  (12-piece slabs — a 44-channel head as ONE slab — were tried: 180 registers, two workgroups per CU,
// 8 x 44 forward+backward 82 -> 88 ms.)
template <int Q> struct DotTile { static constexpr int ld = Q * 4 + 4; };

#ifndef GGL_EMULATE
// One slab = NQ float4s (4 NQ columns) of every item's x strip.  NQ is a compile-time constant: the slab lives in
// registers between its loads and its LDS stores, nothing is indexed at run time (the first version indexed a shared
// register array under a run-time bound and the backend put it in scratch memory: 2x slower than the kernel it replaced).
template <int NQ>
__device__ __forceinline__ void slab_load(int tid, const int64_t *sx, const float *__restrict__ x, int64_t c0,
                                          float4 (&v)[NQ]) {
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    const int f = tid + kBlock * j, item = f / NQ, part = f - item * NQ;   // 8 consecutive lanes = 128 contiguous bytes
    const int64_t ox = sx[item];
    v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ox >= 0) v[j] = *reinterpret_cast<const float4 *>(x + ox + c0 + part * 4);
  }
}
// the same on the first NQ entries of the pipeline's 8-entry register slab (the narrower last slab of a strip)
template <int NQ, int Q>
__device__ __forceinline__ void slab_load_into(int tid, const int64_t *sx, const float *__restrict__ x, int64_t c0,
                                               float4 (&v)[Q]) {
  static_assert(NQ <= Q, "tail slab wider than the pipeline's");
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    const int f = tid + kBlock * j, item = f / NQ, part = f - item * NQ;
    const int64_t ox = sx[item];
    v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ox >= 0) v[j] = *reinterpret_cast<const float4 *>(x + ox + c0 + part * 4);
  }
}
template <int NQ, int LD, int Q>
__device__ __forceinline__ void slab_store_from(int tid, const float4 (&v)[Q], float (*tx)[LD]) {
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    const int f = tid + kBlock * j, item = f / NQ, part = f - item * NQ;
    *reinterpret_cast<float4 *>(&tx[item][part * 4]) = v[j];
  }
}
template <int NQ, int LD>
__device__ __forceinline__ void slab_store(int tid, const float4 (&v)[NQ], float (*tx)[LD]) {
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    const int f = tid + kBlock * j, item = f / NQ, part = f - item * NQ;
    *reinterpret_cast<float4 *>(&tx[item][part * 4]) = v[j];
  }
}
// this lane's own item: its x slab from LDS, its g slab straight from memory (the g strips of a batch of sorted
// positions are a handful of destination rows: lanes that share a row read the same addresses, L1 serves them)
template <int NQ, int LD>
__device__ __forceinline__ float slab_fold(int tid, float (*tx)[LD], const float *__restrict__ gp, bool valid,
                                           float acc) {
  float4 gg[NQ];
#pragma unroll
  for (int k = 0; k < NQ; ++k) {
    gg[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid) gg[k] = *reinterpret_cast<const float4 *>(gp + k * 4);
  }
#pragma unroll
  for (int k = 0; k < NQ; ++k) {
    const float4 a = *reinterpret_cast<const float4 *>(&tx[tid][k * 4]);
    acc = __fadd_rn(acc, __fmul_rn(a.x, gg[k].x));
    acc = __fadd_rn(acc, __fmul_rn(a.y, gg[k].y));
    acc = __fadd_rn(acc, __fmul_rn(a.z, gg[k].z));
    acc = __fadd_rn(acc, __fmul_rn(a.w, gg[k].w));
  }
  return acc;
}
// TAIL = float4s of the strip's last, narrower slab (0 = the column range is whole slabs): a template parameter, so each
// instantiation carries one tail shape (a run-time switch over seven shapes inside one kernel cost 188 registers
// instead of ~120, i.e. half the resident wavefronts)
template <int Q, int TAIL>
__global__ __launch_bounds__(kBlock) void bspmm_grad_w_sorted_kernel(
    const int32_t *__restrict__ col, const int32_t *__restrict__ rowidx, const int32_t *__restrict__ perm,
    const float *__restrict__ x, const float *__restrict__ g, int64_t total, int64_t H, int64_t C, int64_t c_lo,
    int64_t c_hi, const float *__restrict__ carry_in, float *__restrict__ carry_out, float *__restrict__ gw) {
  constexpr int kDotQ = Q, kDotLd = DotTile<Q>::ld;
  __shared__ __attribute__((aligned(16))) float tx[kBlock][kDotLd];   // Q = 8: 36 KiB, four workgroups per CU
  __shared__ int64_t sx[kBlock];
  const int tid = threadIdx.x;
  const int64_t base = block_id() * (int64_t)kBlock;
  if (base >= total) return;
  const int64_t i = base + tid;
  const bool valid = i < total;
  int64_t p = 0, h = 0;
  if (valid) {
    p = i / H;
    h = i - p * H;
  }
  sx[tid] = valid ? ((int64_t)col[p] * H + h) * C : (int64_t)-1;
  const float *gp = g + (valid ? ((int64_t)rowidx[p] * H + h) * C : 0);
  float acc = (valid && carry_in) ? carry_in[i] : 0.0f;   // the chain so far (sorted order: coalesced)
  __syncthreads();
  int64_t c0 = c_lo;
  const int64_t n_full = (c_hi - c_lo) / (kDotQ * 4);
  // software pipeline: the next slab's loads (a full one, or the tail) are in flight while the current one is folded
  float4 cur[kDotQ];
  if (n_full > 0) slab_load<kDotQ>(tid, sx, x, c0, cur);
  else if constexpr (TAIL > 0) slab_load_into<TAIL>(tid, sx, x, c0, cur);
  for (int64_t s = 0; s < n_full; ++s) {
    slab_store<kDotQ, kDotLd>(tid, cur, tx);
    __syncthreads();
    if (s + 1 < n_full) slab_load<kDotQ>(tid, sx, x, c0 + kDotQ * 4, cur);
    else if constexpr (TAIL > 0) slab_load_into<TAIL>(tid, sx, x, c0 + kDotQ * 4, cur);
    acc = slab_fold<kDotQ, kDotLd>(tid, tx, gp + c0, valid, acc);
    __syncthreads();
    c0 += kDotQ * 4;
  }
  if constexpr (TAIL > 0) {
    slab_store_from<TAIL, kDotLd>(tid, cur, tx);
    __syncthreads();
    acc = slab_fold<TAIL, kDotLd>(tid, tx, gp + c0, valid, acc);
  }
  if (!valid) return;
  if (carry_out) carry_out[i] = acc;
  else gw[(perm ? (int64_t)perm[p] : p) * H + h] = acc;
}
#endif

// the same walk one item per thread, strips read in place: the host-emulation build's stand-in (its "threads" run one
// after another: no LDS, no barriers) and the route for strips that are not made of aligned float4s
__global__ __launch_bounds__(kBlock) void bspmm_grad_w_sorted_plain_kernel(
    const int32_t *__restrict__ col, const int32_t *__restrict__ rowidx, const int32_t *__restrict__ perm,
    const float *__restrict__ x, const float *__restrict__ g, int64_t total, int64_t H, int64_t C,
    float *__restrict__ gw) {
  const int64_t stride = grid_threads();
  for (int64_t i = thread_id(); i < total; i += stride) {
    const int64_t p = i / H, h = i - p * H;
    const float *xr = x + ((int64_t)col[p] * H + h) * C;
    const float *gr = g + ((int64_t)rowidx[p] * H + h) * C;
    const int64_t oi = (perm ? (int64_t)perm[p] : p) * H + h;
    float acc = 0.0f;
    for (int64_t c = 0; c < C; ++c) acc = __fadd_rn(acc, __fmul_rn(xr[c], gr[c]));
    gw[oi] = acc;
  }
}

// ---- gspmm's weight gradient on 16-bit storage (see the header) ---------------------------------------------------------
template <typename T> struct dot_elem { using type = uint16_t; };
template <> struct dot_elem<float> { using type = float; };

#ifndef GGL_EMULATE
// eight consecutive columns of a strip, widened: two float4 of an f32 strip, one 16-byte piece of a 16-bit one
template <typename T> struct Dot8 {
  static constexpr int pieces = 1;   // 16-byte pieces per 8 columns
  static __device__ __forceinline__ void widen(const uint4 (&q)[1], float (&o)[8]) {
    const uint32_t w[4] = {q[0].x, q[0].y, q[0].z, q[0].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[2 * j] = TT<T>::load((uint16_t)(w[j] & 0xffffu));
      o[2 * j + 1] = TT<T>::load((uint16_t)(w[j] >> 16));
    }
  }
};
template <> struct Dot8<float> {
  static constexpr int pieces = 2;
  static __device__ __forceinline__ void widen(const uint4 (&q)[2], float (&o)[8]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      o[4 * j] = __uint_as_float(q[j].x);
      o[4 * j + 1] = __uint_as_float(q[j].y);
      o[4 * j + 2] = __uint_as_float(q[j].z);
      o[4 * j + 3] = __uint_as_float(q[j].w);
    }
  }
};
// NP 16-byte pieces of every item's x strip, starting at byte offset `b0` of the strip: consecutive lanes read
// consecutive pieces of one item (NP = 4: 64 contiguous bytes per 4 lanes; 8: 128 per 8)
template <int NP, int Q>
__device__ __forceinline__ void pieces_load(int tid, const int64_t *sx, const char *__restrict__ x, int64_t b0,
                                            uint4 (&v)[Q]) {
  static_assert(NP <= Q, "tail slab wider than the pipeline's");
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int f = tid + kBlock * j, item = f / NP, part = f - item * NP;
    const int64_t ox = sx[item];
    v[j] = make_uint4(0u, 0u, 0u, 0u);
    if (ox >= 0) v[j] = *reinterpret_cast<const uint4 *>(x + ox + b0 + part * 16);
  }
}
template <int NP, int Q>
__device__ __forceinline__ void pieces_store(int tid, const uint4 (&v)[Q], uint4 (*tx)[Q + 1]) {
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int f = tid + kBlock * j, item = f / NP, part = f - item * NP;
    tx[item][part] = v[j];
  }
}
// this lane's own item over NU units of 8 columns: x from the LDS tile, g straight from memory (see slab_fold)
template <typename XT, typename GT, int NU, int Q>
__device__ __forceinline__ float units_fold(int tid, uint4 (*tx)[Q + 1], const char *__restrict__ gp, bool valid, float acc) {
  constexpr int PX = Dot8<XT>::pieces, PG = Dot8<GT>::pieces;
  uint4 gq[NU][PG];
#pragma unroll
  for (int u = 0; u < NU; ++u)
#pragma unroll
    for (int j = 0; j < PG; ++j) {
      gq[u][j] = make_uint4(0u, 0u, 0u, 0u);
      if (valid) gq[u][j] = *reinterpret_cast<const uint4 *>(gp + (u * PG + j) * 16);
    }
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    uint4 xq[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) xq[j] = tx[tid][u * PX + j];
    float a[8], b[8];
    Dot8<XT>::widen(xq, a);
    Dot8<GT>::widen(gq[u], b);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc = __fadd_rn(acc, __fmul_rn(a[k], b[k]));
  }
  return acc;
}
// The walk of bspmm_grad_w_sorted_kernel with one head, in units of 8 columns; XT / GT = float, mxbf16_t or mxf16_t (at
// least one of them 16-bit).  A slab is 4 units (32 columns); TAIL = units of the column range's last, narrower slab.
template <typename XT, typename GT, int TAIL>
__global__ __launch_bounds__(kBlock) void dot16_kernel(
    const int32_t *__restrict__ col, const int32_t *__restrict__ rowidx, const int32_t *__restrict__ perm,
    const char *__restrict__ x, const char *__restrict__ g, int64_t E, int64_t K, int64_t c_lo, int64_t c_hi,
    const float *__restrict__ carry_in, float *__restrict__ carry_out, float *__restrict__ gw) {
  constexpr int kUnits = 4, PX = Dot8<XT>::pieces, Q = kUnits * PX;
  constexpr int64_t xs = sizeof(typename dot_elem<XT>::type), gs = sizeof(typename dot_elem<GT>::type);
  __shared__ __attribute__((aligned(16))) uint4 tx[kBlock][Q + 1];   // 16-bit x: 20 KiB; f32 x: 36 KiB
  __shared__ int64_t sx[kBlock];                                     // byte offset of the item's x strip
  const int tid = threadIdx.x;
  const int64_t base = block_id() * (int64_t)kBlock;
  if (base >= E) return;
  const int64_t p = base + tid;
  const bool valid = p < E;
  sx[tid] = valid ? (int64_t)col[p] * K * xs : (int64_t)-1;
  const char *gp = g + (valid ? (int64_t)rowidx[p] * K * gs : 0);
  float acc = (valid && carry_in) ? carry_in[p] : 0.0f;
  __syncthreads();
  int64_t c0 = c_lo;
  const int64_t n_full = (c_hi - c_lo) / (kUnits * 8);
  uint4 cur[Q];
  if (n_full > 0) pieces_load<Q, Q>(tid, sx, x, c0 * xs, cur);
  else if constexpr (TAIL > 0) pieces_load<TAIL * PX, Q>(tid, sx, x, c0 * xs, cur);
  for (int64_t s = 0; s < n_full; ++s) {
    pieces_store<Q, Q>(tid, cur, tx);
    __syncthreads();
    if (s + 1 < n_full) pieces_load<Q, Q>(tid, sx, x, (c0 + kUnits * 8) * xs, cur);
    else if constexpr (TAIL > 0) pieces_load<TAIL * PX, Q>(tid, sx, x, (c0 + kUnits * 8) * xs, cur);
    acc = units_fold<XT, GT, kUnits, Q>(tid, tx, gp + c0 * gs, valid, acc);
    __syncthreads();
    c0 += kUnits * 8;
  }
  if constexpr (TAIL > 0) {
    pieces_store<TAIL * PX, Q>(tid, cur, tx);
    __syncthreads();
    acc = units_fold<XT, GT, TAIL, Q>(tid, tx, gp + c0 * gs, valid, acc);
  }
  if (!valid) return;
  if (carry_out) carry_out[p] = acc;
  else gw[perm ? (int64_t)perm[p] : p] = acc;
}
#endif

// one edge per thread, strips read in place and widened element by element: the host build's form for every dtype
// pair, and the GPU's for strips that are not aligned 8-column units
template <typename XT, typename GT>
__global__ __launch_bounds__(kBlock) void dot16_plain_kernel(
    const int32_t *__restrict__ col, const int32_t *__restrict__ rowidx, const int32_t *__restrict__ perm,
    const typename dot_elem<XT>::type *__restrict__ x, const typename dot_elem<GT>::type *__restrict__ g, int64_t E,
    int64_t K, float *__restrict__ gw) {
  const int64_t stride = grid_threads();
  for (int64_t p = thread_id(); p < E; p += stride) {
    const auto *xr = x + (int64_t)col[p] * K;
    const auto *gr = g + (int64_t)rowidx[p] * K;
    float acc = 0.0f;
    for (int64_t k = 0; k < K; ++k) acc = __fadd_rn(acc, __fmul_rn(TT<XT>::load(xr[k]), TT<GT>::load(gr[k])));
    gw[perm ? (int64_t)perm[p] : p] = acc;
  }
}

// mean: out[r, :] = widen(g[r, :]) / count(r), the rounded f32 divide of ggl_spmm_mean_bwd; a row without edges is read by
// no edge and is copied as it is
template <typename GT>
__global__ __launch_bounds__(kBlock) void dot_prescale_kernel(const typename dot_elem<GT>::type *__restrict__ g,
                                                              const int64_t *__restrict__ rowptr, int64_t N, int64_t K,
                                                              float *__restrict__ out) {
  const int64_t stride = grid_threads(), total = N * K;
  for (int64_t i = thread_id(); i < total; i += stride) {
    const int64_t r = i / K;
    const int64_t n = rowptr[r + 1] - rowptr[r];
    const float v = TT<GT>::load(g[i]);
    out[i] = n > 0 ? __fdiv_rn(v, TT<float>::count(n)) : v;
  }
}

}  // namespace ggl

using namespace ggl;

// gw[e, h] for the edges of `plan` (destination-sorted; plan->perm maps sorted positions back to the caller's edge
// order, NULL = already sorted), `col` / `rowidx` = source / destination node of every sorted position.
static int64_t dot_block_width(int64_t E, int64_t N, int64_t C) {   // C = one launch
#ifdef GGL_EMULATE
  (void)E; (void)N;
  return C;
#else
  // the block width is an A/B knob (ggl_set_option "col_block"): the slab loads are float4 and the tail template covers
  // (width % 32) / 4 quads, so a width that is not a multiple of 4 would drop columns from the dot — such a setting
  // runs as ONE launch here instead
  const int64_t bw = options().col_block;
  if (bw > 0 && bw % 4 == 0 && C % 4 == 0 && C >= 2 * bw && N > 0 &&
      E >= options().col_block_min_degree * N && E >= options().col_block_min_edges)
    return bw;
  return C;
#endif
}

// bytes of `scratch` the call below wants (0: it runs as one launch and needs none)
extern "C" size_t ggl_bspmm_grad_w_sorted_scratch_bytes(int64_t E, int64_t N, int64_t H, int64_t C) {
  return dot_block_width(E, N, C) < C ? (size_t)E * (size_t)H * sizeof(float) : 0;
}

extern "C" int ggl_bspmm_grad_w_sorted(const ggl_segplan_t *plan, const int32_t *col, const int32_t *rowidx,
                                       const float *x, const float *g, int64_t H, int64_t C, float *gw,
                                       float *scratch, void *stream) {
  GGL_REQUIRE(plan != nullptr && H > 0 && C > 0 && plan->E >= 0, GGL_EINVAL, "bad sizes");
  const int64_t E = plan->E;
  if (E == 0) return GGL_OK;
  GGL_REQUIRE(col && rowidx && x && g && gw, GGL_EINVAL, "NULL pointer");
  const int64_t total = E * H;
  hipStream_t s = as_stream(stream);
  const bool vec = (C % 4 == 0) && aligned16(x) && aligned16(g) &&
                   !options().force_generic;
#ifndef GGL_EMULATE
  if (vec) {
    // wide strips in 64-column blocks (see the header): only where there are hub rows to keep in L2
    const int64_t bw = scratch ? dot_block_width(E, plan->N, C) : C;
    for (int64_t c0 = 0; c0 < C; c0 += bw) {
      const int64_t c1 = (c0 + bw < C) ? c0 + bw : C;
      const float *cin = c0 > 0 ? scratch : nullptr;
      float *cout = c1 < C ? scratch : nullptr;
#define GGL_DOT_LAUNCH(T)                                                                                         \
  GGL_LAUNCH((bspmm_grad_w_sorted_kernel<8, T>), ceil_div(total, (int64_t)kBlock), kBlock, s, col, rowidx, plan->perm, x, \
             g, total, H, C, c0, c1, cin, cout, gw)
      switch ((int)(((c1 - c0) % 32) / 4)) {
        case 0: GGL_DOT_LAUNCH(0); break;
        case 1: GGL_DOT_LAUNCH(1); break;
        case 2: GGL_DOT_LAUNCH(2); break;
        case 3: GGL_DOT_LAUNCH(3); break;
        case 4: GGL_DOT_LAUNCH(4); break;
        case 5: GGL_DOT_LAUNCH(5); break;
        case 6: GGL_DOT_LAUNCH(6); break;
        default: GGL_DOT_LAUNCH(7); break;
      }
#undef GGL_DOT_LAUNCH
      GGL_LAUNCH_CHECK();
    }
    return GGL_OK;
  }
#endif
  (void)vec;
  int64_t grid = ceil_div(total, (int64_t)kBlock);
  if (grid > 4096) grid = 4096;
  (void)scratch;
  GGL_LAUNCH((bspmm_grad_w_sorted_plain_kernel), grid, kBlock, s, col, rowidx, plan->perm, x, g, total, H, C, gw);
  GGL_LAUNCH_CHECK();
  return GGL_OK;
}

// ---- gspmm's weight gradient ------------------------------------------------------------------------------------------------
static bool dot_dtype_ok(int d) { return d == GGL_F32 || d == GGL_BF16 || d == GGL_F16; }
static size_t align16(size_t b) { return (b + 15u) & ~(size_t)15u; }
// column-block width of the walk over x rows of `x_dtype` (K = one launch): the f32 kernels' own rule, and for 16-bit x
// the blocks of the 16-bit aggregate (option col_block16: the same 256-byte slices), under the same thresholds
static int64_t gradw_block_width(int64_t E, int64_t N, int64_t K, int x_dtype) {
  if (x_dtype == GGL_F32) return dot_block_width(E, N, K);
#ifdef GGL_EMULATE
  return K;
#else
  const int64_t bw = options().col_block16;
  if (bw > 0 && bw % 8 == 0 && K % 8 == 0 && K >= 2 * bw && N > 0 && E >= options().col_block_min_degree * N &&
      E >= options().col_block_min_edges)
    return bw;
  return K;
#endif
}
static size_t gradw_carry_bytes(int64_t E, int64_t N, int64_t K, int x_dtype) {
  return gradw_block_width(E, N, K, x_dtype) < K ? align16((size_t)E * sizeof(float)) : 0;
}

extern "C" size_t ggl_spmm_grad_w_scratch_bytes(int64_t E, int64_t N_dst, int64_t K, int x_dtype, int mean) {
  if (E <= 0 || K <= 0) return 0;
  return gradw_carry_bytes(E, N_dst, K, x_dtype) + (mean ? (size_t)N_dst * (size_t)K * sizeof(float) : 0);
}

template <typename XT, typename GT>
static int gradw16_launch(const ggl_segplan_t *plan, const int32_t *col, const int32_t *rowidx, const void *x,
                          const void *g, int64_t K, float *gw, float *carry, hipStream_t s) {
  const int64_t E = plan->E;
#ifndef GGL_EMULATE
  const bool vec = (K % 8 == 0) && aligned16(x) && aligned16(g) &&
                   !options().force_generic;
  if (vec) {
    // this kernel walks in units of 8 columns and its tail template covers (width % 32) / 8 units: a block width that is
    // a multiple of 4 only (option col_block: the f32 kernels' rule, which sizes the scratch of an f32 x) would drop
    // columns from the dot and misalign the next block's 16-byte pieces — such a setting runs as ONE launch here
    int64_t bw = carry ? gradw_block_width(E, plan->N, K, mx_code<XT>::value ? mx_code<XT>::value : GGL_F32) : K;
    if (bw % 8 != 0) bw = K;
    for (int64_t c0 = 0; c0 < K; c0 += bw) {
      const int64_t c1 = (c0 + bw < K) ? c0 + bw : K;
      const float *cin = c0 > 0 ? carry : nullptr;
      float *cout = c1 < K ? carry : nullptr;
#define GGL_DOT16_LAUNCH(T)                                                                                              \
  GGL_LAUNCH((dot16_kernel<XT, GT, T>), ceil_div(E, (int64_t)kBlock), kBlock, s, col, rowidx, plan->perm,                 \
             static_cast<const char *>(x), static_cast<const char *>(g), E, K, c0, c1, cin, cout, gw)
      switch ((int)(((c1 - c0) % 32) / 8)) {
        case 0: GGL_DOT16_LAUNCH(0); break;
        case 1: GGL_DOT16_LAUNCH(1); break;
        case 2: GGL_DOT16_LAUNCH(2); break;
        default: GGL_DOT16_LAUNCH(3); break;
      }
#undef GGL_DOT16_LAUNCH
      GGL_LAUNCH_CHECK();
    }
    return GGL_OK;
  }
#endif
  (void)carry;
  int64_t grid = ceil_div(E, (int64_t)kBlock);
  if (grid > 4096) grid = 4096;
  GGL_LAUNCH((dot16_plain_kernel<XT, GT>), grid, kBlock, s, col, rowidx, plan->perm,
             static_cast<const typename dot_elem<XT>::type *>(x), static_cast<const typename dot_elem<GT>::type *>(g), E, K,
             gw);
  GGL_LAUNCH_CHECK();
  return GGL_OK;
}

// gw[e] = sum_k x[src_e, k] * g[dst_e, k] (mean_rowptr != NULL: g[dst_e, k] / count(dst_e)) along the destination-sorted
// forward plan; include/ggl_mpops.h has the contract
extern "C" int ggl_spmm_grad_w(const ggl_segplan_t *plan, const int32_t *col, const int32_t *rowidx, int x_dtype,
                               const void *x, int g_dtype, const void *g, const int64_t *mean_rowptr, int64_t K,
                               float *gw, void *scratch, void *stream) {
  GGL_REQUIRE(plan != nullptr && K > 0 && plan->E >= 0, GGL_EINVAL, "bad sizes");
  GGL_REQUIRE(dot_dtype_ok(x_dtype) && dot_dtype_ok(g_dtype), GGL_EDTYPE,
              "spmm_grad_w: x and g are f32, bf16 or f16 (got dtype codes %d, %d)", x_dtype, g_dtype);
  const int64_t E = plan->E, N = plan->N;
  if (E == 0) return GGL_OK;
  GGL_REQUIRE(col && rowidx && x && g && gw, GGL_EINVAL, "NULL pointer");
  hipStream_t s = as_stream(stream);
  const size_t carry_bytes = gradw_carry_bytes(E, N, K, x_dtype);
  GGL_REQUIRE(scratch || (!mean_rowptr && carry_bytes == 0), GGL_EINVAL,
              "spmm_grad_w: scratch of ggl_spmm_grad_w_scratch_bytes() bytes required");
  float *carry = carry_bytes ? static_cast<float *>(scratch) : nullptr;
  if (mean_rowptr) {
    float *panel = reinterpret_cast<float *>(static_cast<char *>(scratch) + carry_bytes);
    int64_t grid = ceil_div(N * K, (int64_t)kBlock);
    if (grid > 16384) grid = 16384;
    if (N * K > 0) {
      if (g_dtype == GGL_F32)
        GGL_LAUNCH((dot_prescale_kernel<float>), grid, kBlock, s, static_cast<const float *>(g), mean_rowptr, N, K, panel);
      else if (g_dtype == GGL_BF16)
        GGL_LAUNCH((dot_prescale_kernel<mxbf16_t>), grid, kBlock, s, static_cast<const uint16_t *>(g), mean_rowptr, N, K, panel);
      else
        GGL_LAUNCH((dot_prescale_kernel<mxf16_t>), grid, kBlock, s, static_cast<const uint16_t *>(g), mean_rowptr, N, K, panel);
      GGL_LAUNCH_CHECK();
    }
    g = panel;
    g_dtype = GGL_F32;
  }
  if (x_dtype == GGL_F32 && g_dtype == GGL_F32)   // one head of bspmm's gradient: the same kernels, the same bits
    return ggl_bspmm_grad_w_sorted(plan, col, rowidx, static_cast<const float *>(x), static_cast<const float *>(g), 1, K,
                                   gw, carry, stream);
#define GGL_GRADW16(XT, GT) return gradw16_launch<XT, GT>(plan, col, rowidx, x, g, K, gw, carry, s)
  if (x_dtype == GGL_F32) {
    if (g_dtype == GGL_BF16) GGL_GRADW16(float, mxbf16_t);
    GGL_GRADW16(float, mxf16_t);
  }
  if (x_dtype == GGL_BF16) {
    if (g_dtype == GGL_F32) GGL_GRADW16(mxbf16_t, float);
    if (g_dtype == GGL_BF16) GGL_GRADW16(mxbf16_t, mxbf16_t);
    GGL_GRADW16(mxbf16_t, mxf16_t);
  }
  if (g_dtype == GGL_F32) GGL_GRADW16(mxf16_t, float);
  if (g_dtype == GGL_BF16) GGL_GRADW16(mxf16_t, mxbf16_t);
  GGL_GRADW16(mxf16_t, mxf16_t);
#undef GGL_GRADW16
}
