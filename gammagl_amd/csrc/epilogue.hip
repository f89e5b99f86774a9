// gammagl_amd/csrc/epilogue.hip — the elementwise step right after every aggregate:
//   GCNConv: out += bias (gcn_conv.py:105-106); GCNModel: relu -> dropout (models/gcn.py:55-59);
//   SAGEConv: + bias, activation (sage_conv.py:102-106).
// torch runs this as add, clamp, dropout (+ a bool mask) forward and masked_scale, threshold, sum(0)
// backward: six passes over [N,K] per hidden layer (measured 4.0 ms of a 110 ms products-sized step,
// profiles/r1_bench_products_summary.txt).  Here it is one pass each way:
//   forward : y = keep(i) * relu(a + bias) / (1 - p)        keep(i) from Philox4x32-10(seed, offset; i)
//   backward: ga = keep(i) * [relu ? y > 0 : 1] * g / (1 - p): the dropout mask is REDRAWN from the
//             {seed, offset} the forward read (no mask tensor is stored; y only tells where the ReLU
//             clipped), and the bias gradient = column sums of ga accumulated in the same pass (two
//             deterministic stages, as in ggl_colsum_f32).
// The RNG state (seed, offset) lives in device memory and is advanced by a one-thread kernel after every
// forward, so a captured hipGraph draws a fresh mask on each replay.  No LDS, no atomics.
#include "common.hpp"

namespace ggl {

// T = float, or mxbf16_t / mxf16_t (common.hpp): 16-bit STORAGE of a / y / g / ga, widened at the load, every operation the
// f32 one, one rounding at the store (ggl_bias_act_{fwd,bwd}_x16).  Four columns per lane either way — an 8-byte access at
// 16 bits — so the row-to-partial geometry, and with it every bit of gbias, is the f32 kernel's.
struct alignas(8) H4 { uint16_t v[4]; };
template <typename T, int VEC> __device__ __forceinline__ void ldv(const typename TT<T>::S *__restrict__ p, float (&t)[VEC]) {
  if constexpr (!std::is_same<T, float>::value) {
    if (VEC == 4) {
      const H4 v = *reinterpret_cast<const H4 *>(p);   // global_load_dwordx2
      t[0] = TT<T>::load(v.v[0]); t[1 % VEC] = TT<T>::load(v.v[1]); t[2 % VEC] = TT<T>::load(v.v[2]); t[3 % VEC] = TT<T>::load(v.v[3]);
    } else {
      t[0] = TT<T>::load(p[0]);
    }
  } else if (VEC == 4) {
    const float4 v = *reinterpret_cast<const float4 *>(p);
    t[0] = v.x; t[1 % VEC] = v.y; t[2 % VEC] = v.z; t[3 % VEC] = v.w;
  } else {
    t[0] = p[0];
  }
}
template <typename T, int VEC> __device__ __forceinline__ void stv(typename TT<T>::S *__restrict__ p, const float (&t)[VEC]) {
  if constexpr (!std::is_same<T, float>::value) {
    if (VEC == 4) {
      H4 o;
      o.v[0] = TT<T>::store(t[0]); o.v[1] = TT<T>::store(t[1 % VEC]); o.v[2] = TT<T>::store(t[2 % VEC]); o.v[3] = TT<T>::store(t[3 % VEC]);
      *reinterpret_cast<H4 *>(p) = o;
    } else {
      p[0] = TT<T>::store(t[0]);
    }
  } else if (VEC == 4) {
    float4 o;
    o.x = t[0]; o.y = t[1 % VEC]; o.z = t[2 % VEC]; o.w = t[3 % VEC];
    *reinterpret_cast<float4 *>(p) = o;
  } else {
    p[0] = t[0];
  }
}
constexpr int kRowUnroll = 4;  // rows in flight per lane: the loads of 4 rows are issued before any is used

// Threads of a block are `groups` groups of `kp` lanes; a lane owns VEC consecutive columns (loaded once
// from bias), a group walks rows r0 + j, + groups, ...  Random word for vector (r, c): Philox(r * KV + c).
template <typename T, int VEC>
__global__ __launch_bounds__(kBlock) void bias_act_fwd_kernel(const typename TT<T>::S *__restrict__ a,
                                                              const float *__restrict__ bias,
                                                              const int64_t *__restrict__ rng,
                                                              typename TT<T>::S *__restrict__ y, int64_t N, int64_t K,
                                                              int64_t nblocks, int64_t rows_per_block, int kp,
                                                              int groups,
                                                              int relu, uint32_t drop_thresh, float scale) {
  const int j = threadIdx.x / kp;
  const int c0 = threadIdx.x - j * kp;
  if (j >= groups) return;
  const int64_t KV = (K + VEC - 1) / VEC;  // vectors per row (VEC = 4 only when K % 4 == 0)
  const int ev = (K % 4 == 0) ? 4 : 1;     // elements per dropout word vector
  const int64_t KVm = K / ev;
  const int64_t r0 = block_id() * rows_per_block;
  if (block_id() >= nblocks) return;  // padding block of a folded grid
  const int64_t r1 = (r0 + rows_per_block < N) ? r0 + rows_per_block : N;
  const uint64_t seed = drop_thresh ? (uint64_t)rng[0] : 0, offset = drop_thresh ? (uint64_t)rng[1] : 0;
  for (int64_t c = c0; c < KV; c += kp) {
    float b[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) b[i] = bias ? bias[c * VEC + i] : 0.0f;
    auto finish = [&](int64_t r, float (&t)[VEC]) {
      uint32_t rw[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
      if (drop_thresh) {
        // the word of element (r, k) depends on K alone (vectors of 4 when K % 4 == 0), not on which kernel
        // variant the pointer alignment selected: the fused SpMM epilogue and the backward draw the same mask
        const U4 u = philox4x32_10((uint64_t)(r * KVm + (c * VEC) / ev), offset, seed);
        rw[0] = u.x; rw[1] = u.y; rw[2] = u.z; rw[3] = u.w;
        if (VEC == 1) rw[0] = rw[(c * VEC) % ev];
      }
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        float v = bias ? __fadd_rn(t[i], b[i]) : t[i];
        if (relu) v = (v < 0.0f) ? 0.0f : v;  // NaN stays NaN, as torch.relu / clamp_min(0)
        if (drop_thresh) v = (rw[i] >= drop_thresh) ? __fmul_rn(v, scale) : 0.0f;  // keep with prob 1 - p
        t[i] = v;
      }
      stv<T, VEC>(y + r * K + c * VEC, t);
    };
    int64_t r = r0 + j;
    for (; r + (int64_t)(kRowUnroll - 1) * groups < r1; r += (int64_t)kRowUnroll * groups) {
      float t[kRowUnroll][VEC];
#pragma unroll
      for (int u = 0; u < kRowUnroll; ++u) ldv<T, VEC>(a + (r + (int64_t)u * groups) * K + c * VEC, t[u]);
#pragma unroll
      for (int u = 0; u < kRowUnroll; ++u) finish(r + (int64_t)u * groups, t[u]);
    }
    for (; r < r1; r += groups) {
      float t[VEC];
      ldv<T, VEC>(a + r * K + c * VEC, t);
      finish(r, t);
    }
  }
}

__global__ void rng_advance_kernel(int64_t *rng, int64_t inc) {
  if (block_id() == 0 && threadIdx.x == 0) rng[1] += inc;
}

// One finished vector of the backward: mask and scale the VEC gradients gv of row r, vector c (the three mask modes below),
// add them to the lane's running column sums and store them.  Shared by bias_act_bwd_kernel, whose gv is a loaded
// gradient, and linear_bias_act_bwd_kernel, whose gv is the g . W it formed in registers: one body, the same bits.
template <typename T, int VEC, int MASKED>
__device__ __forceinline__ void bwd_finish(int64_t r, int64_t c, float (&gv)[VEC], const float (&yv)[VEC], float (&acc)[VEC],
                                           typename TT<T>::S *__restrict__ ga, int64_t K, int64_t KVm, int ev, float scale,
                                           const int64_t *__restrict__ rng, uint32_t drop_thresh) {
  constexpr int masked = MASKED;  // compile-time: the common ReLU case carries no Philox code at all
  uint32_t rw[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  if (MASKED == 3) {  // the mask the forward drew: same word for vector (r, c)
    const U4 u = philox4x32_10((uint64_t)(r * KVm + (c * VEC) / ev), (uint64_t)rng[1], (uint64_t)rng[0]);
    rw[0] = u.x; rw[1] = u.y; rw[2] = u.z; rw[3] = u.w;
    if (VEC == 1) rw[0] = rw[(c * VEC) % ev];
  }
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    // masked: 1 = y > 0 (ReLU, with or without dropout: exact), 2 = y != 0 (dropout without ReLU and
    // without an rng state), 3 = redrawn dropout mask (dropout without ReLU)
    if (masked == 1) gv[i] = (yv[i] > 0.0f) ? __fmul_rn(gv[i], scale) : 0.0f;
    else if (masked == 2) gv[i] = (yv[i] != 0.0f) ? __fmul_rn(gv[i], scale) : 0.0f;
    else if (masked == 3) gv[i] = (rw[i] >= drop_thresh) ? __fmul_rn(gv[i], scale) : 0.0f;
    acc[i] = __fadd_rn(acc[i], gv[i]);  // rows in ascending order, unrolled or not
  }
  stv<T, VEC>(ga + r * K + c * VEC, gv);
}

// backward + first stage of the bias gradient.  Same thread geometry as the forward; every lane keeps a
// running column sum of the ga values it produces and writes it to partial[(block * groups + j), :];
// ggl_colsum_f32 (backward.hip) then reduces the [P, K] partial matrix.
template <typename T, int VEC, int MASKED>
__global__ __launch_bounds__(kBlock) void bias_act_bwd_kernel(const typename TT<T>::S *__restrict__ g,
                                                              const typename TT<T>::S *__restrict__ y,
                                                              typename TT<T>::S *__restrict__ ga, int64_t N,
                                                              int64_t K, int64_t nblocks,
                                                              int64_t rows_per_block, int kp,
                                                              int groups, float scale,
                                                              const int64_t *__restrict__ rng,
                                                              uint32_t drop_thresh,
                                                              float *__restrict__ partial) {
  const int j = threadIdx.x / kp;
  const int c0 = threadIdx.x - j * kp;
  if (j >= groups) return;
  const int64_t KV = (K + VEC - 1) / VEC;
  const int ev = (K % 4 == 0) ? 4 : 1;
  const int64_t KVm = K / ev;
  const int64_t r0 = block_id() * rows_per_block;
  if (block_id() >= nblocks) return;  // padding block of a folded grid
  const int64_t r1 = (r0 + rows_per_block < N) ? r0 + rows_per_block : N;
  for (int64_t c = c0; c < KV; c += kp) {
    float acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
    auto finish = [&](int64_t r, float (&gv)[VEC], const float (&yv)[VEC]) {
      bwd_finish<T, VEC, MASKED>(r, c, gv, yv, acc, ga, K, KVm, ev, scale, rng, drop_thresh);
    };
    int64_t r = r0 + j;
    for (; r + (int64_t)(kRowUnroll - 1) * groups < r1; r += (int64_t)kRowUnroll * groups) {
      float gv[kRowUnroll][VEC], yv[kRowUnroll][VEC];
#pragma unroll
      for (int u = 0; u < kRowUnroll; ++u) {
        ldv<T, VEC>(g + (r + (int64_t)u * groups) * K + c * VEC, gv[u]);
        if (MASKED == 1 || MASKED == 2) ldv<T, VEC>(y + (r + (int64_t)u * groups) * K + c * VEC, yv[u]);
        else yv[u][0] = 0.0f;
      }
#pragma unroll
      for (int u = 0; u < kRowUnroll; ++u) finish(r + (int64_t)u * groups, gv[u], yv[u]);
    }
    for (; r < r1; r += groups) {
      float gv[VEC], yv[VEC];
      ldv<T, VEC>(g + r * K + c * VEC, gv);
      if (MASKED == 1 || MASKED == 2) ldv<T, VEC>(y + r * K + c * VEC, yv);
      else yv[0] = 0.0f;
      finish(r, gv, yv);
    }
    if (partial) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) partial[(block_id() * groups + j) * K + c * VEC + i] = acc[i];
    }
  }
}

// The output layer's input gradient formed inside that pass: s[r, :] = g[r, 0:J] . w[0:J, :] (serial fmas, ascending j,
// from 0.0f) takes the place of the loaded gradient and bwd_finish does the rest, so (ga, partial) are
// bias_act_bwd_kernel<float, 4, MASKED>'s on s, bit for bit — same geometry, same rows per (block, group), ascending.
// The [N, K] product is never written: at K = 256, J = 47 the pass moves g (0.19 KB a row) + y + ga instead of
// s written, s read, y, ga.  w is staged once per block in LDS; a lane carries kLinRows rows, so one 16-byte LDS read
// of w[j, 4c..4c+3] feeds 4 x kLinRows fmas (8 rows: the LDS pipe of a CU then has half the work of its vector pipes,
// at 4 they tie), and the y loads of those rows are issued before the j loop and consumed behind it.
// UNIFORM (a wavefront's lanes share their row and are all live: kp % 64 == 0, KV % kp == 0): lane l loads g[r, l]
// once, coalesced, and g[r, j] comes out of that register with v_readlane; otherwise every lane reads its row's g[r, j].
// The host build reads w and g where they lie (no LDS, no cross-lane reads there).
constexpr int kLinRows = 8;
template <int R, int MASKED, bool UNIFORM>
__device__ __forceinline__ void linear_rows(const float *__restrict__ g, int64_t g_ld, const float4 *wv,
                                            const float *__restrict__ y, float *__restrict__ ga, int64_t J, int64_t K,
                                            int64_t KV, int64_t c, int64_t r, int groups, float scale,
                                            const int64_t *__restrict__ rng, uint32_t drop_thresh, float (&acc)[4]) {
  float s[R][4], yv[R][4];
  float gl[R];
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const int64_t ru = r + (int64_t)u * groups;
    if (MASKED == 1 || MASKED == 2) ldv<float, 4>(y + ru * K + c * 4, yv[u]);
    else yv[u][0] = 0.0f;
    gl[u] = 0.0f;
#ifndef GGL_EMULATE
    if (UNIFORM) {
      const int lane = threadIdx.x & (kWave - 1);
      if (lane < J) gl[u] = g[ru * g_ld + lane];
    }
#endif
    s[u][0] = 0.0f; s[u][1] = 0.0f; s[u][2] = 0.0f; s[u][3] = 0.0f;
  }
  auto step = [&](int64_t jj) {
    const float4 wq = wv[jj * KV + c];
#pragma unroll
    for (int u = 0; u < R; ++u) {
      float gs;
#ifndef GGL_EMULATE
      if (UNIFORM) gs = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gl[u]), (int)jj));
      else
#endif
        gs = g[(r + (int64_t)u * groups) * g_ld + jj];
      s[u][0] = __fmaf_rn(gs, wq.x, s[u][0]);
      s[u][1] = __fmaf_rn(gs, wq.y, s[u][1]);
      s[u][2] = __fmaf_rn(gs, wq.z, s[u][2]);
      s[u][3] = __fmaf_rn(gs, wq.w, s[u][3]);
    }
  };
  // four steps a trip, written out (a loop around a cross-lane read is not unrolled with a remainder for the asking): the LDS
  // reads of the four go out in front of their fmas
  int64_t jj = 0;
  for (; jj + 4 <= J; jj += 4) {
    step(jj); step(jj + 1); step(jj + 2); step(jj + 3);
  }
  for (; jj < J; ++jj) step(jj);
#pragma unroll
  for (int u = 0; u < R; ++u)
    bwd_finish<float, 4, MASKED>(r + (int64_t)u * groups, c, s[u], yv[u], acc, ga, K, K / 4, 4, scale, rng, drop_thresh);
}

template <int MASKED, bool UNIFORM>
__global__ __launch_bounds__(kBlock) void linear_bias_act_bwd_kernel(const float *__restrict__ g, int64_t g_ld,
                                                                     const float *__restrict__ w,
                                                                     const float *__restrict__ y, float *__restrict__ ga,
                                                                     int64_t N, int64_t J, int64_t K, int64_t nblocks,
                                                                     int64_t rows_per_block, int kp, int groups, float scale,
                                                                     const int64_t *__restrict__ rng, uint32_t drop_thresh,
                                                                     float *__restrict__ partial) {
  if (block_id() >= nblocks) return;  // padding block of a folded grid (the whole block: nobody waits at the barrier)
  const int64_t KV = K / 4;
#ifndef GGL_EMULATE
  extern __shared__ float4 w_lds[];   // [J, K / 4]
  for (int64_t i = threadIdx.x; i < J * KV; i += kBlock) w_lds[i] = reinterpret_cast<const float4 *>(w)[i];
  __syncthreads();
  const float4 *wv = w_lds;
#else
  const float4 *wv = reinterpret_cast<const float4 *>(w);
#endif
  const int j = threadIdx.x / kp;
  const int c0 = threadIdx.x - j * kp;
  if (j >= groups) return;
  const int64_t r0 = block_id() * rows_per_block;
  const int64_t r1 = (r0 + rows_per_block < N) ? r0 + rows_per_block : N;
  for (int64_t c = c0; c < KV; c += kp) {
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int64_t r = r0 + j;
    for (; r + (int64_t)(kLinRows - 1) * groups < r1; r += (int64_t)kLinRows * groups)
      linear_rows<kLinRows, MASKED, UNIFORM>(g, g_ld, wv, y, ga, J, K, KV, c, r, groups, scale, rng, drop_thresh, acc);
    for (; r < r1; r += groups)
      linear_rows<1, MASKED, UNIFORM>(g, g_ld, wv, y, ga, J, K, KV, c, r, groups, scale, rng, drop_thresh, acc);
    if (partial) {
#pragma unroll
      for (int i = 0; i < 4; ++i) partial[(block_id() * groups + j) * K + c * 4 + i] = acc[i];
    }
  }
}

// launch geometry shared by both directions: kp lanes x groups rows per block step, `blocks` row ranges
static inline void geometry(int64_t N, int64_t K, bool vec4, int *kp, int *groups, int64_t *blocks,
                            int64_t *rpb) {
  const int64_t KV = vec4 ? K / 4 : K;
  *kp = (int)(KV < kBlock ? (KV > 0 ? KV : 1) : kBlock);
  *groups = kBlock / *kp;
  int64_t b = ceil_div(N > 0 ? N : 1, (int64_t)*groups * 8);
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  *blocks = b;
  *rpb = ceil_div(N > 0 ? N : 1, b);
}

// The first stage of bias_act_bwd_kernel<4, 0> for a gradient that is zero outside a sorted list of rows, from the
// compact [R, K] rows alone: slot (block b, group j) of the SAME geometry(N, K) adds the listed rows r of the block's
// range with (r - r0) % groups == j, ascending — the rows the full kernel adds there minus its +0 ones, so every partial
// (and the column sum ggl_colsum_f32 makes of them) is the number the full pass over the scattered [N, K] matrix gives.
__global__ __launch_bounds__(kBlock) void bias_grad_rows_kernel(const float *__restrict__ g, const int64_t *__restrict__ rows,
                                                                int64_t R, int64_t N, int64_t K, int64_t nblocks,
                                                                int64_t rows_per_block, int kp, int groups,
                                                                float *__restrict__ partial) {
  const int j = threadIdx.x / kp;
  const int c0 = threadIdx.x - j * kp;
  if (j >= groups || block_id() >= nblocks) return;
  const int64_t KV = K / 4;
  const int64_t r0 = block_id() * rows_per_block;
  const int64_t r1 = (r0 + rows_per_block < N) ? r0 + rows_per_block : N;
  int64_t lo = 0, hi = R;   // first listed position with rows[i] >= r0
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (rows[mid] < r0) lo = mid + 1; else hi = mid;
  }
  for (int64_t c = c0; c < KV; c += kp) {
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t i = lo; i < R; ++i) {
      const int64_t r = rows[i];
      if (r >= r1) break;
      if ((int)(r - r0) % groups != j) continue;   // (r - r0 < rows_per_block: fits an int)
      float gv[4];
      ldv<float, 4>(g + i * K + c * 4, gv);
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = __fadd_rn(acc[k], gv[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) partial[(block_id() * groups + j) * K + c * 4 + k] = acc[k];
  }
}

int rng_advance(int64_t *rng_state, void *stream) {
  GGL_LAUNCH((rng_advance_kernel), 1, 64, as_stream(stream), rng_state, (int64_t)1);
  GGL_LAUNCH_CHECK();
  return GGL_OK;
}

}  // namespace ggl

using namespace ggl;

// the 4-column lanes' accesses: 16 bytes of f32, 8 bytes of 16-bit storage
template <typename T> static inline bool aligned_v4(const void *p) {
  return (reinterpret_cast<uintptr_t>(p) & (4 * sizeof(typename TT<T>::S) - 1)) == 0;
}

template <typename T>
static int bias_act_fwd(const typename TT<T>::S *a, const float *bias, int64_t N, int64_t K, int relu, float p_drop,
                        int64_t *rng_state, typename TT<T>::S *y, void *stream) {
  GGL_REQUIRE(N >= 0 && K >= 0 && p_drop >= 0.0f && p_drop < 1.0f, GGL_EINVAL, "bad arguments");
  const int64_t total = N * K;
  if (total == 0) return GGL_OK;
  GGL_REQUIRE(a && y, GGL_EINVAL, "NULL pointer");
  GGL_REQUIRE(p_drop == 0.0f || rng_state, GGL_EINVAL, "dropout needs an rng_state");
  // keep when r >= thresh, r uniform on [0, 2^32): P(drop) = thresh / 2^32
  uint32_t thresh;
  float scale;
  dropout_params(p_drop, &thresh, &scale);
  hipStream_t s = as_stream(stream);
  const bool vec4 = (K % 4 == 0) && aligned_v4<T>(a) && aligned_v4<T>(y);
  int kp, groups;
  int64_t grid, rpb;
  geometry(N, K, vec4, &kp, &groups, &grid, &rpb);
  if (vec4)
    GGL_LAUNCH((bias_act_fwd_kernel<T, 4>), grid, kBlock, s, a, bias, (const int64_t *)rng_state, y, N, K, grid, rpb,
               kp, groups, relu, thresh, scale);
  else
    GGL_LAUNCH((bias_act_fwd_kernel<T, 1>), grid, kBlock, s, a, bias, (const int64_t *)rng_state, y, N, K, grid, rpb,
               kp, groups, relu, thresh, scale);
  GGL_LAUNCH_CHECK();
  if (thresh) return rng_advance(rng_state, stream);
  return GGL_OK;
}

extern "C" int ggl_bias_act_fwd(const float *a, const float *bias, int64_t N, int64_t K, int relu,
                                float p_drop, int64_t *rng_state, float *y, void *stream) {
  return bias_act_fwd<float>(a, bias, N, K, relu, p_drop, rng_state, y, stream);
}

static int x16_dtype_ok(int dtype, const char *what) {
  if (dtype == GGL_F16 || dtype == GGL_BF16) return GGL_OK;
  set_error("x16: %s must be f16 or bf16 (got dtype code %d)", what, dtype);
  return GGL_EDTYPE;
}

// y16 == ggl_bias_act_fwd(a16.float(), ...).to(dtype): same words, same state motion, one rounding at the store
extern "C" int ggl_bias_act_fwd_x16(int dtype, const void *a, const float *bias, int64_t N, int64_t K, int relu,
                                    float p_drop, int64_t *rng_state, void *y, void *stream) {
  if (int rc = x16_dtype_ok(dtype, "a / y")) return rc;
  const uint16_t *a16 = static_cast<const uint16_t *>(a);
  uint16_t *y16 = static_cast<uint16_t *>(y);
  return dtype == GGL_BF16 ? bias_act_fwd<mxbf16_t>(a16, bias, N, K, relu, p_drop, rng_state, y16, stream)
                           : bias_act_fwd<mxf16_t>(a16, bias, N, K, relu, p_drop, rng_state, y16, stream);
}

static inline size_t bwd_partial_bytes(int64_t N, int64_t K) {
  int kp, groups;
  int64_t blocks, rpb;
  geometry(N, K, false, &kp, &groups, &blocks, &rpb);
  size_t a = (size_t)blocks * (size_t)groups;
  geometry(N, K, K % 4 == 0, &kp, &groups, &blocks, &rpb);
  const size_t b = (size_t)blocks * (size_t)groups;
  return ((a > b ? a : b) * (size_t)(K > 0 ? K : 1) * sizeof(float) + 255) & ~(size_t)255;
}

extern "C" size_t ggl_bias_act_bwd_workspace_bytes(int64_t N, int64_t K) {
  const size_t part = bwd_partial_bytes(N, K);
  return part + ggl_colsum_workspace_bytes((int64_t)(part / sizeof(float) / (size_t)(K > 0 ? K : 1)), K);
}

template <typename T>
static int bias_act_bwd(const typename TT<T>::S *g, const typename TT<T>::S *y, int64_t N, int64_t K, int relu,
                        float p_drop, const int64_t *rng_used, typename TT<T>::S *ga, float *gbias,
                        void *workspace, size_t workspace_bytes, void *stream) {
  GGL_REQUIRE(N >= 0 && K >= 0 && p_drop >= 0.0f && p_drop < 1.0f, GGL_EINVAL, "bad arguments");
  if (K == 0) return GGL_OK;
  GGL_REQUIRE((g && ga) || N == 0, GGL_EINVAL, "NULL pointer");
  // rng_used = the {seed, offset} the forward read (a copy taken before it advanced): the dropout mask is
  // redrawn exactly.  Without it the mask is rebuilt from y (y > 0 with ReLU; y != 0 without — exact except
  // for kept activations that are exactly 0).
  // With ReLU the mask read off y is already exact (y > 0 <=> kept and positive; a kept activation that is
  // exactly 0 has zero ReLU gradient anyway), so the redraw — 10 Philox rounds per 4 elements, measured
  // 1.10 -> 1.87 ms on [2.45 M, 256] — is only paid where it is needed: dropout without ReLU.
  const bool redraw = p_drop > 0.0f && rng_used != nullptr && !relu;
  const int masked = relu ? 1 : (redraw ? 3 : (p_drop > 0.0f ? 2 : 0));
  uint32_t thresh;
  float scale;
  dropout_params(p_drop, &thresh, &scale);
  GGL_REQUIRE(!masked || masked == 3 || y || N == 0, GGL_EINVAL, "y is needed to rebuild the ReLU/dropout mask");
  GGL_REQUIRE(!gbias || (workspace && workspace_bytes >= ggl_bias_act_bwd_workspace_bytes(N, K)),
              GGL_EWORKSPACE, "bias_act_bwd workspace too small");
  const bool vec4 = (K % 4 == 0) && aligned_v4<T>(g) && aligned_v4<T>(ga) && (!masked || masked == 3 || aligned_v4<T>(y));
  int kp, groups;
  int64_t blocks, rpb;
  geometry(N, K, vec4, &kp, &groups, &blocks, &rpb);
  hipStream_t s = as_stream(stream);
  float *partial = gbias ? static_cast<float *>(workspace) : nullptr;
#define GGL_BAB(V, M)                                                                                    \
  GGL_LAUNCH((bias_act_bwd_kernel<T, V, M>), blocks, kBlock, s, g, y, ga, N, K, blocks, rpb, kp, groups, scale, \
             redraw ? rng_used : nullptr, thresh, partial)
  if (vec4) {
    if (masked == 0) GGL_BAB(4, 0); else if (masked == 1) GGL_BAB(4, 1); else if (masked == 2) GGL_BAB(4, 2); else GGL_BAB(4, 3);
  } else {
    if (masked == 0) GGL_BAB(1, 0); else if (masked == 1) GGL_BAB(1, 1); else if (masked == 2) GGL_BAB(1, 2); else GGL_BAB(1, 3);
  }
#undef GGL_BAB
  GGL_LAUNCH_CHECK();
  if (gbias) {  // second stage: column sums of the [P, K] partial matrix
    const size_t part = bwd_partial_bytes(N, K);
    return ggl_colsum_f32(partial, blocks * groups, K, gbias, static_cast<char *>(workspace) + part,
                          workspace_bytes - part, stream);
  }
  return GGL_OK;
}

extern "C" int ggl_bias_act_bwd(const float *g, const float *y, int64_t N, int64_t K, int relu,
                                float p_drop, const int64_t *rng_used, float *ga, float *gbias,
                                void *workspace, size_t workspace_bytes, void *stream) {
  return bias_act_bwd<float>(g, y, N, K, relu, p_drop, rng_used, ga, gbias, workspace, workspace_bytes, stream);
}

// ga16 == ggl_bias_act_bwd(g16.float(), y16.float(), ...).ga.to(dtype); gbias is that call's, on the bits: the column sums
// add the f32 values before they are rounded, in the same geometry, and ggl_colsum_f32 finishes them.  The ReLU mask is read
// off the stored y16 > 0.  Workspace: ggl_bias_act_bwd_workspace_bytes(N, K).
extern "C" int ggl_bias_act_bwd_x16(int dtype, const void *g, const void *y, int64_t N, int64_t K, int relu, float p_drop,
                                    const int64_t *rng_used, void *ga, float *gbias, void *workspace,
                                    size_t workspace_bytes, void *stream) {
  if (int rc = x16_dtype_ok(dtype, "g / y / ga")) return rc;
  const uint16_t *g16 = static_cast<const uint16_t *>(g), *y16 = static_cast<const uint16_t *>(y);
  uint16_t *ga16 = static_cast<uint16_t *>(ga);
  return dtype == GGL_BF16
             ? bias_act_bwd<mxbf16_t>(g16, y16, N, K, relu, p_drop, rng_used, ga16, gbias, workspace, workspace_bytes, stream)
             : bias_act_bwd<mxf16_t>(g16, y16, N, K, relu, p_drop, rng_used, ga16, gbias, workspace, workspace_bytes, stream);
}

// The shapes the fused form takes (and wins at): float4 lanes, one coalesced load of a g row per wavefront at most, and
// a staged w of at most 64 KiB so that two blocks and more share a CU's LDS.
extern "C" int ggl_policy_linear_epi_bwd(int64_t N, int64_t J, int64_t K) {
  (void)N;
  return K > 0 && K % 4 == 0 && J >= 1 && J <= 64 && J * K * (int64_t)sizeof(float) <= 64 * 1024;
}

extern "C" int ggl_linear_bias_act_bwd(const float *g, int64_t g_ld, const float *w, const float *y, int64_t N, int64_t J,
                                       int64_t K, int relu, float p_drop, const int64_t *rng_used, float *ga, float *gbias,
                                       void *workspace, size_t workspace_bytes, void *stream) {
  GGL_REQUIRE(N >= 0 && J >= 0 && K >= 0 && g_ld >= J && p_drop >= 0.0f && p_drop < 1.0f, GGL_EINVAL, "bad arguments");
  if (K == 0) return GGL_OK;
  GGL_REQUIRE(ggl_policy_linear_epi_bwd(N, J, K), GGL_EINVAL,
              "linear_bias_act_bwd needs K %% 4 == 0, 1 <= J <= 64 and J * K floats within 64 KiB (got J = %lld, K = %lld)",
              (long long)J, (long long)K);
  GGL_REQUIRE(w && ((g && ga) || N == 0), GGL_EINVAL, "NULL pointer");
  const bool redraw = p_drop > 0.0f && rng_used != nullptr && !relu;   // the modes of ggl_bias_act_bwd, chosen the same way
  const int masked = relu ? 1 : (redraw ? 3 : (p_drop > 0.0f ? 2 : 0));
  uint32_t thresh;
  float scale;
  dropout_params(p_drop, &thresh, &scale);
  GGL_REQUIRE(!masked || masked == 3 || y || N == 0, GGL_EINVAL, "y is needed to rebuild the ReLU/dropout mask");
  GGL_REQUIRE(!gbias || (workspace && workspace_bytes >= ggl_bias_act_bwd_workspace_bytes(N, K)),
              GGL_EWORKSPACE, "linear_bias_act_bwd workspace too small (ggl_bias_act_bwd_workspace_bytes(N, K))");
  GGL_REQUIRE(aligned16(g) && aligned16(w) && aligned16(ga) && (!masked || masked == 3 || aligned16(y)), GGL_EINVAL,
              "g, w, y and ga must be 16-byte aligned");
  int kp, groups;
  int64_t blocks, rpb;
  geometry(N, K, true, &kp, &groups, &blocks, &rpb);   // the float4 geometry of ggl_bias_act_bwd on the [N, K] product
  hipStream_t s = as_stream(stream);
  float *partial = gbias ? static_cast<float *>(workspace) : nullptr;
  const int64_t *rng = redraw ? rng_used : nullptr;
#ifdef GGL_EMULATE
#define GGL_LBAB(M, U)                                                                                               \
  GGL_LAUNCH((linear_bias_act_bwd_kernel<M, false>), blocks, kBlock, s, g, g_ld, w, y, ga, N, J, K, blocks, rpb, kp, groups, \
             scale, rng, thresh, partial)
  const bool uniform = false;
#else
  // (GGL_LAUNCH carries no dynamic LDS: the fold is the same)
#define GGL_LBAB(M, U)                                                                                               \
  do {                                                                                                               \
    unsigned gx_, gy_;                                                                                               \
    fold_grid(blocks, &gx_, &gy_);                                                                                   \
    hipLaunchKernelGGL((linear_bias_act_bwd_kernel<M, U>), dim3(gx_, gy_), dim3((unsigned)kBlock),                    \
                       (size_t)(J * K) * sizeof(float), s, g, g_ld, w, y, ga, N, J, K, blocks, rpb, kp, groups, scale, rng, \
                       thresh, partial);                                                                             \
  } while (0)
  const bool uniform = kp % kWave == 0 && (K / 4) % kp == 0;
#endif
  if (uniform) {
    if (masked == 0) GGL_LBAB(0, true); else if (masked == 1) GGL_LBAB(1, true); else if (masked == 2) GGL_LBAB(2, true); else GGL_LBAB(3, true);
  } else {
    if (masked == 0) GGL_LBAB(0, false); else if (masked == 1) GGL_LBAB(1, false); else if (masked == 2) GGL_LBAB(2, false); else GGL_LBAB(3, false);
  }
#undef GGL_LBAB
  GGL_LAUNCH_CHECK();
  if (gbias) {  // second stage: column sums of the [P, K] partial matrix
    const size_t part = bwd_partial_bytes(N, K);
    return ggl_colsum_f32(partial, blocks * groups, K, gbias, static_cast<char *>(workspace) + part,
                          workspace_bytes - part, stream);
  }
  return GGL_OK;
}

extern "C" int ggl_bias_grad_rows(const float *g, const int64_t *rows, int64_t R, int64_t N, int64_t K, float *gbias,
                                  void *workspace, size_t workspace_bytes, void *stream) {
  GGL_REQUIRE(R >= 0 && N >= 0 && R <= N && K > 0 && K % 4 == 0, GGL_EINVAL,
              "bias_grad_rows needs R <= N rows of a multiple of 4 columns");
  GGL_REQUIRE(gbias && ((g && rows) || R == 0), GGL_EINVAL, "NULL pointer");
  GGL_REQUIRE(aligned16(g), GGL_EINVAL, "g must be 16-byte aligned");
  GGL_REQUIRE(workspace && workspace_bytes >= ggl_bias_act_bwd_workspace_bytes(N, K), GGL_EWORKSPACE,
              "bias_grad_rows workspace too small (ggl_bias_act_bwd_workspace_bytes(N, K))");
  int kp, groups;
  int64_t blocks, rpb;
  geometry(N, K, true, &kp, &groups, &blocks, &rpb);   // the float4 geometry of ggl_bias_act_bwd on the full [N, K] gradient
  float *partial = static_cast<float *>(workspace);
  GGL_LAUNCH((bias_grad_rows_kernel), blocks, kBlock, as_stream(stream), g, rows, R, N, K, blocks, rpb, kp, groups, partial);
  GGL_LAUNCH_CHECK();
  const size_t part = bwd_partial_bytes(N, K);
  return ggl_colsum_f32(partial, blocks * groups, K, gbias, static_cast<char *>(workspace) + part, workspace_bytes - part,
                        stream);
}
