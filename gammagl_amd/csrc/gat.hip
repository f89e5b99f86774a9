// gammagl_amd/csrc/gat.hip — fused GAT edge-softmax + weighted aggregate.
//
// Replaces (a) the external dgNN GATConvFuse CUDA kernel that FusedGATConv calls
// (layers/conv/fusedgat_conv.py:70-71,121 — not in the reference tree, parity unpinned) and (b) the
// unfused chain GATConv.forward runs today (layers/conv/gat_conv.py:103-112 + utils/softmax.py:29-35):
// 2 gathers [E,H,C] + concat + reduce -> leaky_relu -> segment_max -> gather -> exp -> segment_sum ->
// gather -> divide -> gather [E,H,C] * alpha -> segment_sum, i.e. three segment passes and five
// [E,.] intermediates in HBM.
//
// Forward (ONE launch + a tiny combine for hub rows): a lane group owns one destination row, each lane
// VEC channels of one head, and walks the row ONCE with an online softmax (gat_online / gat_fwd_kernel,
// gat_common.hpp: the walk is shared with dotattn.hip): running
// max, denominator and weighted sum, rescaled when the max moves; out = acc / (den + 1e-16).  (The first
// version walked the row three times as the in-tree math does — max, denominator, weighted sum — and
// was latency-bound on the two extra index/el walks: 9.3 ms on the Reddit-sized graph.)
// Lanes of the same head recompute the (cheap) scalar softmax terms redundantly instead of
// exchanging them: no LDS, no shuffles, no atomics.
// Rows longer than plan->chunk (a Reddit-sized R-MAT graph has a 109 110-edge hub: 100 ms on one lane
// group) are cut into chunks reduced by whole wavefronts in the leading blocks of the same launch with
// a chunk-local max (m_c, d_c = sum exp(s - m_c), acc_c = sum exp(s - m_c) x); gat_long_final_kernel
// merges them in chunk order: m = max m_c, d = sum d_c e^{m_c - m}, out = sum acc_c e^{m_c - m} / (d + 1e-16).
//
// Backward: two walks, one per side.
//   gat_bwd_dst_kernel (forward plan, lane = head of a destination row or of a hub chunk): row dot
//     <g_i, out_i>, alpha, de = alpha (<g_i, x_j> - dot) LeakyReLU'(.) -> alpha[E,H], de[E,H], and
//     ger[i,h] = sum_p de in the same walk;
//   gat_bwd_src_kernel (transposed plan): gx[j,h,:] = sum alpha g[dst,h,:] and gel[j,h] = sum de, reading
//     alpha / de through posT.
// (The first version was edge-parallel on the destination side — a row-dot kernel, one thread per
// (position, head), then ggl_segment_sum for ger — and ran bspmm + segment_sum on the source side.)
// Roofline: HBM; algorithmic bytes per edge = 4*H*C (feature row) + 4 (col) + 4*H (el row).
#include "gat_common.hpp"

namespace ggl {

template <typename OT>
__device__ __forceinline__ void gat_long_final_body(
    const int32_t *__restrict__ long_rows, const int64_t *__restrict__ chunk_ptr,
    const float *__restrict__ pacc, const float *__restrict__ pm, const float *__restrict__ pd,
    typename TT<OT>::S *__restrict__ y, float *__restrict__ rowmax, float *__restrict__ rowden, const GatDims &d) {
  const int64_t j = block_id();
  if (j >= d.n_long) return;
  const int64_t row = long_rows[j];
  const int64_t c0 = chunk_ptr[j], c1 = chunk_ptr[j + 1];
  for (int64_t k = threadIdx.x; k < d.K; k += kBlock) {
    const int64_t h = k / d.C;
    float m = -FLT_MAX;
    for (int64_t c = c0; c < c1; ++c)
      if (m < pm[c * d.H + h]) m = pm[c * d.H + h];
    float den = 0.0f, acc = 0.0f;
    for (int64_t c = c0; c < c1; ++c) {
      const float sc = GGL_EXPF(__fadd_rn(pm[c * d.H + h], -m));
      den = __fadd_rn(den, __fmul_rn(pd[c * d.H + h], sc));
      acc = __fadd_rn(acc, __fmul_rn(pacc[c * d.K + k], sc));
    }
    y[row * d.K + k] = TT<OT>::store(__fdiv_rn(acc, __fadd_rn(den, 1e-16f)));
    if (k == h * d.C) {
      rowmax[row * d.H + h] = m;
      rowden[row * d.H + h] = den;
    }
  }
}
__global__ __launch_bounds__(kBlock) void gat_long_final_kernel(
    const int32_t *__restrict__ long_rows, const int64_t *__restrict__ chunk_ptr,
    const float *__restrict__ pacc, const float *__restrict__ pm, const float *__restrict__ pd,
    float *__restrict__ y, float *__restrict__ rowmax, float *__restrict__ rowden, const GatDims d) {
  gat_long_final_body<float>(long_rows, chunk_ptr, pacc, pm, pd, y, rowmax, rowden, d);
}
template <typename OT>  // the same merge of the same f32 partials; only the store rounds
__global__ __launch_bounds__(kBlock) void gat_long_final16_kernel(
    const int32_t *__restrict__ long_rows, const int64_t *__restrict__ chunk_ptr,
    const float *__restrict__ pacc, const float *__restrict__ pm, const float *__restrict__ pd,
    uint16_t *__restrict__ y, float *__restrict__ rowmax, float *__restrict__ rowden, const GatDims d) {
  gat_long_final_body<OT>(long_rows, chunk_ptr, pacc, pm, pd, y, rowmax, rowden, d);
}

// Destination-major half of the backward in ONE walk of the forward plan.  A work item is a short row or
// one chunk of a long row; a group of 2^logL >= H lanes owns it, lane = head.  Per head the lane computes
// dot_i = <g_i, out_i> once, then walks the item's positions in order:
//   alpha_p = exp(s_p - m_i) / (den_i + 1e-16),  dalpha_p = <g_i[h,:], x_j[h,:]>,
//   de_p = alpha_p (dalpha_p - dot_i) LeakyReLU'(raw_p)          -> alpha[E,H], de[E,H] (sorted positions)
//   ger[i,h] = sum_p de_p  (in position order; chunk partials are combined in chunk order afterwards)
// CREG > 0: C is known at compile time and g_i[h,:] lives in registers; 0 = any C, g_i re-read (cached).
// Replaces three launches (row dots, an edge-parallel alpha/de kernel, segment_sum(de) for ger: 0.3 + 5.7
// + 2.7 ms on the Reddit-sized graph) with the same rounded operations in the same order.
// XT: storage of x; GT: storage of g AND of the saved out (the forward's out type).  16-bit elements are widened at the
// load; the dots run over the channels in ascending order whatever VEC is, so the bits do not depend on the load form.
// LS = kLogitEdge (`el` = z, `er` = plan->perm): s_p = z[e_p, h] and no activation, so dv = ds; `de` is gz [E, H] and is
// stored at e_p, the caller's edge number (no pass permutes it afterwards); alpha stays in position order.  alpha or de
// may be NULL (x resp. z needs no gradient) and is then not stored; there is no per-row sum, ger / pger are not touched.
template <typename XT, typename GT, int VEC, int CREG, int LS = kLogitSeparable>
__global__ __launch_bounds__(kBlock) void gat_bwd_dst_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const int32_t *__restrict__ row_order, const int32_t *__restrict__ long_rows,
    const int64_t *__restrict__ chunk_ptr, const float *__restrict__ el, typename Logit<LS>::Aux __restrict__ er,
    const typename TT<XT>::S *__restrict__ x, const typename TT<GT>::S *__restrict__ g,
    const typename TT<GT>::S *__restrict__ out,
    const float *__restrict__ rowmax, const float *__restrict__ rowden, float *__restrict__ alpha,
    float *__restrict__ de, float *__restrict__ ger, float *__restrict__ pger,
    const int64_t *__restrict__ rng, const GatDims d) {
  using XS = typename TT<XT>::S;
  using GS = typename TT<GT>::S;
  using LP = Logit<LS>;
  const int64_t H = d.H, K = d.K;
  const int64_t C = CREG > 0 ? (int64_t)CREG : d.C;
  const uint64_t seed = d.drop_thresh ? (uint64_t)rng[0] : 0, offset = d.drop_thresh ? (uint64_t)rng[1] : 0;
  const int LG = 1 << d.logL;
  const int64_t item = (block_id() * kBlock + threadIdx.x) >> d.logL;
  const int li = threadIdx.x & (LG - 1);
  if (item >= d.n_chunks + d.N) return;
  const bool is_chunk = item < d.n_chunks;
  int64_t row, beg, end;
  if (is_chunk) {  // chunks carry the lowest item ids: the hub work is dispatched first
    const HubChunk hc = hub_chunk(rowptr, long_rows, chunk_ptr, d.n_long, d.chunk, item);
    row = hc.row; beg = hc.beg; end = hc.end;
  } else {
    const int64_t slot = item - d.n_chunks;
    row = row_order ? (int64_t)row_order[slot] : slot;
    beg = rowptr[row];
    end = rowptr[row + 1];
    if (end - beg > d.chunk) return;  // long row: its chunks are separate items
  }
  for (int64_t h = li; h < H; h += LG) {
    const GS *__restrict__ gi = g + row * K + h * C;
    const GS *__restrict__ oi = out + row * K + h * C;
    float gr[CREG > 0 ? CREG : 1];
    float dot = 0.0f;
    if (CREG > 0) {
#pragma unroll
      for (int c = 0; c < (CREG > 0 ? CREG : 1); ++c) {
        gr[c] = TT<GT>::load(gi[c]);
        dot = __fadd_rn(dot, __fmul_rn(gr[c], TT<GT>::load(oi[c])));
      }
    } else {
      for (int64_t c = 0; c < C; ++c) dot = __fadd_rn(dot, __fmul_rn(TT<GT>::load(gi[c]), TT<GT>::load(oi[c])));
    }
    const float er_i = LP::row(er, row * H + h);
    const float m = rowmax[row * H + h];
    const float inv = __fadd_rn(rowden[row * H + h], 1e-16f);
    float gsum = 0.0f;
    auto edge = [&](int64_t p, int64_t e, uint32_t word, float elv, const XS *__restrict__ xj) {
      const float raw = LP::raw(elv, er_i);
      const float al = __fdiv_rn(GGL_EXPF(__fadd_rn(LP::act(raw, d.slope), -m)), inv);
      float da = 0.0f;
      if (CREG > 0) {
#pragma unroll
        for (int c = 0; c < (CREG > 0 ? CREG : 1); c += VEC) {
          float xv[VEC];
          RowV<XT, VEC>::load(xj + c, xv);
#pragma unroll
          for (int q = 0; q < VEC; ++q) da = __fadd_rn(da, __fmul_rn(gr[(c + q) % (CREG > 0 ? CREG : 1)], xv[q]));
        }
      } else {
        for (int64_t c = 0; c < C; c += VEC) {
          float gv[VEC], xv[VEC];
          RowV<GT, VEC>::load(gi + c, gv);
          RowV<XT, VEC>::load(xj + c, xv);
#pragma unroll
          for (int q = 0; q < VEC; ++q) da = __fadd_rn(da, __fmul_rn(gv[q], xv[q]));
        }
      }
      float alk = al;  // the weight the edge carried forward: alpha, or keep * alpha / (1 - p)
      if (d.drop_thresh) {  // same draw as the forward (same seed, offset, index)
        const bool keep = word >= d.drop_thresh;
        alk = keep ? __fmul_rn(al, d.drop_scale) : 0.0f;
        da = keep ? __fmul_rn(da, d.drop_scale) : 0.0f;  // d out / d alpha_p = keep/(1-p) <g_i, x_j>
      }
      const float ds = __fmul_rn(al, __fadd_rn(da, -dot));
      const float dv = LP::dact(raw, ds, d.slope);
      if constexpr (LS == kLogitEdge) {
        if (alpha) alpha[p * H + h] = alk;
        if (de) de[e * H + h] = dv;
      } else {
        alpha[(p * H + h) * d.es] = alk;
        de[(p * H + h) * d.es] = dv;
        gsum = __fadd_rn(gsum, dv);
      }
    };
    auto single = [&](int64_t q) {
      const int64_t s0 = col[q];
      const int64_t e0 = LP::rec(er, col, q, s0);
      edge(q, e0, d.drop_thresh ? drop_word(q, H, h, offset, seed) : 0u, el[e0 * H + h], x + s0 * K + h * C);
    };
    int64_t p = beg;
    if (d.drop_thresh) {
      for (; p < end && (p & 3) != 0; ++p) single(p);
    }
    for (; p + 4 <= end; p += 4) {
      int64_t sj[4], ej[4];
      float ev[4];
      U4 rw{0u, 0u, 0u, 0u};
      if (d.drop_thresh) rw = drop_words4(p >> 2, H, h, offset, seed);
#pragma unroll
      for (int u = 0; u < 4; ++u) { sj[u] = col[p + u]; ej[u] = LP::rec(er, col, p + u, sj[u]); }
#pragma unroll
      for (int u = 0; u < 4; ++u) ev[u] = el[ej[u] * H + h];
#pragma unroll
      for (int u = 0; u < 4; ++u) edge(p + u, ej[u], pick_word(rw, u), ev[u], x + sj[u] * K + h * C);
    }
    for (; p < end; ++p) single(p);
    if constexpr (LS == kLogitSeparable) {
      if (is_chunk) pger[item * H + h] = gsum;
      else ger[row * H + h] = gsum;
    }
  }
}

// ---- wide heads (C > 16), GPU build only.  The lane-per-head walk above reads each lane's C-float strip
// with C/4 strided 16-byte loads and collapsed on the Reddit GAT's last layer (8 heads x 41 classes: 222 ms at
// C = 40, 870 ms at C = 41).  Here a GROUP of 2^LOGG lanes owns the row (or hub chunk) and the lanes split
// the CHANNELS of every head: lane s holds g_i[h, 4s..4s+3] for all HH heads in registers, reads the same
// slice of x_j per head (a head's strip is one coalesced read, the HH reads of an edge cover its whole
// contiguous row), and the per-edge dots <g_i[h,:], x_j[h,:]> are reduced across the group with a butterfly
// of wave shuffles — the one place this library reduces across lanes: GAT gradients are held to 1e-5
// relative, not bit-exact, so the association may change.  After the butterflies every lane holds every
// dot; lane h finishes head h (alpha, de, running ger sum in position order).  The host emulation build
// cannot shuffle between its sequentially executed lanes and keeps using gat_bwd_dst_kernel for every C.
#ifndef GGL_EMULATE
// 16-bit storage (XT / GT as in gat_bwd_dst_kernel) keeps the f32 form's ASSIGNMENT: four channels per lane (8-byte
// loads of 16-bit rows), the same LOGG and HH for a head shape.  The butterfly's association depends on which
// channels a lane holds, so this is what keeps alpha / de / ger equal, bit for bit, to the f32 kernel on the widened
// rows; eight channels per lane would halve the loads and would have to give that equality up.  A 16-bit panel that
// is not 8-byte aligned keeps the assignment too and reads its four channels one by one (d.vl = 0).
template <typename T, int VEC, bool MAYBE>
__device__ __forceinline__ void gat_wide_load(int vl, const typename TT<T>::S *__restrict__ p, float (&v)[VEC]) {
  if constexpr (!MAYBE || VEC == 1) {
    RowV<T, VEC>::load(p, v);
  } else {
    if (vl) {
      RowV<T, VEC>::load(p, v);
    } else {
#pragma unroll
      for (int i = 0; i < VEC; ++i) v[i] = TT<T>::load(p[i]);
    }
  }
}

// LS: as in gat_bwd_dst_kernel.
template <typename XT, typename GT, int VEC, int LOGG, int HH, int LS = kLogitSeparable>
__global__ __launch_bounds__(kBlock) void gat_bwd_dst_wide_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const int32_t *__restrict__ row_order, const int32_t *__restrict__ long_rows,
    const int64_t *__restrict__ chunk_ptr, const float *__restrict__ el, typename Logit<LS>::Aux __restrict__ er,
    const typename TT<XT>::S *__restrict__ x, const typename TT<GT>::S *__restrict__ g,
    const typename TT<GT>::S *__restrict__ out,
    const float *__restrict__ rowmax, const float *__restrict__ rowden, float *__restrict__ alpha,
    float *__restrict__ de, float *__restrict__ ger, float *__restrict__ pger,
    const int64_t *__restrict__ rng, const GatDims d) {
  using LP = Logit<LS>;
  constexpr int G = 1 << LOGG;
  constexpr bool MB = gat_is16<XT>::value;  // only the 16-bit entry points can meet a panel aligned to less than VEC
  static_assert(G >= HH, "lane h finishes head h");
  const int64_t H = d.H, C = d.C, K = d.K;  // H <= HH: HH is the compile-time bound of the head loops
  const int64_t item = thread_id() >> LOGG;
  const int sub = (int)(threadIdx.x & (G - 1));
  if (item >= d.n_chunks + d.N) return;  // whole groups leave together: the shuffles below stay in-group
  const bool is_chunk = item < d.n_chunks;
  int64_t row, beg, end;
  if (is_chunk) {
    const HubChunk hc = hub_chunk(rowptr, long_rows, chunk_ptr, d.n_long, d.chunk, item);
    row = hc.row; beg = hc.beg; end = hc.end;
  } else {
    const int64_t slot = item - d.n_chunks;
    row = row_order ? (int64_t)row_order[slot] : slot;
    beg = rowptr[row];
    end = rowptr[row + 1];
    if (end - beg > d.chunk) return;
  }
  const int64_t c0 = (int64_t)sub * VEC;
  const bool act = c0 < C;  // C % VEC == 0 on this path
  float gr[HH][VEC], dots[HH];
#pragma unroll
  for (int h = 0; h < HH; ++h) {
    float ov[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) { gr[h][q] = 0.0f; ov[q] = 0.0f; }
    if (act && h < H) {
      gat_wide_load<GT, VEC, MB>(d.vl, g + row * K + h * C + c0, gr[h]);
      gat_wide_load<GT, VEC, MB>(d.vl, out + row * K + h * C + c0, ov);
    }
    float t = 0.0f;
#pragma unroll
    for (int q = 0; q < VEC; ++q) t = __fadd_rn(t, __fmul_rn(gr[h][q], ov[q]));
    dots[h] = group_sum<LOGG>(t);
  }
  // lane h keeps the row constants of head h
  float my_dot = 0.0f, my_er = 0.0f, my_m = 0.0f, my_inv = 1.0f;
#pragma unroll
  for (int h = 0; h < HH; ++h)
    if (sub == h) my_dot = dots[h];
  if (sub < H) {
    my_er = LP::row(er, row * H + sub);
    my_m = rowmax[row * H + sub];
    my_inv = __fadd_rn(rowden[row * H + sub], 1e-16f);
  }
  const uint64_t seed = d.drop_thresh ? (uint64_t)rng[0] : 0, offset = d.drop_thresh ? (uint64_t)rng[1] : 0;
  float gsum = 0.0f;
  auto one_edge = [&](int64_t p, int64_t e, const float (&xv)[HH][VEC]) {  // e: the edge's record of el
    float part[HH];
#pragma unroll
    for (int h = 0; h < HH; ++h) {
      float t = 0.0f;
#pragma unroll
      for (int q = 0; q < VEC; ++q) t = __fadd_rn(t, __fmul_rn(gr[h][q], xv[h][q]));
      part[h] = group_sum<LOGG>(t);
    }
    if (sub < H) {
      float da = 0.0f;
#pragma unroll
      for (int h = 0; h < HH; ++h)
        if (sub == h) da = part[h];
      const float raw = LP::raw(el[e * H + sub], my_er);
      const float al = __fdiv_rn(GGL_EXPF(__fadd_rn(LP::act(raw, d.slope), -my_m)), my_inv);
      float alk = al;
      if (d.drop_thresh) {
        const bool keep = drop_word(p, H, sub, offset, seed) >= d.drop_thresh;
        alk = keep ? __fmul_rn(al, d.drop_scale) : 0.0f;
        da = keep ? __fmul_rn(da, d.drop_scale) : 0.0f;
      }
      const float ds = __fmul_rn(al, __fadd_rn(da, -my_dot));
      const float dv = LP::dact(raw, ds, d.slope);
      if constexpr (LS == kLogitEdge) {
        if (alpha) alpha[p * H + sub] = alk;
        if (de) de[e * H + sub] = dv;
      } else {
        alpha[(p * H + sub) * d.es] = alk;
        de[(p * H + sub) * d.es] = dv;
        gsum = __fadd_rn(gsum, dv);
      }
    }
  };
  int64_t p = beg;
  for (; p + 2 <= end; p += 2) {  // two feature rows (2 x HH slices per lane) in flight
    const int64_t j0 = col[p], j1 = col[p + 1];
    const int64_t e0 = LP::rec(er, col, p, j0), e1 = LP::rec(er, col, p + 1, j1);
    float x0[HH][VEC], x1[HH][VEC];
#pragma unroll
    for (int h = 0; h < HH; ++h) {
#pragma unroll
      for (int q = 0; q < VEC; ++q) { x0[h][q] = 0.0f; x1[h][q] = 0.0f; }
      if (act && h < H) {
        gat_wide_load<XT, VEC, MB>(d.vl, x + j0 * K + h * C + c0, x0[h]);
        gat_wide_load<XT, VEC, MB>(d.vl, x + j1 * K + h * C + c0, x1[h]);
      }
    }
    one_edge(p, e0, x0);
    one_edge(p + 1, e1, x1);
  }
  for (; p < end; ++p) {
    const int64_t j0 = col[p];
    const int64_t e0 = LP::rec(er, col, p, j0);
    float x0[HH][VEC];
#pragma unroll
    for (int h = 0; h < HH; ++h) {
#pragma unroll
      for (int q = 0; q < VEC; ++q) x0[h][q] = 0.0f;
      if (act && h < H) gat_wide_load<XT, VEC, MB>(d.vl, x + j0 * K + h * C + c0, x0[h]);
    }
    one_edge(p, e0, x0);
  }
  if constexpr (LS == kLogitSeparable) {
    if (sub < H) {
      if (is_chunk) pger[item * H + sub] = gsum;
      else ger[row * H + sub] = gsum;
    }
  }
}
#endif  // !GGL_EMULATE

__global__ __launch_bounds__(kBlock) void gat_bwd_dst_final_kernel(const int32_t *__restrict__ long_rows,
                                                                   const int64_t *__restrict__ chunk_ptr,
                                                                   const float *__restrict__ pger,
                                                                   float *__restrict__ ger, int64_t n_long,
                                                                   int64_t H) {
  const int64_t stride = grid_threads();
  for (int64_t t = thread_id(); t < n_long * H; t += stride) {
    const int64_t j = t / H, h = t - j * H;
    float a = 0.0f;
    for (int64_t c = chunk_ptr[j]; c < chunk_ptr[j + 1]; ++c) a = __fadd_rn(a, pger[c * H + h]);
    ger[(int64_t)long_rows[j] * H + h] = a;
  }
}

// Source-major half of the backward in ONE walk of the transposed plan (rows = source nodes j):
//   gx[j,h,:] = sum_q alpha[posT[q],h] * g[colT[q],h,:]        gel[j,h] = sum_q de[posT[q],h]
// posT maps a transposed position to the forward (destination-sorted) position alpha / de were written
// at.  Same lane layout as the forward; the first lane of each head also carries the gel sum.  Same
// rounded operations in the same order as the bspmm + segment_sum pair this replaces (two walks, two
// gathers of posT: 6.0 + 3.7 ms on the Reddit-sized graph), so the results are bit-identical to it.
// GT: storage of g (widened at the load); OT (kernel): storage of gx, rounded once at the store.
// GEL = false (the edge-softmax aggregate: no [N_src, H] result is wanted, and its gz is not in position order): no lane
// leads, so de is never read and gel / pgel never written — both may be NULL.
template <typename GT, int VEC>
__device__ __forceinline__ void gat_src_walk(const int32_t *__restrict__ colT, const int32_t *__restrict__ posT,
                                             const float *__restrict__ alpha, const float *__restrict__ de,
                                             const typename TT<GT>::S *__restrict__ g, int64_t H, int64_t K, int64_t h,
                                             int64_t es, int64_t kk, bool lead, int64_t beg, int64_t end,
                                             float (&acc)[VEC], float &gl) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
  gl = 0.0f;
  int64_t q = beg;
  for (; q + 4 <= end; q += 4) {
    int64_t r[4], e[4];
    float v[4][VEC], a[4], dv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { r[u] = colT[q + u]; e[u] = posT[q + u]; }
#pragma unroll
    for (int u = 0; u < 4; ++u) RowV<GT, VEC>::load(g + r[u] * K + kk, v[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a[u] = alpha[(e[u] * H + h) * es];
      dv[u] = lead ? de[(e[u] * H + h) * es] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = __fadd_rn(acc[i], __fmul_rn(a[u], v[u][i]));
      gl = __fadd_rn(gl, dv[u]);
    }
  }
  for (; q < end; ++q) {
    const int64_t r0 = colT[q], e0 = posT[q];
    float v0[VEC];
    RowV<GT, VEC>::load(g + r0 * K + kk, v0);
    const float a0 = alpha[(e0 * H + h) * es];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = __fadd_rn(acc[i], __fmul_rn(a0, v0[i]));
    if (lead) gl = __fadd_rn(gl, de[(e0 * H + h) * es]);
  }
}

template <typename GT, typename OT, int VEC, bool GEL = true>
__global__ __launch_bounds__(kBlock) void gat_bwd_src_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colT, const int32_t *__restrict__ posT,
    const int32_t *__restrict__ row_order, const int32_t *__restrict__ long_rows,
    const int64_t *__restrict__ chunk_ptr, const float *__restrict__ alpha, const float *__restrict__ de,
    const typename TT<GT>::S *__restrict__ g, typename TT<OT>::S *__restrict__ gx, float *__restrict__ gel,
    float *__restrict__ pacc, float *__restrict__ pgel, const GatDims d) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int64_t H = d.H, K = d.K;
  if (block_id() < d.chunk_blocks) {  // one wavefront per chunk of a long row
    const int64_t cid = block_id() * kWavesPerBlock + wave;
    if (cid >= d.n_chunks) return;
    const HubChunk hc = hub_chunk(rowptr, long_rows, chunk_ptr, d.n_long, d.chunk, cid);
    const int64_t beg = hc.beg, end = hc.end;
    for (int64_t kk = (int64_t)lane * VEC; kk < K; kk += (int64_t)kWave * VEC) {
      const int64_t h = kk / d.C;
      const bool lead = GEL && (kk == h * d.C);
      float acc[VEC], gl;
      gat_src_walk<GT, VEC>(colT, posT, alpha, de, g, H, K, h, d.es, kk, lead, beg, end, acc, gl);
      F32V<VEC>::store(pacc + cid * K + kk, acc);
      if (lead) pgel[cid * H + h] = gl;
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
    const int64_t h = kk / d.C;
    const bool lead = GEL && (kk == h * d.C);
    float acc[VEC], gl;
    gat_src_walk<GT, VEC>(colT, posT, alpha, de, g, H, K, h, d.es, kk, lead, beg, end, acc, gl);
    RowV<OT, VEC>::store(gx + row * K + kk, acc);
    if (lead) gel[row * H + h] = gl;
  }
}

// long source rows: partial sums combined in chunk order (deterministic)
template <typename OT, bool GEL = true>
__device__ __forceinline__ void gat_bwd_src_final_body(
    const int32_t *__restrict__ long_rows, const int64_t *__restrict__ chunk_ptr,
    const float *__restrict__ pacc, const float *__restrict__ pgel, typename TT<OT>::S *__restrict__ gx,
    float *__restrict__ gel, const GatDims &d) {
  const int64_t j = block_id();
  if (j >= d.n_long) return;
  const int64_t row = long_rows[j];
  const int64_t c0 = chunk_ptr[j], c1 = chunk_ptr[j + 1];
  for (int64_t k = threadIdx.x; k < d.K + (GEL ? d.H : 0); k += kBlock) {
    float acc = 0.0f;
    if (k < d.K) {
      for (int64_t c = c0; c < c1; ++c) acc = __fadd_rn(acc, pacc[c * d.K + k]);
      gx[row * d.K + k] = TT<OT>::store(acc);
    } else {
      const int64_t h = k - d.K;
      for (int64_t c = c0; c < c1; ++c) acc = __fadd_rn(acc, pgel[c * d.H + h]);
      gel[row * d.H + h] = acc;
    }
  }
}
__global__ __launch_bounds__(kBlock) void gat_bwd_src_final_kernel(
    const int32_t *__restrict__ long_rows, const int64_t *__restrict__ chunk_ptr,
    const float *__restrict__ pacc, const float *__restrict__ pgel, float *__restrict__ gx,
    float *__restrict__ gel, const GatDims d) {
  gat_bwd_src_final_body<float>(long_rows, chunk_ptr, pacc, pgel, gx, gel, d);
}
__global__ __launch_bounds__(kBlock) void gat_bwd_src_final_gx_kernel(  // GEL = false: the gx partials alone
    const int32_t *__restrict__ long_rows, const int64_t *__restrict__ chunk_ptr,
    const float *__restrict__ pacc, float *__restrict__ gx, const GatDims d) {
  gat_bwd_src_final_body<float, false>(long_rows, chunk_ptr, pacc, nullptr, gx, nullptr, d);
}
template <typename OT>
__global__ __launch_bounds__(kBlock) void gat_bwd_src_final16_kernel(
    const int32_t *__restrict__ long_rows, const int64_t *__restrict__ chunk_ptr,
    const float *__restrict__ pacc, const float *__restrict__ pgel, uint16_t *__restrict__ gx,
    float *__restrict__ gel, const GatDims d) {
  gat_bwd_src_final_body<OT>(long_rows, chunk_ptr, pacc, pgel, gx, gel, d);
}


}  // namespace ggl

using namespace ggl;

extern "C" size_t ggl_gat_partial_bytes(int64_t n_chunks, int64_t H, int64_t C) { return gat_fwd_partial_bytes(n_chunks, H, C); }
// the destination walk's ger partials, [n_chunks, H] floats (gat_bwd_dst_impl; the edge-logit form asks for them and writes none)
extern "C" size_t ggl_gat_bwd_dst_partial_bytes(int64_t n_chunks, int64_t H) { return ggl_partial_bytes(GGL_F32, n_chunks, H, 0); }
// the source walk's gx then gel partials, [n_chunks, H * C] and [n_chunks, H] floats (gat_bwd_src_impl, ggl_gat_fast_bwd)
extern "C" size_t ggl_gat_bwd_src_partial_bytes(int64_t n_chunks, int64_t H, int64_t C) {
  return ggl_partial_bytes(GGL_F32, n_chunks, H * C + H, 0);
}


// The three launchers are written once for every storage: XT = x / gx, OT = out, GT = g and the saved out.  float
// everywhere is the reference op (ggl_gat_fused_*); a 16-bit XT is ggl_gat_fused_*_x16.  Load forms: VEC = 4 where C % 4 == 0
// and every vector-accessed pointer is aligned to 4 elements (16 bytes of f32, 8 of 16-bit), 16-bit rows also VEC = 8
// (C % 8 == 0, 16 bytes), single elements otherwise.  No sum's order depends on VEC (the wide backward kernel keeps its
// assignment, see there), so a 16-bit call computes the f32 call's bits on the widened rows whatever form it takes.
// LS = kLogitEdge (ggl_edge_softmax_agg_*, f32 only): `el` is z [E, H], `er` plan->perm; slope is not read.
template <typename XT, typename OT, int LS = kLogitSeparable>
static int gat_fwd_impl(const ggl_segplan_t *plan, const int32_t *col, const float *el, typename Logit<LS>::Aux er,
                        const typename TT<XT>::S *x, float slope, int64_t H, int64_t C, float p_drop,
                        int64_t *rng_state, typename TT<OT>::S *out, float *rowmax, float *rowden, void *stream) {
  WalkPlan p;
  if (int rc = walk_plan(plan, "plan", "plan is NULL", "H, C and chunk must be positive",
                         gat_fwd_partial_bytes(hub_chunks(plan), H, C), p))
    return rc;
  GGL_REQUIRE(H > 0 && C > 0, GGL_EINVAL, "H, C and chunk must be positive");
  const int64_t N = p.N;
  if (N == 0) return GGL_OK;
  GGL_REQUIRE((LS == kLogitEdge || er) && out && rowmax && rowden, GGL_EINVAL, "NULL pointer");
  GGL_REQUIRE((col && el && x) || p.E == 0, GGL_EINVAL, "NULL pointer");
  GatFwd f;
  if (int rc = gat_fwd_setup(p, slope, H, C, p_drop, rng_state, f)) return rc;
  const GatDims &d = f.d;
  auto vec_ok = [&](int v) {
    return (C % v == 0) && gat_aligned<XT>(x, v) && gat_aligned<OT>(out, v) && gat_aligned<float>(f.pacc, v) &&
           !options().force_generic;
  };
  const bool vec8 = gat_is16<XT>::value && vec_ok(8);
  const bool vec4 = vec8 || vec_ok(4);
  const int vec = vec8 ? 8 : (vec4 ? 4 : 1);
  if (int rc = gat_fwd_grid(f, vec)) return rc;
#define GGL_GAT_FWD(V, DR)                                                                                           \
  GGL_LAUNCH((gat_fwd_kernel<XT, OT, V, DR, LS>), f.grid, kBlock, as_stream(stream), plan->rowptr, col, p.order,     \
             plan->long_rows, plan->chunk_ptr, el, er, x, out, rowmax, rowden, f.pacc, f.pm, f.pd,                   \
             (const int64_t *)rng_state, d)
  if (vec == 8) {  // (16-bit rows only: the f32 op has no such instantiation)
    if constexpr (gat_is16<XT>::value) {
      if (d.drop_thresh) GGL_GAT_FWD(8, true);
      else GGL_GAT_FWD(8, false);
    }
  } else if (vec4 && d.drop_thresh) GGL_GAT_FWD(4, true);
  else if (vec4) GGL_GAT_FWD(4, false);
  else if (d.drop_thresh) GGL_GAT_FWD(1, true);
  else GGL_GAT_FWD(1, false);
#undef GGL_GAT_FWD
  return gat_fwd_finish<OT>(plan, f, out, rowmax, rowden, rng_state, stream);
}

extern "C" int ggl_gat_fused_fwd(const ggl_segplan_t *plan, const int32_t *col, const float *el,
                                 const float *er, const float *x, float slope, int64_t H, int64_t C,
                                 float p_drop, int64_t *rng_state, float *out, float *rowmax,
                                 float *rowden, void *stream) {
  return gat_fwd_impl<float, float>(plan, col, el, er, x, slope, H, C, p_drop, rng_state, out, rowmax, rowden, stream);
}

// LS = kLogitEdge: `el` is z, `er` plan->perm, `de` gz in the caller's edge order; alpha or de may be NULL (not stored),
// ger and plan->partial are not written.
template <typename XT, typename GT, int LS = kLogitSeparable>
static int gat_bwd_dst_impl(const ggl_segplan_t *plan, const int32_t *col, const float *el, typename Logit<LS>::Aux er,
                            const typename TT<XT>::S *x, const typename TT<GT>::S *g,
                            const typename TT<GT>::S *out, const float *rowmax, const float *rowden, float slope,
                            int64_t H, int64_t C, float p_drop, const int64_t *rng_used, float *alpha, float *de,
                            float *ger, void *stream) {
  WalkPlan p;
  if (int rc = walk_plan(plan, "plan", "plan is NULL", "H, C and chunk must be positive",
                         ggl_gat_bwd_dst_partial_bytes(hub_chunks(plan), H), p))
    return rc;
  GGL_REQUIRE(H > 0 && C > 0, GGL_EINVAL, "H, C and chunk must be positive");
  const int64_t N = p.N, E = p.E;
  if (N == 0) return GGL_OK;
  constexpr bool edge = LS == kLogitEdge;
  GGL_REQUIRE((edge || (er && ger)) && g && out && rowmax && rowden, GGL_EINVAL, "NULL pointer");
  GGL_REQUIRE((col && el && x && (edge || (alpha && de))) || E == 0, GGL_EINVAL, "NULL pointer");
  if (edge && !alpha && !de) return GGL_OK;  // neither gradient is wanted
  GatDims d{};
  d.slope = slope; d.N = N; d.H = H; d.C = C; d.K = H * C; d.E = E;
  d.es = (!edge && de == alpha + 1) ? 2 : 1;  // de == alpha + 1: one interleaved [E,H,2] buffer
  d.chunk = p.chunk; d.n_long = p.n_long; d.n_chunks = p.n_chunks;
  if (int rc = set_dropout(d, p_drop, rng_used)) return rc;
  float *pger = p.partial;
  d.logL = pow2_log2(H);  // lanes per work item: the next power of two >= H, at most 64
  const int64_t items = d.n_chunks + N;
  const int64_t grid = ceil_div(items << d.logL, (int64_t)kBlock);
  GGL_REQUIRE(grid < ((int64_t)1 << 31), GGL_EINVAL, "too many rows for one launch");
  const int32_t *order = p.order;
  hipStream_t s = as_stream(stream);
  constexpr bool x16 = gat_is16<XT>::value;
  // (out is read by vectors in the wide kernel only; the f32 entry keeps its two tests, every torch allocation passes all)
  auto vec_ok = [&](int v) {
    return (C % v == 0) && gat_aligned<XT>(x, v) && gat_aligned<GT>(g, v) && (!x16 || gat_aligned<GT>(out, v)) &&
           !options().force_generic;
  };
  const bool vec8 = x16 && vec_ok(8);
  const bool vec4 = vec8 || vec_ok(4);
#ifndef GGL_EMULATE
  // wide heads: lanes split the channels, shuffle-reduced dots (gat_bwd_dst_wide_kernel); needs a head count
  // the kernel is instantiated for and a head that fits one group (C <= 64 * vec)
  {
    // 16-bit rows: the assignment the f32 op takes on the widened (always 16-byte aligned) panel, i.e. by C alone;
    // whether the four channels arrive in one load is d.vl
    const bool wide4 = x16 ? ((C % 4 == 0) && !options().force_generic) : vec4;
    d.vl = vec4 ? 1 : 0;
    const int vec = wide4 ? 4 : 1;
    const bool h_ok = H <= 16;  // instantiated head-loop bounds: 1, 2, 4, 8, 16 (the next one >= H is used)
    if (C > 16 && h_ok && C <= 64 * vec && !options().force_generic) {
      int logg = pow2_log2(ceil_div(C, vec));
      if (logg < 4) logg = 4;  // >= 16 lanes: covers H <= 16 finishing lanes
      const int64_t wgrid = ceil_div(items << logg, (int64_t)kBlock);
#define GGL_GAT_WIDE(V, LG, HH)                                                                          \
  GGL_LAUNCH((gat_bwd_dst_wide_kernel<XT, GT, V, LG, HH, LS>), wgrid, kBlock, s, plan->rowptr, col, order,    \
             plan->long_rows, plan->chunk_ptr, el, er, x, g, out, rowmax, rowden, alpha, de, ger, pger,   \
             rng_used, d)
#define GGL_GAT_WIDE_H(V, LG)                                                                            \
  do {                                                                                                   \
    if (H == 1) GGL_GAT_WIDE(V, LG, 1);                                                                  \
    else if (H == 2) GGL_GAT_WIDE(V, LG, 2);                                                             \
    else if (H <= 4) GGL_GAT_WIDE(V, LG, 4);                                                             \
    else if (H <= 8) GGL_GAT_WIDE(V, LG, 8);                                                             \
    else GGL_GAT_WIDE(V, LG, 16);                                                                        \
  } while (0)
      if (wide4) {
        if (logg == 4) GGL_GAT_WIDE_H(4, 4);
        else if (logg == 5) GGL_GAT_WIDE_H(4, 5);
        else GGL_GAT_WIDE_H(4, 6);
      } else {
        if (logg <= 5) { logg = 5; GGL_GAT_WIDE_H(1, 5); }
        else GGL_GAT_WIDE_H(1, 6);
      }
#undef GGL_GAT_WIDE_H
#undef GGL_GAT_WIDE
      GGL_LAUNCH_CHECK();
      if (!edge && plan->n_long > 0) {
        GGL_LAUNCH((gat_bwd_dst_final_kernel), gat_grid_for(plan->n_long * H), kBlock, s, plan->long_rows,
                   plan->chunk_ptr, (const float *)pger, ger, plan->n_long, H);
        GGL_LAUNCH_CHECK();
      }
      return GGL_OK;
    }
  }
#endif
#define GGL_GAT_DST(V, CR)                                                                              \
  GGL_LAUNCH((gat_bwd_dst_kernel<XT, GT, V, CR, LS>), grid, kBlock, s, plan->rowptr, col, order, plan->long_rows, \
             plan->chunk_ptr, el, er, x, g, out, rowmax, rowden, alpha, de, ger, pger, rng_used, d)
  if (vec8) {  // (16-bit rows only)
    if constexpr (x16) {
      if (C == 8) GGL_GAT_DST(8, 8);
      else if (C == 16) GGL_GAT_DST(8, 16);
      else GGL_GAT_DST(8, 0);
    }
  } else if (vec4 && C == 8) GGL_GAT_DST(4, 8);
  else if (vec4 && C == 16) GGL_GAT_DST(4, 16);
  else if (vec4) GGL_GAT_DST(4, 0);
  else GGL_GAT_DST(1, 0);
#undef GGL_GAT_DST
  GGL_LAUNCH_CHECK();
  if (!edge && plan->n_long > 0) {
    GGL_LAUNCH((gat_bwd_dst_final_kernel), gat_grid_for(plan->n_long * H), kBlock, s, plan->long_rows,
               plan->chunk_ptr, (const float *)pger, ger, plan->n_long, H);
    GGL_LAUNCH_CHECK();
  }
  return GGL_OK;
}

extern "C" int ggl_gat_fused_bwd_dst(const ggl_segplan_t *plan, const int32_t *col,
                                     const int32_t *rowidx, const float *el, const float *er,
                                     const float *x, const float *g, const float *out,
                                     const float *rowmax, const float *rowden, float slope, int64_t H,
                                     int64_t C, float p_drop, const int64_t *rng_used, float *alpha,
                                     float *de, float *ger, float *dot_ws, void *stream) {
  (void)rowidx; (void)dot_ws;  // needed by the first (edge-parallel) version; accepted, unused
  return gat_bwd_dst_impl<float, float>(plan, col, el, er, x, g, out, rowmax, rowden, slope, H, C, p_drop, rng_used,
                                        alpha, de, ger, stream);
}

// Source-major half of the backward (gat_bwd_src_kernel above).  planT->partial: ggl_gat_bwd_src_partial_bytes.
// GEL = false: gx alone (ggl_edge_softmax_agg_bwd_src); de and gel are NULL.
template <typename GT, typename OT, bool GEL = true>
static int gat_bwd_src_impl(const ggl_segplan_t *planT, const int32_t *colT, const int32_t *posT, const float *alpha,
                            const float *de, const typename TT<GT>::S *g, int64_t H, int64_t C,
                            typename TT<OT>::S *gx, float *gel, void *stream) {
  WalkPlan p;
  if (int rc = walk_plan(planT, "transposed plan", "planT is NULL", "H, C and chunk must be positive",
                         ggl_gat_bwd_src_partial_bytes(hub_chunks(planT), H, C), p))
    return rc;
  GGL_REQUIRE(H > 0 && C > 0, GGL_EINVAL, "H, C and chunk must be positive");
  const int64_t N = p.N;
  if (N == 0) return GGL_OK;
  GGL_REQUIRE(gx && (gel || !GEL), GGL_EINVAL, "NULL pointer");
  GGL_REQUIRE((colT && posT && alpha && (de || !GEL) && g) || p.E == 0, GGL_EINVAL, "NULL pointer");
  GatDims d{};
  d.N = N; d.H = H; d.C = C; d.K = H * C; d.E = p.E;
  d.es = (GEL && de == alpha + 1) ? 2 : 1;
  d.chunk = p.chunk; d.n_long = p.n_long; d.n_chunks = p.n_chunks;
  float *pacc = p.partial, *pgel = nullptr;
  if (p.n_long > 0) {
    pgel = pacc + p.n_chunks * d.K;
    d.chunk_blocks = ceil_div(p.n_chunks, kWavesPerBlock);
  }
  auto vec_ok = [&](int v) {
    return (C % v == 0) && gat_aligned<GT>(g, v) && gat_aligned<OT>(gx, v) && gat_aligned<float>(pacc, v) &&
           !options().force_generic;
  };
  const bool vec8 = gat_is16<OT>::value && vec_ok(8);
  const bool vec4 = vec8 || vec_ok(4);
  const int vec = vec8 ? 8 : (vec4 ? 4 : 1);
  d.logL = pow2_log2(ceil_div(d.K, vec));
  d.nblocks = ceil_div(N, (int64_t)kWavesPerBlock * (kWave >> d.logL));
  const int64_t grid = d.chunk_blocks + d.nblocks;
  GGL_REQUIRE(grid < ((int64_t)1 << 31), GGL_EINVAL, "too many rows for one launch");
  hipStream_t s = as_stream(stream);
#define GGL_GAT_SRC(V)                                                                                          \
  GGL_LAUNCH((gat_bwd_src_kernel<GT, OT, V, GEL>), grid, kBlock, s, planT->rowptr, colT, posT, p.order, planT->long_rows, \
             planT->chunk_ptr, alpha, de, g, gx, gel, pacc, pgel, d)
  if (vec == 8) {  // (16-bit gx only)
    if constexpr (gat_is16<OT>::value) GGL_GAT_SRC(8);
  } else if (vec4) GGL_GAT_SRC(4);
  else GGL_GAT_SRC(1);
#undef GGL_GAT_SRC
  GGL_LAUNCH_CHECK();
  if (planT->n_long > 0) {
    if constexpr (!GEL)
      GGL_LAUNCH((gat_bwd_src_final_gx_kernel), planT->n_long, kBlock, s, planT->long_rows, planT->chunk_ptr,
                 (const float *)pacc, gx, d);
    else if constexpr (std::is_same<OT, float>::value)
      GGL_LAUNCH((gat_bwd_src_final_kernel), planT->n_long, kBlock, s, planT->long_rows, planT->chunk_ptr,
                 (const float *)pacc, (const float *)pgel, gx, gel, d);
    else
      GGL_LAUNCH((gat_bwd_src_final16_kernel<OT>), planT->n_long, kBlock, s, planT->long_rows, planT->chunk_ptr,
                 (const float *)pacc, (const float *)pgel, gx, gel, d);
    GGL_LAUNCH_CHECK();
  }
  return GGL_OK;
}

extern "C" int ggl_gat_fused_bwd_src(const ggl_segplan_t *planT, const int32_t *colT,
                                     const int32_t *posT, const float *alpha, const float *de,
                                     const float *g, int64_t H, int64_t C, float *gx, float *gel,
                                     void *stream) {
  return gat_bwd_src_impl<float, float>(planT, colT, posT, alpha, de, g, H, C, gx, gel, stream);
}

// ---- The same three walks on per-edge logits z [E, H] in the caller's edge order (any attention layer that calls
// segment_softmax on its logits and sums alpha * x[src]): the kernels above with the kLogitEdge policy, f32 only.
// Contract in include/ggl_mpops.h; on z = LeakyReLU(el[src] + er[dst]) every output has ggl_gat_fused_*'s bits.
extern "C" int ggl_edge_softmax_agg_fwd(const ggl_segplan_t *plan, const int32_t *col, const float *z, const float *x,
                                        int64_t H, int64_t C, float p_drop, int64_t *rng_state, float *out,
                                        float *rowmax, float *rowden, void *stream) {
  return gat_fwd_impl<float, float, kLogitEdge>(plan, col, z, plan ? plan->perm : nullptr, x, 1.0f, H, C, p_drop,
                                                rng_state, out, rowmax, rowden, stream);
}

extern "C" int ggl_edge_softmax_agg_bwd_dst(const ggl_segplan_t *plan, const int32_t *col, const float *z,
                                            const float *x, const float *g, const float *out, const float *rowmax,
                                            const float *rowden, int64_t H, int64_t C, float p_drop,
                                            const int64_t *rng_used, float *alpha, float *gz, void *stream) {
  return gat_bwd_dst_impl<float, float, kLogitEdge>(plan, col, z, plan ? plan->perm : nullptr, x, g, out, rowmax, rowden,
                                                    1.0f, H, C, p_drop, rng_used, alpha, gz, nullptr, stream);
}

extern "C" int ggl_edge_softmax_agg_bwd_src(const ggl_segplan_t *planT, const int32_t *colT, const int32_t *posT,
                                            const float *alpha, const float *g, int64_t H, int64_t C, float *gx,
                                            void *stream) {
  return gat_bwd_src_impl<float, float, false>(planT, colT, posT, alpha, nullptr, g, H, C, gx, nullptr, stream);
}

// ---- 16-bit storage (an extension: the reference's GAT is f32 only).  Contract in include/ggl_mpops.h: the f32 entry
// points above are F, these compute F's bits on the widened rows and round out / gx once.
#define GGL_GAT16_PAIR(XD, OD, CALL)                                                       \
  do {                                                                                     \
    if ((XD) == GGL_BF16 && (OD) == GGL_BF16) { using XT = mxbf16_t; using OT = mxbf16_t; CALL; } \
    if ((XD) == GGL_BF16 && (OD) == GGL_F32) { using XT = mxbf16_t; using OT = float; CALL; }     \
    if ((XD) == GGL_F16 && (OD) == GGL_F16) { using XT = mxf16_t; using OT = mxf16_t; CALL; }     \
    if ((XD) == GGL_F16 && (OD) == GGL_F32) { using XT = mxf16_t; using OT = float; CALL; }       \
  } while (0)

extern "C" int ggl_gat_fused_fwd_x16(const ggl_segplan_t *plan, const int32_t *col, const float *el, const float *er,
                                     int x_dtype, const void *x, float slope, int64_t H, int64_t C, float p_drop,
                                     int64_t *rng_state, int out_dtype, void *out, float *rowmax, float *rowden,
                                     void *stream) {
  GGL_GAT16_PAIR(x_dtype, out_dtype,
                 return (gat_fwd_impl<XT, OT>(plan, col, el, er, static_cast<const uint16_t *>(x), slope, H, C, p_drop,
                                              rng_state, static_cast<typename TT<OT>::S *>(out), rowmax, rowden,
                                              stream)));
  GGL_REQUIRE(false, GGL_EDTYPE, "gat_fused_fwd_x16: x must be bf16 / f16 and out x's dtype or f32 (got %d -> %d)",
              x_dtype, out_dtype);
}

extern "C" int ggl_gat_fused_bwd_dst_x16(const ggl_segplan_t *plan, const int32_t *col, const float *el,
                                         const float *er, int x_dtype, const void *x, int g_dtype, const void *g,
                                         int out_dtype, const void *out, const float *rowmax, const float *rowden,
                                         float slope, int64_t H, int64_t C, float p_drop, const int64_t *rng_used,
                                         float *alpha, float *de, float *ger, void *stream) {
  if (g_dtype == out_dtype)
    GGL_GAT16_PAIR(x_dtype, out_dtype,
                   return (gat_bwd_dst_impl<XT, OT>(plan, col, el, er, static_cast<const uint16_t *>(x),
                                                    static_cast<const typename TT<OT>::S *>(g),
                                                    static_cast<const typename TT<OT>::S *>(out), rowmax, rowden,
                                                    slope, H, C, p_drop, rng_used, alpha, de, ger, stream)));
  GGL_REQUIRE(false, GGL_EDTYPE,
              "gat_fused_bwd_dst_x16: x must be bf16 / f16, out x's dtype or f32, g out's dtype (got x %d, g %d, out %d)",
              x_dtype, g_dtype, out_dtype);
}

extern "C" int ggl_gat_fused_bwd_src_x16(const ggl_segplan_t *planT, const int32_t *colT, const int32_t *posT,
                                         const float *alpha, const float *de, int g_dtype, const void *g, int64_t H,
                                         int64_t C, int gx_dtype, void *gx, float *gel, void *stream) {
  GGL_GAT16_PAIR(gx_dtype, g_dtype,  // XT = storage of gx, OT = storage of g
                 return (gat_bwd_src_impl<OT, XT>(planT, colT, posT, alpha, de,
                                                  static_cast<const typename TT<OT>::S *>(g), H, C,
                                                  static_cast<uint16_t *>(gx), gel, stream)));
  GGL_REQUIRE(false, GGL_EDTYPE, "gat_fused_bwd_src_x16: gx must be bf16 / f16 and g gx's dtype or f32 (got %d -> %d)",
              g_dtype, gx_dtype);
}
#undef GGL_GAT16_PAIR

// =====================================================================================================================
// Edge softmax as an op of its own: ggl_segment_softmax_fwd / _bwd (gammagl/utils/softmax.py:29-35, the function every
// attention layer calls on its [E, H] logits).  Replaces, per direction, the chain segment_max -> gather -> sub / exp ->
// segment_sum -> gather -> add / div (8+ launches, four [E, H] temporaries, two narrow-K segment reductions) by one walk
// kernel, plus a chunk pass and a per-row merge in front (and, backward, a winner fix-up behind) when the plan has long rows.
//
// Shape: one or more lanes per (work item, column); work item = a row of at most plan->chunk elements, or one chunk of a
// longer row.  The K lanes of an item sit next to each other, so a gathered record x[perm[p], 0:K] is ONE 4K-byte access
// of the group and perm[p] a broadcast.  No LDS, no barriers, no atomics.  With one lane per (item, column) — the host
// build's only form — a lane walks its item's sorted positions serially and 64 / K rows share a wavefront; the GPU build
// may split an item's positions between S lanes (see "Sub-lanes" below).
//   forward : walk 1 m = max x;  walk 2 D = sum exp(x - m) in double;  walk 3 y = exp(x - m) / (f32(D) + 1e-16f).
//             Walk 1 fetches the row's records from HBM; walks 2 and 3 find them in L2 (a wavefront's 64 / K rows of mean
//             length L hold 256 L bytes: 25-130 KiB at L = 100-500) or, for rows that fell out of it, in the MALL.
//             For a row walked in one piece the numerators of walk 3 and the terms of walk 2 are the SAME rounded exp
//             values, which keeps its y summing to 1 within 3 x 2^-24 — an online (one-walk) max / sum would evaluate
//             them at different maxima.  (Long rows DO: their D is merged from chunk-local maxima, see below; their sum
//             is held to the tested 1e-6, not to that derived bound.)
//   backward: walk 1 S = sum y g in double and the winner (largest y, first among equals);  walk 2 gx = y * f32(g - S) for
//             everyone else, their double sum T on the way, then gx[winner] = f32(-T).
//   long rows: ssm_*_chunk_kernel leaves chunk-local (m_c, D_c) / (S_c, ymax_c, p_c) in plan->partial; ssm_*_merge_kernel
//             merges them ONCE per (row, column) in chunk order (m = max m_c, D = sum D_c exp(m_c - m), the factor in
//             double; S = sum S_c, winner = largest ymax_c, first chunk among equals) into a per-row slot; the chunk items
//             of the walk kernel read that slot and write their chunk; backward, ssm_bwd_final_kernel adds the chunks' T_c
//             in chunk order and writes the winner.  A long row costs one more read of its elements than a short one.
// =====================================================================================================================
#ifndef GGL_EMULATE
#define GGL_EXPD(x) exp(x)
#else
#define GGL_EXPD(x) std::exp(x)
#endif

namespace ggl {

constexpr int kSsmU = 4;  // gathered loads a lane keeps in flight

struct SsmDims {
  int64_t N, K, chunk, n_long, n_chunks;
};

__device__ __forceinline__ int64_t ssm_elem(const int32_t *__restrict__ perm, int64_t p) {
  return perm ? (int64_t)perm[p] : p;
}

// Sub-lanes (GPU build only).  With LOGS > 0 a work item's column is shared by S = 2^LOGS lanes that take every S-th
// sorted position (lane s: beg + s, beg + s + S, ...): for K = 1 a 64-lane load of perm is 64 consecutive entries, a row
// of 500 elements is 8 steps of a wavefront instead of 500 of a lane, and the lanes of a wavefront finish together.
// Thread t -> (item, s, k) = (t / (S K), (t / K) % S, t % K); K is a power of two with S K <= 64, so the S lanes of an
// (item, column) sit K apart inside ONE wavefront and combine their maxima / double sums / winners with an xor butterfly
// (every lane ends with the same bits, and the same bits every run).  The host build has no cross-lane exchange and
// instantiates LOGS = 0 only, where these are the identity.
#ifndef GGL_EMULATE
template <int LOGS> __device__ __forceinline__ float ssm_all_max(float v, int K) {
#pragma unroll
  for (int i = 0; i < LOGS; ++i) {
    const float o = __shfl_xor(v, K << i, 64);
    if (v < o) v = o;
  }
  return v;
}
template <int LOGS> __device__ __forceinline__ double ssm_all_sum(double v, int K) {
#pragma unroll
  for (int i = 0; i < LOGS; ++i) v = __dadd_rn(v, __shfl_xor(v, K << i, 64));
  return v;
}
// largest y, smallest position among equals
template <int LOGS> __device__ __forceinline__ void ssm_all_winner(float &ym, int64_t &pw, int K) {
#pragma unroll
  for (int i = 0; i < LOGS; ++i) {
    const float oy = __shfl_xor(ym, K << i, 64);
    const int64_t op = (int64_t)__shfl_xor((long long)pw, K << i, 64);
    if (ym < oy || (ym == oy && op < pw)) { ym = oy; pw = op; }
  }
}
#else
template <int LOGS> __device__ __forceinline__ float ssm_all_max(float v, int) { return v; }
template <int LOGS> __device__ __forceinline__ double ssm_all_sum(double v, int) { return v; }
template <int LOGS> __device__ __forceinline__ void ssm_all_winner(float &, int64_t &, int) {}
#endif

template <int LOGS>
__device__ __forceinline__ void ssm_decode(int64_t K, int64_t &item, int64_t &k, int64_t &s) {
  const int64_t t = thread_id();
  const int64_t q = t / K;
  k = t - q * K;
  s = q & (((int64_t)1 << LOGS) - 1);
  item = q >> LOGS;
}

// One walk over the sorted positions beg, beg + step, ... < end for column k with kSsmU gathered loads in flight:
// f(p, e, a[e, k]) resp. f(p, e, a[e, k], b[e, k]) in position order.
template <typename F>
__device__ __forceinline__ void ssm_walk1(const float *__restrict__ a, const int32_t *__restrict__ perm, int64_t K,
                                          int64_t k, int64_t beg, int64_t end, int64_t step, F &&f) {
  constexpr int U = kSsmU;
  int64_t p = beg;
  for (; p + (U - 1) * step < end; p += U * step) {
    int64_t e[U];
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) e[u] = ssm_elem(perm, p + u * step);
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = a[e[u] * K + k];
#pragma unroll
    for (int u = 0; u < U; ++u) f(p + u * step, e[u], v[u]);
  }
  for (; p < end; p += step) {
    const int64_t e0 = ssm_elem(perm, p);
    f(p, e0, a[e0 * K + k]);
  }
}
template <typename F>
__device__ __forceinline__ void ssm_walk2(const float *__restrict__ a, const float *__restrict__ b,
                                          const int32_t *__restrict__ perm, int64_t K, int64_t k, int64_t beg,
                                          int64_t end, int64_t step, F &&f) {
  constexpr int U = kSsmU;
  int64_t p = beg;
  for (; p + (U - 1) * step < end; p += U * step) {
    int64_t e[U];
    float v[U], w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) e[u] = ssm_elem(perm, p + u * step);
#pragma unroll
    for (int u = 0; u < U; ++u) { v[u] = a[e[u] * K + k]; w[u] = b[e[u] * K + k]; }
#pragma unroll
    for (int u = 0; u < U; ++u) f(p + u * step, e[u], v[u], w[u]);
  }
  for (; p < end; p += step) {
    const int64_t e0 = ssm_elem(perm, p);
    f(p, e0, a[e0 * K + k], b[e0 * K + k]);
  }
}

// m = max x, D = sum exp(x - m) (double) over [beg, end), the item's lanes together
template <int LOGS>
__device__ __forceinline__ void ssm_max_den(const float *__restrict__ x, const int32_t *__restrict__ perm, int64_t K,
                                            int64_t k, int64_t s, int64_t beg, int64_t end, float &m, double &D) {
  constexpr int64_t S = (int64_t)1 << LOGS;
  float mm = -FLT_MAX;  // unsorted_segment_max: lowest() fill, strict <
  ssm_walk1(x, perm, K, k, beg + s, end, S, [&](int64_t, int64_t, float v) { if (mm < v) mm = v; });
  mm = ssm_all_max<LOGS>(mm, (int)K);
  double dd = 0.0;
  ssm_walk1(x, perm, K, k, beg + s, end, S,
            [&](int64_t, int64_t, float v) { dd = __dadd_rn(dd, (double)GGL_EXPF(__fadd_rn(v, -mm))); });
  m = mm;
  D = ssm_all_sum<LOGS>(dd, (int)K);
}

// forward partials of one chunk and column: part[(cid * K + k) * 2 + {0, 1}] = {m_c, D_c}
template <int LOGS>
__global__ __launch_bounds__(kBlock) void ssm_fwd_chunk_kernel(const int64_t *__restrict__ rowptr,
                                                               const int32_t *__restrict__ perm,
                                                               const int32_t *__restrict__ long_rows,
                                                               const int64_t *__restrict__ chunk_ptr,
                                                               const float *__restrict__ x, double *__restrict__ part,
                                                               const SsmDims d) {
  int64_t cid, k, s;
  ssm_decode<LOGS>(d.K, cid, k, s);
  if (cid >= d.n_chunks) return;  // whole lane groups leave together: the butterflies stay inside a group
  const HubChunk hc = hub_chunk(rowptr, long_rows, chunk_ptr, d.n_long, d.chunk, cid);
  const int64_t beg = hc.beg, end = hc.end;
  float m;
  double D;
  ssm_max_den<LOGS>(x, perm, d.K, k, s, beg, end, m, D);
  if (s == 0) {
    part[(cid * d.K + k) * 2] = (double)m;
    part[(cid * d.K + k) * 2 + 1] = D;
  }
}

// long rows, once per (row, column): the chunks' (m_c, D_c) merged in chunk order by the online-softmax identity
// (m = max m_c, D = sum D_c exp(m_c - m), the factor in double) into rowp[(j * K + k) * 2 + {0, 1}] = {m, D}
__global__ __launch_bounds__(kBlock) void ssm_fwd_merge_kernel(const int64_t *__restrict__ chunk_ptr,
                                                               const double *__restrict__ part,
                                                               double *__restrict__ rowp, const SsmDims d) {
  const int64_t t = thread_id();
  const int64_t j = t / d.K, k = t - j * d.K;
  if (j >= d.n_long) return;
  const int64_t c0 = chunk_ptr[j], c1 = chunk_ptr[j + 1];
  float m = -FLT_MAX;
  for (int64_t c = c0; c < c1; ++c) {
    const float mc = (float)part[(c * d.K + k) * 2];
    if (m < mc) m = mc;
  }
  double D = 0.0;
  for (int64_t c = c0; c < c1; ++c)
    D = __dadd_rn(D, part[(c * d.K + k) * 2 + 1] * GGL_EXPD(part[(c * d.K + k) * 2] - (double)m));
  rowp[(j * d.K + k) * 2] = (double)m;
  rowp[(j * d.K + k) * 2 + 1] = D;
}

template <int LOGS>
__global__ __launch_bounds__(kBlock) void ssm_fwd_kernel(const int64_t *__restrict__ rowptr,
                                                         const int32_t *__restrict__ perm,
                                                         const int32_t *__restrict__ row_order,
                                                         const int32_t *__restrict__ long_rows,
                                                         const int64_t *__restrict__ chunk_ptr,
                                                         const float *__restrict__ x, float *__restrict__ y,
                                                         const double *__restrict__ rowp, const SsmDims d) {
  constexpr int64_t S = (int64_t)1 << LOGS;
  int64_t item, k, s;
  ssm_decode<LOGS>(d.K, item, k, s);
  if (item >= d.n_chunks + d.N) return;
  int64_t beg, end;
  float m;
  double D;
  if (item < d.n_chunks) {  // chunks carry the lowest item ids: the hub work is dispatched first
    const HubChunk hc = hub_chunk(rowptr, long_rows, chunk_ptr, d.n_long, d.chunk, item);
    beg = hc.beg; end = hc.end;
    m = (float)rowp[(hc.slot * d.K + k) * 2];  // merged once per row by ssm_fwd_merge_kernel
    D = rowp[(hc.slot * d.K + k) * 2 + 1];
  } else {
    const int64_t slot = item - d.n_chunks;
    const int64_t row = row_order ? (int64_t)row_order[slot] : slot;
    beg = rowptr[row];
    end = rowptr[row + 1];
    if (end == beg || end - beg > d.chunk) return;  // empty: nothing to write; long: its chunks are separate items
    ssm_max_den<LOGS>(x, perm, d.K, k, s, beg, end, m, D);
  }
  const float den = __fadd_rn((float)D, 1e-16f);  // softmax.py:35: exp / (sum + 1e-16)
  ssm_walk1(x, perm, d.K, k, beg + s, end, S, [&](int64_t, int64_t e, float v) {
    y[e * d.K + k] = __fdiv_rn(GGL_EXPF(__fadd_rn(v, -m)), den);
  });
}

// S = sum y g (double), the winner's y and sorted position (largest y, first among equals) over [beg, end)
template <int LOGS>
__device__ __forceinline__ void ssm_bwd_stats(const float *__restrict__ y, const float *__restrict__ g,
                                              const int32_t *__restrict__ perm, int64_t K, int64_t k, int64_t s,
                                              int64_t beg, int64_t end, double &Ssum, float &ymax, int64_t &pwin) {
  constexpr int64_t S = (int64_t)1 << LOGS;
  double ss = 0.0;
  float ym = -1.0f;  // y >= 0: the first element wins an all-zero column
  int64_t pw = beg + s < end ? beg + s : INT64_MAX;
  ssm_walk2(y, g, perm, K, k, beg + s, end, S, [&](int64_t p, int64_t, float yv, float gv) {
    ss = __dadd_rn(ss, (double)yv * (double)gv);
    if (ym < yv) { ym = yv; pw = p; }
  });
  ssm_all_winner<LOGS>(ym, pw, (int)K);
  Ssum = ssm_all_sum<LOGS>(ss, (int)K);
  ymax = ym;
  pwin = pw;
}

// gx = y * f32(g - S) for this lane's positions of [beg, end) but pwin; returns the double sum of what the item's lanes wrote
template <int LOGS>
__device__ __forceinline__ double ssm_bwd_write(const float *__restrict__ y, const float *__restrict__ g,
                                                const int32_t *__restrict__ perm, int64_t K, int64_t k, int64_t s,
                                                int64_t beg, int64_t end, double Ssum, int64_t pwin,
                                                float *__restrict__ gx) {
  constexpr int64_t S = (int64_t)1 << LOGS;
  double T = 0.0;
  ssm_walk2(y, g, perm, K, k, beg + s, end, S, [&](int64_t p, int64_t e, float yv, float gv) {
    if (p == pwin) return;
    const float r = __fmul_rn(yv, (float)((double)gv - Ssum));
    gx[e * K + k] = r;
    T = __dadd_rn(T, (double)r);
  });
  return ssm_all_sum<LOGS>(T, (int)K);
}

// backward partials of one chunk and column: part[(cid * K + k) * 4 + {0, 1, 2}] = {S_c, ymax_c, p_c}; slot 3 (T_c) is the
// walk kernel's
template <int LOGS>
__global__ __launch_bounds__(kBlock) void ssm_bwd_chunk_kernel(const int64_t *__restrict__ rowptr,
                                                               const int32_t *__restrict__ perm,
                                                               const int32_t *__restrict__ long_rows,
                                                               const int64_t *__restrict__ chunk_ptr,
                                                               const float *__restrict__ y, const float *__restrict__ g,
                                                               double *__restrict__ part, const SsmDims d) {
  int64_t cid, k, s;
  ssm_decode<LOGS>(d.K, cid, k, s);
  if (cid >= d.n_chunks) return;
  const HubChunk hc = hub_chunk(rowptr, long_rows, chunk_ptr, d.n_long, d.chunk, cid);
  const int64_t beg = hc.beg, end = hc.end;
  double Ssum;
  float ym;
  int64_t pw;
  ssm_bwd_stats<LOGS>(y, g, perm, d.K, k, s, beg, end, Ssum, ym, pw);
  if (s == 0) {
    double *q = part + (cid * d.K + k) * 4;
    q[0] = Ssum;
    q[1] = (double)ym;
    q[2] = (double)pw;  // positions < 2^53: exact
  }
}

// the row's S and winner position from its chunks' partials, chunk order
__device__ __forceinline__ void ssm_bwd_merge(const double *__restrict__ part, int64_t K, int64_t k, int64_t c0,
                                              int64_t c1, double &Ssum, int64_t &pwin) {
  double ss = 0.0, ym = -1.0, pw = 0.0;
  for (int64_t c = c0; c < c1; ++c) {
    const double *q = part + (c * K + k) * 4;
    ss = __dadd_rn(ss, q[0]);
    if (c == c0 || ym < q[1]) { ym = q[1]; pw = q[2]; }
  }
  Ssum = ss;
  pwin = (int64_t)pw;
}

// long rows, once per (row, column): rowp[(j * K + k) * 2 + {0, 1}] = {S, winner position}
__global__ __launch_bounds__(kBlock) void ssm_bwd_merge_kernel(const int64_t *__restrict__ chunk_ptr,
                                                               const double *__restrict__ part,
                                                               double *__restrict__ rowp, const SsmDims d) {
  const int64_t t = thread_id();
  const int64_t j = t / d.K, k = t - j * d.K;
  if (j >= d.n_long) return;
  double Ssum;
  int64_t pwin;
  ssm_bwd_merge(part, d.K, k, chunk_ptr[j], chunk_ptr[j + 1], Ssum, pwin);
  rowp[(j * d.K + k) * 2] = Ssum;
  rowp[(j * d.K + k) * 2 + 1] = (double)pwin;
}

template <int LOGS>
__global__ __launch_bounds__(kBlock) void ssm_bwd_kernel(const int64_t *__restrict__ rowptr,
                                                         const int32_t *__restrict__ perm,
                                                         const int32_t *__restrict__ row_order,
                                                         const int32_t *__restrict__ long_rows,
                                                         const int64_t *__restrict__ chunk_ptr,
                                                         const float *__restrict__ y, const float *__restrict__ g,
                                                         float *__restrict__ gx, double *__restrict__ part,
                                                         const double *__restrict__ rowp, const SsmDims d) {
  int64_t item, k, s;
  ssm_decode<LOGS>(d.K, item, k, s);
  if (item >= d.n_chunks + d.N) return;
  if (item < d.n_chunks) {
    const HubChunk hc = hub_chunk(rowptr, long_rows, chunk_ptr, d.n_long, d.chunk, item);
    const double Ssum = rowp[(hc.slot * d.K + k) * 2];  // merged once per row by ssm_bwd_merge_kernel
    const int64_t pwin = (int64_t)rowp[(hc.slot * d.K + k) * 2 + 1];
    const double T = ssm_bwd_write<LOGS>(y, g, perm, d.K, k, s, hc.beg, hc.end, Ssum, pwin, gx);
    if (s == 0) part[(item * d.K + k) * 4 + 3] = T;
    return;
  }
  const int64_t slot = item - d.n_chunks;
  const int64_t row = row_order ? (int64_t)row_order[slot] : slot;
  const int64_t beg = rowptr[row], end = rowptr[row + 1];
  if (end == beg || end - beg > d.chunk) return;
  double Ssum;
  float ym;
  int64_t pwin;
  ssm_bwd_stats<LOGS>(y, g, perm, d.K, k, s, beg, end, Ssum, ym, pwin);
  const double T = ssm_bwd_write<LOGS>(y, g, perm, d.K, k, s, beg, end, Ssum, pwin, gx);
  if (s == 0) gx[ssm_elem(perm, pwin) * d.K + k] = (float)(0.0 - T);
}

// long rows: the winner's gradient = -(sum of the chunks' T_c, chunk order)
__global__ __launch_bounds__(kBlock) void ssm_bwd_final_kernel(const int32_t *__restrict__ perm,
                                                               const int64_t *__restrict__ chunk_ptr,
                                                               const double *__restrict__ part,
                                                               const double *__restrict__ rowp, float *__restrict__ gx,
                                                               const SsmDims d) {
  const int64_t t = thread_id();
  const int64_t j = t / d.K, k = t - j * d.K;
  if (j >= d.n_long) return;
  const int64_t c0 = chunk_ptr[j], c1 = chunk_ptr[j + 1];
  const int64_t pwin = (int64_t)rowp[(j * d.K + k) * 2 + 1];
  double T = 0.0;
  for (int64_t c = c0; c < c1; ++c) T = __dadd_rn(T, part[(c * d.K + k) * 4 + 3]);
  gx[ssm_elem(perm, pwin) * d.K + k] = (float)(0.0 - T);
}

// lanes per (item, column) as log2: the library's policy on the GPU, one lane on the host
static inline int ssm_logs(const ggl_segplan_t *plan, int64_t K) {
#ifndef GGL_EMULATE
  int64_t S = ggl_policy_softmax_sublanes(K, plan->E, plan->N);
  if (S < 1 || (K & (K - 1)) != 0) S = 1;
  int l = 0;
  while (l < 6 && ((int64_t)2 << l) <= S && (((int64_t)2 << l) * K) <= kWave) ++l;
  return l;
#else
  (void)plan; (void)K;
  return 0;
#endif
}

static inline int ssm_setup(const ggl_segplan_t *plan, int64_t K, SsmDims &d, double *&part, const int32_t *&order,
                            int &logs) {
  WalkPlan p;
  if (int rc = walk_plan(plan, "plan", "plan is NULL", "chunk must be positive",
                         ggl_segment_softmax_partial_bytes(hub_chunks(plan), K), p))
    return rc;
  GGL_REQUIRE(ggl_segment_softmax_supported(K), GGL_EINVAL, "segment_softmax: K = %lld is outside [1, 64]", (long long)K);
  d.N = p.N; d.K = K;
  d.n_long = p.n_long;
  d.n_chunks = p.n_chunks;
  d.chunk = d.n_long > 0 ? p.chunk : INT64_MAX;  // no long-row table: every row in one piece
  order = p.order;
  part = p.partial ? reinterpret_cast<double *>((reinterpret_cast<uintptr_t>(p.partial) + 7u) & ~(uintptr_t)7u) : nullptr;
  logs = ssm_logs(plan, K);
  GGL_REQUIRE(ceil_div(((d.n_chunks + d.N) * K) << logs, kBlock) < ((int64_t)1 << 31), GGL_EINVAL,
              "too many rows for one launch");
  return GGL_OK;
}

}  // namespace ggl

// KERN<LOGS> for the run-time `logs`; the host build has LOGS = 0 only
#ifndef GGL_EMULATE
#define GGL_SSM_LAUNCH(KERN, GRID, ...)                                              \
  do {                                                                               \
    switch (logs) {                                                                  \
      case 1: GGL_LAUNCH((KERN<1>), GRID, kBlock, s, __VA_ARGS__); break;            \
      case 2: GGL_LAUNCH((KERN<2>), GRID, kBlock, s, __VA_ARGS__); break;            \
      case 3: GGL_LAUNCH((KERN<3>), GRID, kBlock, s, __VA_ARGS__); break;            \
      case 4: GGL_LAUNCH((KERN<4>), GRID, kBlock, s, __VA_ARGS__); break;            \
      case 5: GGL_LAUNCH((KERN<5>), GRID, kBlock, s, __VA_ARGS__); break;            \
      case 6: GGL_LAUNCH((KERN<6>), GRID, kBlock, s, __VA_ARGS__); break;            \
      default: GGL_LAUNCH((KERN<0>), GRID, kBlock, s, __VA_ARGS__); break;           \
    }                                                                                \
  } while (0)
#else
#define GGL_SSM_LAUNCH(KERN, GRID, ...) GGL_LAUNCH((KERN<0>), GRID, kBlock, s, __VA_ARGS__)
#endif

extern "C" int ggl_segment_softmax_supported(int64_t K) { return (K >= 1 && K <= 64) ? 1 : 0; }

extern "C" size_t ggl_segment_softmax_partial_bytes(int64_t n_chunks, int64_t K) {
  if (n_chunks <= 0 || K <= 0) return 0;
  // per chunk and column {S, ymax, p, T} (forward: {m, D}), then per long row and column {S, p} ({m, D}); n_long <= n_chunks
  return (size_t)n_chunks * (size_t)K * 6 * sizeof(double) + 64;
}

extern "C" int ggl_segment_softmax_fwd(const float *x, const ggl_segplan_t *plan, int64_t K, float *y, void *stream) {
  SsmDims d{};
  double *part = nullptr;
  const int32_t *order = nullptr;
  int logs = 0;
  if (int rc = ssm_setup(plan, K, d, part, order, logs)) return rc;
  if (plan->E == 0 || d.N == 0) return GGL_OK;
  GGL_REQUIRE(x && y, GGL_EINVAL, "NULL pointer");
  double *rowp = part ? part + d.n_chunks * K * 4 : nullptr;  // the long rows' merged statistics
  hipStream_t s = as_stream(stream);
  if (d.n_chunks > 0) {
    GGL_SSM_LAUNCH(ssm_fwd_chunk_kernel, ceil_div((d.n_chunks * K) << logs, kBlock), plan->rowptr, plan->perm,
                   plan->long_rows, plan->chunk_ptr, x, part, d);
    GGL_LAUNCH_CHECK();
    GGL_LAUNCH((ssm_fwd_merge_kernel), ceil_div(d.n_long * K, kBlock), kBlock, s, plan->chunk_ptr, (const double *)part,
               rowp, d);
    GGL_LAUNCH_CHECK();
  }
  GGL_SSM_LAUNCH(ssm_fwd_kernel, ceil_div(((d.n_chunks + d.N) * K) << logs, kBlock), plan->rowptr, plan->perm, order,
                 plan->long_rows, plan->chunk_ptr, x, y, (const double *)rowp, d);
  GGL_LAUNCH_CHECK();
  return GGL_OK;
}

extern "C" int ggl_segment_softmax_bwd(const float *y, const float *g, const ggl_segplan_t *plan, int64_t K, float *gx,
                                       void *stream) {
  SsmDims d{};
  double *part = nullptr;
  const int32_t *order = nullptr;
  int logs = 0;
  if (int rc = ssm_setup(plan, K, d, part, order, logs)) return rc;
  if (plan->E == 0 || d.N == 0) return GGL_OK;
  GGL_REQUIRE(y && g && gx, GGL_EINVAL, "NULL pointer");
  double *rowp = part ? part + d.n_chunks * K * 4 : nullptr;
  hipStream_t s = as_stream(stream);
  if (d.n_chunks > 0) {
    GGL_SSM_LAUNCH(ssm_bwd_chunk_kernel, ceil_div((d.n_chunks * K) << logs, kBlock), plan->rowptr, plan->perm,
                   plan->long_rows, plan->chunk_ptr, y, g, part, d);
    GGL_LAUNCH_CHECK();
    GGL_LAUNCH((ssm_bwd_merge_kernel), ceil_div(d.n_long * K, kBlock), kBlock, s, plan->chunk_ptr, (const double *)part,
               rowp, d);
    GGL_LAUNCH_CHECK();
  }
  GGL_SSM_LAUNCH(ssm_bwd_kernel, ceil_div(((d.n_chunks + d.N) * K) << logs, kBlock), plan->rowptr, plan->perm, order,
                 plan->long_rows, plan->chunk_ptr, y, g, gx, part, (const double *)rowp, d);
  GGL_LAUNCH_CHECK();
  if (d.n_long > 0) {
    GGL_LAUNCH((ssm_bwd_final_kernel), ceil_div(d.n_long * K, kBlock), kBlock, s, plan->perm, plan->chunk_ptr,
               (const double *)part, (const double *)rowp, gx, d);
    GGL_LAUNCH_CHECK();
  }
  return GGL_OK;
}

// ---- GATv2: the logit's part of the backward (ggl_gatv2_logit_bwd); its forward is gatv2.hip ----
#include "gatv2_bwd.hpp"
