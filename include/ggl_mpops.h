/*
 * include/ggl_mpops.h — C ABI of libggl_mpops_hip.so: the MI355X (gfx950) message-passing backend
 * that replaces GammaGL's gammagl/mpops/torch_ext (`_torch_ext`) for the torch backend.
 *
 * Boundary.  The reference binds its native ops to Python through a pybind11 module with seven
 * free functions (gammagl/mpops/torch_ext/src/operators.cpp:51-59):
 *     c_segment_sum / c_segment_mean / c_segment_max (Tensor x, Tensor index, int64 N) -> Tensor
 *     c_spmm_sum / c_spmm_mean / c_spmm_max / c_bspmm_sum (Tensor index, Tensor weight, Tensor x)
 * each a torch::autograd::Function (include/<op>.h, src/<op>.cpp) that dispatches to a CPU loop
 * (cpu/<op>_cpu.cpp) or an atomic CUDA kernel (cuda/<op>_cuda.cu).  This header is what an FFI for that path
 * binds instead: plain device pointers, sizes and a HIP stream — no torch types.  Every entry
 * point cites the reference function it supersedes.  The ctypes stub a GammaGL maintainer would
 * add is in INTEGRATION.md; gammagl_amd/mpops.py is that stub, complete.
 *
 * Conventions
 *   - All data pointers are DEVICE pointers on the current HIP device unless named *_host.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Every compute entry
 *     point is asynchronous and stream-ordered and performs NO host synchronisation; the
 *     ggl_plan_* entry points are synchronous (they return host-side facts about the graph) and are
 *     meant to run once per edge list, not once per step.
 *   - Return value: GGL_OK or a negative GGL_E* code; ggl_last_error() gives a message.
 *   - Feature rows are contiguous, row-major: x[e*K + k].  K = product of trailing dims
 *     (segment_sum_cpu.cpp:44: K = x.numel() / x.size(0)).
 *   - No atomics anywhere on the reduction path: every output row is produced by exactly one
 *     wavefront group that walks the row's edges in ascending ORIGINAL edge order, which makes the
 *     results run-to-run deterministic and, for rows shorter than the long-row threshold,
 *     bit-identical to the reference's serial CPU loops (same order of the same rounded adds).
 */
#ifndef GGL_MPOPS_H
#define GGL_MPOPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 5 (round 3): + ggl_bspmm_grad_w_sorted[_scratch_bytes]; v4's number had not been raised for the symbols added
 * late in round 2 (ggl_sample_hop, ggl_block_transpose, ggl_gat_sh_*, ggl_segment_hub16*, ggl_spmm_col_blocks) */
/* 6 (round 4): + ggl_calib_stream (bench.py's achievable-rate yardstick) */
/* 7 (round 4): ggl_segplan_t GREW by `long_order` and `max_len` (appended; hubf32.hip's serial hub walk); + ggl_spmm_max_bwd32;
 *   ggl_policy_gradw_sorted takes (H, C).  Because the struct grew, a caller compiled against ABI <= 6 would hand the
 *   library a SHORTER struct than it reads: every caller MUST check ggl_abi_version() == GGL_ABI_VERSION before it passes
 *   a ggl_segplan_t (gammagl_amd/_lib.py bind(), ggl_torch.cpp api_for() both refuse a mismatching library). */
/* 8 (round 5): + ggl_invert_perm, ggl_spmm_max_mask[_bytes], ggl_spmm_max_bwd_mask (gspmm max backward through a 1-bit
 *   winner mask), ggl_spmm_max_mask_words; ggl_spmm_max_bwd_mask takes mask_pos; ggl_gat_fast_bwd's plan->partial holds four
 *   doubles per chunk and head; ggl_segplan_t.xcd_run_rows < 0 is a hint (see the field); + ggl_sample_hop_ex; options
 *   hub_one_launch, hub_priority, hub_pipe, maxbwd_mask*, gat_sh_waves, hop_fused_scans.  No struct change. */
/* 9 (round 6): + ggl_policy_maxbwd_form (the gspmm-max backward's form gated on the winner mask's footprint; option
 *   maxbwd_mask_kmax), ggl_gat_sh_bwd's forward-plan partial holds four doubles per chunk and head, + ggl_spmm_col_blocks_plan (128-column blocks for plans whose node order carries locality), option gat_sh_pk.
 *   No struct change. */
/* 10: + ggl_segment_softmax_{fwd,bwd,supported,partial_bytes} (the edge softmax of utils/softmax.py as one op each way),
 *   ggl_policy_softmax_sublanes, option softmax_sublanes.  No struct change. */
/* still 10: + ggl_spmm_{sum,mean,mean_bwd}_x16, ggl_spmm_col_blocks_x16, option col_block16 (the mixed-precision aggregate).
 *   Purely ADDITIVE symbols: no struct, no existing signature and no existing behaviour changed, so a caller built against 10
 *   keeps working and the number stays (hosts that want the new entry points look them up by name). */
/* 11: the forms that lost their measurements are gone (DESIGN.md "Forms removed in ABI 11"; last present in 992473a):
 *   ggl_spmm_max_mask loses `tpos` and ggl_spmm_max_mask_words loses `forward_order` (records are in forward position order,
 *   always), ggl_spmm_max_bwd_mask REQUIRES mask_pos, - ggl_invert_perm; options gat_sh_{pk,pipe,glds,prefetch,zlds,waves},
 *   hop_fused_scans, hop_small_scans, hub_priority, hub_pipe and maxbwd_mask_{scatter,wlane,cols} no longer exist (set answers
 *   GGL_EINVAL, get -1); ggl_sample_hop_workspace_bytes shrinks; + ggl_option_name (the option table's enumerator); every
 *   option reads GGL_<NAME> from the environment.  No struct change. */
/* still 11: + ggl_gat_fused_{fwd,bwd_dst,bwd_src}_x16 (the fused GAT on bf16 / f16 rows).  Purely additive, as the _x16
 *   aggregates were in 10. */
/* still 11: + ggl_spmm_grad_w, ggl_spmm_grad_w_scratch_bytes (gspmm's sum / mean gradient with respect to the edge weights, on
 *   f32 / bf16 / f16 rows).  Purely additive again. */
/* still 11: + ggl_spmm_epi_x16, ggl_bias_act_fwd_x16, ggl_bias_act_bwd_x16 (the fused epilogue and the bias / ReLU / dropout
 *   pass on bf16 / f16 rows: f32 arithmetic, one rounding at the store).  Purely additive again. */
/* still 11: + ggl_edge_softmax_agg_{fwd,bwd_dst,bwd_src} (the fused GAT walks on per-edge logits: edge softmax + weighted
 *   aggregate for any attention layer).  Purely additive again. */
/* still 11: + ggl_dot_attn_supported, ggl_dot_attn_fwd, ggl_policy_dot_attn_fused (scaled dot-product graph attention: the
 *   logit formed inside the aggregate's walk).  Purely additive again. */
/* still 11: + ggl_linear_bias_act_bwd, ggl_policy_linear_epi_bwd (the epilogue's backward on a gradient that is a narrow
 *   product, formed in registers).  Purely additive again. */
/* still 11: + ggl_gatv2_supported, ggl_policy_gatv2_fused, ggl_gatv2_fwd, ggl_gatv2_logit_bwd, ggl_gatv2_logit_bwd_partial_bytes
 *   (GATv2's additive attention: the logit formed inside the aggregate's walk, and its backward walk).  Purely additive again. */
/* still 11: + ggl_segment_multi_fwd, ggl_segment_multi_bwd, ggl_segment_multi_partial_bytes and the codes GGL_AGG_* (sum, mean,
 *   min, max, var and std of the same message rows in one walk).  Purely additive again. */
/* 12: ggl_segplan_t GREW by `partial_bytes` (appended, as 7 did): the bytes the caller owns at `partial`.  Every entry point
 *   that carves plan->partial checks it against the *_partial_bytes export that sizes its walk and answers GGL_EWORKSPACE to a
 *   buffer that is too small; a caller built against <= 11 hands over a shorter struct and is refused by the version check.
 *   + ggl_gat_bwd_dst_partial_bytes, ggl_gat_bwd_src_partial_bytes, ggl_gat_fast_bwd_dst_partial_bytes,
 *   ggl_gat_sh_bwd_dst_partial_bytes, ggl_gat_sh_bwd_src_partial_bytes (every walk has a sizer of its own; each returns what
 *   the header documented for it before). */
#define GGL_ABI_VERSION 12

/* dtype codes (AT_DISPATCH_ALL_TYPES_AND2(Half, BFloat16), segment_sum_cpu.cpp:32-33) */
enum {
  GGL_U8 = 0, GGL_I8 = 1, GGL_I16 = 2, GGL_I32 = 3, GGL_I64 = 4,
  GGL_F16 = 5, GGL_BF16 = 6, GGL_F32 = 7, GGL_F64 = 8
};

enum {
  GGL_OK = 0,
  GGL_EINVAL = -1,   /* bad argument (TORCH_CHECK in the reference -> RuntimeError) */
  GGL_EINDEX = -2,   /* id out of range (TORCH_CHECK_INDEX -> IndexError, segment_max_cpu.cpp:50) */
  GGL_EDTYPE = -3,   /* unsupported dtype ("expected scalar type Float", spmm_sum_cpu.cpp:22) */
  GGL_EHIP = -4,     /* HIP runtime error */
  GGL_EWORKSPACE = -5 /* workspace too small */
};

int ggl_abi_version(void);
const char *ggl_last_error(void);          /* thread-local message of the last failing call */
/* compute-unit count, wavefront size and gfx arch string of the current device (host query) */
int ggl_device_info(int *cus_host, int *wave_host, char *arch_host, int arch_len);

/* ------------------------------------------------------------------------------------------------
 * Segment plan: a destination-sorted (CSR-like) view of an unsorted id vector.
 * The reference walks `index[e]` for e = 0..E-1 and scatters (segment_sum_cpu.cpp:47-56;
 * CUDA: one atomicAdd per (e,k), segment_sum_cuda.cu:19-31).  Here the ids are stably sorted once
 * per edge list (rocPRIM LSD radix sort on (id, e) pairs), giving
 *   perm[p]   : original element index of the p-th element in sorted order (ascending e inside
 *               a segment), or no perm at all when the ids already arrive sorted;
 *   rowptr[s] : first sorted position of segment s (int64, N+1 entries).
 * Rows longer than `chunk` are listed in long_rows and are reduced chunk-by-chunk into a partial
 * buffer and then combined in chunk order (still deterministic).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ggl_segplan {
  const int64_t *rowptr;    /* [N+1] */
  const int32_t *perm;      /* [E] or NULL when the ids were already sorted */
  const int32_t *long_rows; /* [n_long] row ids with more than `chunk` elements, or NULL */
  const int64_t *chunk_ptr; /* [n_long+1] exclusive prefix of per-long-row chunk counts, or NULL */
  int64_t n_long;
  int64_t n_chunks;         /* chunk_ptr[n_long] */
  int64_t chunk;            /* elements per chunk == long-row threshold (> 0) */
  void *partial;            /* workspace: the entry point's *_partial_bytes(...) bytes, or NULL when n_long == 0 */
  int64_t N;                /* number of segments (output rows) */
  int64_t E;                /* number of elements (edges) */
  const int32_t *row_order; /* [N] rows sorted by length (longest first) or NULL: the order in which
                               row slots are handed to wavefronts — scheduling only, results identical */
  int64_t xcd_run_rows;     /* > 0: the node order carries locality — hand each XCD runs of this many consecutive row
                               slots (its private L2 then serves one neighbourhood instead of 1/8 of every one);
                               0: the library default (round-robin); < 0 (ABI 8): no runs, but the plan's long rows LEAD the id
                               range (a degree-sorted node order) — a column-blocked aggregate then walks its hub rows once
                               over the full width (option hub_one_launch = 2).  Scheduling only (ABI 5). */
  const int32_t *long_order; /* [n_long] positions in long_rows by descending row length, or NULL: the order in which the
                               serial hub walk (hubf32.hip) starts its rows — longest first, so that the one add chain
                               nobody can shorten runs under everything else.  Scheduling only (ABI 6). */
  int64_t max_len;          /* elements of the longest row (ggl_plan_build's *max_len_host), or 0 = unknown.  The serial hub
                               walk adds a row's elements one after the other (~3.5 ns each): a plan whose longest row
                               exceeds the option `exact_long_max` (2^21 elements; a star graph's centre) keeps the
                               chunked walk — within rounding of the reference instead of its bits — rather than wait
                               for one add chain (ABI 7). */
  size_t partial_bytes;     /* bytes the caller owns at `partial` (ABI 12); ignored when n_long == 0.  An entry point that
                               needs more answers GGL_EWORKSPACE and launches nothing. */
} ggl_segplan_t;

/* bytes of workspace ggl_plan_build needs */
size_t ggl_plan_workspace_bytes(int64_t E, int64_t N);

/* Build perm/rowptr from ids[E] (int64 on device, the reference's index dtype:
 * segment_sum_cpu.cpp:36 data_ptr<int64_t>).  SYNCHRONOUS: one host read for E <= 2^22 (flags, sort, row
 * pointer and longest row are queued behind it: a fresh edge list per mini-batch costs ~0.1 ms), two above (the
 * first decides whether an already sorted 10^8-element list skips its sort).  perm may be written even when the
 * input turns out sorted (then *is_sorted_host = 1 and the caller may drop it).
 * Errors: GGL_EINDEX if any id < 0 or >= N (the reference: IndexError for max,
 * segment_max_cpu.cpp:50; silent out-of-bounds write for sum/mean). */
int ggl_plan_build(const int64_t *ids, int64_t E, int64_t N, int32_t *perm, int64_t *rowptr,
                   void *workspace, size_t workspace_bytes, void *stream, int32_t *is_sorted_host,
                   int64_t *max_len_host);

/* Long-row bookkeeping (SYNCHRONOUS): count, then fill long_rows[n_long] (ascending row id) and
 * chunk_ptr[n_long+1].  Both need ggl_plan_long_workspace_bytes(N) bytes of scratch. */
size_t ggl_plan_long_workspace_bytes(int64_t N);
int ggl_plan_long_count(const int64_t *rowptr, int64_t N, int64_t chunk, void *workspace,
                        size_t workspace_bytes, void *stream, int64_t *n_long_host,
                        int64_t *n_chunks_host);
int ggl_plan_long_fill(const int64_t *rowptr, int64_t N, int64_t chunk, int64_t n_long,
                       int32_t *long_rows, int64_t *chunk_ptr, void *workspace,
                       size_t workspace_bytes, void *stream);
/* ------------------------------------------------------------------------------------------------
 * Restricted plan pair (still ABI 10: additive) — the plans of a graph cut down to a SORTED, DUPLICATE-FREE list
 * rows[R] (int64) of destination rows, built from the full pair without a sort.  An aggregate whose consumer reads
 * only those rows (a loss over the training nodes) then walks only the edges that end in them, and its backward
 * gathers a compact [R, K] gradient instead of an [N_dst, K] one that is zero elsewhere:
 *   forward   R x N_src : row r = the slice rowptr[rows[r]] .. rowptr[rows[r] + 1] of the full plan's col / weights;
 *   transposed N_src x R: the full transposed plan filtered to the elements whose destination is listed (flag,
 *                         exclusive scan, compact), colT_r = rank of the destination in rows[].
 * Every row keeps its elements in the full plan's order, so its sum has the same bits; the skipped terms are w * (+0).
 * col_r / colT_r / w_r are in sorted order (launch with w_by_pos = 1, perm = NULL); long-row bookkeeping as for any
 * plan (ggl_plan_long_count / _fill on rowptr_r / rowptrT_r).  w (or NULL) is read at wperm[p] when wperm != NULL (the
 * plan's perm: caller's edge order), at p otherwise.
 *   ggl_plan_rows_rank       SYNCHRONOUS: validates rows (GGL_EINDEX out of [0, N); GGL_EINVAL unsorted / repeated) and
 *                            writes rank[N] (int32: position in rows[], -1 = not listed)
 *   ggl_plan_rows_fwd_rowptr SYNCHRONOUS: rowptr_r[R + 1], *E_r_host = elements kept
 *   ggl_plan_rows_fwd_fill   col_r[E_r], w_r[E_r]
 *   ggl_plan_rows_bwd_rowptr SYNCHRONOUS: pos[E + 1] (int32 scratch: exclusive scan of the keep flags) and
 *                            rowptrT_r[N_src + 1] read off it at the old row boundaries; *E_r_host = elements kept
 *   ggl_plan_rows_bwd_fill   colT_r[E_r], w_r[E_r]
 * workspace: ggl_plan_rows_workspace_bytes(E, N, R) bytes serve every call above.
 * ---------------------------------------------------------------------------------------------- */
size_t ggl_plan_rows_workspace_bytes(int64_t E, int64_t N, int64_t R);
int ggl_plan_rows_rank(const int64_t *rows, int64_t R, int64_t N, int32_t *rank, void *workspace,
                       size_t workspace_bytes, void *stream);
int ggl_plan_rows_fwd_rowptr(const int64_t *rowptr, const int64_t *rows, int64_t R, int64_t *rowptr_r, void *workspace,
                             size_t workspace_bytes, void *stream, int64_t *E_r_host);
int ggl_plan_rows_fwd_fill(const int64_t *rowptr, const int32_t *col, const float *w, const int32_t *wperm,
                           const int64_t *rows, int64_t R, const int64_t *rowptr_r, int64_t E_r, int32_t *col_r,
                           float *w_r, void *stream);
int ggl_plan_rows_bwd_rowptr(const int64_t *rowptrT, const int32_t *colT, int64_t N_src, int64_t E, const int32_t *rank,
                             int32_t *pos, int64_t *rowptrT_r, void *workspace, size_t workspace_bytes, void *stream,
                             int64_t *E_r_host);
int ggl_plan_rows_bwd_fill(const int32_t *colT, const float *w, const int32_t *wperm, int64_t E, const int32_t *rank,
                           const int32_t *pos, int32_t *colT_r, float *w_r, void *stream);

/* plan->partial of the segment reductions and of gspmm / bspmm and their backward walks, for a plan with n_chunks hub chunks:
 * K features of dtype per chunk (value + int64 arg for max; K = H * C for bspmm; GGL_F32 for the _x16 entry points, whose
 * partials are f32).  Every entry point named below checks plan->partial_bytes against the export that sizes its walk, called
 * with the plan's n_chunks and its own arguments, and answers GGL_EWORKSPACE when the buffer is smaller. */
size_t ggl_partial_bytes(int dtype, int64_t n_chunks, int64_t K, int with_arg);

/* p[0..n) = v */
int ggl_fill_i64(int64_t *p, int64_t n, int64_t v, void *stream);

/* out_i32[p] = (int32) src_i64[perm ? perm[p] : p]   — e.g. the CSR column array from edge_index[0] */
int ggl_gather_i64_to_i32(const int64_t *src, const int32_t *perm, int64_t E, int32_t *out,
                          void *stream);
/* out[p, :] = src[perm[p], :] for rows of H floats (edge weights into sorted order) */
int ggl_gather_rows_f32(const float *src, const int32_t *perm, int64_t E, int64_t H, float *out,
                        void *stream);
/* out[i, 0:K] = src[idx[i], 0:K], row strides src_ld / out_ld (elements, >= K): the send buffer of one
 * feature-column block of the halo exchange gathered straight from the activation matrix (no reference
 * counterpart: SURVEY.md §8e; replaces h[:, c0:c1].index_select(0, idx).contiguous()) */
int ggl_gather_rows_f32_ex(const float *src, int64_t src_ld, const int64_t *idx, int64_t n, int64_t K,
                           float *out, int64_t out_ld, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Format conversion: device-side ind2ptr / ptr2ind (gammagl/ops/sparse,
 * cpu/convert.cpp:58-128, cuda/convert.cu:41-104) and sort_edge_index (utils/sort_edge_index.py:30-44).
 *   ggl_ind2ptr   : ptr[M+1] = exclusive prefix of the histogram of ind[E] (int64; SYNCHRONOUS:
 *                   validates 0 <= ind < M like ggl_plan_build)
 *   ggl_ptr2ind   : ind[p] = r with ptr[r] <= p < ptr[r+1]
 *   ggl_sort_edges: perm[E] = stable argsort of major[i] * N + minor[i]
 * ---------------------------------------------------------------------------------------------- */
size_t ggl_ind2ptr_workspace_bytes(int64_t E, int64_t M);
int ggl_ind2ptr(const int64_t *ind, int64_t E, int64_t M, int64_t *ptr, void *workspace,
                size_t workspace_bytes, void *stream);
int ggl_ptr2ind(const int64_t *ptr, int64_t M, int64_t E, int64_t *ind, void *stream);
size_t ggl_sort_edges_workspace_bytes(int64_t E, int64_t N);
int ggl_sort_edges(const int64_t *major, const int64_t *minor, int64_t E, int64_t N, int32_t *perm,
                   void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Segment reductions — supersede segment_{sum,mean,max}_{cpu,cuda}_forward
 * (cpu/segment_sum_cpu.cpp:11-60, cpu/segment_mean_cpu.cpp:11-80, cpu/segment_max_cpu.cpp:11-69;
 *  cuda/segment_sum_cuda.cu:33-116, cuda/segment_mean_cuda.cu, cuda/segment_max_cuda.cu).
 * x [E,K] of `dtype`, out [N,K] (every element written).  Semantics are those of the CPU
 * extension: accumulate in the storage dtype; mean = sum / count with count held in the storage
 * dtype and applied only where count > 1 (integer dtypes: truncating division); max pre-fills
 * with numeric_limits<T>::lowest(), strict `<` so the smallest e wins ties and NaN never wins;
 * if E*K == 0 max returns zeros.  arg [N,K] int64 = winning element index, `arg_fill` for empty
 * segments (the caller passes E; the reference's N aliases real rows — see DESIGN.md).
 * ---------------------------------------------------------------------------------------------- */
int ggl_segment_sum(int dtype, const void *x, const ggl_segplan_t *plan, int64_t K, void *out,
                    void *stream);
int ggl_segment_mean(int dtype, const void *x, const ggl_segplan_t *plan, int64_t K, void *out,
                     void *stream);
/* Wide f32 SpMM-sum / mean launches are cut into column blocks (64 wide; csrc/reduce.hip launch_f32_cols, options
 * "col_block" / "col_block_min_edges" / "col_block_min_degree"): the number of kernel launches one call over E edges,
 * K columns and N output rows makes. */
int64_t ggl_spmm_col_blocks(int64_t E, int64_t K, int64_t N);
/* ... for a plan: as above, blocks twice as wide where plan->xcd_run_rows > 0 (a node order with locality; ABI 9) */
int64_t ggl_spmm_col_blocks_plan(const ggl_segplan_t *plan, int64_t K);

/* f16 / bf16 sums accumulate in the storage type (segment_sum_cpu.cpp:47-56), so their hub rows cannot be chunked:
 * ggl_segment_hub16 reduces the plan's LONG rows (plan->long_rows) in the reference's serial order with a workgroup
 * per (row, 64-column slab) that prefetches through LDS (GPU build only: ggl_segment_hub16_supported; rows of a
 * multiple of 8 columns move as 16-byte pieces, other widths element by element).  Pair it with ggl_segment_{sum,mean} on the same plan with the long-row table withheld
 * (n_long = 0, chunk kept): that launch skips rows longer than chunk. */
int ggl_segment_hub16_supported(int dtype, int64_t K, const void *x, const void *out);
int ggl_segment_hub16(int dtype, int mean, const void *x, const ggl_segplan_t *plan, int64_t K, void *out,
                      void *stream);
int ggl_segment_max(int dtype, const void *x, const ggl_segplan_t *plan, int64_t K, void *out,
                    int64_t *arg, int64_t arg_fill, void *stream);

/* Backward passes — supersede SegmentSum/Mean/Max::backward (src/segment_sum.cpp:43-54,
 * src/segment_mean.cpp:44-63, src/segment_max.cpp:48-61).  f16/bf16/f32/f64 gradients.
 *   sum : gin[e,:]  = gout[ids[e],:]
 *   mean: gin[e,:]  = gout[ids[e],:] / count[ids[e]]       (count from rowptr)
 *   max : gin = 0;  gin[arg[s,k],k] = gout[s,k] for arg < E (empty segments contribute nothing) */
int ggl_segment_sum_bwd(int dtype, const void *gout, const int64_t *ids, int64_t E, int64_t K,
                        void *gin, void *stream);
int ggl_segment_mean_bwd(int dtype, const void *gout, const int64_t *ids, const int64_t *rowptr,
                         int64_t E, int64_t K, void *gin, void *stream);
int ggl_segment_max_bwd(int dtype, const void *gout, const int64_t *arg, int64_t E, int64_t N,
                        int64_t K, void *gin, void *stream);

/* ------------------------------------------------------------------------------------------------
 * gspmm — CSR x dense SpMM, f32; supersedes spmm_{sum,mean,max}_cpu_{forward,backward}
 * (cpu/spmm_sum_cpu.cpp:5-80, cpu/spmm_mean_cpu.cpp:5-105, cpu/spmm_max_cpu.cpp:5-99) and
 * spmm_sum_cuda_{forward,backward} (cuda/spmm_sum_cuda.cu:15-87).
 * plan  : rows = destination nodes (N_out = plan->N), sorted positions p = rowptr[i]..rowptr[i+1]
 * col   : [E] int32, source node of sorted position p
 * w     : [E] f32 edge weights or NULL (= all ones).  w_by_pos != 0: indexed by sorted position p;
 *         w_by_pos == 0: indexed by original edge id (through plan->perm when present).
 * x     : [N_in, K] f32;  out : [N_out, K] f32
 *   sum : out[i,:] = sum_p  w[p] * x[col[p],:]          (rounded multiply, then rounded add)
 *   mean: sum / (number of edges into i), only where that count > 0   (spmm_mean_cpu.cpp:51-58)
 *   max : out pre-filled with -FLT_MAX; arg [N_out,K] int64 = SOURCE NODE id of the winner
 *         (spmm_max_cpu.cpp:47), 0 where the row is empty.
 * The backward of `sum` w.r.t. x is the same call on the transposed plan (rows = source nodes,
 * col = destination nodes), which is exactly spmm_sum_cpu_backward's gx[src] += w[e] * g[dst].
 * ---------------------------------------------------------------------------------------------- */
/* Strided / accumulating forms of ggl_spmm_sum and ggl_segment_sum: x rows x_ld elements apart, out rows
 * out_ld apart (0 = K; >= K otherwise), and with accumulate != 0 the row sums are ADDED to what out holds
 * (the previous value first in the summation order).  They let the multi-GPU layer aggregate a column block
 * of a wider matrix in place and add the halo-source edges onto the local-source result without a
 * temporary and an extra pass. */
int ggl_spmm_sum_ex(const ggl_segplan_t *plan, const int32_t *col, const float *w, int w_by_pos,
                    const float *x, int64_t x_ld, int64_t K, float *out, int64_t out_ld, int accumulate,
                    void *stream);
int ggl_segment_sum_ex(int dtype, const void *x, int64_t x_ld, const ggl_segplan_t *plan, int64_t K,
                       void *out, int64_t out_ld, int accumulate, void *stream);
int ggl_spmm_sum(const ggl_segplan_t *plan, const int32_t *col, const float *w, int w_by_pos,
                 const float *x, int64_t K, float *out, void *stream);
int ggl_spmm_mean(const ggl_segplan_t *plan, const int32_t *col, const float *w, int w_by_pos,
                  const float *x, int64_t K, float *out, void *stream);
int ggl_spmm_max(const ggl_segplan_t *plan, const int32_t *col, const float *w, int w_by_pos,
                 const float *x, int64_t K, float *out, int64_t *argsrc, void *stream);
/* planT: rows = source nodes; colT[p] = destination node; fwd_rowptr = forward plan's rowptr
 *   mean bwd: gx[j,:] = sum_p (g[colT[p],:] / count[colT[p]]) * w[p]     (spmm_mean_cpu.cpp:95-101)
 *   max  bwd: gx[j,k] = sum_p [argsrc[colT[p],k] == j] w[p] * g[colT[p],k] (spmm_max_cpu.cpp:88-93) */
int ggl_spmm_mean_bwd(const ggl_segplan_t *planT, const int32_t *colT, const float *w, int w_by_pos,
                      const float *g, const int64_t *fwd_rowptr, int64_t K, float *gx,
                      void *stream);
int ggl_spmm_max_bwd(const ggl_segplan_t *planT, const int32_t *colT, const float *w, int w_by_pos,
                     const float *g, const int64_t *argsrc, int64_t K, float *gx, void *stream);
/* Mixed-precision aggregate (an extension: the reference's gspmm is f32 only).  x [N_in, K] is stored as GGL_BF16 or
 * GGL_F16, w stays f32; every element is widened at the load (exact), every product and add is the f32 one of
 * ggl_spmm_sum / ggl_spmm_mean in the same order, and the finished sum is rounded to nearest-even ONCE, at the store
 * (out_dtype == x_dtype), or not at all (out_dtype == GGL_F32).  With F = the f32 entry point on the same plan and weights:
 *     out_dtype == x_dtype : out == round(F(widen(x)))      out_dtype == GGL_F32 : out == F(widen(x))
 * bit for bit, under the conditions under which F itself is the serial sum (host build: always; GPU: hub rows through the
 * exact walk, i.e. E < 2^31 and max_len <= option exact_long_max; chunked otherwise, with F32 partials like F's).  Any other
 * dtype pair returns GGL_EDTYPE.  x_ld / out_ld: row strides in elements (0 = K).  plan->partial holds F32 partials:
 * ggl_partial_bytes(GGL_F32, n_chunks, K, 0), checked.  ggl_spmm_mean_bwd_x16 is ggl_spmm_mean_bwd on a 16-bit g (divide and
 * multiply in f32); the backward of the sum is ggl_spmm_sum_x16 on the transposed plan.
 * Wide rows are cut into column blocks of option "col_block16" columns: ggl_spmm_col_blocks_x16 = launches per call. */
int ggl_spmm_sum_x16(const ggl_segplan_t *plan, const int32_t *col, const float *w, int w_by_pos, int x_dtype,
                     const void *x, int64_t x_ld, int64_t K, int out_dtype, void *out, int64_t out_ld, void *stream);
int ggl_spmm_mean_x16(const ggl_segplan_t *plan, const int32_t *col, const float *w, int w_by_pos, int x_dtype,
                      const void *x, int64_t x_ld, int64_t K, int out_dtype, void *out, int64_t out_ld, void *stream);
int ggl_spmm_mean_bwd_x16(const ggl_segplan_t *planT, const int32_t *colT, const float *w, int w_by_pos, int g_dtype,
                          const void *g, const int64_t *fwd_rowptr, int64_t K, int gx_dtype, void *gx, void *stream);
int64_t ggl_spmm_col_blocks_x16(const ggl_segplan_t *plan, int64_t K);
/* the same walk with the witnesses in a compact int32 copy of argsrc (node ids index int32 arrays everywhere in this
 * library): the lookup is per edge AND column, 8 of the walk's 12 bytes per element with int64 witnesses.  NOT yet the
 * hosts' default: unmeasured on the GPU (the Engine takes it with the option `maxbwd_arg32`; results identical). */
int ggl_spmm_max_bwd32(const ggl_segplan_t *planT, const int32_t *colT, const float *w, int w_by_pos,
                       const float *g, const int32_t *argsrc32, int64_t K, float *gx, void *stream);
/* The max backward through a WINNER MASK (round 5; same sums in the same order as ggl_spmm_max_bwd, spmm_max_cpu.cpp:88-93):
 *   ggl_spmm_max_mask  walks the FORWARD plan (rows = destinations, where argsrc's row is wave-uniform) and writes one
 *     record per edge, bit k = [argsrc[dst, k] == colF[p]] for the edge at forward position p:
 *     records in FORWARD position order, ggl_spmm_max_mask_words(K) words each (ceil(K/32) rounded up to 1, 2, 4 or a
 *     multiple of 8), written as coalesced 32-record blocks; bit k of a record: word k/32, bit k%32.
 *     mask: ggl_spmm_max_mask_bytes(E, K) bytes, 16-byte aligned, every record fully overwritten;
 *   ggl_spmm_max_bwd_mask  is the transposed walk reading K/8 mask bytes per edge instead of 8K witness bytes: record
 *     mask_pos[t] for transposed position t — mask_pos = posT, the hosts' GraphPlan.posT, required where E * K > 0. */
int64_t ggl_spmm_max_mask_words(int64_t K);
size_t ggl_spmm_max_mask_bytes(int64_t E, int64_t K);
int ggl_spmm_max_mask(const ggl_segplan_t *planF, const int32_t *colF, const int64_t *argsrc, int64_t K, uint32_t *mask,
                      void *stream);
int ggl_spmm_max_bwd_mask(const ggl_segplan_t *planT, const int32_t *colT, const float *w, int w_by_pos,
                          const float *g, const uint32_t *mask, const int32_t *mask_pos, int64_t K, float *gx,
                          void *stream);

/* ------------------------------------------------------------------------------------------------
 * bspmm — multi-head SpMM, f32; supersedes bspmm_sum_cpu_{forward,backward}
 * (cpu/bspmm_sum_cpu.cpp:7-56, 58-113).  x [N_in,H,C], w [E,H], out [N_out,H,C]:
 *   out[i,h,c] = sum_p w[p,h] * x[col[p],h,c]
 * backward: gx = the same call on the transposed plan with g in place of x;
 *           gw[e,h] = sum_c x[src[e],h,c] * g[dst[e],h,c]  (edge-parallel, original edge order).
 * ---------------------------------------------------------------------------------------------- */
int ggl_bspmm_sum(const ggl_segplan_t *plan, const int32_t *col, const float *w, int w_by_pos,
                  const float *x, int64_t H, int64_t C, float *out, void *stream);
int ggl_bspmm_grad_w(const int64_t *index /* [2,E] int64 */, const float *x, const float *g,
                     int64_t E, int64_t H, int64_t C, float *gw, void *stream);
/* The same weight gradient (bspmm_sum_cpu.cpp:95-107: serial over c, rounded multiply then rounded add — bit for
 * bit) computed along the destination-sorted FORWARD plan: col[p] / rowidx[p] = source / destination node of sorted
 * position p, the result goes to gw[perm[p], h] (the caller's edge order).  Strips are staged through LDS with
 * coalesced 16-byte loads (csrc/edgedot.hip); `scratch` = ggl_bspmm_grad_w_sorted_scratch_bytes(...) bytes (0 -> may be
 * NULL): wide heads then run as launches over 64-column blocks that carry the running dot in it. */
size_t ggl_bspmm_grad_w_sorted_scratch_bytes(int64_t E, int64_t N, int64_t H, int64_t C);
int ggl_bspmm_grad_w_sorted(const ggl_segplan_t *plan, const int32_t *col, const int32_t *rowidx, const float *x,
                            const float *g, int64_t H, int64_t C, float *gw, float *scratch, void *stream);
/* gspmm's gradient with respect to its edge weights (an extension: gspmm.cpp:79 returns none), sum and mean; max has none
 * (its witnesses are source-node ids: with duplicate edges "the winner's weight" is ambiguous).  Along the destination-
 * sorted FORWARD plan, as above:
 *     gw[e] = sum_k x[src_e, k] * g'[dst_e, k]        k ascending, rounded multiply then rounded add, never contracted
 *   sum  (mean_rowptr == NULL): g' = g
 *   mean (mean_rowptr = the forward plan's rowptr): g'[r, :] = g[r, :] / count(r), count(r) = the row's edge count as f32
 *        and the division the rounded f32 one — (g / count) * w, ggl_spmm_mean_bwd's order.  It is made once per row,
 *        into an f32 [N_dst, K] panel in the scratch.
 * x [N_src, K] and g [N_dst, K] are each GGL_F32, GGL_BF16 or GGL_F16, independently (g is f32 under 16-bit rows when the
 * forward returned f32).  A 16-bit element is widened at the load (exact); products and adds are the f32 ones in the f32
 * order and gw [E] is f32, never rounded:  gw(x16, g16) == gw(widen(x16), widen(g16)), and for f32 x and g the sum form
 * == ggl_bspmm_grad_w_sorted(H = 1, C = K) (it runs those kernels), bit for bit, for every K.  gw is in the caller's edge
 * order (through plan->perm; NULL = already sorted).  16-bit operands take the LDS-staged kernel for K % 8 == 0 and
 * 16-byte aligned panels, f32 ones for K % 4 == 0; the rest, and the host build, walk one edge per thread.
 * scratch: ggl_spmm_grad_w_scratch_bytes(E, N_dst, K, x_dtype, mean != 0) bytes, 16-byte aligned (0 -> may be NULL): the
 * carried chain of launches over column blocks (options col_block / col_block16 by x's dtype, under the col_block_min_*
 * thresholds), then the mean panel. */
size_t ggl_spmm_grad_w_scratch_bytes(int64_t E, int64_t N_dst, int64_t K, int x_dtype, int mean);
int ggl_spmm_grad_w(const ggl_segplan_t *plan, const int32_t *col, const int32_t *rowidx, int x_dtype, const void *x,
                    int g_dtype, const void *g, const int64_t *mean_rowptr, int64_t K, float *gw, void *scratch,
                    void *stream);

/* ------------------------------------------------------------------------------------------------
 * Column sums of a row-major [N,K] f32 matrix: out[k] = sum_r g[r,k] — the gradient of the
 * "+ bias" that follows every aggregate (gcn_conv.py:105-106, sage_conv.py:102-103).  Two
 * deterministic stages (no atomics); needs ggl_colsum_workspace_bytes(N, K) bytes of scratch.
 * ---------------------------------------------------------------------------------------------- */
size_t ggl_colsum_workspace_bytes(int64_t N, int64_t K);
int ggl_colsum_f32(const float *g, int64_t N, int64_t K, float *out, void *workspace,
                   size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Fused epilogue of an aggregate: "+ bias" (gcn_conv.py:105-106), ReLU and
 * dropout (models/gcn.py:55-59) in one pass each way.
 *   fwd: y = keep * relu(a + bias) / (1 - p_drop); keep ~ Bernoulli(1 - p_drop) from Philox4x32-10 keyed
 *        on rng_state = {seed, offset} (device int64[2]; offset is advanced on the stream after the
 *        launch, so a captured graph draws a new mask per replay).  bias [K] or NULL; p_drop = 0: no RNG.
 *        The word of element (r, k): Philox(counter = r * (K / v) + k / v)[k % v], v = 4 if K % 4 == 0 else 1.
 *   bwd: ga = keep * [relu ? y > 0 : 1] * g / (1 - p_drop).  With ReLU the mask is read off y (y > 0: exact).
 *        Without ReLU `rng_used` = a copy of the {seed, offset} the forward READ (taken before it advanced)
 *        lets the dropout mask be redrawn exactly; rng_used == NULL: y != 0 stands in for it (exact except
 *        for kept activations that are exactly 0).  gbias[K] = column sums of ga (same pass; NULL to skip).
 * ---------------------------------------------------------------------------------------------- */
int ggl_bias_act_fwd(const float *a, const float *bias, int64_t N, int64_t K, int relu, float p_drop,
                     int64_t *rng_state, float *y, void *stream);
/* ggl_spmm_sum with that forward epilogue applied to every finished row before its only store:
 * out = dropout(relu(A x + bias)).  Identical (values and dropout mask) to ggl_spmm_sum followed by
 * ggl_bias_act_fwd on the same rng_state; the backward is ggl_bias_act_bwd(g, out) then the transposed
 * ggl_spmm_sum.  It is ggl_spmm_epi_ex (below) with contiguous rows, sum, no add, and forwards to it. */
int ggl_spmm_sum_bias_act(const ggl_segplan_t *plan, const int32_t *col, const float *w, int w_by_pos,
                          const float *x, int64_t K, const float *bias, int relu, float p_drop,
                          int64_t *rng_state, float *out, void *stream);
size_t ggl_bias_act_bwd_workspace_bytes(int64_t N, int64_t K);
int ggl_bias_act_bwd(const float *g, const float *y, int64_t N, int64_t K, int relu, float p_drop,
                     const int64_t *rng_used, float *ga, float *gbias, void *workspace,
                     size_t workspace_bytes, void *stream);
/* ggl_bias_act_bwd on a gradient that is a narrow product, s = g[N, J] . w[J, K], WITHOUT writing s: the backward of
 * dropout(relu(. + bias)) followed by a Linear whose weight is w (GCN: the last hidden layer's epilogue under the output
 * layer).  s[r, k] = sum_j g[r, j] * w[j, k], serial fused multiply-adds in ascending j from 0.0f (one rounding each;
 * NOT a BLAS summation order), formed in registers; (ga, gbias) are then ggl_bias_act_bwd(s, y, ...)'s bit for bit — the
 * same mask modes, geometry, partial sums and ggl_colsum_f32.  relu = 0, p_drop = 0, gbias = NULL returns s itself.
 * g rows have stride g_ld >= J (47 classes in rows of 48); w is the row-major [J, K] Linear weight, staged in LDS.
 * Shapes: K % 4 == 0, 1 <= J <= 64, J * K * 4 <= 64 KiB (else GGL_EINVAL); g, w, y, ga 16-byte aligned.
 * workspace: ggl_bias_act_bwd_workspace_bytes(N, K) (needed with gbias only).
 * ggl_policy_linear_epi_bwd: 1 = take this form for an [N, J] x [J, K] product (those shapes), 0 = GEMM, then
 * ggl_bias_act_bwd.  At K = 256, J = 47 the fused pass moves 5.5 GB where the two launches move 10.5 GB
 * (profiles/lin_epi_bwd.txt). */
int ggl_linear_bias_act_bwd(const float *g, int64_t g_ld, const float *w, const float *y, int64_t N, int64_t J, int64_t K,
                            int relu, float p_drop, const int64_t *rng_used, float *ga, float *gbias, void *workspace,
                            size_t workspace_bytes, void *stream);
int ggl_policy_linear_epi_bwd(int64_t N, int64_t J, int64_t K);
/* The bias gradient of ggl_bias_act_bwd(relu = 0, p_drop = 0) for a gradient that is zero outside the sorted rows[R] of
 * an [N, K] matrix, from the compact g[R, K] alone (K % 4 == 0, g 16-byte aligned): the same partial matrix — same
 * geometry, every listed row added into the slot and at the position its id gives it — reduced by the same
 * ggl_colsum_f32, so gbias[K] is the number the pass over the scattered [N, K] gradient gives (it only adds +0 rows
 * more).  workspace: ggl_bias_act_bwd_workspace_bytes(N, K). */
int ggl_bias_grad_rows(const float *g, const int64_t *rows, int64_t R, int64_t N, int64_t K, float *gbias,
                       void *workspace, size_t workspace_bytes, void *stream);
/* General form of the fused epilogue (sage_conv.py:100-108, gcn_conv.py:105-106):
 *   out[i, 0:K] = dropout(relu(reduce_{p in row i} w * x[col[p], 0:K] (+ out[i, 0:K] if accumulate)
 *                              + add[i, 0:K] + bias[0:K]))
 * reduce = sum, or mean (divide by the row's edge count; not with accumulate).  x / out / add rows are
 * x_ld / out_ld / add_ld elements apart (0 = K): a column block [epi_col0, epi_col0 + K) of an epi_K-wide
 * row (epi_K = 0: K), bias / add pointing at the block's first column, and the dropout word of element
 * (i, epi_col0 + k) is the one the full-width launch draws.  accumulate: a second edge set (halo-source
 * edges of the multi-GPU path) is added onto the partial result already in `out`, epilogue included.
 * advance_rng != 0 steps rng_state afterwards (once per layer: on the last column block). */
int ggl_spmm_epi_ex(const ggl_segplan_t *plan, const int32_t *col, const float *w, int w_by_pos,
                    const float *x, int64_t x_ld, int64_t K, float *out, int64_t out_ld, int accumulate,
                    int mean, const float *add, int64_t add_ld, const float *bias, int relu, float p_drop,
                    int64_t *rng_state, int64_t epi_K, int64_t epi_col0, int advance_rng, void *stream);
/* ggl_spmm_epi_ex on 16-bit rows (an extension, as ggl_spmm_*_x16): x and add are stored as GGL_BF16 or GGL_F16 (add has
 * x's dtype), w and bias stay f32.  The sum (or mean), + add, + bias, ReLU and the dropout scale are each the f32 operation
 * ggl_spmm_epi_ex makes, in its order, and the row is rounded ONCE, at the store (out_dtype == x_dtype), or not at all
 * (out_dtype == GGL_F32).  With F = ggl_spmm_epi_ex on the same plan, weights and rng state:
 *     out == round(F(widen(x), widen(add), bias, ...))  /  out == F(...)      bit for bit, the dropout mask included
 * (the word of element (i, k) is F's; epi_col0 a multiple of 4 keeps the 16-byte lanes), and rng_state moves as F moves it.
 * Any other dtype pair returns GGL_EDTYPE.  There is no accumulate: adding onto a rounded partial result would round twice.
 * Wide rows run as column blocks of option "col_block16" columns, bias / add / the mask following the block. */
int ggl_spmm_epi_x16(const ggl_segplan_t *plan, const int32_t *col, const float *w, int w_by_pos, int x_dtype, const void *x,
                     int64_t x_ld, int64_t K, int out_dtype, void *out, int64_t out_ld, int mean, const void *add,
                     int64_t add_ld, const float *bias, int relu, float p_drop, int64_t *rng_state, int64_t epi_K,
                     int64_t epi_col0, int advance_rng, void *stream);
/* ggl_bias_act_fwd / ggl_bias_act_bwd on 16-bit a / y / g / ga (dtype = GGL_BF16 or GGL_F16, else GGL_EDTYPE); bias, gbias
 * and the partials stay f32:
 *     y  == round(ggl_bias_act_fwd(widen(a), ...))            same words, same motion of rng_state
 *     ga == round(ggl_bias_act_bwd(widen(g), widen(y), ...))   gbias == that call's gbias, bit for bit (the column sums add
 *           the f32 values before they are rounded, in the f32 kernel's row-to-partial geometry)
 * The ReLU mask is read off the stored y > 0.  workspace: ggl_bias_act_bwd_workspace_bytes(N, K). */
int ggl_bias_act_fwd_x16(int dtype, const void *a, const float *bias, int64_t N, int64_t K, int relu, float p_drop,
                         int64_t *rng_state, void *y, void *stream);
int ggl_bias_act_bwd_x16(int dtype, const void *g, const void *y, int64_t N, int64_t K, int relu, float p_drop,
                         const int64_t *rng_used, void *ga, float *gbias, void *workspace, size_t workspace_bytes,
                         void *stream);
/* segment_sum / segment_mean of f32 messages x[E, K] with the same epilogue on each finished row (the
 * message() + aggregate() route of a sampled SAGEConv block): bit-identical to ggl_segment_{sum,mean}
 * followed by "+ add + bias, relu, dropout". */
int ggl_segment_epi(const float *x, const ggl_segplan_t *plan, int64_t K, int mean, const float *add,
                    int64_t add_ld, const float *bias, int relu, float p_drop, int64_t *rng_state, float *out,
                    void *stream);

/* ------------------------------------------------------------------------------------------------
 * Fused GAT edge-softmax + weighted aggregate: ONE kernel per direction.  Replaces the external
 * dgNN GATConvFuse that FusedGATConv calls (layers/conv/fusedgat_conv.py:70-71,121) and the
 * unfused chain in GATConv.forward (layers/conv/gat_conv.py:103-112 + utils/softmax.py:29-35):
 *   s[p,h]   = LeakyReLU_slope(el[col[p],h] + er[i,h])       for p in row i
 *   m[i,h]   = max_p s;  d[i,h] = sum_p exp(s - m)           (saved for backward)
 *   out[i,h,:] = sum_p exp(s[p,h]-m[i,h]) / (d[i,h] + 1e-16) * x[col[p],h,:]
 * el/er [N,H] f32 (source / destination attention terms), x [N_in,H,C] f32.
 * Rows longer than plan->chunk are reduced chunk-wise with chunk-local maxima and merged in chunk
 * order (online-softmax identity); short rows use the formula above verbatim.
 * Backward (edge-parallel, then source-major):
 *   ggl_gat_fused_bwd_dst: ONE walk of the forward plan (lane = head of a row / of a hub chunk):
 *       dot[i,h] = <g_i, out_i>; per (sorted position, head): alpha, de = alpha (<g_i, x_j> - dot)
 *       lrelu'(.) -> alpha[E,H], de[E,H] (forward sorted positions); ger[N,H] = row sums of de
 *   ggl_gat_fused_bwd_src: ONE walk of the transposed plan: gx[j,h,:] = sum_p alpha * g[dst,h,:] and
 *       gel[j,h] = sum_p de, reading alpha/de through posT (transposed position -> forward position);
 *       planT->partial: ggl_gat_bwd_src_partial_bytes(n_chunks, H, C) bytes, checked
 * ---------------------------------------------------------------------------------------------- */
/* p_drop > 0: attention dropout (gat_conv.py:104 `dropout(segment_softmax(.))`, GATConvFuse's last
 * argument): edge (sorted position p, head h) is kept when the 32-bit word mix(seed, offset, p * H + h)
 * (a counter-based multiply-xor mix with xxHash32's avalanche, gat.hip drop_word; ABI 4 — ABI 3 drew it from
 * Philox4x32-10, whose ten rounds per scattered position dominated the backward's source walks) is
 * >= p_drop * 2^32, and then weighs alpha / (1 - p_drop); the softmax itself runs over all edges.  rng_state = device int64 {seed, offset},
 * offset advanced after the launch; the backward needs the values the forward READ (rng_used). */
int ggl_gat_fused_fwd(const ggl_segplan_t *plan, const int32_t *col, const float *el,
                      const float *er, const float *x, float slope, int64_t H, int64_t C,
                      float p_drop, int64_t *rng_state, float *out, float *rowmax, float *rowden,
                      void *stream);
/* plan->partial of the forward walks when the plan has long rows (chunk-local softmax partials; checked): ggl_gat_fused_fwd[_x16],
 * ggl_edge_softmax_agg_fwd, ggl_dot_attn_fwd, ggl_gatv2_fwd, ggl_gat_fast_fwd */
size_t ggl_gat_partial_bytes(int64_t n_chunks, int64_t H, int64_t C);
/* ... of the destination walks ggl_gat_fused_bwd_dst[_x16] and ggl_edge_softmax_agg_bwd_dst (the ger partials of the hub chunks,
 * n_chunks * H floats), and of the source walks ggl_gat_fused_bwd_src[_x16], ggl_edge_softmax_agg_bwd_src and ggl_gat_fast_bwd's
 * planT (the gx and gel partials, n_chunks * (H*C + H) floats) */
size_t ggl_gat_bwd_dst_partial_bytes(int64_t n_chunks, int64_t H);
size_t ggl_gat_bwd_src_partial_bytes(int64_t n_chunks, int64_t H, int64_t C);
/* alpha / de: two [E,H] f32 arrays, or ONE interleaved [E,H,2] buffer passed as (base, base + 1) — then
 * an edge's alpha and de share a 64-byte line for the source-side walk (same convention in
 * ggl_gat_fused_bwd_src).  rowidx, dot_ws: unused since ABI 3 (may be NULL); plan->partial: ggl_gat_bwd_dst_partial_bytes(n_chunks,
 * H) bytes, checked */
int ggl_gat_fused_bwd_dst(const ggl_segplan_t *plan, const int32_t *col, const int32_t *rowidx,
                          const float *el, const float *er, const float *x, const float *g,
                          const float *out, const float *rowmax, const float *rowden, float slope,
                          int64_t H, int64_t C, float p_drop, const int64_t *rng_used, float *alpha,
                          float *de, float *ger, float *dot_ws, void *stream);
int ggl_gat_fused_bwd_src(const ggl_segplan_t *planT, const int32_t *colT, const int32_t *posT,
                          const float *alpha, const float *de, const float *g, int64_t H,
                          int64_t C, float *gx, float *gel, void *stream);
/* 16-bit STORAGE forms of the three walks above (an extension: the reference's GAT is f32 only; ABI still 11, the symbols are
 * purely additive).  x [N_src,H,C] is GGL_BF16 or GGL_F16 (x_dtype); out is x_dtype or GGL_F32 (a last layer's logits); g has
 * out's dtype (g_dtype == out_dtype) and `out` in the backward is the tensor the forward RETURNED (rounded, if it was rounded:
 * no f32 copy is kept); gx has x's dtype.  Any other dtype pair returns GGL_EDTYPE.  el, er, rowmax, rowden, alpha, de, gel, ger
 * and every hub-chunk partial stay f32: plan->partial is sized, and checked, as for the f32 entry points.  x, g and out are widened at the load (exact), every operation in between is the f32 one
 * of ggl_gat_fused_fwd / _bwd_dst / _bwd_src (call them F) in F's order, and out / gx are rounded ONCE, at the store:
 *   forward   out(x16)          == F.out(x16 as f32) rounded to x_dtype      bit for bit
 *             out(x16, GGL_F32) == F.out(x16 as f32)                         bit for bit
 *             rowmax, rowden    == F's                                       bit for bit
 *   backward  alpha, de, gel, ger == F_bwd(x16 as f32, g as f32, out as f32, rowmax, rowden)'s, gx == that gx rounded to x_dtype
 * (F is NOT ggl_gat_fast_*, which is held to a tolerance.)  The attention-dropout word depends on (position, head, seed, offset)
 * only, so with the same rng values the mask is F's.  A lane reads 16 bytes (8 channels) where C % 8 == 0 and the pointers
 * are 16-byte aligned, 8 bytes where C % 4 == 0 and they are 8-byte aligned, single elements otherwise (a panel that starts one
 * element into a buffer is fine); the bits do not depend on which. */
int ggl_gat_fused_fwd_x16(const ggl_segplan_t *plan, const int32_t *col, const float *el, const float *er, int x_dtype,
                          const void *x, float slope, int64_t H, int64_t C, float p_drop, int64_t *rng_state,
                          int out_dtype, void *out, float *rowmax, float *rowden, void *stream);
int ggl_gat_fused_bwd_dst_x16(const ggl_segplan_t *plan, const int32_t *col, const float *el, const float *er,
                              int x_dtype, const void *x, int g_dtype, const void *g, int out_dtype, const void *out,
                              const float *rowmax, const float *rowden, float slope, int64_t H, int64_t C, float p_drop,
                              const int64_t *rng_used, float *alpha, float *de, float *ger, void *stream);
int ggl_gat_fused_bwd_src_x16(const ggl_segplan_t *planT, const int32_t *colT, const int32_t *posT, const float *alpha,
                              const float *de, int g_dtype, const void *g, int64_t H, int64_t C, int gx_dtype, void *gx,
                              float *gel, void *stream);
/* Edge softmax + weighted aggregate on PER-EDGE logits (agnn_conv.py:54-66 and every layer that calls segment_softmax on its
 * [E, H] logits and sums alpha * x[src]): the three general GAT walks above with the logit read from z instead of built from
 * el / er.  f32 only.
 *   out[i,h,:] = sum_{p in row i} drop(softmax_i(z[:,h]))[p] * x[col[p],h,:],   s[p,h] = z[e_p,h],  e_p = perm ? perm[p] : p
 * z [E,H] is in the CALLER's edge order (plan->perm maps a sorted position to it; NULL for ids that arrived sorted) and is
 * used as it is: no activation.  Everything behind s is ggl_gat_fused_*'s code: -FLT_MAX start and strict <, one-walk online
 * softmax, out = acc / (den + 1e-16f), zeros for an empty row, hub chunks merged in chunk order, the same dropout word of
 * (sorted position, head, seed, offset).  So on z = LeakyReLU(el[src] + er[dst]) (computed in f32) out, rowmax, rowden, alpha
 * and gx are ggl_gat_fused_fwd / _bwd_dst / _bwd_src's bit for bit, and gz is their `de` in the caller's order.  A row
 * whose logits are all -inf gives zeros like an empty row (no -inf beats the -FLT_MAX start, every exp(-inf + FLT_MAX) is 0),
 * one that holds a NaN keeps the maximum of the others (NaN loses the strict <) and gets NaN sums: what the GAT kernels
 * give for the same s.
 *   ggl_edge_softmax_agg_fwd     : plan->partial: ggl_gat_partial_bytes(n_chunks, H, C) bytes, checked.
 *   ggl_edge_softmax_agg_bwd_dst : alpha[E,H] by SORTED POSITION (what _bwd_src reads through posT), gz[E,H] = alpha (keep/(1-p)
 *       <g_i, x_j> - <g_i, out_i>) by the CALLER's edge number, written by the walk itself.  alpha or gz may be NULL: that
 *       store is skipped (x resp. z needs no gradient).  plan->partial: ggl_gat_bwd_dst_partial_bytes(n_chunks, H) bytes, checked
 *       (the shared preamble asks for it; there is no row sum to keep in it).
 *   ggl_edge_softmax_agg_bwd_src : gx[j,h,:] = sum_q alpha[posT[q],h] * g[colT[q],h,:]; planT->partial:
 *       ggl_gat_bwd_src_partial_bytes(n_chunks, H, C) bytes, checked. */
int ggl_edge_softmax_agg_fwd(const ggl_segplan_t *plan, const int32_t *col, const float *z, const float *x, int64_t H,
                             int64_t C, float p_drop, int64_t *rng_state, float *out, float *rowmax, float *rowden,
                             void *stream);
int ggl_edge_softmax_agg_bwd_dst(const ggl_segplan_t *plan, const int32_t *col, const float *z, const float *x,
                                 const float *g, const float *out, const float *rowmax, const float *rowden, int64_t H,
                                 int64_t C, float p_drop, const int64_t *rng_used, float *alpha, float *gz, void *stream);
int ggl_edge_softmax_agg_bwd_src(const ggl_segplan_t *planT, const int32_t *colT, const int32_t *posT, const float *alpha,
                                 const float *g, int64_t H, int64_t C, float *gx, void *stream);
/* Scaled dot-product graph attention, forward (hgt_conv.py:115-153 and every graph-transformer layer), f32, GPU build only
 * (csrc/dotattn.hip; the host build answers supported = 0 and fails the launch):
 *   z[e,h]     = scale * <q[dst(e),h,:], k[src(e),h,:]>            q [N_dst,H,C], k, v [N_src,H,C]
 *   out[i,h,:] = sum_{p in row i} drop(softmax_i(z[:,h]))[p] * v[col[p],h,:]
 * in ONE walk of the destination-sorted plan: the g = C / 4 lanes of a head multiply their four channels (ascending) and add
 * the partial sums with a butterfly of wave shuffles, which leaves the same bits in every lane; everything behind z is
 * ggl_edge_softmax_agg_fwd's code.  Hence the contract: with z_out != NULL the logits the walk used are stored, [E,H] in the
 * CALLER's edge order (through plan->perm), and out / rowmax / rowden are ggl_edge_softmax_agg_fwd(plan, col, z_out, v, ...)'s
 * bit for bit — hub chunks and dropout with the same rng_state included; with z_out == NULL out has the same bits and no
 * [E,H] array is touched.  z itself is within gamma_{C+1} |scale| sum_c |q_c k_c| of the exact value (gamma_n = n u / (1 - n u),
 * u = 2^-24); it does not have the bits of ggl_bspmm_grad_w*, which adds the C products serially.  The backward is composed
 * by the caller from ggl_edge_softmax_agg_bwd_dst / _bwd_src on z_out and two ggl_bspmm_sum walks with gz * scale.
 * q, k, v, out and plan->partial must be 16-byte aligned; plan->partial: ggl_gat_partial_bytes(n_chunks, H, C) bytes, checked;
 * rng_state as ggl_gat_fused_fwd.
 *   ggl_dot_attn_supported(H, C)           : 1 for C = 8, 16, 32, 64 and any H > 0.
 *   ggl_policy_dot_attn_fused(H, C, E, N_in): 1 where the fused forward is the default over edge dot + ggl_edge_softmax_agg_fwd
 *       (profiles/dot_attention.txt); never 1 for an unsupported shape. */
int ggl_dot_attn_supported(int64_t H, int64_t C);
int ggl_policy_dot_attn_fused(int64_t H, int64_t C, int64_t E, int64_t N_in);
int ggl_dot_attn_fwd(const ggl_segplan_t *plan, const int32_t *col, const float *q, const float *k, const float *v,
                     float scale, int64_t H, int64_t C, float p_drop, int64_t *rng_state, float *out, float *rowmax,
                     float *rowden, float *z_out, void *stream);
/* GATv2 (additive) graph attention, f32:
 *   z[e,h]     = sum_c att[h,c] * LeakyReLU(xl[src(e),h,c] + xr[dst(e),h,c])     xl [N_src,H,C], xr [N_dst,H,C], att [H,C]
 *   out[i,h,:] = sum_{p in row i} drop(softmax_i(z[:,h]))[p] * xl[col[p],h,:]
 * ggl_gatv2_fwd (csrc/gatv2.hip, GPU build only; the host build answers supported = 0 and fails the launch): ONE walk of the
 * destination-sorted plan.  The g = C / 4 lanes of a head form __fmul_rn(att, lrelu(__fadd_rn(xl, xr))) for their four channels
 * from the value row the walk gathers anyway, add them ascending from 0.0f and finish with ggl_dot_attn_fwd's butterfly;
 * everything behind z is ggl_edge_softmax_agg_fwd's code.  Hence the contract of ggl_dot_attn_fwd: with z_out != NULL the
 * logits are stored, [E,H] in the CALLER's edge order (through plan->perm), and out / rowmax / rowden are
 * ggl_edge_softmax_agg_fwd(plan, col, z_out, xl, ...)'s bit for bit; with z_out == NULL out has the same bits and no [E,H]
 * array is touched.  z is within gamma_{C+2} sum_c |att_c| |lrelu(xl_c + xr_c)| of the exact value (gamma_n = n u / (1 - n u),
 * u = 2^-24).  xl, xr, att, out and plan->partial must be 16-byte aligned; plan->partial: ggl_gat_partial_bytes(n_chunks, H, C)
 * bytes, checked; rng_state as ggl_gat_fused_fwd.
 *   ggl_gatv2_supported(H, C)            : 1 for C = 8, 16, 32, 64 and any H > 0.
 *   ggl_policy_gatv2_fused(H, C, E, N_in): 1 where the fused forward is the default over logits composed in front of
 *       ggl_edge_softmax_agg_fwd (profiles/gatv2_attention.txt); never 1 for an unsupported shape.
 * The backward runs ggl_edge_softmax_agg_bwd_dst / _bwd_src on z (alpha, gz, the value part gv of xl's gradient) and then
 * ggl_gatv2_logit_bwd (csrc/gatv2_bwd.hpp, every build), which carries LeakyReLU's derivative inside the channel dimension.
 * For row r of the plan it is given, head h, channel c, positions p ascending, e_p = plan->perm ? plan->perm[p] : p:
 *   s = __fadd_rn(other[col[p],h,c], self[r,h,c]);  w = gz[e_p,h]
 *   accD = __fadd_rn(accD, s > 0 ? w : __fmul_rn(w, slope))
 *   accA = __fadd_rn(accA, __fmul_rn(w, s > 0 ? s : __fmul_rn(s, slope)))              (only with att_rows != NULL)
 *   g_self[r,h,c] = add ? __fadd_rn(add[r,h,c], __fmul_rn(att[h,c], accD)) : __fmul_rn(att[h,c], accD);  att_rows[r,h,c] = accA
 * Rows longer than plan->chunk are walked in pieces of chunk positions, each summed from 0.0f, and merged in ascending chunk
 * order from 0.0f before the att multiply and the add; plan->partial: ggl_gatv2_logit_bwd_partial_bytes(n_chunks, H, C,
 * att_rows != NULL) bytes, checked.  Forward plan (col, self = xr, other = xl, att_rows = R): g_xr, and
 * g_att = column sums of R.  Transposed plan (colT, perm = the caller's edge number of every position, self = xl,
 * other = xr, add = gv): the whole g_xl. */
int ggl_gatv2_supported(int64_t H, int64_t C);
int ggl_policy_gatv2_fused(int64_t H, int64_t C, int64_t E, int64_t N_in);
int ggl_gatv2_fwd(const ggl_segplan_t *plan, const int32_t *col, const float *xl, const float *xr, const float *att,
                  float slope, int64_t H, int64_t C, float p_drop, int64_t *rng_state, float *out, float *rowmax,
                  float *rowden, float *z_out, void *stream);
size_t ggl_gatv2_logit_bwd_partial_bytes(int64_t n_chunks, int64_t H, int64_t C, int with_att_rows);
int ggl_gatv2_logit_bwd(const ggl_segplan_t *plan, const int32_t *col, const float *other, const float *self,
                        const float *gz, const float *att, float slope, int64_t H, int64_t C, const float *add,
                        float *g_self, float *att_rows, void *stream);
/* Several statistics of the same message rows in ONE walk of the plan (csrc/multiagg.hpp, every build; f32): what PNA's
 * aggregate composes from four to five segment ops and an [E, K] tensor of squares (pna_conv.py:159-201).
 *   aggs : n_aggs (1..6) DISTINCT codes of the enum below, in output order (host memory).  C divides K.
 *   out  : [N, K / C, A, C] contiguous, A = n_aggs: column k of statistic number a at (k / C) * A * C + a * C + k % C — C = K is
 *          cat(outs, -1), x [E, T, F] with C = F the per-tower concatenation [N, T, A * F].
 * Per row i with n elements and per column, positions ascending (e = perm ? perm[p] : p, v = x[e, k]), every step one rounded
 * f32 operation:
 *   S = __fadd_rn(S, v) from 0.0f;  Q = __fadd_rn(Q, __fmul_rn(v, v)) from 0.0f
 *   max: from -FLT_MAX, `if (mx < v) { mx = v; argmax = e; }`;  min: from +FLT_MAX, `if (v < mn) { mn = v; argmin = e; }`
 *   nf = (float)min(n, 2^24);  mean = n > 1 ? __fdiv_rn(S, nf) : S;  msq = n > 1 ? __fdiv_rn(Q, nf) : Q   (ggl_segment_mean's rule)
 *   var = __fsub_rn(msq, __fmul_rn(mean, mean));  std = sqrtf(__fadd_rn(fmaxf(var, 0.0f), 1e-5f)), correctly rounded
 * Empty rows: sum = mean = var = 0, std = sqrt(1e-5f), min / max +-FLT_MAX (0.0f with empty_zero != 0), witnesses E.
 * mean [N, K] (optional; needs one of sum / mean / var / std among the aggs) and the witnesses argmin / argmax [N, K] int32
 * (optional; the element index in the caller's order) are written when their pointer is given.
 * Rows longer than plan->chunk are cut into pieces of chunk positions, each reduced from the start values into a partial
 * (S, Q, mn, mx, amin, amax: only the panels the aggs need, [n_chunks, K] each, in that order); the partials are merged in
 * ascending piece order, sums from 0.0f, min / max with the strict rule.  plan->partial:
 * ggl_segment_multi_partial_bytes(n_chunks, K, aggs, n_aggs) bytes, checked (GGL_EWORKSPACE).
 * Backward: g [N, A * K] in out's layout; gx [E, K], every element written.  Per (row, column), n' = max(n, 1),
 * nf = (float)min(n', 2^24), s0 = sqrtf(1e-5f):
 *   gv = g_var (0.0f without var);  with std: t = std > s0 ? __fdiv_rn(g_std, __fmul_rn(2.0f, std)) : 0.0f,
 *        gv = var requested ? __fadd_rn(gv, t) : t             ("var > 0" re-derived from the stored std: var is not stored)
 *   c1 = __fdiv_rn(__fmul_rn(2.0f, gv), nf)
 *   c0 = 0.0f; sum: c0 = __fadd_rn(c0, g_sum); mean: c0 = __fadd_rn(c0, __fdiv_rn(g_mean, nf));
 *        var or std: c0 = __fsub_rn(c0, __fmul_rn(c1, mean))
 * and per position: t = var or std ? __fadd_rn(c0, __fmul_rn(c1, x[e, k])) : c0; if (argmax == e) t = __fadd_rn(t, g_max);
 * if (argmin == e) t = __fadd_rn(t, g_min); gx[e, k] = t.  x and mean are read only with var / std, out only with std, the
 * witnesses only with min / max: the other pointers may be NULL.  No partial buffer.
 * Refused with GGL_EINVAL: C not dividing K, duplicate or unknown codes, a missing pointer the aggs require (named in the
 * message), a plan with long rows and no plan->partial (forward). */
enum { GGL_AGG_SUM = 0, GGL_AGG_MEAN = 1, GGL_AGG_MIN = 2, GGL_AGG_MAX = 3, GGL_AGG_VAR = 4, GGL_AGG_STD = 5 };
size_t ggl_segment_multi_partial_bytes(int64_t n_chunks, int64_t K, const int *aggs_host, int n_aggs);
int ggl_segment_multi_fwd(const float *x, const ggl_segplan_t *plan, int64_t K, int64_t C, const int *aggs_host, int n_aggs,
                          int empty_zero, float *out, float *mean_or_null, int32_t *argmin_or_null, int32_t *argmax_or_null,
                          void *stream);
int ggl_segment_multi_bwd(const float *g, const float *x_or_null, const float *out_or_null, const float *mean_or_null,
                          const int32_t *argmin_or_null, const int32_t *argmax_or_null, const ggl_segplan_t *plan, int64_t K,
                          int64_t C, const int *aggs_host, int n_aggs, float *gx, void *stream);
/* Fast path of the same op for heads of C = 4, 8, 16, 32 or 64 channels with H * C <= 256
 * (ggl_gat_fast_supported; e.g. the Reddit GAT's 8 x 8): same walks with ~5x fewer vector-ALU instructions
 * (v_exp_f32, one rescale per 4-8 edges, 16-byte index loads, 32-bit panel offsets, FMA) and a backward that
 * RECOMPUTES alpha / de in both walks from per-row constants instead of writing them to [E, H, 2] and
 * gathering them back through posT (cross-lane dot products: results within the 1e-5 / 1e-4 relative
 * parity bar of the GAT op, not bit-identical to the kernels above).
 *   ggl_gat_fast_fwd : as ggl_gat_fused_fwd; N_src = rows of x (selects 32-bit offsets when the panel is < 4 GiB)
 *   ggl_gat_fast_bwd : destination walk (stats[N,H,4] = {er, m, 1/(den + 1e-16), <g_i, out_i>}, ger) then
 *                      source walk (gx, gel).  stats: workspace of N * H * 4 floats; plan->partial:
 *                      ggl_gat_fast_bwd_dst_partial_bytes(n_chunks, H) bytes, 8-byte aligned (four double sums per chunk and
 *                      head since ABI 8); planT->partial: ggl_gat_bwd_src_partial_bytes(n_chunksT, H, C); both checked;
 *                      posT is only read with p_drop > 0 (the keep bit lives at the forward position). */
int ggl_gat_fast_supported(int64_t H, int64_t C);
size_t ggl_gat_fast_bwd_dst_partial_bytes(int64_t n_chunks, int64_t H);
int ggl_gat_fast_fwd(const ggl_segplan_t *plan, const int32_t *col, const float *el, const float *er,
                     const float *x, int64_t N_src, float slope, int64_t H, int64_t C, float p_drop,
                     int64_t *rng_state, float *out, float *rowmax, float *rowden, void *stream);
int ggl_gat_fast_bwd(const ggl_segplan_t *plan, const int32_t *col, const ggl_segplan_t *planT,
                     const int32_t *colT, const int32_t *posT, const float *el, const float *er,
                     const float *x, const float *g, const float *out, const float *rowmax,
                     const float *rowden, float slope, int64_t H, int64_t C, float p_drop,
                     const int64_t *rng_used, float *stats, float *gx, float *gel, float *ger, void *stream);
/* Head-mean GAT layer aggregated BEFORE it is transformed (the output layer of models/gat.py: concat=False,
 * gat_conv.py:114-122): y_i = 1/H sum_h (sum_j alpha_ijh x_j) W_h, so the per-edge gather is the F-float INPUT row
 * shared by all heads instead of the H x C transformed row (Reddit GAT: 256 B instead of 1408 B), and in the
 * backward the source walk gathers the C-float output gradient g_i (dL/dA_ih = g_i W_h^T / H).  H = 8, F and the
 * padded class width Cp <= 64 (multiples of 4): ggl_gat_sh_supported.  GPU build only (DPP row broadcasts and a
 * 16-lane reduce-scatter); parity bar as for the fused GAT op (1e-5 / 1e-4 relative).
 *   ggl_gat_sh_fwd : rowmax[N,8], A[N,8,F] = sum_j alpha_ijh x_j, den[N,8]; plan->partial:
 *                    ggl_gat_sh_partial_bytes(n_chunks, F) bytes, checked
 *   ggl_gat_sh_bwd : ger[N,8] (destination walk: G[N,8,F] = dL/dA and stats[N,8,4] = {er, m, 1/(den+1e-16),
 *                    <G_ih, A_ih>} per row, x gathered) and T[N_src,8,Cp] = sum_i alpha_ijh gy_i, gel[N_src,8]
 *                    (source walk: z[N_src,8,Cp] = the rows' own x_j W_h, gy[N,Cp] gathered); plan->partial:
 *                    ggl_gat_sh_bwd_dst_partial_bytes(n_chunks) bytes (four double row sums per chunk and head since ABI 9),
 *                    planT->partial: ggl_gat_sh_bwd_src_partial_bytes(n_chunksT, Cp) bytes; both checked */
int ggl_gat_sh_supported(int64_t H, int64_t F, int64_t C);
size_t ggl_gat_sh_partial_bytes(int64_t n_chunks, int64_t F);
size_t ggl_gat_sh_bwd_dst_partial_bytes(int64_t n_chunks);
size_t ggl_gat_sh_bwd_src_partial_bytes(int64_t n_chunks, int64_t Cp);
int ggl_gat_sh_fwd(const ggl_segplan_t *plan, const int32_t *col, const float *el, const float *er, const float *x,
                   int64_t F, float slope, float p_drop, int64_t *rng_state, float *rowmax, float *A, float *den,
                   void *stream);
int ggl_gat_sh_bwd(const ggl_segplan_t *plan, const int32_t *col, const ggl_segplan_t *planT, const int32_t *colT,
                   const int32_t *posT, const float *el, const float *x, int64_t F, const float *G,
                   const float *stats, const float *z, const float *gy, int64_t Cp, float slope, float p_drop,
                   const int64_t *rng_used, float *ger, float *T, float *gel, void *stream);
/* (ABI 8) the stats panel ggl_gat_sh_bwd reads, in one pass: stats[i,h,:] = {er, rowmax, 1 / (den + 1e-16), <G[i,h,:], A[i,h,:]>};
 * er / rowmax / den [N,8], G / A [N,8,F] (F % 4 == 0, 16-byte aligned), stats [N,8,4] */
int ggl_gat_sh_stats(const float *er, const float *rowmax, const float *den, const float *G, const float *A, int64_t N,
                     int64_t F, float *stats, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Edge softmax — supersedes the composition gammagl/utils/softmax.py:29-35 runs on the segment ops
 * (segment_max -> gather -> sub / exp -> segment_sum -> gather -> add / div, and the same chain backwards under
 * autograd) for the [E, H] logits of every attention layer.  f32; K = product of the trailing dims; x, y, g, gx are
 * [E, K] in the CALLER's element order (the kernels go through plan->perm); nothing [N, K] is returned or saved.
 *   fwd, per segment s and column k:  m = max x (start value -FLT_MAX, strict <, NaN never wins: segment_max_cpu.cpp:40-62),
 *        D = sum exp(x[e] - m) accumulated in DOUBLE and rounded to f32 once,  y[e] = exp(x[e] - m) / (D + 1e-16f).
 *        An all -inf column gives y = 0; empty segments write nothing; E == 0 is a no-op.
 *   bwd, from y and g alone:  S = sum y[e] g[e] in DOUBLE,  gx[e] = y[e] * f32(g[e] - S)  (the difference formed in
 *        double), except for the element with the largest y of its (segment, column) (smallest element index among
 *        equals): gx = -(sum of the other elements' gx, in double), so that a row's gradients sum to 0 as they do in
 *        exact arithmetic.  Without it a row dominated by one logit loses its gradient to the cancellation in g - S.
 * No atomics, no host synchronisation, every element of y / gx written exactly once.  Rows longer than plan->chunk go
 * through the long-row table: chunk-local (m, D) — resp. (S, winner) — in plan->partial
 * (ggl_segment_softmax_partial_bytes(n_chunks, K) bytes, checked; 8-byte aligned), merged in chunk order.  A plan presented
 * WITHOUT its long-row table (n_long == 0) has every row walked in one piece.
 * ggl_segment_softmax_supported(K): 1 <= K <= 64 (one or more lanes per (row, column)); wider rows are the caller's to compose.
 * ---------------------------------------------------------------------------------------------- */
int ggl_segment_softmax_supported(int64_t K);
size_t ggl_segment_softmax_partial_bytes(int64_t n_chunks, int64_t K);
int ggl_segment_softmax_fwd(const float *x, const ggl_segplan_t *plan, int64_t K, float *y, void *stream);
int ggl_segment_softmax_bwd(const float *y, const float *g, const ggl_segplan_t *plan, int64_t K, float *gx,
                            void *stream);

/* ------------------------------------------------------------------------------------------------
 * Uniform neighbour sampling — supersedes ops/sparse sample_adj
 * (cpu/sample.cpp:10-135).  CSR (rowptr [M+1], col [nnz]) int64; seeds [B] int64 row ids.
 *   ggl_sample_count: out_deg[i] = deg (fanout < 0) | fanout if deg > 0 (replace) | min(deg, fanout)
 *   ggl_sample_pick : given out_rowptr = exclusive prefix of out_deg, writes for every seed its sampled
 *                     positions e_pos (indices into col) and neighbours nbr = col[e_pos]; distinct
 *                     positions by Floyd's algorithm when !replace (sample.cpp:75-83); Philox4x32-10 on
 *                     rng_state = {seed, offset} (device int64[2], offset advanced after the launch).
 * ---------------------------------------------------------------------------------------------- */
int ggl_sample_count(const int64_t *rowptr, const int64_t *seeds, int64_t B, int64_t num_nodes, int64_t fanout, int replace,
                     int64_t *out_deg, void *stream);
int ggl_sample_pick(const int64_t *rowptr, const int64_t *col, const int64_t *seeds, int64_t B,
                    int64_t fanout, int replace, const int64_t *out_rowptr, int64_t *rng_state,
                    int64_t *e_pos, int64_t *nbr, void *stream);
/* One hop with DEVICE-side sizes and fixed capacities — nothing is read back, so a whole mini-batch step
 * (sampling, feature gather, layers, loss, backward, optimizer) captures into one hipGraph.
 *   seeds[B_cap] of which the first *n_seeds_dev are valid; fanout > 0 (min(deg, fanout) distinct neighbours per
 *   seed, Floyd's algorithm as sample.cpp:75-83); first_pos: int64 scratch of one entry per graph node, every
 *   entry == 2^62 on entry and again on exit.
 *   Capacities: E_cap <= B_cap * fanout edge slots, S_cap in [B_cap, B_cap + E_cap] node slots (the worst
 *   case is rarely met: a caller sizes them from measured batches and checks the overflow flag).
 *   out_rowptr[B_cap + 1] (rows past the valid seeds are empty), out_col[E_cap] int32 LOCAL ids, each row
 *   ascending (sample.cpp:112-118), out_eid[E_cap] CSR positions of the sampled edges (or NULL),
 *   out_nid[S_cap]: the seeds verbatim, then the new nodes in first-seen order (sample.cpp:24-55), zero-padded;
 *   out_counts[3] = {nodes in out_nid, sampled edges, overflow} (device): overflow = 1 when a capacity was
 *   hit (rows cut at E_cap / nodes past S_cap dropped — memory-safe, but the block is incomplete). */
size_t ggl_sample_hop_workspace_bytes(int64_t B_cap, int64_t E_cap);
int ggl_sample_hop(const int64_t *rowptr, const int64_t *col, const int64_t *seeds, const int64_t *n_seeds_dev,
                   int64_t B_cap, int64_t num_nodes, int64_t fanout, int64_t E_cap, int64_t S_cap, int64_t *rng_state,
                   int64_t *first_pos, int64_t *out_rowptr, int32_t *out_col, int64_t *out_eid, int64_t *out_nid,
                   int64_t *out_counts, void *workspace, size_t workspace_bytes, void *stream);
/* (ABI 8) the same hop; overflow_total (device, or NULL): += 1 when this hop hit a capacity — the caller's running count
 * of truncated hops, kept by the hop's own kernels instead of a host-side add per hop */
int ggl_sample_hop_ex(const int64_t *rowptr, const int64_t *col, const int64_t *seeds, const int64_t *n_seeds_dev,
                      int64_t B_cap, int64_t num_nodes, int64_t fanout, int64_t E_cap, int64_t S_cap, int64_t *rng_state,
                      int64_t *first_pos, int64_t *out_rowptr, int32_t *out_col, int64_t *out_eid, int64_t *out_nid,
                      int64_t *out_counts, void *workspace, size_t workspace_bytes, int64_t *overflow_total, void *stream);
/* CSC of such a block without a host read: rowptrT[N_src_cap + 1], dstT[E_cap] = destination rows of each source
 * row's block edges (ascending); E_cap entries of col of which rowptr[N_dst] are valid. */
size_t ggl_block_transpose_workspace_bytes(int64_t E_cap, int64_t N_src_cap);
int ggl_block_transpose(const int64_t *rowptr, const int32_t *col, int64_t N_dst, int64_t N_src_cap, int64_t E_cap,
                        int64_t *rowptrT, int32_t *dstT, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Tuning knobs (process-wide; each is also read once from the environment, as GGL_ + its upper-cased name: GGL_UNROLL,
 * GGL_ROW_ORDER, ...).  One table (GGL_OPTIONS, csrc/common.hpp) declares them all.  An unknown name: set answers
 * GGL_EINVAL ("unknown option <name>"), get answers -1.  ggl_option_name(i) enumerates the names, NULL past the end.
 * ---------------------------------------------------------------------------------------------- */
int ggl_set_option(const char *name, int64_t value);
int64_t ggl_get_option(const char *name);
const char *ggl_option_name(int i);

/* ------------------------------------------------------------------------------------------------
 * Host policy, ONE copy (round 4).  Two hosts drive these kernels — gammagl_amd/ops.py (ctypes) and
 * gammagl_amd/csrc/torch/ggl_torch.cpp (TORCH_LIBRARY) — and both must take the same launch decisions (they are checked
 * against each other bit for bit).  The decisions live here, measured constants and their reasons included; the hosts
 * only ask.  Pure host functions, no device access.
 * ---------------------------------------------------------------------------------------------- */
/* long-row threshold (= elements per chunk) of a plan of E elements: the largest power of two <= E / (256 CUs x 32
 * resident wavefronts), clamped to [256, 4096] — one wavefront walks a row serially, so on a small graph a 4096-element
 * walk is the whole launch (arxiv-sized K = 256 SpMM: 0.685 ms at 4096, 0.284 ms at 256).  GGL_LONG_ROW overrides. */
int64_t ggl_policy_chunk(int64_t E);
/* width a 2-D f32 matrix [N_in, K] is zero-padded to before an SpMM over E edges (== K: as it is).  reduce: 0 = sum /
 * mean, 1 = max.  sum / mean: K > 256 not a multiple of 64 -> next multiple of 64 (whole cache lines per 64-column
 * block: products-sized K = 602 55 -> 42 ms); K % 4 != 0, K >= 8 -> next multiple of 4 (16-byte rows: K = 47 9.3 -> 5.8 ms);
 * max: K > 128 with K % 4 != 0 -> next multiple of 4 (K = 602 69 -> 60 ms).  Only where the copy is paid back:
 * E >= 8 N_in. */
int64_t ggl_policy_spmm_width(int reduce, int64_t K, int64_t E, int64_t N_in);
/* channels per head a [N_in, H, C] tensor is zero-padded to for bspmm / the fused GAT (41 classes -> 44) */
int64_t ggl_policy_head_channels(int64_t C, int64_t E, int64_t N_in);
/* 1: the spmm-mean backward divides the rows of g by their count ONCE and runs the plain transposed SpMM-sum (same
 * bits; products-sized K = 256 23.0 -> 15.5 ms) — where a row has edges to amortise the pass over g: E >= 4 N_in */
int ggl_policy_mean_bwd_prescale(int64_t E, int64_t N_in);
/* form of the gspmm(max) backward over E edges into [N_dst, K] witnesses: 2 = 1-bit winner mask (ggl_spmm_max_mask +
 * ggl_spmm_max_bwd_mask; a transient of ggl_spmm_max_mask_bytes(E, K)), 1 = int32 witness copy (ggl_spmm_max_bwd32),
 * 0 = int64 witnesses (ggl_spmm_max_bwd).  The mask for option maxbwd_mask (128) <= K <= option maxbwd_mask_kmax (256):
 * measured faster on the products- AND the Reddit-sized graph up to K = 256, slower and 96 B per edge at K = 602
 * (profiles/r6_maxbwd_forms.txt).  Hosts also fall back to 1 when the mask cannot be allocated. */
int ggl_policy_maxbwd_form(int64_t E, int64_t N_dst, int64_t K);
/* 1: the bspmm weight gradient walks the destination-sorted plan with LDS-staged strips (edgedot.hip); 0: one thread
 * per (edge, head) in COO order — channel counts that are not multiples of 4, and heads of <= 16 channels unless they
 * are 12 / 16 wide in a row of >= 256 columns (measured on the products-sized graph, forward + backward: 16 x 16
 * 63.7 vs 67.5 ms; 32 x 8 the other way, 82.4 vs 67.0; 8 x 8 equal).  Takes (H, C) since ABI 7. */
int ggl_policy_gradw_sorted(int64_t H, int64_t C);
/* rows per XCD run of a plan (0: round-robin blocks) given the share of its edges whose endpoints lie within N / 64 ids
 * of each other: 2048 for E >= 2^22 and locality > 0.5 (planted-community graph in cluster order: K = 256 13.4 ->
 * 10.8 ms; R-MAT orders lose 7-8 % with it).  GGL_XCD_RUN_ROWS overrides. */
int64_t ggl_policy_xcd_run_rows(int64_t E, double locality);
/* the row hand-out order: rows of >= *heavy elements first, longest first; the rest by length inside windows of
 * *window consecutive ids (0: one global sort).  GGL_ROW_ORDER_WINDOW overrides the window. */
int ggl_policy_row_order(int64_t *window_host, int64_t *heavy_host);
/* lanes of the GPU build that share one (row, column) of the edge-softmax walks (a power of two, lanes x K <= 64) for rows of K
 * columns, E elements in N segments.  1 = a lane walks its row alone: the default (the measured form, profiles/segment_softmax.txt),
 * the only form for widths that are not a power of two and on the host build.  Option softmax_sublanes > 0 asks for more (A/B;
 * same formulas, double sums in another association). */
int64_t ggl_policy_softmax_sublanes(int64_t K, int64_t E, int64_t N);

/* Measurement aid (bench.py's roofline leg): a grid-stride pass over `n_vec4` 16-byte vectors of `src`, 16 bytes per
 * lane and four independent loads in flight — mode 0: read-only (every wavefront folds what it read into ONE float of
 * `dst`, which must hold at least 65536 floats), mode 1: copy to `dst`.  The rate it reaches is "what a streaming kernel
 * achieves on this part" next to the 8 TB/s spec peak; no reference counterpart. */
int ggl_calib_stream(const float *src, float *dst, int64_t n_vec4, int mode, void *stream);

/* Profiling aid: run `reps` launches of the dominant SpMM-sum kernel bracketed by hipEvents on
 * `stream` and return the average milliseconds per launch in *ms_host (SYNCHRONOUS). */
int ggl_time_spmm_sum(const ggl_segplan_t *plan, const int32_t *col, const float *w, int w_by_pos,
                      const float *x, int64_t K, float *out, void *stream, int reps,
                      float *ms_host);

#ifdef __cplusplus
}
#endif
#endif /* GGL_MPOPS_H */
