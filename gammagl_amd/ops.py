"""Host side of the MI355X message-passing backend: the ``Engine`` — the ops over the C ABI (include/ggl_mpops.h), their
argument checks, plan builders and plan caches.  PyTorch is plumbing here (device memory, streams, autograd graph).

The plans it builds and caches (``SegPlan``, ``GraphPlan``, ``RowsPlan``) live in ``plans.py``, the autograd formulas its
methods apply in ``autograd.py``, the dtype codes and the ctypes binding in ``_lib.py``.

``Engine`` takes the ctypes library as a constructor argument; the product singleton
(``gammagl_amd.engine()``) is always built on the HIP library and refuses non-GPU tensors.
"""
import ctypes
import math
import os

import torch
from torch.multiprocessing.reductions import StorageWeakRef

from . import _lib, autograd
from ._lib import _DTYPE_CODE, _FLOAT_DTYPES, _X16_DTYPES, _ptr
from .plans import GraphPlan, RowsPlan, SegPlan, _PlanCache

DEFAULT_CHUNK = int(os.environ.get("GGL_LONG_ROW", "0"))  # 0 = automatic, see Engine.auto_chunk


def sqrt_rn(t):
    """The correctly rounded square root of an f32 tensor (taken in float64 and rounded once: 53 >= 2 * 24 + 2 bits make the
    double rounding exact), as the kernels' sqrt is.  torch.sqrt's vectorised CPU kernel is one ulp off for about 0.6 % of its
    inputs, which would make the composed statistics differ from the fused walk's in the last bit.  Node-sized tensors only."""
    return torch.sqrt(t.double()).to(t.dtype) if t.dtype == torch.float32 else torch.sqrt(t)


class Engine:
    def __init__(self, lib, require_cuda=True, cpu_only=False):
        self.lib = lib
        self.require_cuda = require_cuda
        self.is_product = False       # set by gammagl_amd.engine() / host_engine(): bound to the shipped library (dist._default_route)
        self.cpu_only = cpu_only      # the host build: its kernels dereference host pointers
        self.seg_cache = _PlanCache()
        self.graph_cache = _PlanCache()
        self.w_cache = _PlanCache(cap=8)
        self.rows_cache = _PlanCache(cap=8)   # restricted plan pairs (rows_plan), keyed on the row list
        self._rng = {}
        self.stats = {"plans_built": 0, "plan_hits": 0}
        self.chunk = DEFAULT_CHUNK  # long-row threshold == elements per chunk; 0 = auto_chunk(E)
        self.gat_fast = True        # fused GAT: the low-VALU kernels where the head shape allows (GPU build only)
        self.hub16 = True           # f16 / bf16 sums: LDS-pipelined hub rows (GPU build only; A/B switch)
        self.hub16_overlap = True   # ... launched on a side stream beside the walk over the other rows (A/B switch)
        self._side = {}
        self.mean_bwd_prescale = True  # spmm mean backward = rows pre-divided by their count + plain SpMM-sum (A/B switch)
        # the launch policy's constants come from the kernel library (ggl_policy_*, include/ggl_mpops.h): ONE copy for this
        # host and the C++ one (csrc/torch/ggl_torch.cpp); the attributes below are A/B overrides for tests and probes
        win, heavy = ctypes.c_int64(0), ctypes.c_int64(0)
        lib.ggl_policy_row_order(ctypes.byref(win), ctypes.byref(heavy))
        self.row_order_window, self.row_order_heavy = int(win.value), int(heavy.value)   # see _row_order (0 = global sort)
        self.xcd_run_rows = -1   # -1 = per graph (ggl_policy_xcd_run_rows on the plan's locality), >= 0 forces it
        self.gradw_sorted = True    # bspmm weight gradient along the sorted plan with LDS-staged strips (A/B switch)
        self.dot_attn_fused = True  # dot-product attention: the dot inside the aggregate's walk (GPU build only; A/B switch)
        self.gatv2_fused = True     # GATv2 attention: the additive logit inside the aggregate's walk (GPU build only; A/B switch)
        self.segment_multi_fused = True   # segment_multi: one walk for all statistics; off = composed from the segment ops (A/B switch)

    def clear_caches(self):
        """Drop every cached plan, sorted-weight copy and graph-constant (e.g. GCN norms).  Plans are keyed on
        the identity + version counter of the id tensor: call this after editing an edge list through `.data`
        or memory shared with numpy, or to hand the HBM back."""
        self.seg_cache.clear()
        self.graph_cache.clear()
        self.w_cache.clear()
        self.rows_cache.clear()

    # ---- plumbing ----------------------------------------------------------------------------
    def _check(self, rc):
        if rc == _lib.GGL_OK:
            return
        msg = (self.lib.ggl_last_error() or b"").decode("utf-8", "replace")
        if rc == _lib.GGL_EINDEX:
            raise IndexError(msg)
        raise RuntimeError(f"ggl_mpops error {rc}: {msg}")

    def _dev(self, *tensors):
        dev = None
        for t in tensors:
            if t is None or isinstance(t, GraphPlan):
                continue
            if self.require_cuda and not t.is_cuda:
                raise RuntimeError(
                    "this is the MI355X engine (libggl_mpops_hip.so): got a tensor on %s; CPU tensors go through "
                    "gammagl_amd.engine(tensor) / gammagl_amd.mpops, which route them to the host build" % t.device)
            if self.cpu_only and t.is_cuda:
                raise RuntimeError("this is the host build of the kernels (CPU tensors only): got a tensor on %s"
                                   % t.device)
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise RuntimeError("Tensor device inconsistent error.")  # segment_sum.cpp:31
        return dev

    def _side_stream(self, dev):
        s = self._side.get(str(dev))
        if s is None:
            s = torch.cuda.Stream(device=dev)
            self._side[str(dev)] = s
        return s

    @staticmethod
    def _stream(dev):
        if dev is not None and dev.type == "cuda":
            return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        return None

    @staticmethod
    def _code(t):
        try:
            return _DTYPE_CODE[t.dtype]
        except KeyError:
            raise RuntimeError(f"unsupported dtype {t.dtype}") from None

    # ---- plans -------------------------------------------------------------------------------
    def _check_range(self, ids, n):
        if ids.numel() == 0:
            return
        # one-off (per plan) validation of the gathered side of an edge list (one host read)
        lo, hi = torch.stack(torch.aminmax(ids)).tolist()
        if lo < 0 or hi >= n:
            raise IndexError(f"node id out of range [0, {n})")

    def auto_chunk(self, E):
        """Long-row threshold for a plan of E elements: `ggl_policy_chunk` (include/ggl_mpops.h) — the ONE copy of the
        rule both hosts use (the largest power of two <= E / resident wavefronts, clamped to [256, 4096]:
        profiles/r1_arxiv_chunk_sweep.txt)."""
        return int(self.lib.ggl_policy_chunk(int(E)))

    def build_plan(self, ids, N, chunk=None):
        """Sort `ids` (int64 [E]) into a SegPlan.  Synchronous; run once per edge list."""
        dev = self._dev(ids)
        ids = ids.contiguous()
        if ids.dtype != torch.int64:
            ids = ids.to(torch.int64)
        E, N = int(ids.shape[0]), int(N)
        chunk = int(chunk or self.chunk or self.auto_chunk(E))
        rowptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
        perm = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
        wsb = self.lib.ggl_plan_workspace_bytes(E, N)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        is_sorted, max_len = ctypes.c_int32(0), ctypes.c_int64(0)
        self._check(self.lib.ggl_plan_build(_ptr(ids), E, N, _ptr(perm), _ptr(rowptr), _ptr(ws),
                                            wsb, self._stream(dev), ctypes.byref(is_sorted), ctypes.byref(max_len)))
        p = self._finish_plan(SegPlan(N, E, rowptr, chunk, max_len.value, dev, perm=None if is_sorted.value else perm[:E],
                                      is_sorted=bool(is_sorted.value)))
        # do the long rows lead the id range (degree-sorted node order)?  One more host read, at plan build only.
        p.hub_first = bool(p.n_long >= 8 and int(p.long_rows[-1]) < 4 * p.n_long)
        return p

    def _finish_plan(self, p):
        """What every plan this engine builds gets after its rowptr: the long-row table (rows of more than `chunk`
        elements) with its `long_order`, the deferred row-order hook, and its number."""
        if p.max_len > p.chunk:
            dev, st = p.device, self._stream(p.device)
            lwb = self.lib.ggl_plan_long_workspace_bytes(p.N)
            lws = torch.empty(lwb, dtype=torch.uint8, device=dev)
            nl, nc = ctypes.c_int64(0), ctypes.c_int64(0)
            self._check(self.lib.ggl_plan_long_count(_ptr(p.rowptr), p.N, p.chunk, _ptr(lws), lwb, st,
                                                     ctypes.byref(nl), ctypes.byref(nc)))
            p.n_long, p.n_chunks = int(nl.value), int(nc.value)
            p.long_rows = torch.empty(p.n_long, dtype=torch.int32, device=dev)
            p.chunk_ptr = torch.empty(p.n_long + 1, dtype=torch.int64, device=dev)
            self._check(self.lib.ggl_plan_long_fill(_ptr(p.rowptr), p.N, p.chunk, p.n_long,
                                                    _ptr(p.long_rows), _ptr(p.chunk_ptr), _ptr(lws), lwb, st))
            p.long_order = self._long_order(p)
        # scheduling aid: rows by descending length inside id windows, see _row_order / ggl_segplan.row_order —
        # computed when the plan is launched a second time (SegPlan.c_struct)
        p.order_fn = self._row_order if p.N > 1 else None
        self.stats["plans_built"] += 1
        p.uid = self.stats["plans_built"]
        return p

    @staticmethod
    def _long_order(p):
        """positions in `long_rows` by descending row length (ggl_segplan.long_order): the serial hub walk starts its
        longest add chains first.  No host read."""
        if not p.n_long:
            return None
        lens = (p.rowptr[1:] - p.rowptr[:-1])[p.long_rows.long()]
        return torch.argsort(lens, descending=True, stable=True).to(torch.int32)

    def _row_order(self, counts):
        """The order rows are handed to lane groups in (kernels where several rows share a wavefront): rows of similar
        length next to each other, so the lanes of a wave finish together (measured K = 64: 7.7 -> 5.9 ms).  A GLOBAL
        sort by length does that but scatters the row ids a workgroup — and the whole chip at any moment — works on
        over the entire graph: on a graph whose node order carries locality (partition.cluster_order, real
        co-purchase / citation graphs) the sources gathered at one time then span every community and L2 keeps
        nothing.  So: rows of `row_order_heavy` elements or more first, longest first (they bound the launch's tail);
        everything else sorted by length inside windows of `row_order_window` consecutive ids, windows in id
        order.  No host read."""
        N = int(counts.shape[0])
        W = int(self.row_order_window)
        if W <= 0 or N <= W:
            return torch.argsort(counts, descending=True, stable=True).to(torch.int32)
        ar = torch.arange(N, device=counts.device, dtype=torch.int64)
        group = torch.where(counts >= int(self.row_order_heavy), torch.zeros_like(ar), 1 + ar // W)
        key = (group << 32) | ((1 << 31) - counts.clamp(max=(1 << 31) - 1))
        return torch.argsort(key, stable=True).to(torch.int32)

    def plan_from_rowptr(self, rowptr, E, max_len=None, chunk=None):
        """SegPlan for elements that are ALREADY grouped by segment (CSR: a sampler's block, a sorted edge
        list): no sort, and no host sync when the caller knows ``max_len`` (e.g. the fan-out).  ``chunk``: the
        long-row threshold of the plan these rows were cut from (rows_plan), instead of the policy's for this E."""
        dev = self._dev(rowptr)
        N = int(rowptr.shape[0]) - 1
        rowptr = rowptr.contiguous().to(torch.int64)
        if max_len is None:
            max_len = int((rowptr[1:] - rowptr[:-1]).max()) if N > 0 else 0
        # (hub_first stays unset: it would cost a host read, and this builder is sync-free when the caller knows max_len)
        return self._finish_plan(SegPlan(N, E, rowptr, chunk or self.chunk or self.auto_chunk(E), max_len, dev))

    def adopt_plan(self, ids, N, plan):
        """Register a plan built elsewhere (e.g. straight from a sampler's CSR block) for the id tensor
        the layers will pass to unsorted_segment_*: the call then hits the cache — no sort, no sync."""
        self.seg_cache.put(ids, (int(N), self.chunk), plan)

    def segment_reduce(self, x, plan, op="sum"):
        """sum / mean / max of x[E, ...] over an explicit plan (no autograd): the aggregate of a sampled
        block whose edges are already grouped by destination."""
        self._dev(x)
        out, arg = self._segment_fwd(op, x.contiguous(), plan)
        return out if op != "max" else (out, arg)

    def seg_plan(self, ids, N):
        plan = self.seg_cache.get(ids, (int(N), self.chunk))
        if plan is None:
            plan = self.build_plan(ids, N)
            self.seg_cache.put(ids, (int(N), self.chunk), plan)
        else:
            self.stats["plan_hits"] += 1
        return plan

    def graph_plan(self, index, n_dst, n_src=None):
        n_src = n_dst if n_src is None else n_src
        gp = self.graph_cache.get(index, (int(n_dst), int(n_src), self.chunk))
        if gp is None:
            self._dev(index)
            if index.dim() != 2 or index.shape[0] != 2:
                raise RuntimeError("index must have shape [2, num_edges]")
            idx = index if index.dtype == torch.int64 else index.to(torch.int64)
            gp = GraphPlan(self, idx.contiguous(), n_dst, n_src)
            self.graph_cache.put(index, (int(n_dst), int(n_src), self.chunk), gp)
        else:
            self.stats["plan_hits"] += 1
        return gp

    def graph_plan_from_csr(self, row_ptr, col_ind, col_ptr, row_ind, permute, n_rows=None, n_cols=None):
        """GraphPlan of prebuilt CSR + CSC + permutation (FusedGATConv's keyword arguments), cached on `row_ptr`."""
        n_rows = int(row_ptr.shape[0]) - 1 if n_rows is None else int(n_rows)
        n_cols = int(col_ptr.shape[0]) - 1 if n_cols is None else int(n_cols)
        extra = ("csr", n_rows, n_cols, self.chunk) + tuple(_PlanCache.key(t, ()) for t in (col_ind, col_ptr, row_ind, permute))
        gp = self.graph_cache.get(row_ptr, extra)
        if gp is not None and any(r.expired() for r in gp.aux.get("_csr_refs", ())):
            # one of the four other tensors died: its storage address (part of the key) may since have been handed to
            # a different tensor of the same shape — identity + version cannot tell, so this is a miss
            gp = None
        if gp is None:
            gp = GraphPlan.from_csr(self, row_ptr, col_ind, col_ptr, row_ind, permute, n_rows, n_cols)
            gp.aux["_csr_refs"] = tuple(StorageWeakRef(t.untyped_storage()) for t in (col_ind, col_ptr, row_ind, permute))
            self.graph_cache.put(row_ptr, extra, gp)
        else:
            self.stats["plan_hits"] += 1
        return gp

    def rows_plan(self, gp, weight, rows):
        """The restricted plan pair of `gp` for the sorted, duplicate-free destination list `rows` (int64 [R]) with the
        edge weights `weight` (or None) copied into sorted order: cached next to the full plan on the identity + version
        of `rows` (and of the weights), so it is built once per (graph, weights, row list) — in warm-up, never inside a
        hipGraph capture (the build reads sizes back)."""
        if rows.dim() != 1 or rows.dtype != torch.int64:
            raise RuntimeError(f"rows must be a 1-D int64 tensor, got {tuple(rows.shape)} {rows.dtype}")
        self._dev(rows, weight)
        extra = ("rows", gp.fwd.uid, gp.N_dst, gp.N_src) + (_PlanCache.key(weight, ()) if weight is not None else (None,))
        rp = self.rows_cache.get(rows, extra)
        if rp is not None and (rp.w_ref is None or not rp.w_ref.expired()):
            self.stats["plan_hits"] += 1
            return rp
        if rows.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("spmm_rows: the restricted plan of this row list must be built before a hipGraph capture "
                               "(run one eager step first)")
        rows = rows.contiguous()
        dev, L, st = rows.device, self.lib, self._stream(rows.device)
        R, N, E = int(rows.shape[0]), gp.N_dst, gp.E
        wsb = L.ggl_plan_rows_workspace_bytes(E, max(gp.N_dst, gp.N_src), R)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        rank = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
        self._check(L.ggl_plan_rows_rank(_ptr(rows), R, N, _ptr(rank), _ptr(ws), wsb, st))
        bwd, colT = gp.bwd, gp.colT
        w = weight
        rp = RowsPlan()
        rp.R, rp.N_dst, rp.N_src, rp.rows = R, gp.N_dst, gp.N_src, rows
        rp.w_ref = StorageWeakRef(weight.untyped_storage()) if weight is not None else None
        # forward: a segmented copy of the listed rows' slices
        rowptr_r = torch.empty(R + 1, dtype=torch.int64, device=dev)
        n = ctypes.c_int64(0)
        self._check(L.ggl_plan_rows_fwd_rowptr(_ptr(gp.fwd.rowptr), _ptr(rows), R, _ptr(rowptr_r), _ptr(ws), wsb, st,
                                               ctypes.byref(n)))
        E_r = int(n.value)
        rp.col = torch.empty(E_r, dtype=torch.int32, device=dev)
        rp.w_fwd = torch.empty(E_r, dtype=torch.float32, device=dev) if w is not None else None
        wperm = gp.fwd.perm if gp.fwd.perm is not None else gp.fwd.wperm
        self._check(L.ggl_plan_rows_fwd_fill(_ptr(gp.fwd.rowptr), _ptr(gp.col), _ptr(w), _ptr(wperm), _ptr(rows), R,
                                             _ptr(rowptr_r), E_r, _ptr(rp.col), _ptr(rp.w_fwd), st))
        rp.fwd = self.plan_from_rowptr(rowptr_r, E_r, chunk=gp.fwd.chunk)   # the full plan's threshold: the same rows are long
        # transposed: the full transposed plan filtered to the listed destinations (flag, scan, compact)
        pos = torch.empty(E + 1, dtype=torch.int32, device=dev)
        rowptrT_r = torch.empty(gp.N_src + 1, dtype=torch.int64, device=dev)
        self._check(L.ggl_plan_rows_bwd_rowptr(_ptr(bwd.rowptr), _ptr(colT), gp.N_src, E, _ptr(rank), _ptr(pos),
                                               _ptr(rowptrT_r), _ptr(ws), wsb, st, ctypes.byref(n)))
        if int(n.value) != E_r:
            raise RuntimeError(f"restricted plans disagree: {E_r} forward elements, {int(n.value)} transposed")
        rp.colT = torch.empty(E_r, dtype=torch.int32, device=dev)
        rp.w_bwd = torch.empty(E_r, dtype=torch.float32, device=dev) if w is not None else None
        wpermT = bwd.perm if bwd.perm is not None else bwd.wperm
        self._check(L.ggl_plan_rows_bwd_fill(_ptr(colT), _ptr(w), _ptr(wpermT), E, _ptr(rank), _ptr(pos), _ptr(rp.colT),
                                             _ptr(rp.w_bwd), st))
        rp.bwd = self.plan_from_rowptr(rowptrT_r, E_r, chunk=bwd.chunk)
        del pos, rank, ws
        self.rows_cache.put(rows, extra, rp)
        return rp

    def spmm_rows(self, gp, weight, x, rows, bias=None):
        """(A x + bias)[rows] for a sorted, duplicate-free int64 row list, computed on the rows alone: [R, K] f32,
        K % 4 == 0.  Equal to spmm_epi(gp, weight, x, bias=bias)[rows], gradients included.  A weight that requires grad
        is refused (c_bspmm_sum is the op with a weight gradient)."""
        self._dev(x, weight, bias, rows)
        self._check_f32("x", x)
        if x.dim() != 2 or x.shape[1] % 4 != 0 or x.shape[1] == 0:
            raise RuntimeError(f"spmm_rows needs a 2-D f32 x whose width is a multiple of 4, got {tuple(x.shape)}")
        if int(x.shape[0]) != gp.N_src:
            raise RuntimeError(f"spmm_rows: x has {int(x.shape[0])} rows, the graph {gp.N_src} source nodes")
        if weight is not None and weight.requires_grad:
            raise RuntimeError("spmm_rows has no gradient for the edge weights: pass detached weights (c_bspmm_sum is the "
                               "op with a weight gradient)")
        weight = self._check_weight(weight, gp)
        if bias is not None:
            self._check_f32("bias", bias)
            if bias.numel() != x.shape[1]:
                raise RuntimeError("bias must hold one value per column")
        return autograd.SpMMRows.apply(self, gp, weight, x.contiguous(), rows, bias)

    def gather_i32(self, src_i64, perm):
        dev = src_i64.device
        src_i64 = src_i64.contiguous()
        E = int(src_i64.shape[0])
        out = torch.empty(E, dtype=torch.int32, device=dev)
        self._check(self.lib.ggl_gather_i64_to_i32(_ptr(src_i64), _ptr(perm), E, _ptr(out),
                                                   self._stream(dev)))
        return out

    @staticmethod
    def _hub_partial(plan, nbytes, dev):
        """The partial buffer of the plan's long rows, `nbytes(n_chunks)` bytes + 16 of slack, or None for a plan
        without long rows.  It must outlive the launch: keep the tensor in a local."""
        if plan.n_long == 0:
            return None
        return torch.empty(nbytes(plan.n_chunks) + 16, dtype=torch.uint8, device=dev)

    # One sizer per export: a call site names the walk it launches, the library owns that walk's layout and checks the size
    # SegPlan.c_struct declares (plan->partial_bytes).
    def _partial(self, plan, dtype, K, with_arg, dev):
        """segment reductions, gspmm / bspmm and their backward walks (ggl_partial_bytes)"""
        return self._hub_partial(
            plan, lambda n: self.lib.ggl_partial_bytes(_DTYPE_CODE[dtype], n, K, 1 if with_arg else 0), dev)

    def _softmax_partial(self, plan, K, dev):
        return self._hub_partial(plan, lambda n: self.lib.ggl_segment_softmax_partial_bytes(n, K), dev)

    def _gat_partial(self, plan, H, C, dev):
        """the forward walks: ggl_gat_fused_fwd[_x16], ggl_gat_fast_fwd, ggl_edge_softmax_agg_fwd, ggl_dot_attn_fwd, ggl_gatv2_fwd"""
        return self._hub_partial(plan, lambda n: self.lib.ggl_gat_partial_bytes(n, H, C), dev)

    def _gat_bwd_dst_partial(self, plan, H, dev):
        return self._hub_partial(plan, lambda n: self.lib.ggl_gat_bwd_dst_partial_bytes(n, H), dev)

    def _gat_bwd_src_partial(self, plan, H, C, dev):
        return self._hub_partial(plan, lambda n: self.lib.ggl_gat_bwd_src_partial_bytes(n, H, C), dev)

    def _gat_fast_bwd_dst_partial(self, plan, H, dev):
        return self._hub_partial(plan, lambda n: self.lib.ggl_gat_fast_bwd_dst_partial_bytes(n, H), dev)

    def _gat_sh_partial(self, plan, F, dev):
        return self._hub_partial(plan, lambda n: self.lib.ggl_gat_sh_partial_bytes(n, F), dev)

    def _gat_sh_bwd_dst_partial(self, plan, dev):
        return self._hub_partial(plan, self.lib.ggl_gat_sh_bwd_dst_partial_bytes, dev)

    def _gat_sh_bwd_src_partial(self, plan, Cp, dev):
        return self._hub_partial(plan, lambda n: self.lib.ggl_gat_sh_bwd_src_partial_bytes(n, Cp), dev)

    def _softmax_width(self, x, plan):
        E = int(x.shape[0])
        if E != plan.E:
            raise IndexError("fisrt dimension of x and index should be same")
        self._check_f32("x", x)
        K = int(math.prod(x.shape[1:]))
        if not self.lib.ggl_segment_softmax_supported(K):
            raise RuntimeError(f"segment_softmax: no kernel for rows of {K} columns (ggl_segment_softmax_supported); "
                               "gammagl_amd.utils.segment_softmax composes such rows from the segment ops")
        return K

    def _softmax_fwd(self, x, plan):
        """y = softmax of x[E, ...] over the plan's segments (ggl_segment_softmax_fwd), caller's element order."""
        K = self._softmax_width(x, plan)
        dev = x.device
        y = torch.empty_like(x)
        part = self._softmax_partial(plan, K, dev)   # must outlive the launch
        cs = plan.c_struct(part)
        self._check(self.lib.ggl_segment_softmax_fwd(_ptr(x), ctypes.byref(cs), K, _ptr(y), self._stream(dev)))
        return y

    def _softmax_bwd(self, y, g, plan):
        """gx from y and g alone (ggl_segment_softmax_bwd)."""
        K = self._softmax_width(y, plan)
        dev = y.device
        g = g.contiguous()
        gx = torch.empty_like(y)
        part = self._softmax_partial(plan, K, dev)
        cs = plan.c_struct(part)
        self._check(self.lib.ggl_segment_softmax_bwd(_ptr(y), _ptr(g), ctypes.byref(cs), K, _ptr(gx), self._stream(dev)))
        return gx

    # ---- raw (non-autograd) forward launches -------------------------------------------------
    def _segment_fwd(self, op, x, plan):
        dev = x.device
        E = int(x.shape[0])
        if E != plan.E:
            raise IndexError("fisrt dimension of x and index should be same")  # segment_sum_cpu.cpp:17-19
        K = x.numel() // E if E > 0 else int(math.prod(x.shape[1:]))
        out = torch.empty((plan.N,) + tuple(x.shape[1:]), dtype=x.dtype, device=dev)
        st = self._stream(dev)
        code = self._code(x)
        # f16 / bf16 sums accumulate in the storage type (segment_sum_cpu.cpp:47-56): the result depends on
        # the serial order well beyond rounding (a running f16 sum of ones sticks at 2048), so combining
        # chunk partials would not reproduce the reference: those rows are always walked in one piece
        unsplit = op != "max" and x.dtype in (torch.float16, torch.bfloat16)
        # ... but only their ADD chain is serial, not the loads: where the library has the LDS-pipelined hub kernel
        # (GPU build, hub16.hip) the hub rows get a launch of their own, a workgroup per (row, 64-column slab)
        hubs = bool(unsplit and plan.n_long > 0 and self.hub16 and
                    self.lib.ggl_segment_hub16_supported(code, K, _ptr(x), _ptr(out)))
        part = None if unsplit else self._partial(plan, x.dtype, K, op == "max", dev)
        cs = plan.c_struct(part, unsplit=unsplit and not hubs, skip_long=hubs)
        if op in ("sum", "mean"):
            fn = self.lib.ggl_segment_sum if op == "sum" else self.lib.ggl_segment_mean
            side = None
            if hubs:
                # the hub rows' serial add chains (16-24 ns per element: 2.4-3.5 ms for a 147 000-element hub) run BESIDE
                # the launch over all other rows, on a side stream — they write disjoint rows of `out`
                full = plan.c_struct(None)
                if dev.type == "cuda" and self.hub16_overlap:
                    cur = torch.cuda.current_stream(dev)
                    side = self._side_stream(dev)
                    side.wait_stream(cur)
                    self._check(self.lib.ggl_segment_hub16(code, 0 if op == "sum" else 1, _ptr(x), ctypes.byref(full), K,
                                                           _ptr(out), ctypes.c_void_p(side.cuda_stream)))
            self._check(fn(code, _ptr(x), ctypes.byref(cs), K, _ptr(out), st))
            if hubs and side is None:
                self._check(self.lib.ggl_segment_hub16(code, 0 if op == "sum" else 1, _ptr(x), ctypes.byref(full), K,
                                                       _ptr(out), st))
            if side is not None:
                torch.cuda.current_stream(dev).wait_stream(side)
            return out, None
        arg = torch.empty((plan.N,) + tuple(x.shape[1:]), dtype=torch.int64, device=dev)
        self._check(self.lib.ggl_segment_max(code, _ptr(x), ctypes.byref(cs), K, _ptr(out), _ptr(arg),
                                             E, st))
        return out, arg

    def _segment_bwd(self, g, ids, x_shape, rowptr=None):
        """gx[e] = g[ids[e]] (segment_sum), divided by the segment's length with the plan's `rowptr` (segment_mean)."""
        g = g.contiguous()
        E, K = int(x_shape[0]), int(math.prod(x_shape[1:]))
        gx = torch.empty(x_shape, dtype=g.dtype, device=g.device)
        st = self._stream(g.device)
        if rowptr is None:
            self._check(self.lib.ggl_segment_sum_bwd(self._code(g), _ptr(g), _ptr(ids), E, K, _ptr(gx), st))
        else:
            if g.dtype not in _FLOAT_DTYPES:
                raise RuntimeError("segment_mean backward needs a floating dtype")
            self._check(self.lib.ggl_segment_mean_bwd(self._code(g), _ptr(g), _ptr(ids), _ptr(rowptr), E, K, _ptr(gx), st))
        return gx

    @staticmethod
    def _row_stride(t, what, dtype=torch.float32):
        if t.dim() != 2 or t.stride(1) != 1 or t.dtype != dtype:
            raise RuntimeError(f"{what} must be a 2-D {'f32' if dtype == torch.float32 else dtype} matrix with unit "
                               "column stride (a column block is fine)")
        return int(t.stride(0))

    def spmm_sum_into(self, plan, col, w, x, out, accumulate=False):
        """out (+)= A x for 2-D f32 x / out that may be column blocks of wider matrices (row strides are
        passed down: no contiguous copy, no temporary, no separate add) — ggl_spmm_sum_ex."""
        dev = x.device
        K = int(x.shape[1])
        if out.shape[1] != K or out.shape[0] != plan.N:
            raise RuntimeError("out must be [plan rows, x columns]")
        part = self._partial(plan, torch.float32, K, False, dev)
        w, w_by_pos, wp = self._weights(plan, w)
        cs = plan.c_struct(part, wp)
        self._check(self.lib.ggl_spmm_sum_ex(ctypes.byref(cs), _ptr(col), _ptr(w), w_by_pos, _ptr(x),
                                             self._row_stride(x, "x"), K, _ptr(out), self._row_stride(out, "out"),
                                             int(bool(accumulate)), self._stream(dev)))
        return out

    def gather_rows_into(self, src, idx, out):
        """out[i, :] = src[idx[i], :] for 2-D f32 src / out that may be column blocks of wider matrices (one
        kernel, no strided view + index_select + contiguous copy) — ggl_gather_rows_f32_ex."""
        dev = src.device
        n, K = int(idx.shape[0]), int(src.shape[1])
        if out.shape[0] != n or out.shape[1] != K or idx.dtype != torch.int64:
            raise RuntimeError("gather_rows_into: out must be [len(idx), columns of src], idx int64")
        self._check(self.lib.ggl_gather_rows_f32_ex(_ptr(src), self._row_stride(src, "src"), _ptr(idx), n, K,
                                                    _ptr(out), self._row_stride(out, "out"), self._stream(dev)))
        return out

    def spmm_epi_into(self, plan, col, w, x, out, accumulate=False, mean=False, add=None, bias=None, relu=False,
                      p_drop=0.0, rng=None, epi_K=0, col0=0, advance_rng=True):
        """out = dropout(relu(reduce(A x) (+ out) + add + bias)) on column blocks, no autograd — ggl_spmm_epi_ex.
        `bias` [>= col0 + K] is the full-width bias; `add` a [N, K] block view.  bf16 / f16 `x` (and `add`) take
        ggl_spmm_epi_x16: f32 arithmetic, `out` in x's dtype (rounded once) or f32; no accumulate there."""
        dev = x.device
        K = int(x.shape[1])
        if out.shape[1] != K or out.shape[0] != plan.N:
            raise RuntimeError("out must be [plan rows, x columns]")
        part = self._partial(plan, torch.float32, K, False, dev)
        w, w_by_pos, wp = self._weights(plan, w)
        cs = plan.c_struct(part, wp)
        b = None
        if bias is not None:
            b = ctypes.c_void_p(bias.data_ptr() + 4 * int(col0))
        if x.dtype in _X16_DTYPES:
            if accumulate:
                raise RuntimeError("spmm_epi_into: no accumulate on 16-bit rows (a rounded partial result would round twice)")
            self._check(self.lib.ggl_spmm_epi_x16(
                ctypes.byref(cs), _ptr(col), _ptr(w), w_by_pos, _DTYPE_CODE[x.dtype], _ptr(x),
                self._row_stride(x, "x", x.dtype), K, _DTYPE_CODE[out.dtype], _ptr(out),
                self._row_stride(out, "out", out.dtype), int(bool(mean)), _ptr(add),
                (self._row_stride(add, "add", x.dtype) if add is not None else 0), b, int(bool(relu)), float(p_drop),
                _ptr(rng), int(epi_K), int(col0), int(bool(advance_rng)), self._stream(dev)))
            return out
        self._check(self.lib.ggl_spmm_epi_ex(
            ctypes.byref(cs), _ptr(col), _ptr(w), w_by_pos, _ptr(x), self._row_stride(x, "x"), K, _ptr(out),
            self._row_stride(out, "out"), int(bool(accumulate)), int(bool(mean)), _ptr(add),
            (self._row_stride(add, "add") if add is not None else 0), b, int(bool(relu)), float(p_drop),
            _ptr(rng), int(epi_K), int(col0), int(bool(advance_rng)), self._stream(dev)))
        return out

    def segment_sum_into(self, x, plan, out, accumulate=False):
        """out (+)= segment_sum(x) over `plan`, same strided / in-place conventions — ggl_segment_sum_ex."""
        dev = x.device
        K = int(x.shape[1])
        if int(x.shape[0]) != plan.E or out.shape[1] != K or out.shape[0] != plan.N:
            raise IndexError("segment_sum_into: shapes do not match the plan")
        part = self._partial(plan, torch.float32, K, False, dev)
        cs = plan.c_struct(part)
        self._check(self.lib.ggl_segment_sum_ex(self._code(x), _ptr(x), self._row_stride(x, "x"), ctypes.byref(cs), K,
                                                _ptr(out), self._row_stride(out, "out"), int(bool(accumulate)),
                                                self._stream(dev)))
        return out

    def _spmm_fwd16(self, op, plan, col, w, x, n_out, perm_override=None, aux=None, out_dtype=None):
        """sum / mean / mean_bwd on rows stored as bf16 / f16 (ggl_spmm_*_x16): widened at the load, the f32 op's products
        and adds in its order, rounded once at the store — or not at all with out_dtype=torch.float32.  Any width: rows
        that are not multiples of 8 columns take the ragged / one-element-per-lane kernels, nothing is padded."""
        dev = x.device
        K = int(math.prod(x.shape[1:]))
        out_dtype = x.dtype if out_dtype is None else out_dtype
        if out_dtype not in (x.dtype, torch.float32):
            raise RuntimeError(f"gspmm on {x.dtype} rows returns {x.dtype} or torch.float32, not {out_dtype}")
        out = torch.empty((n_out,) + tuple(x.shape[1:]), dtype=out_dtype, device=dev)
        st = self._stream(dev)
        part = self._partial(plan, torch.float32, K, False, dev)      # f32 partials: a 16-bit one would round twice
        w, w_by_pos, wp = self._weights(plan, w, perm_override)
        cs = plan.c_struct(part, wp)
        L = self.lib
        xc, oc = _DTYPE_CODE[x.dtype], _DTYPE_CODE[out_dtype]
        if op == "sum":
            self._check(L.ggl_spmm_sum_x16(ctypes.byref(cs), _ptr(col), _ptr(w), w_by_pos, xc, _ptr(x), 0, K, oc,
                                           _ptr(out), 0, st))
        elif op == "mean":
            self._check(L.ggl_spmm_mean_x16(ctypes.byref(cs), _ptr(col), _ptr(w), w_by_pos, xc, _ptr(x), 0, K, oc,
                                            _ptr(out), 0, st))
        elif op == "mean_bwd":
            # (no pre-scaled copy of g as on the f32 route: it would be an f32 [N, K] pass, the bytes this path saves)
            self._check(L.ggl_spmm_mean_bwd_x16(ctypes.byref(cs), _ptr(col), _ptr(w), w_by_pos, xc, _ptr(x), _ptr(aux),
                                                K, oc, _ptr(out), st))
        else:
            raise ValueError(op)
        return out, None

    def _spmm_fwd(self, op, plan, col, w, x, n_out, perm_override=None, aux=None, gp=None, out_dtype=None):
        """op in sum/mean/max/mean_bwd/max_bwd.  x [N_in, *]; returns out [n_out, *] (+argsrc)."""
        if x.dtype in _X16_DTYPES and op in ("sum", "mean", "mean_bwd"):
            return self._spmm_fwd16(op, plan, col, w, x, n_out, perm_override, aux, out_dtype)
        dev = x.device
        K = int(math.prod(x.shape[1:]))
        if op in ("sum", "mean", "max") and x.dim() == 2:
            # ggl_policy_spmm_width (include/ggl_mpops.h): rows wider than 256 columns that are not whole cache lines
            # (602 Reddit features) -> a multiple of 64 for the 64-column blocks (products-sized K = 602: 55 -> 42 ms);
            # class-count widths (47, 41, 7 ...) -> a multiple of 4 for the float4 kernels (K = 47: 9.3 -> 5.8 ms); the
            # max walk of wide rows that are not 16-byte pieces -> a multiple of 4 (K = 602: 69 -> 60 ms).  One
            # zero-padded copy of x; the pad columns (values and argmax) are dropped.
            Kp = int(self.lib.ggl_policy_spmm_width(1 if op == "max" else 0, K, plan.E, int(x.shape[0])))
            if Kp != K:
                xp = torch.nn.functional.pad(x, (0, Kp - K))
                out, arg = self._spmm_fwd(op, plan, col, w, xp, n_out, perm_override, aux)
                return out[:, :K].contiguous(), (arg[:, :K].contiguous() if arg is not None else None)
        out = torch.empty((n_out,) + tuple(x.shape[1:]), dtype=torch.float32, device=dev)
        st = self._stream(dev)
        part = self._partial(plan, torch.float32, K, op == "max", dev)
        w, w_by_pos, wp = self._weights(plan, w, perm_override)
        cs = plan.c_struct(part, wp)
        L = self.lib
        if op == "sum":
            self._check(L.ggl_spmm_sum(ctypes.byref(cs), _ptr(col), _ptr(w), w_by_pos, _ptr(x), K,
                                       _ptr(out), st))
        elif op == "mean":
            self._check(L.ggl_spmm_mean(ctypes.byref(cs), _ptr(col), _ptr(w), w_by_pos, _ptr(x), K,
                                        _ptr(out), st))
        elif op == "max":
            arg = torch.empty(out.shape, dtype=torch.int64, device=dev)
            self._check(L.ggl_spmm_max(ctypes.byref(cs), _ptr(col), _ptr(w), w_by_pos, _ptr(x), K,
                                       _ptr(out), _ptr(arg), st))
            return out, arg
        elif op == "mean_bwd":
            if self.mean_bwd_prescale and x.dim() == 2 and self.lib.ggl_policy_mean_bwd_prescale(plan.E, int(x.shape[0])):
                # gx[src] += (g[dst] / count[dst]) * w (spmm_mean_cpu.cpp:90-100): the division depends on the
                # destination row only, so it is done ONCE per row (the same rounded divide on the same operands) and
                # the walk is the plain transposed SpMM-sum — no per-edge degree lookup (a random 16-byte read, i.e. one
                # more line per edge), and the 64-column blocks apply: products-sized K = 256 23.0 -> 15.5 ms, same bits
                cnt = (aux[1:] - aux[:-1]).clamp(min=1).to(torch.float32).unsqueeze(1)
                xs = x / cnt
                self._check(L.ggl_spmm_sum(ctypes.byref(cs), _ptr(col), _ptr(w), w_by_pos, _ptr(xs), K,
                                           _ptr(out), st))
            else:
                self._check(L.ggl_spmm_mean_bwd(ctypes.byref(cs), _ptr(col), _ptr(w), w_by_pos, _ptr(x),
                                                _ptr(aux), K, _ptr(out), st))
        elif op == "max_bwd":
            # the form is the library's decision (ggl_policy_maxbwd_form): the winner mask is an E x K/8-byte transient, taken only
            # where it is smaller than a multiple of the witness matrix it replaces and that matrix is not cache-resident
            form = int(L.ggl_policy_maxbwd_form(plan.E, int(aux.shape[0]), K)) if gp is not None else (
                1 if int(L.ggl_get_option(b"maxbwd_arg32")) else 0)
            mask = None
            if form == 2:
                try:
                    mask = torch.empty(int(L.ggl_spmm_max_mask_bytes(plan.E, K)) // 4 + 4, dtype=torch.int32, device=dev)
                except torch.OutOfMemoryError:
                    form = 1                    # no room for the transient: the int32 witness copy ([N, K] x 4 bytes)
            if form == 2:
                # a 1-bit winner mask built in DESTINATION order (the witness row is wave-uniform there), read in the
                # transposed walk's own order: K / 8 bytes per edge instead of 8K (include/ggl_mpops.h)
                fs = gp.fwd.c_struct(None)
                # records in forward order (coalesced writes); the walk reads record posT[t]
                self._check(L.ggl_spmm_max_mask(ctypes.byref(fs), _ptr(gp.col), _ptr(aux), K, _ptr(mask), st))
                self._check(L.ggl_spmm_max_bwd_mask(ctypes.byref(cs), _ptr(col), _ptr(w), w_by_pos, _ptr(x), _ptr(mask),
                                                    _ptr(gp.posT), K, _ptr(out), st))
            elif form == 1:   # witnesses from a compact int32 copy (one [N, K] pass)
                aux32 = aux.to(torch.int32)
                self._check(L.ggl_spmm_max_bwd32(ctypes.byref(cs), _ptr(col), _ptr(w), w_by_pos, _ptr(x),
                                                 _ptr(aux32), K, _ptr(out), st))
            else:
                self._check(L.ggl_spmm_max_bwd(ctypes.byref(cs), _ptr(col), _ptr(w), w_by_pos, _ptr(x),
                                               _ptr(aux), K, _ptr(out), st))
        else:
            raise ValueError(op)
        return out, None

    def _weights(self, plan, w, perm_override=None):
        """(weights, w_by_pos, perm for the launch struct) of one walk over `plan`: weights that came back a second time
        are streamed in sorted order (`_sorted_weights`); otherwise the kernel reads w[perm[p]] — through the plan's own
        permutation, or, on the CSC side of a CSR-built plan, through `wperm` (GraphPlan.from_csr)."""
        if perm_override is not None or w is None:
            return w, 0, perm_override
        wp = plan.perm if plan.perm is not None else plan.wperm
        if wp is None:
            return w, 0, None
        w, by_pos = self._sorted_weights(plan, w, wp)
        return w, by_pos, (wp if plan.perm is None else None)

    def _sorted_weights(self, plan, w, perm=None):
        """Edge weights in the plan's sorted order, for weights that are REUSED.

        The kernels can read w[perm[p]] themselves (one random 4-byte read per edge).  A weight tensor
        seen for the second time on the same plan (GCN: the same normalisation weights feed every layer,
        forward and backward, every step) is gathered once into sorted order and cached by the
        identity + version of its storage, after which every launch streams it (w_by_pos = 1)."""
        key_extra = (plan.uid,)
        hit = self.w_cache.get(w, key_extra)
        if hit is None:
            self.w_cache.put(w, key_extra, False)  # first sight: remember it, gather in-kernel
            return w, 0
        if hit is False:
            E = int(plan.E)
            H = w.numel() // E if E > 0 else 1
            ws = torch.empty_like(w)
            self._check(self.lib.ggl_gather_rows_f32(_ptr(w), _ptr(plan.perm if perm is None else perm), E, max(H, 1), _ptr(ws),
                                                     self._stream(w.device)))
            self.w_cache.put(w, key_extra, ws)
            hit = ws
        return hit, 1

    def _bspmm_fwd(self, plan, col, w, x, n_out, perm_override=None):
        dev = x.device
        H, C = int(x.shape[1]), int(x.shape[2])
        out = torch.empty((n_out, H, C), dtype=torch.float32, device=dev)
        part = self._partial(plan, torch.float32, H * C, False, dev)
        w, w_by_pos, wp = self._weights(plan, w, perm_override)
        cs = plan.c_struct(part, wp)
        self._check(self.lib.ggl_bspmm_sum(ctypes.byref(cs), _ptr(col), _ptr(w), w_by_pos, _ptr(x), H, C,
                                           _ptr(out), self._stream(dev)))
        return out

    @staticmethod
    def _check_f32(name, t):
        if t.dtype != torch.float32:
            # spmm_sum_cpu.cpp:22 data_ptr<float>() on a non-float tensor
            raise RuntimeError(f"expected scalar type Float but found {t.dtype} for {name}")

    @staticmethod
    def _check_f32_or_x16(name, t):
        """gspmm sum / mean: f32 as the reference, or bf16 / f16 storage (an extension: f32 sums, rounded once)."""
        if t.dtype != torch.float32 and t.dtype not in _X16_DTYPES:
            raise RuntimeError(f"expected scalar type Float (or Half / BFloat16 storage) but found {t.dtype} for {name}")

    def _spmm_bwd_x(self, gp, w, g, x_dtype, mean):
        """gx of sum / mean in x's dtype: the transposed walk on g as it arrives (mean: it divides by the destination
        row's length).  An f32 g for 16-bit rows (the forward returned f32: out_dtype) is walked in f32 and rounded once."""
        g = g.contiguous()
        if mean:
            gx, _ = self._spmm_fwd("mean_bwd", gp.bwd, gp.colT, w, g, gp.N_src, aux=gp.fwd.rowptr)
        else:
            gx, _ = self._spmm_fwd("sum", gp.bwd, gp.colT, w, g, gp.N_src)
        return gx if gx.dtype == x_dtype else gx.to(x_dtype)

    def _spmm_grad_w(self, gp, x, g, mean):
        """gw [E] of gspmm sum / mean (ggl_spmm_grad_w): gw[e] = sum_k x[src_e, k] * g[dst_e, k], g divided by
        the destination row's edge count first for mean.  f32 [E] whatever x and g are stored as (f32 / bf16 / f16 each:
        widened at the load, f32 products and adds in the serial order); along the destination-sorted forward plan."""
        g = g.contiguous()
        K = int(math.prod(x.shape[1:]))
        if gp.E == 0 or K == 0:
            return torch.zeros(gp.E, dtype=torch.float32, device=g.device)
        gw = torch.empty(gp.E, dtype=torch.float32, device=g.device)     # every entry is written (through perm)
        xc, gc = _DTYPE_CODE[x.dtype], _DTYPE_CODE[g.dtype]
        sb = self.lib.ggl_spmm_grad_w_scratch_bytes(gp.E, gp.N_dst, K, xc, int(bool(mean)))
        scratch = torch.empty(sb // 4, dtype=torch.float32, device=g.device) if sb else None
        cs = gp.fwd.c_struct(None)
        self._check(self.lib.ggl_spmm_grad_w(ctypes.byref(cs), _ptr(gp.col), _ptr(gp.rowidx), xc, _ptr(x), gc, _ptr(g),
                                             _ptr(gp.fwd.rowptr) if mean else None, K, _ptr(gw), _ptr(scratch),
                                             self._stream(g.device)))
        return gw

    # ---- the seven reference entry points (src/operators.cpp:51-59) + the fused GAT op ---------
    def _seg_args(self, x, index, N):
        self._dev(x, index)
        if index.dim() != 1:
            raise IndexError(f"index dimension should be 1, but got {index.dim()}")
        if x.shape[0] != index.shape[0]:
            raise IndexError("fisrt dimension of x and index should be same")
        if index.dtype != torch.int64:
            raise RuntimeError(f"expected scalar type Long but found {index.dtype}")
        return x.contiguous(), index, int(N)

    def c_segment_sum(self, x, index, N):
        return autograd.SegmentSum.apply(self, *self._seg_args(x, index, N))

    def c_segment_mean(self, x, index, N):
        return autograd.SegmentMean.apply(self, *self._seg_args(x, index, N))

    def c_segment_max(self, x, index, N):
        return autograd.SegmentMax.apply(self, *self._seg_args(x, index, N))[0]

    def segment_max_with_arg(self, x, index, N):
        return autograd.SegmentMax.apply(self, *self._seg_args(x, index, N))

    # ---- several statistics of the same rows in one walk (ggl_segment_multi_*, csrc/multiagg.hpp) ----
    AGG_CODES = {"sum": 0, "mean": 1, "min": 2, "max": 3, "var": 4, "std": 5}   # enum GGL_AGG_* (include/ggl_mpops.h)

    @classmethod
    def agg_codes(cls, aggs):
        """names (or codes) -> a tuple of distinct GGL_AGG_* codes, in the caller's order"""
        codes = []
        for a in aggs:
            c = cls.AGG_CODES.get(a) if isinstance(a, str) else (int(a) if 0 <= int(a) <= 5 else None)
            if c is None:
                raise ValueError(f"segment_multi: unknown aggregator {a!r}; choose from {sorted(cls.AGG_CODES)}")
            if c in codes:
                raise ValueError(f"segment_multi: aggregator {a!r} is given twice")
            codes.append(c)
        if not 1 <= len(codes) <= 6:
            raise ValueError("segment_multi: between 1 and 6 aggregators")
        return tuple(codes)

    def _segment_multi_fwd(self, x, plan, codes, C, empty_zero, want_mean=False):
        """(out [N, A * K], mean [N, K] or None, argmin, argmax [N, K] int32 or None) of x [E, K] f32 contiguous"""
        dev, E, K, A = x.device, int(x.shape[0]), int(x.shape[1]), len(codes)
        if E != plan.E:
            raise IndexError("fisrt dimension of x and index should be same")
        out = torch.empty((plan.N, A * K), dtype=torch.float32, device=dev)
        mean = torch.empty((plan.N, K), dtype=torch.float32, device=dev) if want_mean else None
        amin = torch.empty((plan.N, K), dtype=torch.int32, device=dev) if 2 in codes else None
        amax = torch.empty((plan.N, K), dtype=torch.int32, device=dev) if 3 in codes else None
        arr = (ctypes.c_int * A)(*codes)
        part = self._hub_partial(plan, lambda n: self.lib.ggl_segment_multi_partial_bytes(n, K, arr, A), dev)
        cs = plan.c_struct(part)
        self._check(self.lib.ggl_segment_multi_fwd(_ptr(x), ctypes.byref(cs), K, C, arr, A, int(bool(empty_zero)), _ptr(out),
                                                   _ptr(mean), _ptr(amin), _ptr(amax), self._stream(dev)))
        return out, mean, amin, amax

    def _segment_multi_bwd(self, g, x, out, mean, amin, amax, plan, K, C, codes):
        dev, A = g.device, len(codes)
        g = g.contiguous()
        gx = torch.empty((plan.E, K), dtype=torch.float32, device=dev)
        arr = (ctypes.c_int * A)(*codes)
        cs = plan.c_struct(None)
        self._check(self.lib.ggl_segment_multi_bwd(_ptr(g), _ptr(x), _ptr(out), _ptr(mean), _ptr(amin), _ptr(amax),
                                                   ctypes.byref(cs), K, C, arr, A, _ptr(gx), self._stream(dev)))
        return gx

    def _segment_multi_composed(self, x, ids, N, codes, C, empty_zero):
        """The same statistics from the existing segment ops (the A/B partner of the fused walk and PNAConv's
        fused=False): mean, sum and max as they are, min = -max(-x), var = mean(x * x) - mean * mean,
        std = sqrt(relu(var) + 1e-5) (pna_conv.py:159-181)."""
        E, K = int(x.shape[0]), int(x.shape[1])
        mean = self.c_segment_mean(x, ids, N) if any(c in codes for c in (1, 4, 5)) else None
        var = None
        if 4 in codes or 5 in codes:
            var = self.c_segment_mean(x * x, ids, N) - mean * mean
        cnt = None
        if empty_zero and (2 in codes or 3 in codes):
            cnt = torch.bincount(ids, minlength=N).unsqueeze(1)
        outs = []
        for c in codes:
            if c == 0:
                o = self.c_segment_sum(x, ids, N)
            elif c == 1:
                o = mean
            elif c == 2:
                o = -self.c_segment_max(-x, ids, N)
            elif c == 3:
                o = self.c_segment_max(x, ids, N)
            elif c == 4:
                o = var
            else:
                o = sqrt_rn(torch.relu(var) + 1e-5)
            if cnt is not None and c in (2, 3):
                o = torch.where(cnt > 0, o, torch.zeros_like(o))
            outs.append(o.reshape(N, K // C, 1, C))
        return torch.cat(outs, 2).reshape(N, len(codes) * K)

    def segment_multi(self, x, ids_or_plan, N=None, aggs=("mean", "min", "max", "std"), C=None, empty_zero=False,
                      return_witnesses=False):
        """Several statistics of x [E, K] f32 over the segments of `ids_or_plan` (int64 ids [E], or a SegPlan) in one walk:
        out [N, K / C, A, C] stored as [N, A * K] — column k of statistic a at (k / C) * A * C + a * C + k % C; C = K (the
        default) is cat(outs, -1), x [E, T * F] with C = F the per-tower concatenation.  `aggs`: distinct names from sum,
        mean, min, max, var, std, in output order.  Empty segments: 0 for sum / mean / var, sqrt(1e-5) for std, -+FLT_MAX for
        max / min or 0 with `empty_zero`.  Differentiable in x; with `return_witnesses` also (argmin, argmax) [N, K] int32
        (None where not requested).  With `self.segment_multi_fused` off the statistics are composed from the segment ops."""
        codes = self.agg_codes(aggs)
        self._check_f32("x", x)
        if x.dim() != 2:
            raise RuntimeError(f"segment_multi expects x [E, K], got {tuple(x.shape)}")
        K = int(x.shape[1])
        C = K if C is None else int(C)
        if C <= 0 or (K % C and K > 0):
            raise RuntimeError(f"segment_multi: C = {C} does not divide K = {K}")
        if isinstance(ids_or_plan, SegPlan):
            self._dev(x)
            plan, ids = ids_or_plan, None
        else:
            x, ids, N = self._seg_args(x, ids_or_plan, N)
            plan = None
        if not self.segment_multi_fused and ids is not None and not return_witnesses:
            self.stats["segment_multi"] = {"route": "composed", "saved": ()}
            return self._segment_multi_composed(x, ids, N, codes, C, empty_zero)
        if plan is None:
            plan = self.seg_plan(ids, N)
        out, amin, amax = autograd.SegmentMulti.apply(self, x.contiguous(), plan, codes, C, bool(empty_zero),
                                                            bool(x.requires_grad and torch.is_grad_enabled()))
        return (out, amin, amax) if return_witnesses else out

    def segment_softmax_supported(self, x):
        """Does the native edge softmax take `x` (f32, rows of a width the library has a kernel for)?"""
        K = int(math.prod(x.shape[1:]))
        return x.dtype == torch.float32 and x.dim() >= 1 and bool(self.lib.ggl_segment_softmax_supported(K))

    def segment_softmax(self, x, index, N=None):
        """utils/softmax.py:10-36 as ONE op with its own backward: y[e] = exp(x[e] - max) / (sum + 1e-16) over the
        elements that share a segment id, per trailing column.  x: [E], [E, H] or [E, H, C] f32; `index`: int64 ids
        [E] (plan from the cache) or a SegPlan built with build_plan / plan_from_rowptr (explicit-plan form, as
        segment_reduce is for the sums)."""
        if isinstance(index, SegPlan):
            self._dev(x)
            return autograd.SegmentSoftmax.apply(self, x.contiguous(), index)
        x, index, N = self._seg_args(x, index, N)
        return autograd.SegmentSoftmax.apply(self, x, self.seg_plan(index, N))

    def _spmm_args(self, index, weight, x, x16=False):
        self._dev(index, weight, x)
        (self._check_f32_or_x16 if x16 else self._check_f32)("x", x)
        if weight is not None:
            self._check_f32("weight", weight)
            weight = weight.contiguous()
        gp = self.graph_plan(index, x.shape[0])
        return gp, weight, x.contiguous()

    def c_spmm_sum(self, index, weight, x, out_dtype=None):
        """c_spmm_sum of the reference for f32 x; bf16 / f16 x (an extension) is summed in f32 and returned in x's dtype,
        or unrounded with out_dtype=torch.float32."""
        return autograd.SpMMSum.apply(self, *self._spmm_args(index, weight, x, True), self._out_dtype(x, out_dtype))

    def c_spmm_mean(self, index, weight, x, out_dtype=None):
        return autograd.SpMMMean.apply(self, *self._spmm_args(index, weight, x, True), self._out_dtype(x, out_dtype))

    @staticmethod
    def _out_dtype(x, out_dtype):
        if out_dtype is None or out_dtype == x.dtype:
            return None
        if x.dtype not in _X16_DTYPES or out_dtype != torch.float32:
            raise RuntimeError(f"out_dtype={out_dtype}: only torch.float32 from bf16 / f16 rows (x is {x.dtype})")
        return out_dtype

    def spmm_grad_w(self, index, x, grad, mean=False):
        """The weight gradient of c_spmm_sum / c_spmm_mean as an op of its own: f32 [E], gw[e] = sum_k x[src_e, k] *
        grad[dst_e, k] (mean: grad divided by the destination row's edge count first); x and grad f32, bf16 or f16."""
        self._dev(index, x, grad)
        self._check_f32_or_x16("x", x)
        self._check_f32_or_x16("grad", grad)
        if math.prod(x.shape[1:]) != math.prod(grad.shape[1:]):
            raise RuntimeError(f"spmm_grad_w: x {tuple(x.shape)} and grad {tuple(grad.shape)} differ in row width")
        gp = self.graph_plan(index, grad.shape[0], x.shape[0])
        return self._spmm_grad_w(gp, x.contiguous(), grad, mean)

    def c_spmm_max(self, index, weight, x):
        return autograd.SpMMMax.apply(self, *self._spmm_args(index, weight, x))

    def c_bspmm_sum(self, index, weight, x):
        if x.dim() != 3:
            raise RuntimeError("bspmm expects x of shape [num_nodes, heads, channels]")
        gp, weight, x = self._spmm_args(index, weight, x)
        if weight is None or weight.dim() != 2 or weight.shape[1] != x.shape[1]:
            raise RuntimeError("bspmm expects weight of shape [num_edges, heads]")
        return self._head_padded(gp, x, lambda xp: autograd.BSpMMSum.apply(self, gp, weight, xp.contiguous()))

    def _head_padded(self, gp, x, apply):
        """apply(x [N, H, C]) with the head width padded to `ggl_policy_head_channels` and the pad sliced off the result:
        odd channel counts (41 classes per head: [N, H, 44]) get one zero-padded copy of x, which keeps the row walks and
        the per-edge weight-gradient dots on 16-byte slices (Reddit-sized fused GAT, 8 x 41: forward 50 -> 20 ms); the pad
        channels aggregate to zero and are dropped."""
        C = int(x.shape[2])
        Cp = int(self.lib.ggl_policy_head_channels(C, gp.E, int(x.shape[0])))
        if Cp != C:
            return apply(torch.nn.functional.pad(x, (0, Cp - C)))[:, :, :C]
        return apply(x)

    def gat_fused(self, index, el, er, x, negative_slope=0.2, num_nodes=None, dropout_rate=0.0, training=True,
                  out_dtype=None):
        """out[i,h,:] = sum_{j->i} dropout(softmax_i(LeakyReLU(el[j,h] + er[i,h]))) * x[j,h,:]
        (dropout on the attention coefficients as gat_conv.py:104 / GATConvFuse(..., dropout_rate)).
        x may be STORED as bf16 / f16 (an extension; el / er stay f32): the softmax and the sums are the f32 op's on the
        widened rows, out is rounded once to x's dtype, or returned unrounded with out_dtype=torch.float32."""
        self._dev(index, el, er, x)
        for n, t in (("el", el), ("er", er)):
            self._check_f32(n, t)
        self._check_f32_or_x16("x", x)
        out_dtype = self._out_dtype(x, out_dtype)
        n = x.shape[0] if num_nodes is None else num_nodes
        gp = index if isinstance(index, GraphPlan) else self.graph_plan(index, n, x.shape[0])
        p = float(dropout_rate) if training else 0.0
        if not 0.0 <= p < 1.0:
            raise ValueError("dropout_rate must be in [0, 1)")
        return self._head_padded(gp, x, lambda xp: autograd.GATFused.apply(
            self, gp, el.contiguous(), er.contiguous(), xp.contiguous(), negative_slope, p, out_dtype))

    def _attn_plan(self, op, index, num_nodes, src, dst, dropout_rate, training):
        """(gp, p) of a logit attention op: `index` as a GraphPlan over (num_nodes, or dst's rows) destinations and src's rows
        sources, its rows checked against `dst` and `src` — (name, tensor) pairs, dst None where no tensor has a row per
        destination — and the attention dropout rate actually applied: 0 outside training, else dropout_rate in [0, 1)."""
        rows = (dst or src)[1].shape[0]
        n = rows if num_nodes is None else num_nodes
        gp = index if isinstance(index, GraphPlan) else self.graph_plan(index, n, src[1].shape[0])
        if dst is not None and (gp.N_dst != rows or gp.N_src != src[1].shape[0]):
            raise RuntimeError(f"{op}: the graph has {gp.N_dst} destinations and {gp.N_src} sources, {dst[0]} has "
                               f"{rows} rows and {src[0]} {src[1].shape[0]}")
        p = float(dropout_rate) if training else 0.0
        if not 0.0 <= p < 1.0:
            raise ValueError("dropout_rate must be in [0, 1)")
        return gp, p

    @staticmethod
    def _attn_leaves(*ts):
        """contiguous inputs; detached when nothing will run backward, so that no logits are kept (or, fused, formed) for it"""
        if not torch.is_grad_enabled():
            ts = [t.detach() for t in ts]
        return [t.contiguous() for t in ts]

    def edge_softmax_aggregate(self, index, logits, x, num_nodes=None, dropout_rate=0.0, training=True):
        """out[i,h,:] = sum_{e->i} dropout(softmax_i(logits[:,h]))[e] * x[src_e,h,:] in one kernel per direction
        (ggl_edge_softmax_agg_*): gat_fused with the logit of every edge GIVEN — `logits` [E, H] f32 in the order of
        `index`'s columns, used as they are — instead of built from el / er; what agnn_conv.py:54-66 and every layer that
        calls segment_softmax on its logits and sums alpha * x[src] compose from three ops.  `index` [2, E] or a GraphPlan;
        x [N_src, H, C] f32; logits [E] with x [N_src, K] are one head.  Gradients for logits and x."""
        if logits.dim() == 1 and x.dim() == 2:
            return self.edge_softmax_aggregate(index, logits.unsqueeze(1), x.unsqueeze(1), num_nodes, dropout_rate,
                                               training).squeeze(1)
        self._dev(index, logits, x)
        self._check_f32("logits", logits)
        self._check_f32("x", x)
        gp, p = self._attn_plan("edge_softmax_aggregate", index, num_nodes, ("x", x), None, dropout_rate, training)
        if x.dim() != 3 or logits.dim() != 2 or logits.shape[0] != gp.E or logits.shape[1] != x.shape[1]:
            raise RuntimeError(f"edge_softmax_aggregate expects logits [E, H] and x [N_src, H, C]: got logits "
                               f"{tuple(logits.shape)}, x {tuple(x.shape)} for {gp.E} edges")
        return self._head_padded(gp, x, lambda xp: autograd.EdgeSoftmaxAgg.apply(
            self, gp, logits.contiguous(), xp.contiguous(), p))

    def dot_attention(self, index, q, k, v, num_nodes=None, scale=None, dropout_rate=0.0, training=True,
                      return_logits=False):
        """Scaled dot-product graph attention (hgt_conv.py:115-153, every graph-transformer layer):
        out[i,h,:] = sum_{e->i} dropout(softmax_i(z[:,h]))[e] * v[src_e,h,:] with z[e,h] = scale * <q[dst_e,h,:], k[src_e,h,:]>.
        q [N_dst, H, C], k and v [N_src, H, C] f32 (q [N, C] with k, v [N, C] are one head); `scale` a float, 1/sqrt(C) by
        default; a per-head factor (HGT's p_rel) belongs on q.  `index` [2, E] or a GraphPlan; rectangular graphs, empty rows,
        dropout and `training` as edge_softmax_aggregate.  On the GPU the dot is formed inside the aggregate's walk
        (ggl_dot_attn_fwd) for C = 8, 16, 32, 64; other widths and CPU tensors compose the edge dot with
        edge_softmax_aggregate.  Either way everything behind z is edge_softmax_aggregate on (z, v), bit for bit, and z is
        stored only for a backward.  Gradients for q, k and v.  return_logits=True returns (out, z), z [E, H] in the order
        of `index`'s columns, detached."""
        if q.dim() == 2 and k.dim() == 2 and v.dim() == 2:
            r = self.dot_attention(index, q.unsqueeze(1), k.unsqueeze(1), v.unsqueeze(1), num_nodes, scale, dropout_rate,
                                   training, return_logits)
            return (r[0].squeeze(1), r[1].squeeze(1)) if return_logits else r.squeeze(1)
        self._dev(index, q, k, v)
        for name, t in (("q", q), ("k", k), ("v", v)):
            self._check_f32(name, t)
        if q.dim() != 3 or k.dim() != 3 or v.dim() != 3 or k.shape[0] != v.shape[0] or k.shape[1:] != q.shape[1:] \
                or v.shape[1] != q.shape[1]:
            raise RuntimeError(f"dot_attention expects q [N_dst, H, C] and k, v [N_src, H, C]: got q {tuple(q.shape)}, "
                               f"k {tuple(k.shape)}, v {tuple(v.shape)}")
        if v.shape[2] != q.shape[2]:
            raise RuntimeError(f"dot_attention needs v of k's head width (Cv == C): got C = {q.shape[2]}, Cv = {v.shape[2]}")
        gp, p = self._attn_plan("dot_attention", index, num_nodes, ("k", k), ("q", q), dropout_rate, training)
        sc = 1.0 / math.sqrt(q.shape[2]) if scale is None else float(scale)
        out, z = autograd.DotAttention.apply(self, gp, *self._attn_leaves(q, k, v), sc, p, bool(return_logits))
        return (out, z) if return_logits else out

    def gatv2_attention(self, index, xl, xr, att, num_nodes=None, negative_slope=0.2, dropout_rate=0.0, training=True,
                        return_logits=False):
        """GATv2's additive graph attention ("How Attentive are Graph Attention Networks?"):
        out[i,h,:] = sum_{e->i} dropout(softmax_i(z[:,h]))[e] * xl[src_e,h,:] with
        z[e,h] = sum_c att[h,c] * LeakyReLU(xl[src_e,h,c] + xr[dst_e,h,c]) — the LeakyReLU inside the channel sum.
        xl [N_src, H, C], xr [N_dst, H, C], att [H, C] f32 (2-d xl, xr with 1-d att are one head).  `index` [2, E] or a
        GraphPlan; rectangular graphs, empty rows, dropout and `training` as edge_softmax_aggregate.  On the GPU the logit
        is formed inside the aggregate's walk (ggl_gatv2_fwd) for C = 8, 16, 32, 64; other widths, CPU tensors and
        `gatv2_fused = False` form z with torch in edge blocks in front of edge_softmax_aggregate's forward.  Either way
        everything behind z is edge_softmax_aggregate on (z, xl), bit for bit, z is stored only for a backward, and no
        [E, H, C] array is kept.  Gradients for xl, xr and att (ggl_gatv2_logit_bwd).  return_logits=True returns (out, z),
        z [E, H] in the order of `index`'s columns, detached."""
        if xl.dim() == 2 and xr.dim() == 2 and att.dim() == 1:
            r = self.gatv2_attention(index, xl.unsqueeze(1), xr.unsqueeze(1), att.unsqueeze(0), num_nodes, negative_slope,
                                     dropout_rate, training, return_logits)
            return (r[0].squeeze(1), r[1].squeeze(1)) if return_logits else r.squeeze(1)
        self._dev(index, xl, xr, att)
        for name, t in (("xl", xl), ("xr", xr), ("att", att)):
            self._check_f32(name, t)
        if xl.dim() != 3 or xr.dim() != 3 or xl.shape[1:] != xr.shape[1:]:
            raise RuntimeError(f"gatv2_attention expects xl [N_src, H, C] and xr [N_dst, H, C]: got xl {tuple(xl.shape)}, "
                               f"xr {tuple(xr.shape)}")
        if att.dim() != 2 or att.shape != xl.shape[1:]:
            raise RuntimeError(f"gatv2_attention expects att [H, C] = {tuple(xl.shape[1:])}: got {tuple(att.shape)}")
        gp, p = self._attn_plan("gatv2_attention", index, num_nodes, ("xl", xl), ("xr", xr), dropout_rate, training)
        out, z = autograd.GATv2Attention.apply(self, gp, *self._attn_leaves(xl, xr, att), float(negative_slope), p,
                                               bool(return_logits))
        return (out, z) if return_logits else out

    def _check_weight(self, weight, gp):
        """An edge-weight vector handed to a kernel as a raw pointer: f32 (spmm_sum_cpu.cpp:22 would raise
        "expected scalar type Float"), one value per edge."""
        if weight is None:
            return None
        self._check_f32("weight", weight)
        if weight.numel() != gp.E:
            raise RuntimeError(f"edge weight must hold one value per edge: got {tuple(weight.shape)} for "
                               f"{gp.E} edges")
        return weight.reshape(-1).contiguous()

    # rectangular / explicit-plan variants used by the harness and the multi-GPU layer
    def spmm(self, gp, weight, x, reduce="sum", out_dtype=None):
        """sum / mean also take bf16 / f16 rows (f32 arithmetic, the result rounded once to x's dtype, or returned as
        f32 with out_dtype=torch.float32 — a last layer's logits); max is f32 only."""
        self._dev(x, weight)
        (self._check_f32 if reduce == "max" else self._check_f32_or_x16)("x", x)
        weight = self._check_weight(weight, gp)
        fn = {"sum": autograd.SpMMSum, "mean": autograd.SpMMMean, "max": autograd.SpMMMax}[reduce]
        if reduce == "max":
            if out_dtype not in (None, x.dtype):
                raise RuntimeError("spmm(max) returns x's dtype")
            return fn.apply(self, gp, weight, x.contiguous())
        return fn.apply(self, gp, weight, x.contiguous(), self._out_dtype(x, out_dtype))

    def colsum(self, g):
        """out[k] = sum_r g[r, k] for a row-major f32 [N, K] matrix (deterministic two-stage kernel)."""
        dev = self._dev(g)
        self._check_f32("g", g)
        g = g.contiguous()
        N, K = self._rows_cols(g)
        out = torch.empty(tuple(g.shape[1:]), dtype=torch.float32, device=dev)
        wsb = self.lib.ggl_colsum_workspace_bytes(N, K)
        ws = torch.empty(max(wsb, 4), dtype=torch.uint8, device=dev)
        self._check(self.lib.ggl_colsum_f32(_ptr(g), N, K, _ptr(out), _ptr(ws), wsb, self._stream(dev)))
        return out

    def bias_add(self, x, bias):
        """x + bias with the bias gradient computed by ggl_colsum_f32 (gcn_conv.py:105-106)."""
        return autograd.BiasAdd.apply(self, x, bias)

    def _rng_state(self, dev):
        """Device-resident Philox state {seed, offset} for the fused dropout, seeded from torch's RNG."""
        st = self._rng.get(str(dev))
        if st is None:
            seed = int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())  # follows torch.manual_seed
            st = torch.tensor([seed, 0], dtype=torch.int64, device=dev)
            self._rng[str(dev)] = st
        return st

    def _draw(self, dev, p_drop):
        """One fused-dropout draw on `dev`: (rng, rng_used) — the device state the launch reads and then advances by one,
        and a clone of the {seed, offset} it reads, which the backward is handed to redraw the mask.  (None, None) at
        rate 0: nothing is drawn and the state does not move."""
        if not p_drop > 0:
            return None, None
        rng = self._rng_state(dev)
        return rng, rng.clone()

    @staticmethod
    def _rows_cols(t):
        """(N, K) of a row-major [N, ...] tensor walked as an [N, K] matrix."""
        N = int(t.shape[0])
        return N, (t.numel() // N if N > 0 else int(math.prod(t.shape[1:])))

    def _epi_fwd(self, a, bias, relu, p_drop, rng):
        """y = dropout(relu(a + bias)) of a contiguous f32 `a` in one kernel (ggl_bias_act_fwd); `rng` from _draw.
        A bf16 / f16 `a` takes ggl_bias_act_fwd_x16: the same f32 operations and words, y rounded once to a's dtype."""
        N, K = self._rows_cols(a)
        y = torch.empty_like(a)
        b = bias.contiguous().reshape(-1) if bias is not None else None
        if a.dtype in _X16_DTYPES:
            self._check(self.lib.ggl_bias_act_fwd_x16(_DTYPE_CODE[a.dtype], _ptr(a), _ptr(b), N, K, int(relu), float(p_drop),
                                                      _ptr(rng), _ptr(y), self._stream(a.device)))
            return y
        self._check(self.lib.ggl_bias_act_fwd(_ptr(a), _ptr(b), N, K, int(relu), float(p_drop), _ptr(rng), _ptr(y),
                                              self._stream(a.device)))
        return y

    def _epi_bwd(self, g, y, relu, p_drop, rng_used, bias_shape):
        """Back through dropout / ReLU / + bias (/ + add) in one pass (ggl_bias_act_bwd): the mask is redrawn from
        `rng_used` (the forward's _draw) and the ReLU read off the saved output `y`.  Returns (ga, gbias), gbias in
        `bias_shape` or None without a bias; g itself when there is nothing to undo.  bf16 / f16 g and y (the
        forward's dtype) take ggl_bias_act_bwd_x16: ga in that dtype, gbias f32 and never rounded."""
        g = g.contiguous()
        if not (relu or p_drop > 0 or bias_shape is not None):
            return g, None
        if g.dtype != y.dtype:
            raise RuntimeError(f"expected scalar type Float: the gradient ({g.dtype}) must have the output's dtype ({y.dtype})")
        dev = g.device
        N, K = self._rows_cols(g)
        ga = torch.empty_like(g)
        gb = torch.empty(K, dtype=torch.float32, device=dev) if bias_shape is not None else None
        wsb = self.lib.ggl_bias_act_bwd_workspace_bytes(N, K)
        ws = torch.empty(max(wsb, 4), dtype=torch.uint8, device=dev)
        if g.dtype in _X16_DTYPES:
            self._check(self.lib.ggl_bias_act_bwd_x16(_DTYPE_CODE[g.dtype], _ptr(g), _ptr(y), N, K, int(relu), float(p_drop),
                                                      _ptr(rng_used), _ptr(ga), _ptr(gb), _ptr(ws), wsb, self._stream(dev)))
        else:
            self._check(self.lib.ggl_bias_act_bwd(_ptr(g), _ptr(y), N, K, int(relu), float(p_drop), _ptr(rng_used),
                                                  _ptr(ga), _ptr(gb), _ptr(ws), wsb, self._stream(dev)))
        return ga, (gb.reshape(bias_shape) if gb is not None else None)

    def linear_epi_bwd(self, g, w, y, relu, p_drop, rng_used, bias_shape):
        """`_epi_bwd(g[:, :J] @ w, y, ...)` without the [N, K] product in memory (ggl_linear_bias_act_bwd): `g` [N, >= J] f32
        rows (the output layer's gradient, 47 classes in rows of 48), `w` the [J, K] Linear weight, `y` the saved [N, K]
        output.  The product is summed in ascending j with fused multiply-adds, not in a BLAS order; everything behind it
        is _epi_bwd's on the bits.  Shapes ggl_policy_linear_epi_bwd accepts only.  Returns (ga, gbias)."""
        g, w, y = g.contiguous(), w.contiguous(), y.contiguous()
        self._check_f32("g", g)
        self._check_f32("w", w)
        self._check_f32("y", y)
        dev = g.device
        N, J, K = int(g.shape[0]), int(w.shape[0]), int(w.shape[1])
        if g.dim() != 2 or g.shape[1] < J or tuple(y.shape) != (N, K):
            raise RuntimeError(f"linear_epi_bwd: g {tuple(g.shape)}, w {tuple(w.shape)}, y {tuple(y.shape)} do not fit")
        ga = torch.empty_like(y)
        gb = torch.empty(K, dtype=torch.float32, device=dev) if bias_shape is not None else None
        wsb = self.lib.ggl_bias_act_bwd_workspace_bytes(N, K)
        ws = torch.empty(max(wsb, 4), dtype=torch.uint8, device=dev)
        self._check(self.lib.ggl_linear_bias_act_bwd(_ptr(g), int(g.shape[1]), _ptr(w), _ptr(y), N, J, K, int(relu), float(p_drop),
                                                     _ptr(rng_used), _ptr(ga), _ptr(gb), _ptr(ws), wsb, self._stream(dev)))
        return ga, (gb.reshape(bias_shape) if gb is not None else None)

    def reseed(self, seed=None):
        """Forget the fused-dropout RNG state (the next use draws a new seed from torch's generator) — of this engine AND, for
        a product engine, of the C++ operator library (torch.ops.ggl keeps its own counter stream; since round 6 a one-rank
        training step takes that route, dist._default_route, so a reseed that skipped it was no reseed)."""
        self._rng.clear()
        if getattr(self, "is_product", False):
            from . import cpp_ops

            if cpp_ops._loaded:
                torch.ops.ggl.reseed()
        if seed is not None:
            torch.manual_seed(seed)

    def bias_act(self, a, bias=None, relu=False, p_drop=0.0, training=True):
        """dropout(relu(a + bias)) — the step after every aggregate (gcn_conv.py:105-106, models/gcn.py:55-59).
        `a` f32, or bf16 / f16 storage (f32 arithmetic, the result rounded once to a's dtype); `bias` stays f32."""
        self._dev(a, bias)
        self._check_f32_or_x16("a", a)
        if bias is not None:
            self._check_f32("bias", bias)
        p = float(p_drop) if training else 0.0
        return autograd.BiasAct.apply(self, a, bias, bool(relu), p)

    def spmm_bias_act(self, gp, weight, x, bias=None, relu=False, p_drop=0.0, training=True):
        """dropout(relu(A x + bias)) for a GraphPlan `gp` (what GCNConv + the model's ReLU/dropout compute,
        gcn_conv.py:78-108, models/gcn.py:55-59).  One kernel when the feature width is a multiple of 4
        (16-byte rows); otherwise the SpMM and the epilogue kernel run back to back — same values."""
        return self.spmm_epi(gp, weight, x, "sum", None, bias, relu, p_drop, training)

    def spmm_epi(self, gp, weight, x, reduce="sum", add=None, bias=None, relu=False, p_drop=0.0, training=True,
                 out_dtype=None):
        """dropout(relu(reduce_{j->i} w x_j + add_i + bias)), reduce in {'sum', 'mean'}: one kernel for 16-byte
        rows (feature width a multiple of 4), the reduce op followed by the adds and the epilogue pass otherwise.
        bf16 / f16 `x` (with `add` in x's dtype; weight and bias stay f32): every operation is the f32 one on the widened
        rows and the result is rounded once, at the store — or returned as f32 with out_dtype=torch.float32; one kernel
        at every width."""
        self._dev(x, weight, bias, add)
        self._check_f32_or_x16("x", x)
        weight = self._check_weight(weight, gp)
        if bias is not None:
            self._check_f32("bias", bias)
        if add is not None and add.dtype != x.dtype:
            raise RuntimeError(f"expected scalar type Float (add in x's dtype, {x.dtype}) but found {add.dtype} for add")
        out_dtype = self._out_dtype(x, out_dtype)
        if add is not None and tuple(add.shape) != (gp.N_dst, x.shape[1]):
            raise RuntimeError("add must be [destination rows, feature width]")
        p = float(p_drop) if training else 0.0
        if x.dtype in _X16_DTYPES:
            if x.dim() != 2:
                raise RuntimeError("spmm_epi on bf16 / f16 rows expects x of shape [num_nodes, features]")
            return autograd.SpMMEpi.apply(self, gp, weight, x.contiguous(), reduce == "mean", add, bias, bool(relu), p,
                                          out_dtype)
        if x.dim() == 2 and x.shape[1] % 4 == 0:
            return autograd.SpMMEpi.apply(self, gp, weight, x.contiguous(), reduce == "mean", add, bias, bool(relu), p)
        out = self.spmm(gp, weight, x, reduce)
        if add is not None:
            out = out + add
        return autograd.BiasAct.apply(self, out, bias, bool(relu), p)

    def segment_epi(self, msg, ids, N, reduce="mean", add=None, bias=None, relu=False):
        """relu(segment_{sum,mean}(msg, ids, N) + add + bias) for f32 messages [E, K] — one kernel."""
        self._dev(msg, ids, bias, add)
        self._check_f32("msg", msg)
        msg, ids, N = self._seg_args(msg, ids, N)
        if msg.dim() != 2:
            raise RuntimeError("segment_epi expects [E, K] messages")
        for n, t in (("bias", bias), ("add", add)):
            if t is not None:
                self._check_f32(n, t)
        if add is not None and tuple(add.shape) != (N, msg.shape[1]):
            raise RuntimeError("add must be [num_segments, feature width]")
        return autograd.SegmentEpi.apply(self, msg, ids, N, reduce == "mean", add, bias, bool(relu))

    def gat_headmean_supported(self, heads, in_channels, out_channels):
        return bool(self.gat_fast and self.lib.ggl_gat_sh_supported(int(heads), int(in_channels), int(out_channels)))

    def gat_headmean(self, index, x, W, att, negative_slope=0.2, num_nodes=None, dropout_rate=0.0, training=True):
        """mean over the 8 heads of a GAT layer's output (before the bias): [N, C] from x [N, F], W [F, 8 C],
        att [1, 8, 2 C] — the layer aggregated before it is transformed (see GATHeadMean)."""
        self._dev(index, x, W, att)
        for n, t in (("x", x), ("W", W), ("att", att)):
            self._check_f32(n, t)
        n = x.shape[0] if num_nodes is None else int(num_nodes)
        if n != x.shape[0]:
            raise RuntimeError("gat_headmean runs on square graphs (every destination is also a source row)")
        gp = index if isinstance(index, GraphPlan) else self.graph_plan(index, n, n)
        p = float(dropout_rate) if training else 0.0
        return autograd.GATHeadMean.apply(self, gp, x.contiguous(), W.contiguous(), att.contiguous(), negative_slope, p)

    def block_mean_epi(self, x, blk, add=None, bias=None, relu=False):
        """SAGEConv(mean) over a sampler Block: relu(mean of the sampled neighbours + add + bias), one kernel."""
        self._dev(x, add, bias)
        self._check_f32("x", x)
        return autograd.BlockMeanEpi.apply(self, x.contiguous(), blk, add, bias, bool(relu))

    def set_option(self, name, value):
        self._check(self.lib.ggl_set_option(name.encode(), int(value)))

    def time_spmm_sum(self, gp, weight, x, reps=10):
        """Average ms per launch of the dominant SpMM-sum kernel (hipEvents on the current stream)."""
        dev = x.device
        K = int(math.prod(x.shape[1:]))
        out = torch.empty((gp.N_dst,) + tuple(x.shape[1:]), dtype=torch.float32, device=dev)
        part = self._partial(gp.fwd, torch.float32, K, False, dev)
        cs = gp.fwd.c_struct(part)
        if gp.fwd.order_fn is not None:
            # a plan's row hand-out order is computed on its SECOND launch (SegPlan.c_struct); the kernel is timed the way a training
            # step runs it — on a plan that comes back.  (Round 6: with the step on torch.ops.ggl this engine's plan can arrive
            # here unused; without the order the products aggregate measured 23.7 instead of 13.5 ms.)
            cs = gp.fwd.c_struct(part)
        ms = ctypes.c_float(0.0)
        w_by_pos = 0
        if weight is not None and gp.fwd.perm is not None:
            self._sorted_weights(gp.fwd, weight)  # a reused weight vector: timed the way the step runs it
            weight, w_by_pos = self._sorted_weights(gp.fwd, weight)
        self._check(self.lib.ggl_time_spmm_sum(ctypes.byref(cs), _ptr(gp.col), _ptr(weight), w_by_pos, _ptr(x),
                                               K, _ptr(out), self._stream(dev), int(reps),
                                               ctypes.byref(ms)))
        return float(ms.value)
