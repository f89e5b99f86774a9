"""The plans of the MI355X message-passing backend: what is sorted once per edge list and handed to every launch.

* ``SegPlan``    : perm / rowptr / long-row lists for one id vector (struct ggl_segplan + the tensors that own it).  ONE
                   constructor sets every slot; the builders (Engine.build_plan, Engine.plan_from_rowptr, sampler.Block)
                   pass what they know.
* ``GraphPlan``  : the pair of SegPlans (by destination, by source) for one ``edge_index`` plus the int32 column arrays —
                   CSR for the forward SpMM, CSC for its backward.
* ``RowsPlan``   : a GraphPlan cut down to a list of destination rows (Engine.rows_plan).
* ``_PlanCache`` : the LRU the Engine keeps them in, keyed on the identity + version counter of the id tensor's storage.
"""
import os
from collections import OrderedDict

import torch
from torch.multiprocessing.reductions import StorageWeakRef

from ._lib import SegPlanC


class SegPlan:
    """Destination-sorted view of one id vector (struct ggl_segplan + the tensors that own it).

    Every slot is set here; what a builder does not pass decides what the kernels are handed:

    * no `order_fn` (a sampler Block): the plan never gets a row order, so nothing is allocated during a hipGraph capture;
    * no `hub_first` (every plan but Engine.build_plan's): `xcd_run_rows` is never reported as -1;
    * `wperm` is set only on the CSC side of a CSR-built GraphPlan (GraphPlan.from_csr), `xcd_run` by GraphPlan._schedule;
    * `uid` > 0 only for plans an Engine counted: the key of its sorted-weight cache."""

    __slots__ = ("N", "E", "rowptr", "perm", "is_sorted", "max_len", "chunk", "long_rows", "chunk_ptr", "n_long", "n_chunks",
                 "device", "row_order", "uid", "xcd_run", "order_fn", "uses", "wperm", "long_order", "hub_first")

    def __init__(self, N, E, rowptr, chunk, max_len, device, perm=None, is_sorted=True, n_long=0, n_chunks=0, long_rows=None,
                 chunk_ptr=None, long_order=None, row_order=None, order_fn=None, uses=0, xcd_run=0, hub_first=False,
                 wperm=None, uid=-1):
        self.N, self.E, self.rowptr, self.chunk, self.max_len, self.device = int(N), int(E), rowptr, int(chunk), int(max_len), device
        self.perm, self.is_sorted = perm, is_sorted
        self.n_long, self.n_chunks, self.long_rows, self.chunk_ptr, self.long_order = n_long, n_chunks, long_rows, chunk_ptr, long_order
        self.row_order, self.order_fn, self.uses = row_order, order_fn, uses
        self.xcd_run, self.hub_first, self.wperm, self.uid = xcd_run, hub_first, wperm, uid

    def c_struct(self, partial=None, perm_override=None, unsplit=False, skip_long=False):
        """`unsplit`: present the plan without its long-row table, every row walked in one piece.
        `skip_long`: withhold the long-row table but keep the threshold — rows longer than `chunk` are left out
        of the launch (ggl_segment_hub16 fills them in)."""
        perm = self.perm if perm_override is None else perm_override
        n_long = 0 if (unsplit or skip_long) else self.n_long
        lo = self.long_order
        fn = self.order_fn
        if fn is not None:
            # the row hand-out order is a scheduling aid worth ~100 us of sorting: a plan that is used ONCE (a fresh
            # edge list per mini-batch) never pays for it, a plan that comes back gets it on its second launch
            self.uses += 1
            # never while a hipGraph is being recorded: the argsort would be allocated in the capture pool and only
            # FILLED on replay, and an eager launch of this plan before the first replay would read garbage row ids
            if self.uses >= 2 and not (self.rowptr.is_cuda and torch.cuda.is_current_stream_capturing()):
                self.order_fn = None
                self.row_order = fn(self.counts())
        return SegPlanC(
            rowptr=self.rowptr.data_ptr(), perm=(perm.data_ptr() if perm is not None else None),
            long_rows=(self.long_rows.data_ptr() if n_long else None),
            chunk_ptr=(self.chunk_ptr.data_ptr() if n_long else None),
            n_long=n_long, n_chunks=(self.n_chunks if n_long else 0),
            chunk=((1 << 62) if unsplit else self.chunk),
            partial=(partial.data_ptr() if partial is not None else None),
            partial_bytes=(partial.numel() * partial.element_size() if partial is not None else 0), N=self.N, E=self.E,
            row_order=(self.row_order.data_ptr() if self.row_order is not None else None),
            # > 0: XCD runs (a node order with locality); -1: no runs, but the long rows LEAD the id range (a degree-sorted
            # order): the hub walk of a column-blocked aggregate then runs once over the full width (include/ggl_mpops.h)
            xcd_run_rows=(self.xcd_run or (-1 if (n_long and self.hub_first) else 0)),
            long_order=(lo.data_ptr() if (n_long and lo is not None) else None),
            max_len=self.max_len)

    def counts(self):
        return self.rowptr[1:] - self.rowptr[:-1]


class GraphPlan:
    """CSR (rows = destination) and, lazily, CSC (rows = source) plans of one edge_index."""

    __slots__ = ("engine", "index", "N_dst", "N_src", "E", "fwd", "col", "_bwd", "_colT", "_posT", "_rowidx", "aux")

    def __init__(self, engine, index, n_dst, n_src):
        self.engine = engine
        self.index = index
        self.N_dst, self.N_src = int(n_dst), int(n_src)
        self.E = int(index.shape[1])
        # shared with the segment-op cache: degree(dst) / unsorted_segment_*(.., edge_index[1], N)
        # on the same edge list reuse this very plan (and vice versa)
        self.fwd = engine.seg_plan(index[1], self.N_dst)
        engine._check_range(index[0], self.N_src)
        self.col = engine.gather_i32(index[0], self.fwd.perm)
        self._bwd = self._colT = self._posT = self._rowidx = None
        self.aux = {}  # graph-constant tensors callers derive from this edge list (e.g. GCN edge norms)
        self._schedule()

    @classmethod
    def from_csr(cls, engine, row_ptr, col_ind, col_ptr, row_ind, permute, n_rows, n_cols):
        """A GraphPlan from structures the caller already holds, no sort: the CSR of the aggregating rows
        (`row_ptr` [n_rows + 1], `col_ind` [E]: the nodes each row gathers from), its transpose (`col_ptr` [n_cols + 1],
        `row_ind` [E]) and `permute` [E] = the CSR position of every CSC entry — the five tensors FusedGATConv takes as
        keyword arguments (fusedgat_conv.py:95-100) and otherwise rebuilds on the host in every forward (:102-117)."""
        gp = cls.__new__(cls)
        gp.engine, gp.index = engine, None
        gp.N_dst, gp.N_src, gp.E = int(n_rows), int(n_cols), int(col_ind.shape[0])
        for nm, t, n in (("row_ptr", row_ptr, gp.N_dst + 1), ("col_ptr", col_ptr, gp.N_src + 1), ("col_ind", col_ind, gp.E),
                         ("row_ind", row_ind, gp.E), ("permute", permute, gp.E)):
            if t.dim() != 1 or int(t.shape[0]) != n or t.dtype not in (torch.int32, torch.int64):
                raise RuntimeError(f"{nm} must be a 1-D int32 / int64 tensor of {n} elements, got {tuple(t.shape)} {t.dtype}")
        engine._dev(row_ptr, col_ind, col_ptr, row_ind, permute)
        engine._check_range(col_ind, gp.N_src)
        engine._check_range(row_ind, gp.N_dst)
        engine._check_range(permute, max(gp.E, 1))
        for nm, ptr in (("row_ptr", row_ptr), ("col_ptr", col_ptr)):   # one-off (per plan) host reads
            if int(ptr[0]) != 0 or int(ptr[-1]) != gp.E or (ptr.numel() > 1 and bool((ptr[1:] < ptr[:-1]).any())):
                raise RuntimeError(f"{nm} must rise from 0 to the number of edges ({gp.E})")
        def own_i32(t):   # the plan keeps ITS OWN int32 copy: a later in-place edit of the caller's tensor cannot reach it
            return t.to(torch.int32).contiguous() if t.dtype != torch.int32 else t.clone().contiguous()

        gp.fwd = engine.plan_from_rowptr(row_ptr.clone() if row_ptr.dtype == torch.int64 else row_ptr, gp.E)
        gp.col = own_i32(col_ind)
        gp._bwd = engine.plan_from_rowptr(col_ptr.clone() if col_ptr.dtype == torch.int64 else col_ptr, gp.E)
        gp._colT = own_i32(row_ind)
        gp._posT = own_i32(permute)
        # edge weights arrive in CSR order: the transposed walk reads them through `permute` (a COO-built plan's CSC side
        # carries the original edge id of every position in its own `perm` instead)
        gp._bwd.wperm = gp._posT
        gp._rowidx = None
        gp.aux = {}
        gp._schedule()
        return gp

    def locality(self, samples=1 << 16):
        """Share of the edges (a strided sample) whose two endpoints lie within N / 64 ids of each other: ~3 % for
        randomly labelled nodes, 30-40 % for degree-sorted power-law graphs (hub-to-hub edges), 70 %+ when the order
        comes from a clustering (partition.cluster_order) or from the data itself.  One host read."""
        E, N = self.E, max(self.N_dst, self.N_src)
        if E == 0 or self.N_dst != self.N_src:
            return 0.0
        S = min(int(samples), E)
        pos = torch.arange(S, device=self.col.device, dtype=torch.int64) * (E // S)
        rows = torch.searchsorted(self.fwd.rowptr, pos, right=True) - 1
        near = (self.col[pos].long() - rows).abs() < max(N // 64, 4096)
        return float(near.float().mean())

    def _schedule(self):
        """Scheduling hint for the row kernels (results identical either way): on a graph whose node order carries
        locality every XCD gets RUNS of consecutive row slots (SegPlan.xcd_run -> ggl_segplan.xcd_run_rows), so that a
        neighbourhood's source rows are fetched into ONE private L2 instead of all eight — measured on the
        products-sized planted-community graph in cluster order: K = 256 aggregate 13.4 -> 10.9 ms, K = 64
        3.31 -> 2.62 ms; on randomly labelled or degree-sorted R-MAT the same mapping LOSES 7-8 % (nothing to keep,
        and runs of heavy rows unbalance the XCDs), hence the test (profiles/r3_xcd_run_swizzle.txt)."""
        eng = self.engine
        run = int(eng.xcd_run_rows)
        if run < 0:       # automatic: the library's rule on this plan's locality (locality() is one host read)
            need = int(eng.lib.ggl_policy_xcd_run_rows(self.E, 1.0)) > 0 or int(eng.lib.ggl_policy_xcd_run_rows(self.E, 0.0)) > 0
            run = int(eng.lib.ggl_policy_xcd_run_rows(self.E, self.locality() if need else 0.0))
        self.fwd.xcd_run = run
        if self._bwd is not None:
            self._bwd.xcd_run = run

    @property
    def rowidx(self):
        """destination node of every sorted position (int32 [E]): the row each element of the forward walk belongs
        to, for walks that run flat over positions instead of row by row (ggl_bspmm_grad_w_sorted)."""
        if self._rowidx is None:
            if self.index is not None:
                self._rowidx = self.engine.gather_i32(self.index[1], self.fwd.perm)
            else:
                self._rowidx = torch.repeat_interleave(
                    torch.arange(self.N_dst, device=self.fwd.rowptr.device, dtype=torch.int32), self.fwd.counts())
        return self._rowidx

    @property
    def bwd(self):
        if self._bwd is None:
            self._bwd = self.engine.seg_plan(self.index[0], self.N_src)
            self._colT = self.engine.gather_i32(self.index[1], self._bwd.perm)
            self._bwd.xcd_run = self.fwd.xcd_run
        return self._bwd

    @property
    def colT(self):
        self.bwd  # noqa: B018
        return self._colT

    @property
    def posT(self):
        """transposed sorted position -> forward sorted position (int32 [E])."""
        if self._posT is None:
            E, dev = self.E, self.index.device
            ar = torch.arange(E, device=dev, dtype=torch.int32)
            pf = self.fwd.perm if self.fwd.perm is not None else ar
            pt = self.bwd.perm if self.bwd.perm is not None else ar
            inv = torch.empty(E, device=dev, dtype=torch.int32)
            inv[pf.long()] = ar
            self._posT = inv[pt.long()].contiguous()
        return self._posT


class RowsPlan:
    """A GraphPlan cut down to a sorted list of destination rows (Engine.rows_plan): `fwd` R x N_src and `bwd` N_src x R
    SegPlans with their column arrays and the edge weights in sorted order.  `w_ref`: the weight tensor's storage (an
    entry whose weights died is a miss: the address may have been handed to another tensor)."""

    __slots__ = ("R", "N_dst", "N_src", "rows", "fwd", "col", "w_fwd", "bwd", "colT", "w_bwd", "w_ref")


class _PlanCache:
    """LRU keyed on the identity of the id tensor's storage + its version counter, bounded by entry count AND
    by the bytes its plans hold (a products-sized GraphPlan is ~2.5 GB of HBM: a caller that builds a fresh
    edge_index every epoch must not accumulate 16 of them).  An entry dies with its id tensor's storage.

    Identity + version cannot see a mutation made behind autograd's back (`.data`, numpy-shared memory): set
    GGL_VERIFY_PLANS=1 to keep a (first, last, sum) checksum of the ids with every plan and verify it on each
    hit (one device reduction + a host read per call: a debugging aid, off by default)."""

    def __init__(self, cap=16, max_bytes=None):
        self.cap = cap
        self.max_bytes = int(float(os.environ.get("GGL_PLAN_CACHE_GB", "48")) * 2**30) if max_bytes is None else max_bytes
        self.d = OrderedDict()
        self.bytes = 0
        self.verify = os.environ.get("GGL_VERIFY_PLANS", "0") == "1"

    @staticmethod
    def key(t, extra):
        st = t.untyped_storage()
        return (st._cdata, t.storage_offset(), tuple(t.shape), tuple(t.stride()), t._version,
                t.dtype, str(t.device)) + tuple(extra)

    @staticmethod
    def _checksum(t):
        if t.numel() == 0:
            return (0, 0, 0)
        f = t.reshape(-1)
        return (int(f[0]), int(f[-1]), int(f.sum()))

    @staticmethod
    def _nbytes(val):
        """HBM held by a cached value (SegPlan / GraphPlan / tensor), for the byte bound."""
        if isinstance(val, SegPlan):   # the common miss (a fresh id tensor per mini-batch): no generic walk
            own = sum(t.untyped_storage().nbytes() for t in (val.rowptr, val.perm, val.long_rows, val.chunk_ptr)
                      if t is not None)
            return own + 4 * val.N        # (+ the row order it gets if it is launched again)
        seen, total = set(), 0

        def visit(o, depth=0):
            nonlocal total
            if isinstance(o, torch.Tensor):
                k = o.untyped_storage()._cdata
                if k not in seen:
                    seen.add(k)
                    total += o.untyped_storage().nbytes()
            elif depth < 3 and hasattr(o, "__slots__"):
                for a in o.__slots__:
                    if a not in ("engine", "index"):      # (the caller's own edge_index is not ours to count)
                        visit(getattr(o, a, None), depth + 1)
            elif depth < 3 and isinstance(o, dict):
                for v in o.values():
                    visit(v, depth + 1)

        visit(val)
        return total

    def get(self, t, extra):
        k = self.key(t, extra)
        hit = self.d.get(k)
        if hit is not None:
            ref, val, nb, chk = hit
            if not ref.expired():
                if chk is not None and chk != self._checksum(t):
                    raise RuntimeError("gammagl_amd: an id tensor was modified in place behind its version counter "
                                       "(.data / shared memory) after its plan was cached; call "
                                       "Engine.clear_caches() after such edits")
                self.d.move_to_end(k)
                return val
            self.bytes -= nb
            del self.d[k]
        return None

    def put(self, t, extra, val):
        k = self.key(t, extra)
        old = self.d.pop(k, None)
        if old is not None:
            self.bytes -= old[2]
        nb = self._nbytes(val)
        self.d[k] = (StorageWeakRef(t.untyped_storage()), val, nb, self._checksum(t) if self.verify else None)
        self.bytes += nb
        while len(self.d) > 1 and (len(self.d) > self.cap or self.bytes > self.max_bytes):
            _, (_, _, onb, _) = self.d.popitem(last=False)
            self.bytes -= onb

    def clear(self):
        self.d.clear()
        self.bytes = 0
