"""plan->partial_bytes (ABI 12) through the Engine: every op that hands a hub partial to the kernel library, on a graph with
hub rows in both plans, with Engine._hub_partial replaced by one that returns a view of EXACTLY the bytes the library's own
sizer answers (no slack), 256 bytes into a larger allocation filled with a canary pattern and with 256 canary bytes behind it.
SegPlan.c_struct then declares exactly the library's size.

  pass 1, exact size   : forward and backward return the bits of the unpatched Engine on the same seeded inputs and leave both
                         canary bands intact.  A sizing rule that is too small shows as a damaged canary or as a refusal, and
                         never writes outside an allocation.
  pass 2, a byte short : the same view declared one byte shorter (the memory behind it unchanged and still large enough): the
                         call is refused with the GGL_EWORKSPACE text, the canaries and the view itself keep the pattern —
                         nothing was launched.  Once with every partial short (the forward is refused), once with the forward
                         exact and the backward's partials short (the backward is refused, where it takes a partial).

Not a test module: tests/test_partial_bytes_host.py replays HOST_AND_GPU on the host library, tests/test_gpu_partial_bytes.py
HOST_AND_GPU + GPU_ONLY on the MI355X.  Every case takes well under a second."""
import contextlib
import re

import pytest
import torch

from spmm16_cases import same_bits

N, E, CHUNK = 40, 600, 8          # 40 destination and 40 source rows; chunk 8: rows of 9+ elements are hub rows
HUB_DST, HUB_SRC = 3, 5           # a third of the edges go to one destination, a quarter come from one source
CANARY, BAND = 0xA5, 256
SEED = 20260


def make_graph(dev):
    g = torch.Generator().manual_seed(7)
    dst = torch.randint(0, N, (E,), generator=g)
    src = torch.randint(0, N, (E,), generator=g)
    pick = torch.randperm(E, generator=g)
    dst[pick[:E // 3]] = HUB_DST
    src[pick[-(E // 4):]] = HUB_SRC
    return torch.stack([src, dst]).to(dev)


def rnd(dev, *shape, seed=0, dtype=torch.float32, grad=True, lo=None):
    g = torch.Generator().manual_seed(1000 + seed)
    t = torch.randn(*shape, generator=g) if lo is None else lo + torch.rand(*shape, generator=g)
    t = t.to(dtype).to(dev)
    return t.requires_grad_(True) if grad else t


@contextlib.contextmanager
def engine_state(eng, **attrs):
    """chunk = 8 and the case's switches on the process-wide engine, put back afterwards; `option_*` are library options"""
    attrs = dict(chunk=CHUNK, **attrs)
    opts = {k[7:]: v for k, v in attrs.items() if k.startswith("option_")}
    attrs = {k: v for k, v in attrs.items() if not k.startswith("option_")}
    old = {k: getattr(eng, k) for k in attrs}
    old_opts = {k: int(eng.lib.ggl_get_option(k.encode())) for k in opts}
    try:
        for k, v in attrs.items():
            setattr(eng, k, v)
        for k, v in opts.items():
            eng.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(eng, k, v)
        for k, v in old_opts.items():
            eng.set_option(k, v)


# ---- the ops: run(eng, dev, index) -> (outputs, leaves); outputs that are floating tensors are differentiated w.r.t. leaves
def _reduce(op):
    def run(eng, dev, index):
        x = rnd(dev, E, 8, grad=False)
        r = eng.segment_reduce(x, eng.seg_plan(index[1], N), op)
        return (r if isinstance(r, tuple) else (r,)), ()
    return run


def _softmax(eng, dev, index):
    x = rnd(dev, E, 3)
    return (eng.segment_softmax(x, index[1], N),), (x,)


def _spmm(reduce, dtype=torch.float32, K=8):
    def run(eng, dev, index):
        x, w = rnd(dev, N, K, dtype=dtype), rnd(dev, E, seed=1, grad=False, lo=0.5)
        return (eng.spmm(eng.graph_plan(index, N, N), w, x, reduce),), (x,)
    return run


def _bspmm(eng, dev, index):
    x, w = rnd(dev, N, 2, 4), rnd(dev, E, 2, seed=1, lo=0.5)
    return (eng.c_bspmm_sum(index, w, x),), (x, w)


def _spmm_epi(eng, dev, index):
    x, w, b = rnd(dev, N, 8), rnd(dev, E, seed=1, grad=False, lo=0.5), rnd(dev, 8, seed=2)
    return (eng.spmm_epi(eng.graph_plan(index, N, N), w, x, "sum", None, b, relu=True),), (x, b)


def _segment_epi(eng, dev, index):
    m, b = rnd(dev, E, 8), rnd(dev, 8, seed=2)
    return (eng.segment_epi(m, index[1], N, "mean", None, b, relu=True),), (m, b)


def _segment_multi(eng, dev, index):
    x = rnd(dev, E, 8)
    return (eng.segment_multi(x, index[1], N, aggs=("mean", "min", "max", "std"), C=8),), (x,)


def _esa(H, C, p):
    def run(eng, dev, index):
        z, x = rnd(dev, E, H), rnd(dev, N, H, C, seed=1)
        return (eng.edge_softmax_aggregate(index, z, x, N, dropout_rate=p),), (z, x)
    return run


def _gat(H, C, p=0.0, dtype=torch.float32):
    def run(eng, dev, index):
        el, er, x = rnd(dev, N, H), rnd(dev, N, H, seed=1), rnd(dev, N, H, C, seed=2, dtype=dtype)
        return (eng.gat_fused(index, el, er, x, 0.2, N, dropout_rate=p),), (el, er, x)
    return run


def _dot(H, C):
    def run(eng, dev, index):
        q, k, v = rnd(dev, N, H, C), rnd(dev, N, H, C, seed=1), rnd(dev, N, H, C, seed=2)
        return (eng.dot_attention(index, q, k, v, N),), (q, k, v)
    return run


def _gatv2(H, C):
    def run(eng, dev, index):
        xl, xr, att = rnd(dev, N, H, C), rnd(dev, N, H, C, seed=1), rnd(dev, H, C, seed=2)
        return (eng.gatv2_attention(index, xl, xr, att, N),), (xl, xr, att)
    return run


def _headmean(eng, dev, index):
    x, W, att = rnd(dev, N, 8), rnd(dev, 8, 8 * 5, seed=1), rnd(dev, 1, 8, 10, seed=2)
    return (eng.gat_headmean(index, x, W, att, 0.2, N, dropout_rate=0.25),), (x, W, att)


CHUNKED = dict(option_exact_long_rows=0)     # sums and means through the chunk partials (the host build otherwise walks a row whole)
HOST_AND_GPU = {
    "segment_sum": (_reduce("sum"), CHUNKED), "segment_mean": (_reduce("mean"), CHUNKED), "segment_max": (_reduce("max"), {}),
    "segment_softmax_k3": (_softmax, {}),
    "spmm_sum": (_spmm("sum"), CHUNKED), "spmm_mean": (_spmm("mean"), CHUNKED), "spmm_max": (_spmm("max"), {}),
    "spmm_sum_bf16_k16": (_spmm("sum", torch.bfloat16, 16), CHUNKED),
    "spmm_mean_bf16_k16": (_spmm("mean", torch.bfloat16, 16), CHUNKED),
    "bspmm_2x4": (_bspmm, CHUNKED), "spmm_epi": (_spmm_epi, CHUNKED), "segment_epi": (_segment_epi, CHUNKED),
    "segment_multi_pna": (_segment_multi, {}),
    "edge_softmax_aggregate_3x5": (_esa(3, 5, 0.0), {}), "edge_softmax_aggregate_8x8_drop": (_esa(8, 8, 0.3), {}),
    "gat_fused_general_3x5": (_gat(3, 5), dict(gat_fast=False)),
    "gat_fused_general_bf16_2x16": (_gat(2, 16, dtype=torch.bfloat16), dict(gat_fast=False)),
    "dot_attention_2x16": (_dot(2, 16), {}), "dot_attention_2x12_composed": (_dot(2, 12), {}),
    "gatv2_attention_2x16": (_gatv2(2, 16), {}), "gatv2_attention_2x12_composed": (_gatv2(2, 12), {}),
}
GPU_ONLY = {
    "gat_fused_fast_8x8_drop": (_gat(8, 8, 0.3), dict(gat_fast=True)),
    "gat_headmean_f8_c5": (_headmean, dict(gat_fast=True)),
    # exact_long_rows = 1 (the default): the hub rows of an f32 sum go through hubf32.hip's serial walk, [n_long, K] of the partial
    "spmm_sum_serial_hub_walk": (_spmm("sum"), dict(option_exact_long_rows=1)),
    "segment_sum_serial_hub_walk": (_reduce("sum"), dict(option_exact_long_rows=1)),
}


class Partials:
    """the replacement of Engine._hub_partial and the record of what it handed out"""

    def __init__(self):
        self.short = 0          # bytes withheld from the declared size
        self.given = []         # (allocation, bytes the library's sizer answered, bytes withheld)

    def __call__(self, plan, nbytes, dev):
        if plan.n_long == 0:
            return None
        need = int(nbytes(plan.n_chunks))
        assert need > 0, "a plan with long rows needs a partial"
        buf = torch.full((BAND + need + BAND,), CANARY, dtype=torch.uint8, device=dev)
        self.given.append((buf, need, self.short))
        return buf[BAND:BAND + need - self.short]

    def canaries_intact(self):
        return all(bool((b[:BAND] == CANARY).all()) and bool((b[BAND + need:] == CANARY).all()) for b, need, _ in self.given)

    def short_views_untouched(self):
        return all(bool((b == CANARY).all()) for b, _, short in self.given if short)


def _forward(run, eng, dev, index):
    eng.reseed(SEED)            # the same dropout words in every run
    return run(eng, dev, index)


def _backward(outs, leaves):
    if not leaves:
        return ()
    fl = [o for o in outs if o.is_floating_point() and o.requires_grad]
    gs = [rnd(o.device, *o.shape, seed=50 + i, dtype=o.dtype, grad=False) for i, o in enumerate(fl)]
    return torch.autograd.grad(fl, leaves, gs)


def _refused(fn, hub):
    with pytest.raises(RuntimeError) as ei:
        fn()
    msg = str(ei.value)
    m = re.search(r"has long rows and a partial of (\d+) bytes: its walk needs (\d+)", msg)
    assert "ggl_mpops error -5" in msg and m, msg                       # GGL_EWORKSPACE, with both counts
    assert int(m.group(1)) + 1 == int(m.group(2)) and int(m.group(2)) in [need for _, need, short in hub.given if short], msg
    assert hub.canaries_intact() and hub.short_views_untouched()        # nothing was launched on the refused partial


def check_case(eng, dev, name, monkeypatch):
    from gammagl_amd.ops import Engine

    run, state = {**HOST_AND_GPU, **GPU_ONLY}[name]
    index = make_graph(dev)
    with engine_state(eng, **state):
        gp = eng.graph_plan(index, N, N)
        assert gp.fwd.n_long > 0 and gp.bwd.n_long > 0 and gp.fwd.chunk == CHUNK, "both plans are meant to have hub rows"
        outs, leaves = _forward(run, eng, dev, index)                   # the unpatched Engine
        want = [o.detach().clone() for o in outs] + [g.clone() for g in _backward(outs, leaves)]

        hub = Partials()
        monkeypatch.setattr(Engine, "_hub_partial", staticmethod(hub))
        # pass 1: exactly the library's size
        outs, leaves = _forward(run, eng, dev, index)
        n_fwd = len(hub.given)
        assert n_fwd > 0, "the case is meant to hand the library a hub partial"
        got = [o.detach() for o in outs] + list(_backward(outs, leaves))
        n_bwd = len(hub.given) - n_fwd
        assert len(got) == len(want) and all(same_bits(a, b) for a, b in zip(got, want))
        assert hub.canaries_intact()
        # pass 2: one byte short — the forward is refused ...
        hub.short = 1
        _refused(lambda: _forward(run, eng, dev, index), hub)
        # ... and, with the forward exact, the backward (where it takes a partial of its own)
        if n_bwd:
            hub.short = 0
            outs, leaves = _forward(run, eng, dev, index)
            hub.short = 1
            _refused(lambda: _backward(outs, leaves), hub)
        monkeypatch.undo()
