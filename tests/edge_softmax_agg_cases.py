"""Shared cases of the edge-softmax aggregate on per-edge logits (ggl_edge_softmax_agg_{fwd,bwd_dst,bwd_src}: the general GAT
walks with the logit read from z [E, H]) for tests/test_edge_softmax_agg_host.py (host library, CPU tensors) and
tests/test_gpu_edge_softmax_agg.py (MI355X).  Not a test module.

A *route* is a callable ``f(index, z, x, n_dst, p) -> out`` that records autograd.  The three routes: the ctypes engine
(``Engine.edge_softmax_aggregate``), ``torch.ops.ggl_attn`` (C++ registered) and ``torch.ops.gammagl_amd``.

The main contract: with ``z = LeakyReLU(el[src] + er[dst])`` computed in f32 torch, the op returns the bits of the GENERAL f32
GAT entry points (``ggl_gat_fused_fwd / _bwd_dst / _bwd_src`` through the C ABI, gat16_cases.raw_forward / raw_backward; never
gat_fast): out, rowmax, rowden, alpha, gx, and gz = the GAT call's per-edge ds in the caller's edge order (its ``de`` is ds where
the raw logit is positive and ds * slope elsewhere).  Every such comparison is on the integer view of the bits.
"""
import ctypes

import numpy as np
import pytest
import torch

import gat16_cases as gc
from oracle import parity
import softmax_cases as smc
import spmm16_cases as sc
from spmm16_cases import same_bits

N, E = 300, 6000
RECT = (390, 130)      # N_src, N_dst of the rectangular graph
KINDS = sc.KINDS + ("rectangular",)
SHAPES = ((1, 1),      # one column
          (3, 5),      # element loads
          (8, 8),      # CREG = 8
          (2, 16),     # CREG = 16
          (1, 64),     # the wide backward kernel on the GPU, one head
          (4, 24),     # the wide backward kernel
          (8, 41),     # wide, padded to 44 by _head_padded on the routes and raw (element loads) through the C ABI
          (1, 320),    # C > 256: lane per head
          (20, 4))     # H > 16
SLOPE = gc.SLOPE
TOL = parity.TOL       # 1e-5


def engine_route(eng):
    def f(index, z, x, n_dst, p):
        return eng.edge_softmax_aggregate(index, z, x, num_nodes=n_dst, dropout_rate=p, training=True)
    return f


def ops_route(ns):
    """`ns` = torch.ops.ggl_attn (cpp_ops.load_attn()) or torch.ops.gammagl_amd (torch_ops.ops)"""
    def f(index, z, x, n_dst, p):
        return ns.edge_softmax_aggregate(index, z, x, n_dst, p)
    return f


def make_routes(eng):
    from gammagl_amd import cpp_ops, torch_ops

    return {"engine": engine_route(eng), "torch.ops.ggl_attn": ops_route(cpp_ops.load_attn()),
            "torch.ops.gammagl_amd": ops_route(torch_ops.ops)}


def make_graph(kind, gen, dev, n=N, e=E):
    """(edge_index, N_src, N_dst)"""
    if kind == "rectangular":
        ns, nd = RECT
        return torch.stack([torch.randint(0, ns, (e,), generator=gen, device=dev),
                            torch.randint(0, nd, (e,), generator=gen, device=dev)]).contiguous(), ns, nd
    return sc.make_index(kind, n, e, gen, dev), n, n


def make_z(index, el, er, slope=SLOPE):
    """the GAT logits as a per-edge tensor, in f32 torch; also the raw sums (the sign decides the GAT call's de)"""
    raw = el[index[0]] + er[index[1]]
    return torch.where(raw > 0, raw, raw * slope), raw


# ---- the C ABI, called directly -------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def raw_forward(eng, gp, z, x, p, rng):
    """(out, rowmax, rowden) of ggl_edge_softmax_agg_fwd; rng = the {seed, offset} read"""
    dev = x.device
    H, C = int(x.shape[1]), int(x.shape[2])
    out = torch.empty((gp.N_dst, H, C), dtype=torch.float32, device=dev)
    rmax = torch.empty((gp.N_dst, H), dtype=torch.float32, device=dev)
    rden = torch.empty((gp.N_dst, H), dtype=torch.float32, device=dev)
    part = eng._gat_partial(gp.fwd, H, C, dev)
    cs = gp.fwd.c_struct(part)
    r = rng.clone() if p > 0 else None
    eng._check(eng.lib.ggl_edge_softmax_agg_fwd(ctypes.byref(cs), _p(gp.col), _p(z), _p(x), H, C, p, _p(r), _p(out), _p(rmax),
                                                _p(rden), eng._stream(dev)))
    return out, rmax, rden


def raw_backward(eng, gp, z, x, g, out, rmax, rden, p, rng):
    """(alpha [E, H] by sorted position, gz [E, H] in the caller's order, gx) of the two backward walks; alpha and gz are
    blocks of exactly E * H floats"""
    dev = x.device
    H, C = int(x.shape[1]), int(x.shape[2])
    alpha = torch.zeros((gp.E, H), dtype=torch.float32, device=dev)
    gz = torch.zeros((gp.E, H), dtype=torch.float32, device=dev)
    gx = torch.empty((gp.N_src, H, C), dtype=torch.float32, device=dev)
    part_f = eng._partial(gp.fwd, torch.float32, H, False, dev)
    part_t = eng._partial(gp.bwd, torch.float32, H * C + H, False, dev)
    cs, csT = gp.fwd.c_struct(part_f), gp.bwd.c_struct(part_t)
    r = rng if p > 0 else None
    st = eng._stream(dev)
    eng._check(eng.lib.ggl_edge_softmax_agg_bwd_dst(ctypes.byref(cs), _p(gp.col), _p(z), _p(x), _p(g), _p(out), _p(rmax),
                                                    _p(rden), H, C, p, _p(r), _p(alpha), _p(gz), st))
    eng._check(eng.lib.ggl_edge_softmax_agg_bwd_src(ctypes.byref(csT), _p(gp.colT), _p(gp.posT), _p(alpha), _p(g), H, C,
                                                    _p(gx), st))
    return alpha, gz, gx


def gat(eng, gp, el, er, x, g, p, rng):
    """the general f32 GAT entry points on (el, er): out, statistics, alpha / de by sorted position, ger, gx"""
    out, rmax, rden = gc.raw_forward(eng, gp, el, er, x, p, rng)
    ad, _gel, ger, gx = gc.raw_backward(eng, gp, el, er, x, g, out, rmax, rden, p, rng)
    return {"out": out, "rmax": rmax, "rden": rden, "alpha": ad[:gp.E, :, 0].contiguous(), "de": ad[:gp.E, :, 1].contiguous(),
            "ger": ger, "gx": gx}


def sorted_order(gp, t):
    """t [E, ...] in the caller's order -> the plan's sorted-position order"""
    perm = gp.fwd.perm
    return t if perm is None else t[perm.long()]


def same_bits_or_nan(a, b):
    """same bits, except that any NaN matches any NaN (the payload of a NaN that went through torch and one that went through
    the kernel's LeakyReLU need not agree)"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and \
        torch.equal(sc.bits(torch.where(na, torch.zeros_like(a), a)), sc.bits(torch.where(nb, torch.zeros_like(b), b)))


def check_gz_is_de(gp, gz, raw, ref, slope, tag, eq=same_bits):
    """gz (caller's order) is the GAT call's ds: its de is ds where raw > 0 and ds * slope elsewhere"""
    if gp.E == 0:
        return
    ds, rs = sorted_order(gp, gz), sorted_order(gp, raw)
    assert eq(torch.where(rs > 0, ds, ds * slope), ref["de"]), ("gz", tag)


def run_route(route, eng, index, z, x, g, n_dst, p, seed, need=(True, True)):
    """(out, gz, gx) of one route, forward + backward through autograd"""
    za, xa = z.clone().requires_grad_(need[0]), x.clone().requires_grad_(need[1])
    if p > 0:
        gc.reseed(eng, seed)
    out = route(index, za, xa, n_dst, p)
    out.backward(g)
    return out.detach(), za.grad, xa.grad


def check_equality(routes, eng, gp, index, el, er, x, g, n_dst, p, seed, tag, eq=same_bits, raw_abi=True):
    """§1 for one (graph, shape, p): the C entry points on x as it is, and every route (x padded where the policy pads)"""
    dev = x.device
    C = int(x.shape[2])
    z, raw = make_z(index if torch.is_tensor(index) else gp.index, el, er)
    rng = gc.drawn_rng(seed, dev)
    if raw_abi:
        ref = gat(eng, gp, el, er, x, g, p, rng)
        out, rmax, rden = raw_forward(eng, gp, z, x, p, rng)
        assert eq(out, ref["out"]), ("out", tag)
        assert eq(rmax, ref["rmax"]) and eq(rden, ref["rden"]), ("statistics", tag)
        alpha, gz, gx = raw_backward(eng, gp, z, x, g, out, rmax, rden, p, rng)
        assert eq(alpha, ref["alpha"]), ("alpha", tag)
        assert eq(gx, ref["gx"]), ("gx", tag)
        check_gz_is_de(gp, gz, raw, ref, SLOPE, tag, eq)
    xp, gpad = gc.padded(eng, gp, x, g)
    refp = ref if (raw_abi and xp is x) else gat(eng, gp, el, er, xp, gpad, p, rng)
    for name, route in routes.items():
        out, gz, gx = run_route(route, eng, index, z, x, g, n_dst, p, seed)
        t = (name, tag)
        assert eq(out, refp["out"][:, :, :C].contiguous()), ("out", t)
        assert eq(gx, refp["gx"][:, :, :C].contiguous()), ("gx", t)
        check_gz_is_de(gp, gz, raw, refp, SLOPE, t, eq)


def check_contract(routes, eng, dev, kind, shapes=SHAPES, drops=(0.0, 0.5), seed=0):
    """§1 over the shape table on one graph kind; returns the number of (shape, p) cases"""
    gen = torch.Generator(device=dev).manual_seed(seed + len(kind))
    index, n_src, n_dst = make_graph(kind, gen, dev)
    gp = eng.graph_plan(index, n_dst, n_src)
    if kind == "sorted":
        assert gp.fwd.perm is None, "sorted ids are meant to give a plan without perm"
    elif kind != "no_edges":
        assert gp.fwd.perm is not None
    n = 0
    for H, C in shapes:
        el, er, x, g = gc.make_inputs(n_src, n_dst, H, C, gen, dev)
        for p in drops:
            check_equality(routes, eng, gp, index, el, er, x, g, n_dst, p, 11 + n, (kind, H, C, p))
            n += 1
    return n


def check_gz_order(eng, dev, shapes=((3, 5), (8, 8), (4, 24)), seed=5):
    """§2: with slope = 1 (z = el[src] + er[dst]) on a plan without long rows and with unsorted ids, the GAT call's ger[i, h]
    is, on the bits, the serial f32 sum of gz[e, h] over the edges of row i in stable destination order (a plain loop here):
    a missing or inverted perm at the gz store fails this"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    index, n_src, n_dst = make_graph("uniform", gen, dev)
    gp = eng.graph_plan(index, n_dst, n_src)
    assert gp.fwd.n_long == 0 and gp.fwd.perm is not None
    dst = index[1].cpu().numpy()
    old = gc.SLOPE
    gc.SLOPE = 1.0           # gat16_cases' raw calls read it at call time
    try:
        for H, C in shapes:
            el, er, x, g = gc.make_inputs(n_src, n_dst, H, C, gen, dev)
            z = el[index[0]] + er[index[1]]
            for p in (0.0, 0.5):
                rng = gc.drawn_rng(21, dev)
                ref = gat(eng, gp, el, er, x, g, p, rng)
                out, rmax, rden = raw_forward(eng, gp, z, x, p, rng)
                assert same_bits(out, ref["out"]), (H, C, p)
                _, gz, _ = raw_backward(eng, gp, z, x, g, out, rmax, rden, p, rng)
                gzn = gz.cpu().numpy()
                acc = np.zeros((n_dst, H), dtype=np.float32)
                for e in range(gp.E):        # ascending e inside a row = stable destination order
                    acc[dst[e]] = acc[dst[e]] + gzn[e]
                assert same_bits(torch.from_numpy(acc).to(dev), ref["ger"]), (H, C, p)
    finally:
        gc.SLOPE = old


def check_one_edge_per_destination(routes, eng, dev, shapes=((3, 5), (8, 8), (4, 24), (1, 64)), n=257, seed=6):
    """§3: every destination has exactly one edge, sources permuted: out == x[src], every gz is +0 or -0, gx == g[dst]"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    src = torch.randperm(n, generator=gen, device=dev)
    dst = torch.randperm(n, generator=gen, device=dev)
    index = torch.stack([src, dst]).contiguous()
    for H, C in shapes:
        x = torch.randn(n, H, C, generator=gen, device=dev)
        g = torch.randn(n, H, C, generator=gen, device=dev)
        z = torch.randn(n, H, generator=gen, device=dev) * 3
        want_out = torch.empty_like(x)
        want_out[dst] = x[src]
        want_gx = torch.empty_like(x)
        want_gx[src] = g[dst]
        for name, route in routes.items():
            out, gz, gx = run_route(route, eng, index, z, x, g, n, 0.0, 0)
            assert same_bits(out, want_out), (name, H, C)
            assert torch.equal(gz, torch.zeros_like(gz)), (name, H, C)     # +0 == -0
            assert same_bits(gx, want_gx), (name, H, C)


def check_f32_accumulation(routes, dev):
    """§3: 4096 edges into one destination, z = 0, x = 1: every alpha is 1 / 4096 and out is exactly 1.0
    (gat16_cases.check_f32_accumulation's argument)"""
    n = 4096
    ei = torch.stack([torch.arange(n, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)])
    z = torch.zeros(n, 2, device=dev)
    x = torch.ones(n, 2, 8, device=dev)
    for name, route in routes.items():
        out = route(ei, z, x, n, 0.0)
        assert torch.equal(out[0], torch.ones(2, 8, device=dev)), (name, out[0])
        assert torch.equal(out[1:], torch.zeros(n - 1, 2, 8, device=dev)), name


def check_inf_and_nan_rows(routes, eng, dev, shapes=((3, 5), (4, 24)), seed=7):
    """§3: a row whose logits are all -inf gives zeros like an empty row (no -inf beats the -FLT_MAX start, every exp is 0), a
    row with a NaN among its logits gives NaN — what the GAT kernels give for the same s values, pinned against the GAT
    call (NaN matches NaN, everything else on the bits)"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    index, n_src, n_dst = make_graph("uniform", gen, dev)
    gp = eng.graph_plan(index, n_dst, n_src)
    for H, C in shapes:
        el, er, x, g = gc.make_inputs(n_src, n_dst, H, C, gen, dev)
        er[3] = float("-inf")                # every logit of destination 3 is -inf
        el[5] = float("nan")                 # every edge out of source 5 carries a NaN into its destination
        z, _ = make_z(index, el, er)
        assert bool(torch.isinf(z[index[1] == 3]).all()) and bool(torch.isnan(z[index[0] == 5]).all())
        check_equality(routes, eng, gp, index, el, er, x, g, n_dst, 0.0, 0, ("inf / nan", H, C), eq=same_bits_or_nan)
        out = routes["engine"](index, z, x, n_dst, 0.0)
        assert torch.equal(out[3], torch.zeros_like(out[3])), "all -inf: every exp(-inf + FLT_MAX) is 0"
        hit = torch.unique(index[1][index[0] == 5])
        assert bool(torch.isnan(out[hit]).all()), "a NaN logit poisons its row"
        clean = torch.ones(n_dst, dtype=torch.bool, device=dev)
        clean[hit] = False
        clean[3] = False
        assert bool(torch.isfinite(out[clean]).all())


def long_row_graph(eng, dev, chunk=64, n=300, e=20_000, seed=3):
    gen = torch.Generator(device=dev).manual_seed(seed)
    dst = (n * torch.rand(e, generator=gen, device=dev) ** 3).long().clamp_(max=n - 1)
    src = (n * torch.rand(e, generator=gen, device=dev) ** 3).long().clamp_(max=n - 1)
    return torch.stack([src, dst]).contiguous(), gen


def check_long_rows(eng, dev, shapes=((3, 5), (8, 8), (4, 24), (8, 44)), chunk=64, n=300, e=20_000):
    """§4: §1 on a plan with long rows in BOTH directions (hub-chunk items, partials, the merges), the engine on the plan"""
    index, gen = long_row_graph(eng, dev, chunk, n, e)
    old = eng.chunk
    eng.chunk = chunk
    try:
        gp = eng.graph_plan(index, n)
        assert gp.fwd.n_long > 0 and gp.bwd.n_long > 0 and gp.fwd.chunk == chunk
        route = {"engine on the plan": lambda i, z, x, nd, p: engine_route(eng)(gp, z, x, nd, p)}
        k = 0
        for H, C in shapes:
            el, er, x, g = gc.make_inputs(n, n, H, C, gen, dev)
            for p in (0.0, 0.5):
                check_equality(route, eng, gp, index, el, er, x, g, n, p, 40 + k, ("long rows", H, C, p))
                k += 1
        return gp
    finally:
        eng.chunk = old


# ---- §5: against float64 --------------------------------------------------------------------------------------------------
def truth_f64(index, z, x, g, n_dst):
    """(out, gz, gx) of softmax (softmax_cases.truth_f64) then a weighted index_add_, in float64"""
    src, dst = index[0], index[1]
    xd, gd = x.double(), g.double()
    galpha = (gd[dst] * xd[src]).sum(-1)                          # d out / d alpha, [E, H]
    y, gz = smc.truth_f64(z, dst, n_dst, galpha)
    out = torch.zeros((n_dst,) + tuple(x.shape[1:]), dtype=torch.float64, device=x.device)
    out.index_add_(0, dst, y.unsqueeze(-1) * xd[src])
    gx = torch.zeros_like(xd).index_add_(0, src, y.unsqueeze(-1) * gd[dst])
    return out, gz, gx


def composed(index, z, x, n_dst):
    """the f32 composition the op replaces: utils.segment_softmax then mpops.bspmm"""
    from gammagl_amd import mpops
    from gammagl_amd.utils import segment_softmax

    return mpops.bspmm(index, segment_softmax(z, index[1], n_dst), x, "sum")


def tensor_err(got, truth):
    return float((got.double() - truth).abs().max() / truth.abs().max())


def check_against_f64(route, eng, dev, n=2000, e=200_000, shapes=((1, 64), (8, 8), (4, 24), (3, 5)), seed=8):
    """§5: max|got - truth| / max|truth| <= 1e-5 for out, gx and gz, truth in float64, ids power-law and uniform, logits
    randn * 3.  The row-scale errors (softmax_cases.seg_err) of the op and of the f32 composition are printed beside it and
    returned as lines; they are NOT asserted (for gz both sit near 1e-4: the stored f32 out inside <g_i, out_i> bounds them)."""
    lines = []
    for kind in ("power", "uniform"):
        gen = torch.Generator(device=dev).manual_seed(seed)
        index = sc.make_index(kind, n, e, gen, dev)
        for H, C in shapes:
            z = torch.randn(e, H, generator=gen, device=dev) * 3
            x = torch.randn(n, H, C, generator=gen, device=dev)
            g = torch.randn(n, H, C, generator=gen, device=dev)
            t_out, t_gz, t_gx = truth_f64(index, z, x, g, n)
            res = {}
            for name, f in (("fused", lambda zz, xx: route(index, zz, xx, n, 0.0)),
                            ("composed", lambda zz, xx: composed(index, zz, xx, n))):
                za, xa = z.clone().requires_grad_(True), x.clone().requires_grad_(True)
                out = f(za, xa)
                out.backward(g)
                res[name] = {"out": tensor_err(out.detach(), t_out), "gx": tensor_err(xa.grad, t_gx),
                             "gz": tensor_err(za.grad, t_gz), "gz_row": smc.seg_err(za.grad, t_gz, index[1], n)}
            line = (f"{kind:8s} {H:2d} x {C:2d}  " + "  ".join(
                f"{name}: out {r['out']:.2e} gx {r['gx']:.2e} gz {r['gz']:.2e} gz(row scale) {r['gz_row']:.2e}"
                for name, r in res.items()))
            print(line)
            lines.append(line)
            for what in ("out", "gx", "gz"):
                assert res["fused"][what] <= TOL, (kind, H, C, what, res["fused"][what])
    return lines


# ---- §6: dropout state ----------------------------------------------------------------------------------------------------
def check_dropout_state(eng, dev):
    """parity_cases.check_dropout_state_discipline for the new op, on a plan with a hub row walked chunked and in one piece;
    and the mask is the one gat_fused draws from the same state on the same plan"""
    n, e, p = 40, 600, 0.5
    g = torch.Generator(device="cpu").manual_seed(33)
    ei = torch.randint(0, n, (2, e), generator=g)
    ei[1, : e // 3] = 3
    ei = ei.to(dev)
    H, C = 3, 5        # (not a gat_fast shape: Engine.gat_fused takes the general kernels)
    z0 = torch.randn(e, H, generator=g).to(dev)
    x0 = torch.randn(n, H, C, generator=g).to(dev)

    def offset():
        return int(eng._rng_state(dev)[1])

    def run(q, training, gp):
        z, x = z0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
        o0 = offset()
        y = eng.edge_softmax_aggregate(gp, z, x, n, q, training)
        o1 = offset()
        y.backward(torch.ones_like(y))
        return y.detach(), (z.grad, x.grad), (o0, o1, offset())

    old = eng.chunk
    try:
        for chunk in (8, 0):
            eng.chunk = chunk
            eng.graph_cache.clear(); eng.seg_cache.clear()
            gp = eng.graph_plan(ei, n)
            assert (gp.fwd.n_long > 0) == (chunk == 8)
            st = eng._rng_state(dev).clone()
            y1, g1, (o0, o1, o2) = run(p, True, gp)
            assert o1 == o0 + 1, ("the forward advances the offset by exactly 1", chunk, o0, o1)
            assert o2 == o1, ("the backward does not move the state", chunk)
            eng._rng_state(dev).copy_(st)
            y2, g2, _ = run(p, True, gp)
            assert same_bits(y1, y2) and all(same_bits(a, b) for a, b in zip(g1, g2)), ("restored state, same bits", chunk)
            y0, _, _ = run(0.0, True, gp)
            assert not torch.equal(y0, y1), "dropout changed nothing"
            for q, training in ((0.0, True), (p, False)):
                _, _, offs = run(q, training, gp)
                assert offs[0] == offs[1] == offs[2], ("no dropout, no draw", chunk, q, training, offs)
            # the mask: gat_fused on el = 0, er = 0 has s = 0 on every edge; so has the op on z = 0
            zero = torch.zeros(n, H, device=dev)
            eng._rng_state(dev).copy_(st)
            a = eng.gat_fused(gp, zero, zero, x0, 0.2, n, p, True)
            eng._rng_state(dev).copy_(st)
            b = eng.edge_softmax_aggregate(gp, torch.zeros(e, H, device=dev), x0, n, p, True)
            assert same_bits(a, b), ("gat_fused's mask", chunk)
    finally:
        eng.chunk = old
        eng.graph_cache.clear(); eng.seg_cache.clear()


# ---- §7: routes, refusals, autograd plumbing ------------------------------------------------------------------------------
def check_routes_agree(routes, eng, dev):
    gen = torch.Generator(device=dev).manual_seed(9)
    index, n_src, n_dst = make_graph("power", gen, dev)
    for H, C in ((3, 5), (4, 24), (8, 41)):
        z = torch.randn(E, H, generator=gen, device=dev) * 3
        x = torch.randn(n_src, H, C, generator=gen, device=dev)
        g = torch.randn(n_dst, H, C, generator=gen, device=dev)
        for p in (0.0, 0.5):
            res = {name: run_route(r, eng, index, z, x, g, n_dst, p, 17) for name, r in routes.items()}
            first = res["engine"]
            for name, r in res.items():
                assert all(same_bits(a, b) for a, b in zip(r, first)), (name, H, C, p)
    # one head given as logits [E] and x [N, K]
    z1 = torch.randn(E, generator=gen, device=dev)
    x1 = torch.randn(n_src, 7, generator=gen, device=dev)
    for name, r in routes.items():
        a = r(index, z1, x1, n_dst, 0.0)
        b = r(index, z1.unsqueeze(1), x1.unsqueeze(1), n_dst, 0.0)
        assert a.shape == (n_dst, 7) and same_bits(a, b.squeeze(1)), name


def check_refusals(routes, eng, dev):
    gen = torch.Generator(device=dev).manual_seed(2)
    ei = sc.make_index("uniform", 50, 400, gen, dev)
    z = torch.randn(400, 4, generator=gen, device=dev)
    x = torch.randn(50, 4, 8, generator=gen, device=dev)
    for name, route in routes.items():
        for dt in (torch.float64, torch.bfloat16, torch.float16):
            with pytest.raises(RuntimeError, match="Float"):
                route(ei, z.to(dt), x, 50, 0.0)
            with pytest.raises(RuntimeError, match="Float"):
                route(ei, z, x.to(dt), 50, 0.0)
        for bad in (z[:399], z[:, :3], z.reshape(-1)):
            with pytest.raises(RuntimeError):
                route(ei, bad, x, 50, 0.0)
    with pytest.raises(ValueError):
        eng.edge_softmax_aggregate(ei, z, x, 50, dropout_rate=1.0)
    from gammagl_amd.utils import edge_softmax_aggregate

    with pytest.raises(ValueError):
        edge_softmax_aggregate(ei, z, x, 50, dropout_rate=1.0)


def check_one_sided_gradients(routes, eng, dev):
    """only x, or only z, requires grad: the other gradient is None and the wanted one has the two-sided call's bits"""
    gen = torch.Generator(device=dev).manual_seed(10)
    index, n_src, n_dst = make_graph("uniform", gen, dev)
    for H, C in ((3, 5), (4, 24)):
        z = torch.randn(E, H, generator=gen, device=dev)
        x = torch.randn(n_src, H, C, generator=gen, device=dev)
        g = torch.randn(n_dst, H, C, generator=gen, device=dev)
        for name, route in routes.items():
            _, gz, gx = run_route(route, eng, index, z, x, g, n_dst, 0.0, 0)
            _, gz1, gx1 = run_route(route, eng, index, z, x, g, n_dst, 0.0, 0, need=(True, False))
            assert gx1 is None and same_bits(gz1, gz), (name, H, C)
            _, gz2, gx2 = run_route(route, eng, index, z, x, g, n_dst, 0.0, 0, need=(False, True))
            assert gz2 is None and same_bits(gx2, gx), (name, H, C)


def check_public_function(eng, dev):
    """gammagl_amd.utils.edge_softmax_aggregate reaches the op and gives the engine's bits"""
    from gammagl_amd.utils import edge_softmax_aggregate

    gen = torch.Generator(device=dev).manual_seed(12)
    index, n_src, n_dst = make_graph("rectangular", gen, dev)
    z = torch.randn(E, 4, generator=gen, device=dev)
    x = torch.randn(n_src, 4, 8, generator=gen, device=dev)
    a = edge_softmax_aggregate(index, z, x, n_dst)
    assert same_bits(a, eng.edge_softmax_aggregate(index, z, x, n_dst))
    assert same_bits(a, edge_softmax_aggregate(index, z, x, n_dst, dropout_rate=0.5, training=False))


# ---- §8: AGNNConv ---------------------------------------------------------------------------------------------------------
def check_agnn(dev, n=500, e=8000, k=32):
    """fused=True against fused=False in float64: forward, x.grad and beta.grad within the tensor-scale 1e-5"""
    from gammagl_amd import layers

    gen = torch.Generator(device=dev).manual_seed(13)
    ei = layers.add_self_loops(sc.make_index("power", n, e, gen, dev), n)
    x = torch.randn(n, k, generator=gen, device=dev)
    g = torch.randn(n, k, generator=gen, device=dev)
    for require_grad in (True, False):
        torch.manual_seed(0)
        fused = layers.AGNNConv(k, require_grad=require_grad, fused=True).to(dev)
        ref = layers.AGNNConv(k, require_grad=require_grad, fused=False).to(dev).double()
        with torch.no_grad():
            if require_grad:
                fused.beta.fill_(0.75)
            ref.beta.copy_(fused.beta.double())
        assert fused.beta.requires_grad == require_grad and float(fused.beta.detach()) == (0.75 if require_grad else 0.0)
        xa, xd = x.clone().requires_grad_(True), x.double().requires_grad_(True)
        out = fused(xa, ei, n)
        out.backward(g)
        want = ref(xd, ei, n)
        want.backward(g.double())
        assert out.dtype == torch.float32 and out.shape == (n, k)
        assert tensor_err(out.detach(), want.detach()) <= TOL, ("out", require_grad)
        assert tensor_err(xa.grad, xd.grad) <= TOL, ("x.grad", require_grad)
        if require_grad:
            assert tensor_err(fused.beta.grad, ref.beta.grad) <= TOL, "beta.grad"
        else:
            assert fused.beta.grad is None
