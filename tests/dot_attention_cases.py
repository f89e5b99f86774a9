"""Shared cases of scaled dot-product graph attention (Engine.dot_attention, ggl_dot_attn_fwd) for
tests/test_dot_attention_host.py (host library, CPU tensors: the composed route) and tests/test_gpu_dot_attention.py (MI355X: the
fused forward where ggl_dot_attn_supported says so).  Not a test module.

The contract: the forward can return the logits it used, z [E, H] in the caller's edge order, and everything behind z is the
existing op bit for bit — out == edge_softmax_aggregate(z, v), gv == its x gradient, gq == bspmm(index, gz * scale, k),
gk == bspmm(index^T, gz * scale, q) with gz its logits gradient — for both routes.  z itself is held to
|z - z64| <= gamma_{C+1} |scale| sum_c |q_c k_c|, which covers every order of summing the C products.

A *route* is a callable ``f(index, q, k, v, n_dst, scale, p) -> out`` that records autograd."""
import contextlib
import ctypes
import math

import numpy as np
import pytest
import torch

import edge_softmax_agg_cases as ec
import gat16_cases as gc
from spmm16_cases import same_bits

N_DST, N_SRC, E = 48, 64, 1500
HUB, EMPTY = 3, (7, 31)          # one destination owns a third of the edges; two have none
SHAPES = ((1, 8), (8, 8), (2, 16), (3, 16),   # 3 x 16: 12 lanes of a 16-lane row group are active
          (4, 32), (1, 64),
          (5, 64),               # H * C / 4 = 80 lanes' worth: more than one pass of the wavefront
          (2, 12), (1, 5))       # no power-of-two lane group: the composed route on every build
DROPS = (0.0, 0.5)
CHUNKS = (8, 4096)               # the hub row (and most others) walked in chunks of 8, and every row in one piece
U = 2.0 ** -24


def scale_of(H, C):
    """the default 1 / sqrt(C) for half of the shapes, an explicit factor for the others"""
    return None if (H + C) % 3 else 0.37


def make_graph(dev, seed=1, e=E):
    g = torch.Generator(device="cpu").manual_seed(seed)
    src = torch.randint(0, N_SRC, (e,), generator=g)
    dst = torch.randint(0, N_DST - 2, (e,), generator=g)
    dst = dst + (dst >= EMPTY[0]).long()
    dst = dst + (dst >= EMPTY[1]).long()
    dst[: e // 3] = HUB
    order = torch.randperm(e, generator=g)      # the caller's order is not the sorted one
    return torch.stack([src[order], dst[order]]).contiguous().to(dev)


def make_qkv(H, C, dev, seed=2):
    g = torch.Generator(device="cpu").manual_seed(seed + 100 * H + C)
    q = torch.randn(N_DST, H, C, generator=g).to(dev)
    k = torch.randn(N_SRC, H, C, generator=g).to(dev)
    v = torch.randn(N_SRC, H, C, generator=g).to(dev)
    go = torch.randn(N_DST, H, C, generator=g).to(dev)
    return q, k, v, go


@contextlib.contextmanager
def forced_chunk(eng, chunk):
    """edge_softmax_agg_cases' way of forcing hub chunks: the engine's long-row threshold, plans rebuilt"""
    old = eng.chunk
    eng.chunk = chunk
    eng.graph_cache.clear(); eng.seg_cache.clear()
    try:
        yield
    finally:
        eng.chunk = old
        eng.graph_cache.clear(); eng.seg_cache.clear()


def engine_route(eng):
    def f(index, q, k, v, n_dst, scale, p):
        return eng.dot_attention(index, q, k, v, num_nodes=n_dst, scale=scale, dropout_rate=p, training=True)
    return f


def ops_route(ns):
    def f(index, q, k, v, n_dst, scale, p):
        return ns.dot_attention(index, q, k, v, n_dst, scale, p)
    return f


def make_routes(eng):
    from gammagl_amd import cpp_ops, torch_ops

    return {"engine": engine_route(eng), "torch.ops.ggl_attn": ops_route(cpp_ops.load_attn()),
            "torch.ops.gammagl_amd": ops_route(torch_ops.ops)}


def expects_fused(eng, dev, H, C):
    return bool(dev.type == "cuda" and eng.dot_attn_fused and eng.lib.ggl_dot_attn_supported(H, C)
                and eng.lib.ggl_policy_dot_attn_fused(H, C, E, N_SRC))


def run_engine(eng, index, q, k, v, go, scale, p, state, need=(True, True, True)):
    """(out, z, gq, gk, gv) of Engine.dot_attention with the rng state set to `state` first"""
    leaves = [t.clone().requires_grad_(n) for t, n in zip((q, k, v), need)]
    eng._rng_state(q.device).copy_(state)
    out, z = eng.dot_attention(index, *leaves, num_nodes=N_DST, scale=scale, dropout_rate=p, training=True,
                               return_logits=True)
    if any(need):
        out.backward(go)
    return (out.detach(), z) + tuple(t.grad for t in leaves)


def gamma_bound(index, q, k, scale, C):
    """(z64, bound): the logits in float64 from the f32 scale the kernels multiply by, and gamma_{C+1} |scale| sum |q_c k_c|"""
    s = float(np.float32(1.0 / math.sqrt(C) if scale is None else scale))
    prod = q.double()[index[1]] * k.double()[index[0]]
    n = C + 1
    return s * prod.sum(-1), (n * U / (1 - n * U)) * abs(s) * prod.abs().sum(-1)


def square(index, rows, n=max(N_DST, N_SRC)):
    """mpops.bspmm aggregates onto as many rows as x has: x padded with zero rows to the larger side of the graph"""
    return torch.cat([rows, rows.new_zeros((n - rows.shape[0],) + tuple(rows.shape[1:]))]) if rows.shape[0] < n else rows


def check_contract(eng, dev, H, C, p):
    """§1 for one head shape and dropout rate, the hub row chunked and in one piece; returns the routes taken"""
    from gammagl_amd import mpops

    index = make_graph(dev)
    q, k, v, go = make_qkv(H, C, dev)
    scale = scale_of(H, C)
    s32 = float(np.float32(1.0 / math.sqrt(C) if scale is None else scale))
    taken = []
    for chunk in CHUNKS:
        with forced_chunk(eng, chunk):
            gp = eng.graph_plan(index, N_DST, N_SRC)
            assert (gp.fwd.n_long > 0) == (chunk == 8), chunk
            rows = torch.bincount(index[1], minlength=N_DST)
            assert rows[HUB] >= E // 3 and all(rows[r] == 0 for r in EMPTY)
            state = eng._rng_state(dev).clone()
            out, z, gq, gk, gv = run_engine(eng, gp, q, k, v, go, scale, p, state)
            fused = eng.stats["dot_attention"]["fused"]
            assert fused == expects_fused(eng, dev, H, C), (H, C, "route")
            taken.append(fused)
            tag = (H, C, p, chunk, "fused" if fused else "composed")
            # z: the error bound that holds for any order of the C products
            z64, bound = gamma_bound(index, q, k, scale, C)
            assert z.shape == (E, H) and bool(((z.double() - z64).abs() <= bound).all()), tag
            # everything behind z: the existing op on that z, bit for bit
            za, va = z.clone().requires_grad_(True), v.clone().requires_grad_(True)
            eng._rng_state(dev).copy_(state)
            ref = eng.edge_softmax_aggregate(gp, za, va, N_DST, p, True)
            ref.backward(go)
            assert same_bits(out, ref.detach()), tag
            assert same_bits(gv, va.grad), tag
            if p == 0:
                assert float(out[list(EMPTY)].abs().max()) == 0.0, tag
            gs = za.grad * s32                      # one rounded f32 multiply per element
            rq = mpops.bspmm(index, gs, square(index, k), "sum")[:N_DST]
            rk = mpops.bspmm(index.flip(0).contiguous(), gs, square(index, q), "sum")[:N_SRC]
            assert same_bits(gq, rq), tag
            assert same_bits(gk, rk), tag
            # the same forward without the logits, and with nothing to differentiate: the same out
            o2, z2, *_ = run_engine(eng, gp, q, k, v, go, scale, p, state, need=(False, False, False))
            assert same_bits(o2, out) and same_bits(z2, z), tag
            eng._rng_state(dev).copy_(state)
            o3 = eng.dot_attention(gp, q, k, v, N_DST, scale, p, True)
            assert same_bits(o3, out) and o3.grad_fn is None, tag
            st = eng.stats["dot_attention"]
            assert not st["logits_saved"] and (st["logits_bytes"] == 0) == fused, (tag, st)
            # two identical calls, identical bits
            again = run_engine(eng, gp, q, k, v, go, scale, p, state)
            assert all(same_bits(a, b) for a, b in zip(again, (out, z, gq, gk, gv))), tag
    return taken


def check_one_sided_gradients(eng, dev, H=2, C=16):
    """a walk whose gradient nobody needs is skipped, the others keep their bits"""
    index = make_graph(dev)
    q, k, v, go = make_qkv(H, C, dev)
    state = eng._rng_state(dev).clone()
    full = run_engine(eng, index, q, k, v, go, None, 0.5, state)
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        part = run_engine(eng, index, q, k, v, go, None, 0.5, state, need)
        assert same_bits(part[0], full[0])
        for i, n in enumerate(need):
            assert (part[2 + i] is None) != n and (not n or same_bits(part[2 + i], full[2 + i])), (need, i)


def route_chunks(name):
    """the engine's plans can be forced to walk the hub row chunked and whole; the operator namespaces build their own"""
    return CHUNKS if name == "engine" else (None,)


def check_single_needs_against_the_aggregate(routes, eng, dev, H=2, C=16, seed=23):
    """Only v's gradient asked, only q's, only k's, through every route: out and the one gradient have the bits of the SAME
    route's edge_softmax_aggregate on the returned z under the same rng state — gv its x gradient, gq / gk bspmm of its logits
    gradient times scale — and the gradients nobody asked for are None.  Pins which of (gz, gv) the shared backward forms."""
    from gammagl_amd import mpops

    index = make_graph(dev)
    q, k, v, go = make_qkv(H, C, dev)
    scale = scale_of(H, C)
    s32 = float(np.float32(1.0 / math.sqrt(C) if scale is None else scale))
    aggregate = ec.make_routes(eng)
    for name, route in routes.items():
        for chunk in route_chunks(name):
            with forced_chunk(eng, chunk) if chunk else contextlib.nullcontext():
                for p in DROPS:
                    tag = (name, chunk, p)
                    state = eng._rng_state(dev).clone()
                    _, z, *_ = run_engine(eng, index, q, k, v, go, scale, p, state, need=(False, False, False))
                    za, va = z.clone().requires_grad_(True), v.clone().requires_grad_(True)
                    gc.reseed(eng, seed)
                    ref = aggregate[name](index, za, va, N_DST, p)
                    ref.backward(go)
                    gs = za.grad * s32                      # one rounded f32 multiply per element
                    want = (lambda: mpops.bspmm(index, gs, square(index, k), "sum")[:N_DST],
                            lambda: mpops.bspmm(index.flip(0).contiguous(), gs, square(index, q), "sum")[:N_SRC],
                            lambda: va.grad)
                    for i in (2, 0, 1):
                        leaves = [t.clone().requires_grad_(j == i) for j, t in enumerate((q, k, v))]
                        gc.reseed(eng, seed)
                        out = route(index, *leaves, N_DST, scale, p)
                        out.backward(go)
                        assert same_bits(out.detach(), ref.detach()), (tag, i)
                        assert same_bits(leaves[i].grad, want[i]()), (tag, i)
                        assert all(t.grad is None for j, t in enumerate(leaves) if j != i), (tag, i)


def run_route(route, eng, index, q, k, v, go, scale, p, seed):
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    if p > 0:
        gc.reseed(eng, seed)
    out = route(index, *leaves, N_DST, scale, p)
    out.backward(go)
    return (out.detach(),) + tuple(t.grad for t in leaves)


def check_routes_agree(routes, eng, dev):
    index = make_graph(dev)
    for H, C in SHAPES:
        q, k, v, go = make_qkv(H, C, dev)
        for p in DROPS:
            res = {name: run_route(r, eng, index, q, k, v, go, scale_of(H, C), p, 17) for name, r in routes.items()}
            for name, r in res.items():
                assert all(same_bits(a, b) for a, b in zip(r, res["engine"])), (name, H, C, p)
    # one head given as 2-d tensors
    q, k, v, _ = make_qkv(1, 16, dev)
    for name, r in routes.items():
        a = r(index, q[:, 0].contiguous(), k[:, 0].contiguous(), v[:, 0].contiguous(), N_DST, None, 0.0)
        assert a.shape == (N_DST, 16) and same_bits(a, r(index, q, k, v, N_DST, None, 0.0).squeeze(1)), name


def check_refusals(routes, eng, dev):
    index = make_graph(dev)
    q, k, v, _ = make_qkv(2, 8, dev)
    for name, r in routes.items():
        for dt in (torch.float64, torch.bfloat16, torch.float16):
            for i in range(3):
                args = [q, k, v]
                args[i] = args[i].to(dt)
                with pytest.raises(RuntimeError, match="Float"):
                    r(index, *args, N_DST, None, 0.0)
        with pytest.raises(RuntimeError, match="Cv == C"):
            r(index, q, k, torch.cat([v, v], dim=2), N_DST, None, 0.0)
        for bad in ((q[:, :1], k, v), (q, k[:, :, :4], v), (q, k[:10], v), (q, k, v[:, :1]), (q.reshape(N_DST, -1), k, v)):
            with pytest.raises(RuntimeError):
                r(index, *bad, N_DST, None, 0.0)
        with pytest.raises(RuntimeError):
            r(index, q[:40], k, v, N_DST, None, 0.0)     # 48 destinations, 40 query rows
    with pytest.raises(ValueError):
        eng.dot_attention(index, q, k, v, N_DST, None, 1.0)
    from gammagl_amd.utils import dot_attention

    with pytest.raises(ValueError):
        dot_attention(index, q, k, v, N_DST, None, -0.1)


def check_public_function(eng, dev):
    from gammagl_amd import utils

    index = make_graph(dev)
    q, k, v, go = make_qkv(4, 32, dev)
    a = utils.dot_attention(index, q, k, v, N_DST)
    assert same_bits(a, eng.dot_attention(index, q, k, v, N_DST))
    b = utils.dot_attention(index, q, k, v, N_DST, dropout_rate=0.5, training=False)
    assert same_bits(a, b)
    assert "dot_attention" in utils.__all__


# ---- accuracy against float64 ------------------------------------------------------------------------------------------
def keep_mask(eng, gp, H, C, p, state, dev):
    """the attention-dropout mask [E, H] in the caller's order that a forward reading `state` draws: the alpha the backward
    walk stores for constant logits is zero exactly where the edge was dropped"""
    if p == 0:
        return torch.ones(gp.E, H, dtype=torch.float64, device=dev)
    z = torch.zeros(gp.E, H, device=dev)
    x = torch.ones(gp.N_src, H, C, device=dev)
    out, rmax, rden = ec.raw_forward(eng, gp, z, x, p, state)
    alpha, _, _ = ec.raw_backward(eng, gp, z, x, torch.ones(gp.N_dst, H, C, device=dev), out, rmax, rden, p, state)
    keep = torch.empty_like(alpha)
    perm = gp.fwd.perm
    if perm is None:
        keep.copy_(alpha)
    else:
        keep[perm.long()] = alpha
    return (keep != 0).double() / (1 - p)


def truth_f64(index, q, k, v, go, scale, keep):
    """(out, gq, gk, gv) by torch autograd in float64"""
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    src, dst = index[0], index[1]
    z = scale * (qd[dst] * kd[src]).sum(-1)
    m = torch.full((N_DST, z.shape[1]), -torch.inf, dtype=torch.float64, device=z.device)
    m = m.scatter_reduce(0, dst[:, None].expand_as(z), z.detach(), "amax")
    e = torch.exp(z - m[dst])
    den = torch.zeros_like(m).index_add_(0, dst, e)
    alpha = e / den[dst] * keep
    out = torch.zeros(N_DST, *v.shape[1:], dtype=torch.float64, device=z.device).index_add_(0, dst, alpha[:, :, None] * vd[src])
    out.backward(go.double())
    return out.detach(), qd.grad, kd.grad, vd.grad


def check_against_f64(eng, dev):
    """The composed route's distance from float64 (max |got - truth| / max |truth| per tensor) is the existing ops' accuracy;
    the route the engine takes by default must stay within 4x of it, for out and every gradient, on every shape, dropout
    rate and chunking of the table.  Returns the lines it prints and the two worst values."""
    index = make_graph(dev)
    lines, worst = [], {"composed": 0.0, "default": 0.0}
    for H, C in SHAPES:
        q, k, v, go = make_qkv(H, C, dev)
        scale = scale_of(H, C)
        s32 = float(np.float32(1.0 / math.sqrt(C) if scale is None else scale))
        for p in DROPS:
            for chunk in CHUNKS:
                with forced_chunk(eng, chunk):
                    gp = eng.graph_plan(index, N_DST, N_SRC)
                    state = eng._rng_state(dev).clone()
                    truth = truth_f64(index, q, k, v, go, s32, keep_mask(eng, gp, H, C, p, state, dev))
                    err = {}
                    for name, on in (("composed", False), ("default", True)):
                        old = eng.dot_attn_fused
                        eng.dot_attn_fused = on
                        try:
                            got = run_engine(eng, gp, q, k, v, go, scale, p, state)
                            if not on:
                                assert not eng.stats["dot_attention"]["fused"]
                        finally:
                            eng.dot_attn_fused = old
                        err[name] = [ec.tensor_err(got[i], t) for i, t in zip((0, 2, 3, 4), truth)]
                    line = (f"{H} x {C:2d} p={p} chunk={chunk}  " + "  ".join(
                        f"{n}: out {e[0]:.2e} gq {e[1]:.2e} gk {e[2]:.2e} gv {e[3]:.2e}" for n, e in err.items()))
                    print(line)
                    lines.append(line)
                    for i, what in enumerate(("out", "gq", "gk", "gv")):
                        assert err["composed"][i] < 1e-5, (H, C, p, chunk, what, err["composed"][i])   # a wrong truth shows here
                        assert err["default"][i] <= 4 * err["composed"][i], (H, C, p, chunk, what, err)
                    for n in worst:
                        worst[n] = max(worst[n], max(err[n]))
    print("worst tensor-scale error against float64:", worst)
    return lines, worst


# ---- the first consumer -------------------------------------------------------------------------------------------------
def hgt_toy(dev, seed=5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = {"author": 30, "paper": 45}
    metadata = (["author", "paper"], [("author", "writes", "paper"), ("paper", "cites", "paper"), ("paper", "rev", "author")])
    x = {t: torch.randn(c, 32, generator=g).to(dev) for t, c in n.items()}
    ei = {et: torch.stack([torch.randint(0, n[et[0]], (400,), generator=g),
                           torch.randint(0, n[et[2]], (400,), generator=g)]).to(dev) for et in metadata[1]}
    return metadata, x, ei


def check_hgt(dev, heads=4):
    """HGTConv(fused=True) against fused=False with the same parameters and against a float64 copy: outputs of both node
    types and every parameter gradient"""
    from gammagl_amd.layers import HGTConv

    metadata, x, ei = hgt_toy(dev)
    torch.manual_seed(0)
    fused = HGTConv(32, 32, metadata, heads=heads, fused=True).to(dev)
    with torch.no_grad():
        for name, prm in fused.p_rel.items():
            prm.copy_(torch.linspace(0.5, 1.5, heads))
        for prm in list(fused.a_rel.values()) + list(fused.m_rel.values()):
            prm.mul_(8.0)                          # logits of order one instead of 1e-2
    plain = HGTConv(32, 32, metadata, heads=heads, fused=False).to(dev)
    plain.load_state_dict(fused.state_dict())
    wide = HGTConv(32, 32, metadata, heads=heads, fused=False).to(dev)
    wide.load_state_dict(fused.state_dict())
    wide = wide.double()
    gout = {t: torch.randn(v.shape, generator=torch.Generator().manual_seed(9)).to(dev) for t, v in x.items()}

    def run(layer, dt):
        layer.zero_grad()
        out = layer({t: v.to(dt) for t, v in x.items()}, ei)
        sum((out[t] * gout[t].to(dt)).sum() for t in out).backward()
        return out, {n: p.grad for n, p in layer.named_parameters()}

    of, gf = run(fused, torch.float32)
    op, gp_ = run(plain, torch.float32)
    ow, gw = run(wide, torch.float64)
    assert set(gf) == set(gw) and all(g is not None for g in gf.values())
    for t in of:
        assert of[t].shape == x[t].shape
        assert ec.tensor_err(of[t].detach(), ow[t].detach()) <= 1e-5, t
        assert ec.tensor_err(op[t].detach(), ow[t].detach()) <= 1e-5, t
    for n in gf:
        scale = float(gw[n].abs().max())
        assert scale > 0, n
        assert ec.tensor_err(gf[n], gw[n]) <= 1e-5, (n, ec.tensor_err(gf[n], gw[n]))
        assert ec.tensor_err(gp_[n], gw[n]) <= 1e-5, n
    # eval mode: attention dropout is off on both routes
    fused.dropout_rate = plain.dropout_rate = 0.5
    plain.dropout.p = 0.5
    fused.eval(); plain.eval()
    a, b = fused(x, ei), plain(x, ei)
    for t in a:
        assert same_bits(a[t], of[t].detach()) and torch.allclose(a[t], b[t], atol=1e-5)


# ---- the C ABI, called directly (GPU build) ---------------------------------------------------------------------------------
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def raw_dot_forward(eng, gp, q, k, v, scale, p, rng, with_z=True):
    """(rc, out, rowmax, rowden, z) of ggl_dot_attn_fwd; rng = the {seed, offset} read; z is None with with_z=False"""
    dev = v.device
    H, C = int(v.shape[1]), int(v.shape[2])
    out = torch.empty((gp.N_dst, H, C), dtype=torch.float32, device=dev)
    rmax = torch.empty((gp.N_dst, H), dtype=torch.float32, device=dev)
    rden = torch.empty((gp.N_dst, H), dtype=torch.float32, device=dev)
    z = torch.full((gp.E, H), float("nan"), dtype=torch.float32, device=dev) if with_z else None
    part = eng._gat_partial(gp.fwd, H, C, dev)
    cs = gp.fwd.c_struct(part)
    r = rng.clone() if p > 0 else None
    rc = eng.lib.ggl_dot_attn_fwd(ctypes.byref(cs), _p(gp.col), _p(q), _p(k), _p(v), scale, H, C, p, _p(r), _p(out), _p(rmax),
                                  _p(rden), _p(z), eng._stream(dev))
    return rc, out, rmax, rden, z


def check_c_abi(eng, dev):
    """ggl_dot_attn_fwd through ctypes on every supported shape of the table, dropout off and on, hub row chunked and whole:
    z within the gamma bound of float64; out / rowmax / rowden the bits of ggl_edge_softmax_agg_fwd on that z; out with
    z_out = NULL the bits of out with it.  Unsupported shapes are refused.  Returns the number of supported cases."""
    from gammagl_amd import _lib

    index = make_graph(dev)
    n = 0
    for H, C in SHAPES:
        q, k, v, _ = make_qkv(H, C, dev)
        s32 = float(np.float32(0.37))
        for p in DROPS:
            for chunk in CHUNKS:
                with forced_chunk(eng, chunk):
                    gp = eng.graph_plan(index, N_DST, N_SRC)
                    state = eng._rng_state(dev).clone()
                    if not eng.lib.ggl_dot_attn_supported(H, C):
                        assert C in (12, 5)
                        rc, *_ = raw_dot_forward(eng, gp, q, k, v, s32, p, state)
                        assert rc == _lib.GGL_EINVAL and b"ggl_dot_attn_supported" in eng.lib.ggl_last_error()
                        continue
                    rc, out, rmax, rden, z = raw_dot_forward(eng, gp, q, k, v, s32, p, state)
                    assert rc == 0, eng.lib.ggl_last_error()
                    tag = (H, C, p, chunk)
                    z64, bound = gamma_bound(index, q, k, 0.37, C)
                    assert not bool(torch.isnan(z).any()), tag          # every edge and head was stored
                    assert bool(((z.double() - z64).abs() <= bound).all()), tag
                    ro, rm, rd = ec.raw_forward(eng, gp, z, v, p, state)
                    assert same_bits(out, ro) and same_bits(rmax, rm) and same_bits(rden, rd), tag
                    rc, o2, m2, d2, _ = raw_dot_forward(eng, gp, q, k, v, s32, p, state, with_z=False)
                    assert rc == 0 and same_bits(o2, out) and same_bits(m2, rmax) and same_bits(d2, rden), tag
                    n += 1
    return n
