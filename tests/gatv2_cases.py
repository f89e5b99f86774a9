"""Shared cases of GATv2's additive graph attention (Engine.gatv2_attention, ggl_gatv2_fwd, ggl_gatv2_logit_bwd) for
tests/test_gatv2_host.py (host library, CPU tensors: the composed route) and tests/test_gpu_gatv2.py (MI355X: the fused
forward where ggl_gatv2_supported says so).  Not a test module.  Graph and helpers: tests/dot_attention_cases.py.

The contract: the forward can return the logits it used, z [E, H] in the caller's edge order, and everything behind z is the
existing op bit for bit — out == edge_softmax_aggregate(z, xl), and with gz / gv its logits / x gradients,
g_xr == logit_bwd(plan, gz), g_att == colsum(R of that walk), g_xl == logit_bwd(plan^T, gz, add = gv), where logit_bwd is
ggl_gatv2_logit_bwd, itself held to a serial numpy float32 oracle on the bits.  z is held to
|z - z64| <= gamma_{C+2} sum_c |att_c| |lrelu(xl_c + xr_c)|, which covers every order of summing the C terms (one rounding in the
add, one in the slope multiply, one in the product, C - 1 in the sum).

A *route* is a callable ``f(index, xl, xr, att, n_dst, slope, p) -> out`` that records autograd."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import dot_attention_cases as dc
import edge_softmax_agg_cases as ec
import gat16_cases as gc
from dot_attention_cases import (CHUNKS, DROPS, E, EMPTY, HUB, N_DST, N_SRC, SHAPES, U, forced_chunk, keep_mask,  # noqa: F401
                                 make_graph)
from spmm16_cases import same_bits

SLOPE = 0.2


def make_inputs(H, C, dev, seed=3):
    """xl [N_src, H, C], xr [N_dst, H, C], att [H, C] = randn / sqrt(C) (logits of order one), the output gradient"""
    g = torch.Generator(device="cpu").manual_seed(seed + 100 * H + C)
    xl = torch.randn(N_SRC, H, C, generator=g).to(dev)
    xr = torch.randn(N_DST, H, C, generator=g).to(dev)
    att = (torch.randn(H, C, generator=g) / C ** 0.5).to(dev)
    go = torch.randn(N_DST, H, C, generator=g).to(dev)
    return xl, xr, att, go


def engine_route(eng):
    def f(index, xl, xr, att, n_dst, slope, p):
        return eng.gatv2_attention(index, xl, xr, att, num_nodes=n_dst, negative_slope=slope, dropout_rate=p, training=True)
    return f


def ops_route(ns):
    def f(index, xl, xr, att, n_dst, slope, p):
        return ns.gatv2_attention(index, xl, xr, att, n_dst, slope, p)
    return f


def make_routes(eng):
    from gammagl_amd import cpp_ops, torch_ops

    return {"engine": engine_route(eng), "torch.ops.ggl_attn": ops_route(cpp_ops.load_attn()),
            "torch.ops.gammagl_amd": ops_route(torch_ops.ops)}


def expects_fused(eng, dev, H, C):
    return bool(dev.type == "cuda" and eng.gatv2_fused and eng.lib.ggl_gatv2_supported(H, C)
                and eng.lib.ggl_policy_gatv2_fused(H, C, E, N_SRC))


def run_engine(eng, index, xl, xr, att, go, p, state, need=(True, True, True), slope=SLOPE):
    """(out, z, g_xl, g_xr, g_att) of Engine.gatv2_attention with the rng state set to `state` first"""
    leaves = [t.clone().requires_grad_(n) for t, n in zip((xl, xr, att), need)]
    eng._rng_state(xl.device).copy_(state)
    out, z = eng.gatv2_attention(index, *leaves, num_nodes=N_DST, negative_slope=slope, dropout_rate=p, training=True,
                                 return_logits=True)
    if any(need):
        out.backward(go)
    return (out.detach(), z) + tuple(t.grad for t in leaves)


def gamma_bound(index, xl, xr, att, C, slope=SLOPE):
    """(z64, bound, s64): the logits in float64 from the f32 inputs and the f32 slope, and gamma_{C+2} sum_c |att_c| |lrelu(s_c)|"""
    sl = float(np.float32(slope))
    s = xl.double()[index[0]] + xr.double()[index[1]]
    terms = att.double() * torch.where(s > 0, s, s * sl)
    n = C + 2
    return terms.sum(-1), (n * U / (1 - n * U)) * terms.abs().sum(-1), s


def sign_flips(index, xl, xr, s64):
    """edges x heads x channels whose f32 sum xl + xr falls on the other LeakyReLU branch than the float64 sum (fl(a + b) has
    the sign of a + b: none)"""
    s32 = xl[index[0]] + xr[index[1]]
    return int(((s32 > 0) != (s64 > 0)).sum())


# ---- ggl_gatv2_logit_bwd against a serial oracle ---------------------------------------------------------------------------
def logit_bwd(eng, plan, col, other, self_, gz, att, add=None, want_rows=False, slope=SLOPE):
    """(g_self, att_rows) of ggl_gatv2_logit_bwd over `plan` through ctypes, gz read through the plan's permutation"""
    from gammagl_amd import autograd

    return autograd._gatv2_logit_bwd(eng, plan, col, other, self_, gz, att, slope, add, want_rows)


def oracle_logit_bwd(plan, col, other, self_, gz, att, add=None, slope=SLOPE):
    """The kernel's arithmetic in numpy float32, one rounded operation per step, walking the plan's own rowptr / col / perm:
    positions ascending, a row of more than plan.chunk positions in consecutive pieces of chunk positions, each summed from
    0.0f, the partials merged in ascending order from 0.0f, then the att multiply and the add.  (g_self, att_rows)."""
    f = np.float32
    rowptr = plan.rowptr.cpu().numpy()
    colh = col.cpu().numpy()
    perm = plan.perm if plan.perm is not None else plan.wperm
    permh = None if perm is None else perm.cpu().numpy()
    o, s_, w_, a = (t.detach().cpu().numpy() for t in (other, self_, gz, att))
    sl = f(slope)
    chunk = int(plan.chunk)
    g_self, rows = np.empty_like(s_), np.empty_like(s_)
    zero = np.zeros(s_.shape[1:], dtype=f)

    def piece(r, beg, end):
        accD, accA = zero.copy(), zero.copy()
        for p in range(beg, end):
            e = p if permh is None else permh[p]
            s = o[colh[p]] + s_[r]                                   # __fadd_rn
            w = np.broadcast_to(w_[e][:, None], s.shape)
            accD = accD + np.where(s > 0, w, w * sl)
            accA = accA + w * np.where(s > 0, s, s * sl)
        return accD, accA

    for r in range(plan.N):
        beg, end = int(rowptr[r]), int(rowptr[r + 1])
        if end - beg > chunk:
            accD, accA = zero.copy(), zero.copy()
            for b in range(beg, end, chunk):
                pd, pa = piece(r, b, min(b + chunk, end))
                accD, accA = accD + pd, accA + pa
        else:
            accD, accA = piece(r, beg, end)
        g = a * accD
        g_self[r] = g if add is None else add[r].cpu().numpy() + g
        rows[r] = accA
    assert g_self.dtype == f and rows.dtype == f
    dev = self_.device
    return torch.from_numpy(g_self).to(dev), torch.from_numpy(rows).to(dev)


def check_logit_bwd_oracle(eng, dev, H, C):
    """ggl_gatv2_logit_bwd on the bits of the oracle: g_xr and R on the forward plan, the logit part of g_xl (add = NULL) and
    g_xl with add on the transposed plan, both chunkings; g_att the bits of ggl_colsum_f32 on that R"""
    index = make_graph(dev)
    xl, xr, att, go = make_inputs(H, C, dev)
    g = torch.Generator(device="cpu").manual_seed(11 + H + C)
    gz = torch.randn(E, H, generator=g).to(dev)
    gv = torch.randn(N_SRC, H, C, generator=g).to(dev)
    for chunk in CHUNKS:
        with forced_chunk(eng, chunk):
            gp = eng.graph_plan(index, N_DST, N_SRC)
            assert (gp.fwd.n_long > 0) == (chunk == 8) and (gp.bwd.n_long > 0) == (chunk == 8), chunk
            assert gp.fwd.perm is not None and gp.bwd.perm is not None          # the caller's order is not a sorted one
            tag = (H, C, chunk)
            g_xr, R = logit_bwd(eng, gp.fwd, gp.col, xl, xr, gz, att, None, True)
            o_xr, o_R = oracle_logit_bwd(gp.fwd, gp.col, xl, xr, gz, att)
            assert same_bits(g_xr, o_xr) and same_bits(R, o_R), tag
            g2, none = logit_bwd(eng, gp.fwd, gp.col, xl, xr, gz, att, None, False)       # without att_rows: the same g_xr
            assert none is None and same_bits(g2, g_xr), tag
            assert same_bits(eng.colsum(R.reshape(N_DST, H * C)).reshape(H, C),
                             eng.colsum(o_R.reshape(N_DST, H * C)).reshape(H, C)), tag
            l0, _ = logit_bwd(eng, gp.bwd, gp.colT, xr, xl, gz, att, None, False)
            assert same_bits(l0, oracle_logit_bwd(gp.bwd, gp.colT, xr, xl, gz, att)[0]), tag
            l1, _ = logit_bwd(eng, gp.bwd, gp.colT, xr, xl, gz, att, gv, False)
            assert same_bits(l1, oracle_logit_bwd(gp.bwd, gp.colT, xr, xl, gz, att, gv)[0]), tag
            # the gradient is the same number whichever plan adds it up (loosely: the orders differ)
            t = torch.zeros(N_SRC, H, C, dtype=torch.float64, device=dev)
            s = xl.double()[index[0]] + xr.double()[index[1]]
            t.index_add_(0, index[0], att.double() * gz.double()[:, :, None] * torch.where(s > 0, 1.0, float(np.float32(SLOPE))))
            assert ec.tensor_err(l0, t) < 1e-5, tag


# ---- the contract --------------------------------------------------------------------------------------------------------
def check_contract(eng, dev, H, C, p):
    """§1 for one head shape and dropout rate, the hub row chunked and in one piece; returns the routes taken"""
    index = make_graph(dev)
    xl, xr, att, go = make_inputs(H, C, dev)
    taken = []
    for chunk in CHUNKS:
        with forced_chunk(eng, chunk):
            gp = eng.graph_plan(index, N_DST, N_SRC)
            assert (gp.fwd.n_long > 0) == (chunk == 8), chunk
            rows = torch.bincount(index[1], minlength=N_DST)
            assert rows[HUB] >= E // 3 and all(rows[r] == 0 for r in EMPTY)
            state = eng._rng_state(dev).clone()
            out, z, g_xl, g_xr, g_att = run_engine(eng, gp, xl, xr, att, go, p, state)
            fused = eng.stats["gatv2_attention"]["fused"]
            assert fused == expects_fused(eng, dev, H, C), (H, C, "route")
            taken.append(fused)
            tag = (H, C, p, chunk, "fused" if fused else "composed")
            # z: the error bound that holds for any order of the C terms; no LeakyReLU branch differs from float64's
            z64, bound, s64 = gamma_bound(index, xl, xr, att, C)
            assert sign_flips(index, xl, xr, s64) == 0, tag
            assert z.shape == (E, H) and bool(((z.double() - z64).abs() <= bound).all()), tag
            # everything behind z: the existing op on that z, bit for bit
            za, va = z.clone().requires_grad_(True), xl.clone().requires_grad_(True)
            eng._rng_state(dev).copy_(state)
            ref = eng.edge_softmax_aggregate(gp, za, va, N_DST, p, True)
            ref.backward(go)
            gz, gv = za.grad, va.grad
            assert same_bits(out, ref.detach()), tag
            if p == 0:
                assert float(out[list(EMPTY)].abs().max()) == 0.0, tag
            r_xr, R = logit_bwd(eng, gp.fwd, gp.col, xl, xr, gz, att, None, True)
            assert same_bits(g_xr, r_xr), tag                                           # gz has the existing op's bits
            assert float(g_xr[list(EMPTY)].abs().max()) == 0.0, tag
            assert same_bits(g_att, eng.colsum(R.reshape(N_DST, H * C)).reshape(H, C)), tag
            r_xl, _ = logit_bwd(eng, gp.bwd, gp.colT, xr, xl, gz, att, gv, False)
            assert same_bits(g_xl, r_xl), tag                                           # ... and gv
            # the same forward with nothing to differentiate: the same out, no logits saved
            o2, z2, *_ = run_engine(eng, gp, xl, xr, att, go, p, state, need=(False, False, False))
            assert same_bits(o2, out) and same_bits(z2, z), tag
            eng._rng_state(dev).copy_(state)
            o3 = eng.gatv2_attention(gp, xl, xr, att, N_DST, SLOPE, p, True)
            assert same_bits(o3, out) and o3.grad_fn is None, tag
            st = eng.stats["gatv2_attention"]
            assert not st["logits_saved"] and (st["logits_bytes"] == 0) == fused, (tag, st)
            # two identical calls, identical bits
            again = run_engine(eng, gp, xl, xr, att, go, p, state)
            assert all(same_bits(a, b) for a, b in zip(again, (out, z, g_xl, g_xr, g_att))), tag
    return taken


def check_one_sided_gradients(eng, dev, H=2, C=16):
    """every subset of (xl, xr, att) requiring grad: None for the others, the same bits for the rest"""
    index = make_graph(dev)
    xl, xr, att, go = make_inputs(H, C, dev)
    state = eng._rng_state(dev).clone()
    full = run_engine(eng, index, xl, xr, att, go, 0.5, state)
    for m in range(1, 7):
        need = tuple(bool(m >> i & 1) for i in range(3))
        part = run_engine(eng, index, xl, xr, att, go, 0.5, state, need)
        assert same_bits(part[0], full[0])
        for i, n in enumerate(need):
            assert (part[2 + i] is None) != n and (not n or same_bits(part[2 + i], full[2 + i])), (need, i)


def check_single_needs_against_the_aggregate(routes, eng, dev, H=2, C=16, seed=23):
    """Only xl's gradient asked, only xr's, only att's, through every route: out has the bits of the SAME route's
    edge_softmax_aggregate on the returned z under the same rng state, and the one gradient those of ggl_gatv2_logit_bwd on
    that op's gz (and, for g_xl, with its x gradient gv added — held to the serial oracle as well); the gradients nobody asked
    for are None.  Pins which of (gz, gv) the shared backward forms."""
    index = make_graph(dev)
    xl, xr, att, go = make_inputs(H, C, dev)
    aggregate = ec.make_routes(eng)
    for name, route in routes.items():
        for chunk in dc.route_chunks(name):
            with forced_chunk(eng, chunk) if chunk else contextlib.nullcontext():
                gp = eng.graph_plan(index, N_DST, N_SRC)
                for p in DROPS:
                    tag = (name, chunk, p)
                    state = eng._rng_state(dev).clone()
                    _, z, *_ = run_engine(eng, gp, xl, xr, att, go, p, state, need=(False, False, False))
                    za, va = z.clone().requires_grad_(True), xl.clone().requires_grad_(True)
                    gc.reseed(eng, seed)
                    ref = aggregate[name](index, za, va, N_DST, p)
                    ref.backward(go)
                    gz, gv = za.grad, va.grad
                    want = (lambda: logit_bwd(eng, gp.bwd, gp.colT, xr, xl, gz, att, gv, False)[0],
                            lambda: logit_bwd(eng, gp.fwd, gp.col, xl, xr, gz, att, None, False)[0],
                            lambda: eng.colsum(logit_bwd(eng, gp.fwd, gp.col, xl, xr, gz, att, None, True)[1]
                                               .reshape(N_DST, H * C)).reshape(H, C))
                    for i in range(3):
                        leaves = [t.clone().requires_grad_(j == i) for j, t in enumerate((xl, xr, att))]
                        gc.reseed(eng, seed)
                        out = route(index, *leaves, N_DST, SLOPE, p)
                        out.backward(go)
                        assert same_bits(out.detach(), ref.detach()), (tag, i)
                        assert same_bits(leaves[i].grad, want[i]()), (tag, i)
                        assert all(t.grad is None for j, t in enumerate(leaves) if j != i), (tag, i)
                        if i == 0:
                            assert same_bits(leaves[0].grad, oracle_logit_bwd(gp.bwd, gp.colT, xr, xl, gz, att, gv)[0]), tag


def run_route(route, eng, index, xl, xr, att, go, p, seed):
    leaves = [t.clone().requires_grad_(True) for t in (xl, xr, att)]
    if p > 0:
        gc.reseed(eng, seed)
    out = route(index, *leaves, N_DST, SLOPE, p)
    out.backward(go)
    return (out.detach(),) + tuple(t.grad for t in leaves)


def check_routes_agree(routes, eng, dev):
    index = make_graph(dev)
    for H, C in SHAPES:
        xl, xr, att, go = make_inputs(H, C, dev)
        for p in DROPS:
            res = {name: run_route(r, eng, index, xl, xr, att, go, p, 17) for name, r in routes.items()}
            for name, r in res.items():
                assert all(same_bits(a, b) for a, b in zip(r, res["engine"])), (name, H, C, p)
    # one head given as 2-d tensors and a 1-d att
    xl, xr, att, _ = make_inputs(1, 16, dev)
    for name, r in routes.items():
        a = r(index, xl[:, 0].contiguous(), xr[:, 0].contiguous(), att[0].contiguous(), N_DST, SLOPE, 0.0)
        assert a.shape == (N_DST, 16) and same_bits(a, r(index, xl, xr, att, N_DST, SLOPE, 0.0).squeeze(1)), name


def check_refusals(routes, eng, dev):
    index = make_graph(dev)
    xl, xr, att, _ = make_inputs(2, 8, dev)
    for name, r in routes.items():
        for dt in (torch.float64, torch.bfloat16, torch.float16):
            for i in range(3):
                args = [xl, xr, att]
                args[i] = args[i].to(dt)
                with pytest.raises(RuntimeError, match="expected scalar type Float"):
                    r(index, *args, N_DST, SLOPE, 0.0)
        for bad_att in (att[:1], att[:, :4], att.reshape(-1), att[None]):       # att is not [H, C]
            with pytest.raises(RuntimeError, match=r"att \[H, C\]"):
                r(index, xl, xr, bad_att, N_DST, SLOPE, 0.0)
        with pytest.raises(RuntimeError):
            r(index, xl, xr[:40], att, N_DST, SLOPE, 0.0)                        # 48 destinations, 40 rows of xr
        for bad in ((xl[:, :1], xr, att), (xl, xr[:, :, :4], att), (xl[:10], xr, att)):
            with pytest.raises((RuntimeError, IndexError)):
                r(index, *bad, N_DST, SLOPE, 0.0)
    for bad_p in (1.0, -0.1):
        with pytest.raises(ValueError):
            eng.gatv2_attention(index, xl, xr, att, N_DST, SLOPE, bad_p)
        from gammagl_amd.utils import gatv2_attention

        with pytest.raises(ValueError):
            gatv2_attention(index, xl, xr, att, N_DST, SLOPE, bad_p)
        with pytest.raises(RuntimeError, match="dropout_rate"):
            routes["torch.ops.ggl_attn"](index, xl, xr, att, N_DST, SLOPE, bad_p)


def check_public_function(eng, dev):
    from gammagl_amd import utils

    index = make_graph(dev)
    xl, xr, att, go = make_inputs(4, 32, dev)
    a = utils.gatv2_attention(index, xl, xr, att, N_DST)
    assert same_bits(a, eng.gatv2_attention(index, xl, xr, att, N_DST))
    b = utils.gatv2_attention(index, xl, xr, att, N_DST, dropout_rate=0.5, training=False)
    assert same_bits(a, b)
    assert "gatv2_attention" in utils.__all__


# ---- accuracy against float64 ------------------------------------------------------------------------------------------
def truth_f64(index, xl, xr, att, go, slope, keep):
    """(out, g_xl, g_xr, g_att) by torch autograd in float64"""
    ld, rd, ad = (t.double().requires_grad_(True) for t in (xl, xr, att))
    src, dst = index[0], index[1]
    z = (ad * torch.nn.functional.leaky_relu(ld[src] + rd[dst], slope)).sum(-1)
    m = torch.full((N_DST, z.shape[1]), -torch.inf, dtype=torch.float64, device=z.device)
    m = m.scatter_reduce(0, dst[:, None].expand_as(z), z.detach(), "amax")
    e = torch.exp(z - m[dst])
    den = torch.zeros_like(m).index_add_(0, dst, e)
    alpha = e / den[dst] * keep
    out = torch.zeros(N_DST, *xl.shape[1:], dtype=torch.float64, device=z.device).index_add_(0, dst, alpha[:, :, None] * ld[src])
    out.backward(go.double())
    return out.detach(), ld.grad, rd.grad, ad.grad


def check_against_f64(eng, dev):
    """out, g_xl, g_xr and g_att of the route the engine takes by default within the project's 1e-5 of the tensor's maximum of
    torch autograd in float64 with the forward's keep mask, on every shape, dropout rate and chunking of the table.  Prints
    and returns the worst value per tensor."""
    index = make_graph(dev)
    names = ("out", "g_xl", "g_xr", "g_att")
    worst = dict.fromkeys(names, 0.0)
    s32 = float(np.float32(SLOPE))
    for H, C in SHAPES:
        xl, xr, att, go = make_inputs(H, C, dev)
        for p in DROPS:
            for chunk in CHUNKS:
                with forced_chunk(eng, chunk):
                    gp = eng.graph_plan(index, N_DST, N_SRC)
                    state = eng._rng_state(dev).clone()
                    truth = truth_f64(index, xl, xr, att, go, s32, keep_mask(eng, gp, H, C, p, state, dev))
                    got = run_engine(eng, gp, xl, xr, att, go, p, state)
                    err = [ec.tensor_err(got[i], t) for i, t in zip((0, 2, 3, 4), truth)]
                    print(f"{H} x {C:2d} p={p} chunk={chunk} fused={eng.stats['gatv2_attention']['fused']}  "
                          + "  ".join(f"{n} {e:.2e}" for n, e in zip(names, err)))
                    for n, e in zip(names, err):
                        assert e <= 1e-5, (H, C, p, chunk, n, e)
                        worst[n] = max(worst[n], e)
    print("worst tensor-scale error against float64:", {n: f"{e:.2e}" for n, e in worst.items()})
    return worst


# ---- the layer --------------------------------------------------------------------------------------------------------------
def conv_toy(dev, n=60, e=700, f=24, seed=6):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(n, f, generator=g).to(dev)
    ei = torch.stack([torch.randint(0, n, (e,), generator=g), torch.randint(0, n - 3, (e,), generator=g)]).to(dev)
    gout = torch.randn(n, 64, generator=g).to(dev)
    return x, ei, gout


def _run_layer(layer, x, ei, gout, dt):
    layer.zero_grad()
    out = layer(x.to(dt), ei, x.shape[0])
    (out * gout[:, :out.shape[1]].to(dt)).sum().backward()
    return out.detach(), {n: p.grad for n, p in layer.named_parameters()}


def check_conv_paper(dev, heads=4, C=8):
    """GATv2Conv(variant="paper"), fused=True and fused=False, against a float64 copy: outputs and every parameter gradient
    within 1e-5, share_weights and concat both ways; eval mode turns attention dropout off on both routes"""
    from gammagl_amd.layers import GATv2Conv

    x, ei, gout = conv_toy(dev)
    for share in (False, True):
        for concat in (True, False):
            torch.manual_seed(1)
            fused = GATv2Conv(x.shape[1], C, heads=heads, concat=concat, share_weights=share, fused=True).to(dev)
            with torch.no_grad():
                fused.bias.normal_()
            names = {n for n, _ in fused.named_parameters()}
            assert names == ({"lin_l.weight", "lin_l.bias", "att", "bias"} | (set() if share else {"lin_r.weight", "lin_r.bias"}))
            assert fused.att.shape == (heads, C) and fused.bias.shape == ((heads * C,) if concat else (C,))
            plain = GATv2Conv(x.shape[1], C, heads=heads, concat=concat, share_weights=share, fused=False).to(dev)
            plain.load_state_dict(fused.state_dict())
            wide = GATv2Conv(x.shape[1], C, heads=heads, concat=concat, share_weights=share, fused=False).to(dev)
            wide.load_state_dict(fused.state_dict())
            wide = wide.double()
            of, gf = _run_layer(fused, x, ei, gout, torch.float32)
            op, gp_ = _run_layer(plain, x, ei, gout, torch.float32)
            ow, gw = _run_layer(wide, x, ei, gout, torch.float64)
            tag = (share, concat)
            assert of.shape == (x.shape[0], heads * C if concat else C), tag
            assert ec.tensor_err(of, ow) <= 1e-5 and ec.tensor_err(op, ow) <= 1e-5, tag
            assert set(gf) == set(gw) and all(g is not None for g in gf.values())
            for n in gf:
                assert float(gw[n].abs().max()) > 0, (tag, n)
                assert ec.tensor_err(gf[n], gw[n]) <= 1e-5, (tag, n, ec.tensor_err(gf[n], gw[n]))
                assert ec.tensor_err(gp_[n], gw[n]) <= 1e-5, (tag, n)
            fused.dropout_rate = plain.dropout_rate = 0.5
            plain.dropout.p = 0.5
            fused.eval(); plain.eval()
            a, b = fused(x, ei, x.shape[0]), plain(x, ei, x.shape[0])
            assert same_bits(a.detach(), of) and torch.allclose(a, b, atol=1e-5), tag


def check_conv_reference(dev, heads=4, C=8):
    """GATv2Conv(variant="reference") against the reference's message formula restated here in float64:
    weight = mean_c(lrelu(x[src]) * att_src + lrelu(x[dst]) * att_dst) -> segment softmax -> x[src] * alpha, summed"""
    from gammagl_amd.layers import GATv2Conv

    x, ei, gout = conv_toy(dev)
    n = x.shape[0]
    src, dst = ei[0], ei[1]
    for concat in (True, False):
        torch.manual_seed(2)
        fused = GATv2Conv(x.shape[1], C, heads=heads, concat=concat, fused=True, variant="reference").to(dev)
        assert {k for k, _ in fused.named_parameters()} == {"linear.weight", "att_src", "att_dst", "bias"}
        assert fused.att_src.shape == fused.att_dst.shape == (1, heads, C)
        with torch.no_grad():
            fused.bias.normal_()
            fused.att_src.mul_(20.0); fused.att_dst.mul_(20.0)          # logits of order one instead of 1e-2
        plain = GATv2Conv(x.shape[1], C, heads=heads, concat=concat, fused=False, variant="reference").to(dev)
        plain.load_state_dict(fused.state_dict())
        prm = {k: v.detach().double().requires_grad_(True) for k, v in fused.named_parameters()}
        h = (x.double() @ prm["linear.weight"].t()).reshape(-1, heads, C)
        lr = torch.nn.functional.leaky_relu
        w = (lr(h[src], 0.2) * prm["att_src"] + lr(h[dst], 0.2) * prm["att_dst"]).mean(-1)
        m = torch.full((n, heads), -torch.inf, dtype=torch.float64, device=dev)
        m = m.scatter_reduce(0, dst[:, None].expand_as(w), w.detach(), "amax")
        ex = torch.exp(w - m[dst])
        alpha = ex / (torch.zeros_like(m).index_add_(0, dst, ex)[dst] + 1e-16)
        agg = torch.zeros(n, heads, C, dtype=torch.float64, device=dev).index_add_(0, dst, h[src] * alpha[:, :, None])
        ow = (agg.reshape(n, heads * C) if concat else agg.mean(1)) + prm["bias"]
        (ow * gout[:, :ow.shape[1]].double()).sum().backward()
        for layer in (fused, plain):
            o, g = _run_layer(layer, x, ei, gout, torch.float32)
            assert ec.tensor_err(o, ow.detach()) <= 1e-5, (concat, layer.fused)
            for k in prm:
                if k == "att_dst":
                    # the destination term is the same for every edge of a softmax row, so it cancels: the exact gradient
                    # is zero (float64 leaves 1e-17 of rounding), and the yardstick is att_src's gradient
                    scale = float(prm["att_src"].grad.abs().max())
                    assert float(prm[k].grad.abs().max()) <= 1e-12 * scale
                    assert float(g[k].abs().max()) <= 1e-5 * scale, (concat, layer.fused, k)
                    continue
                assert ec.tensor_err(g[k], prm[k].grad) <= 1e-5, (concat, layer.fused, k, ec.tensor_err(g[k], prm[k].grad))


# ---- the C ABI, called directly (GPU build) ---------------------------------------------------------------------------------
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def raw_gatv2_forward(eng, gp, xl, xr, att, p, rng, with_z=True, slope=SLOPE):
    """(rc, out, rowmax, rowden, z) of ggl_gatv2_fwd; rng = the {seed, offset} read; z (pre-filled with NaN) is None with
    with_z=False"""
    dev = xl.device
    H, C = int(xl.shape[1]), int(xl.shape[2])
    out = torch.empty((gp.N_dst, H, C), dtype=torch.float32, device=dev)
    rmax = torch.empty((gp.N_dst, H), dtype=torch.float32, device=dev)
    rden = torch.empty((gp.N_dst, H), dtype=torch.float32, device=dev)
    z = torch.full((gp.E, H), float("nan"), dtype=torch.float32, device=dev) if with_z else None
    part = eng._gat_partial(gp.fwd, H, C, dev)
    cs = gp.fwd.c_struct(part)
    r = rng.clone() if (p > 0 and rng is not None) else None
    rc = eng.lib.ggl_gatv2_fwd(ctypes.byref(cs), _p(gp.col), _p(xl), _p(xr), _p(att), slope, H, C, p, _p(r), _p(out), _p(rmax),
                               _p(rden), _p(z), eng._stream(dev))
    return rc, out, rmax, rden, z


def check_c_abi(eng, dev):
    """ggl_gatv2_fwd through ctypes on every supported shape of the table, dropout off and on, hub row chunked and whole: every
    z element written and within the gamma bound of float64; out / rowmax / rowden the bits of ggl_edge_softmax_agg_fwd on that
    z; out with z_out = NULL the bits of out with it.  Unsupported widths are refused and the refusal names
    ggl_gatv2_supported.  Returns the number of supported cases."""
    from gammagl_amd import _lib

    index = make_graph(dev)
    n = 0
    for H, C in SHAPES:
        xl, xr, att, _ = make_inputs(H, C, dev)
        for p in DROPS:
            for chunk in CHUNKS:
                with forced_chunk(eng, chunk):
                    gp = eng.graph_plan(index, N_DST, N_SRC)
                    state = eng._rng_state(dev).clone()
                    if not eng.lib.ggl_gatv2_supported(H, C):
                        assert C in (12, 5)
                        rc, *_ = raw_gatv2_forward(eng, gp, xl, xr, att, p, state)
                        assert rc == _lib.GGL_EINVAL and b"ggl_gatv2_supported" in eng.lib.ggl_last_error()
                        continue
                    rc, out, rmax, rden, z = raw_gatv2_forward(eng, gp, xl, xr, att, p, state)
                    assert rc == 0, eng.lib.ggl_last_error()
                    tag = (H, C, p, chunk)
                    z64, bound, _ = gamma_bound(index, xl, xr, att, C)
                    assert not bool(torch.isnan(z).any()), tag          # every edge and head was stored
                    assert bool(((z.double() - z64).abs() <= bound).all()), tag
                    ro, rm, rd = ec.raw_forward(eng, gp, z, xl, p, state)
                    assert same_bits(out, ro) and same_bits(rmax, rm) and same_bits(rden, rd), tag
                    rc, o2, m2, d2, _ = raw_gatv2_forward(eng, gp, xl, xr, att, p, state, with_z=False)
                    assert rc == 0 and same_bits(o2, out) and same_bits(m2, rmax) and same_bits(d2, rden), tag
                    n += 1
    return n
