"""Shared cases of the fused GAT on 16-bit rows (ggl_gat_fused_{fwd,bwd_dst,bwd_src}_x16: bf16 / f16 storage of x, g, out and
gx; f32 softmax, sums and statistics; one rounding at the store) for tests/test_gat16_host.py (host library, CPU tensors) and
tests/test_gpu_gat16.py (MI355X).  Not a test module.

A *route* is a callable ``f(index, el, er, x, slope, n_dst, p, out_f32=False) -> out`` that records autograd.  The three
routes: the ctypes engine (``Engine.gat_fused``), ``torch.ops.ggl`` (C++ registered) and ``torch.ops.gammagl_amd``.

The contract (include/ggl_mpops.h).  F is the GENERAL f32 op on the same plan, called through the C ABI
(``ggl_gat_fused_fwd / _bwd_dst / _bwd_src``: never the fast path, which is held to a tolerance):
    out(x16)           == F.out(x16.float()).to(x16.dtype)         out(x16, out_f32) == F.out(x16.float())
    rowmax, rowden     == F's
    alpha / de, gel, ger == F_bwd(x16.float(), g.float(), out.float(), rowmax, rowden)'s,   gx == that gx .to(x16.dtype)
where `out` in the backward is the tensor the 16-bit forward RETURNED.  With p_drop > 0 both sides read the same
{seed, offset}.  Every comparison is torch.equal on the integer view of the bits: no tolerance anywhere.
"""
import ctypes

import pytest
import torch

import spmm16_cases as sc
from spmm16_cases import DTYPES, KINDS, same_bits

# H x C: the smallest shapes at which each load form and kernel form can go wrong
SHAPES = ((1, 1),      # element form
          (3, 5),      # odd, rows of 30 bytes
          (4, 4),      # 8-byte loads
          (2, 12),     # C % 4, not % 8
          (8, 8),      # 16-byte loads; a fast-path shape in f32
          (16, 16),    # H = 16, CREG = 16
          (4, 24),     # the wide backward kernel on the GPU
          (8, 41),     # padded to 44 where the policy pads
          (1, 320))    # C > 256: the wide kernel does not apply
N, E = 200, 3000
RECT = (260, 90)       # N_src, N_dst of the rectangular block
SLOPE = 0.2


def engine_route(eng):
    def f(index, el, er, x, slope, n_dst, p, out_f32=False):
        return eng.gat_fused(index, el, er, x, slope, num_nodes=n_dst, dropout_rate=p, training=True,
                             out_dtype=torch.float32 if out_f32 else None)
    return f


def ops_route(ns):
    """`ns` = torch.ops.ggl (cpp_ops.load()) or torch.ops.gammagl_amd (torch_ops.ops)"""
    def f(index, el, er, x, slope, n_dst, p, out_f32=False):
        if out_f32:
            return ns.gat_fused_x16(index, el, er, x, slope, n_dst, p, True)
        return ns.gat_fused(index, el, er, x, slope, n_dst, p)
    return f


def make_routes(eng):
    from gammagl_amd import cpp_ops, torch_ops

    return {"engine": engine_route(eng), "torch.ops.ggl": ops_route(cpp_ops.load()),
            "torch.ops.gammagl_amd": ops_route(torch_ops.ops)}


def reseed(eng, seed):
    """every route's next forward reads {draw(seed), 0}: the engine and torch.ops.ggl keep a state each, both seeded from torch's
    CPU generator on first use"""
    from gammagl_amd import cpp_ops

    eng.reseed()
    cpp_ops.load().reseed()
    torch.manual_seed(seed)


def drawn_rng(seed, dev):
    """the {seed, offset} a route's forward reads after reseed(eng, seed)"""
    torch.manual_seed(seed)
    return torch.tensor([int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item()), 0], dtype=torch.int64, device=dev)


def make_graph(kind, gen, dev):
    """(edge_index, N_src, N_dst)"""
    if kind == "rectangular":
        ns, nd = RECT
        return torch.stack([torch.randint(0, ns, (E,), generator=gen, device=dev),
                            torch.randint(0, nd, (E,), generator=gen, device=dev)]).contiguous(), ns, nd
    return sc.make_index(kind, N, E, gen, dev), N, N


def make_inputs(n_src, n_dst, H, C, gen, dev):
    """f32 el [N_src, H], er [N_dst, H], x [N_src, H, C], g [N_dst, H, C] (rounded to a dtype by the caller)"""
    return (torch.randn(n_src, H, generator=gen, device=dev), torch.randn(n_dst, H, generator=gen, device=dev),
            torch.randn(n_src, H, C, generator=gen, device=dev), torch.randn(n_dst, H, C, generator=gen, device=dev))


# ---- the C ABI, called directly: F (f32) and the 16-bit entry points on the same plan ---------------------------------------
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_CODE = {torch.float16: 5, torch.bfloat16: 6, torch.float32: 7, torch.float64: 8}


def raw_forward(eng, gp, el, er, x, p, rng, out_dtype=None):
    """(out, rowmax, rowden) of ggl_gat_fused_fwd (f32 x) or ggl_gat_fused_fwd_x16 (16-bit x); rng = {seed, offset} read"""
    dev = x.device
    H, C = int(x.shape[1]), int(x.shape[2])
    out = torch.empty((gp.N_dst, H, C), dtype=out_dtype or x.dtype, device=dev)
    rmax = torch.empty((gp.N_dst, H), dtype=torch.float32, device=dev)
    rden = torch.empty((gp.N_dst, H), dtype=torch.float32, device=dev)
    part = None
    if gp.fwd.n_long > 0:
        part = torch.empty(eng.lib.ggl_gat_partial_bytes(gp.fwd.n_chunks, H, C) + 16, dtype=torch.uint8, device=dev)
    cs = gp.fwd.c_struct(part)
    r = rng.clone() if p > 0 else None        # the launch advances the offset of the state it is given
    st = eng._stream(dev)
    if x.dtype == torch.float32:
        eng._check(eng.lib.ggl_gat_fused_fwd(ctypes.byref(cs), _p(gp.col), _p(el), _p(er), _p(x), SLOPE, H, C, p, _p(r),
                                             _p(out), _p(rmax), _p(rden), st))
    else:
        eng._check(eng.lib.ggl_gat_fused_fwd_x16(ctypes.byref(cs), _p(gp.col), _p(el), _p(er), _CODE[x.dtype], _p(x), SLOPE,
                                                 H, C, p, _p(r), _CODE[out.dtype], _p(out), _p(rmax), _p(rden), st))
    return out, rmax, rden


def raw_backward(eng, gp, el, er, x, g, out, rmax, rden, p, rng):
    """(alpha/de [E, H, 2], gel, ger, gx) of the two backward walks: f32 everywhere, or the 16-bit entry points"""
    dev = x.device
    H, C = int(x.shape[1]), int(x.shape[2])
    ad = torch.zeros((max(gp.E, 1), H, 2), dtype=torch.float32, device=dev)
    alpha, de = ad.data_ptr(), ad.data_ptr() + 4
    ger = torch.empty((gp.N_dst, H), dtype=torch.float32, device=dev)
    gel = torch.empty((gp.N_src, H), dtype=torch.float32, device=dev)
    gx = torch.empty((gp.N_src, H, C), dtype=x.dtype, device=dev)
    part_f = eng._partial(gp.fwd, torch.float32, H, False, dev)
    part_t = eng._partial(gp.bwd, torch.float32, H * C + H, False, dev)
    cs, csT = gp.fwd.c_struct(part_f), gp.bwd.c_struct(part_t)
    r = rng if p > 0 else None
    st = eng._stream(dev)
    if x.dtype == torch.float32:
        eng._check(eng.lib.ggl_gat_fused_bwd_dst(ctypes.byref(cs), _p(gp.col), None, _p(el), _p(er), _p(x), _p(g), _p(out),
                                                 _p(rmax), _p(rden), SLOPE, H, C, p, _p(r), alpha, de, _p(ger), None, st))
        eng._check(eng.lib.ggl_gat_fused_bwd_src(ctypes.byref(csT), _p(gp.colT), _p(gp.posT), alpha, de, _p(g), H, C,
                                                 _p(gx), _p(gel), st))
    else:
        xc, gc = _CODE[x.dtype], _CODE[g.dtype]
        eng._check(eng.lib.ggl_gat_fused_bwd_dst_x16(ctypes.byref(cs), _p(gp.col), _p(el), _p(er), xc, _p(x), gc, _p(g),
                                                     _CODE[out.dtype], _p(out), _p(rmax), _p(rden), SLOPE, H, C, p, _p(r),
                                                     alpha, de, _p(ger), st))
        eng._check(eng.lib.ggl_gat_fused_bwd_src_x16(ctypes.byref(csT), _p(gp.colT), _p(gp.posT), alpha, de, gc, _p(g), H, C,
                                                     xc, _p(gx), _p(gel), st))
    return ad, gel, ger, gx


def padded(eng, gp, x, g=None):
    """x (and g) with the zero channels Engine.gat_fused / torch.ops.ggl add where ggl_policy_head_channels asks for them"""
    C = int(x.shape[2])
    Cp = int(eng.lib.ggl_policy_head_channels(C, gp.E, int(x.shape[0])))
    pad = lambda t: t if t is None or Cp == C else torch.nn.functional.pad(t, (0, Cp - C)).contiguous()  # noqa: E731
    return pad(x), pad(g)


def reference(eng, gp, el, er, x16, g16, p, rng):
    """F on the widened rows, once per (graph, shape, dtype, p): the forward, and the backward for either output dtype fed
    the widened output the 16-bit forward returns (F.out rounded for a 16-bit out, F.out itself for an f32 out)"""
    dt, C = x16.dtype, int(x16.shape[2])
    xp, gp16 = padded(eng, gp, x16, g16)
    xf, gf = xp.float(), gp16.float()
    out, rmax, rden = raw_forward(eng, gp, el, er, xf, p, rng)
    ref = {"out": out[:, :, :C], "rmax": rmax, "rden": rden, "C": C}
    for out_f32 in (False, True):
        seen = out if out_f32 else out.to(dt).float()
        ad, gel, ger, gx = raw_backward(eng, gp, el, er, xf, gf, seen, rmax, rden, p, rng)
        ref[out_f32] = {"ad": ad, "gel": gel, "ger": ger, "gx": gx[:, :, :C].to(dt)}
    return ref


def check_raw(eng, gp, el, er, x16, g16, p, rng, ref, tag):
    """the C entry points themselves: out, statistics, alpha / de, gel, ger, gx"""
    dt, C = x16.dtype, ref["C"]
    xp, gp16 = padded(eng, gp, x16, g16)
    for out_f32 in (False, True):
        od = torch.float32 if out_f32 else dt
        out, rmax, rden = raw_forward(eng, gp, el, er, xp, p, rng, od)
        assert same_bits(out[:, :, :C], ref["out"].to(od)), ("out", out_f32, tag)
        assert same_bits(rmax, ref["rmax"]) and same_bits(rden, ref["rden"]), ("statistics", out_f32, tag)
        ad, gel, ger, gx = raw_backward(eng, gp, el, er, xp, gp16.to(od), out, rmax, rden, p, rng)
        want = ref[out_f32]
        assert same_bits(ad, want["ad"]), ("alpha / de", out_f32, tag)
        assert same_bits(gel, want["gel"]) and same_bits(ger, want["ger"]), ("gel / ger", out_f32, tag)
        assert same_bits(gx[:, :, :C], want["gx"]), ("gx", out_f32, tag)


def run_route(route, eng, index, el, er, x16, g, n_dst, p, out_f32, seed):
    """(out, gel, ger, gx) of one route, forward + backward through autograd"""
    ea, ra, xa = (t.clone().requires_grad_(True) for t in (el, er, x16))
    if p > 0:
        reseed(eng, seed)
    out = route(index, ea, ra, xa, SLOPE, n_dst, p, out_f32)
    out.backward(g)
    return out.detach(), ea.grad, ra.grad, xa.grad


def check_routes(routes, eng, index, el, er, x16, g16, n_dst, p, seed, ref, tag):
    """every route against F, hence against each other"""
    dt = x16.dtype
    for out_f32 in (False, True):
        od = torch.float32 if out_f32 else dt
        want = ref[out_f32]
        for name, route in routes.items():
            out, gel, ger, gx = run_route(route, eng, index, el, er, x16, g16.to(od), n_dst, p, out_f32, seed)
            t = (name, out_f32, tag)
            assert same_bits(out, ref["out"].to(od)), ("out", t)
            assert same_bits(gel, want["gel"]) and same_bits(ger, want["ger"]), ("gel / ger", t)
            assert same_bits(gx, want["gx"]), ("gx", t)


def check_contract(routes, eng, dev, kind, shapes=SHAPES, dtypes=DTYPES, drops=(0.0, 0.5), seed=0):
    """§3 over the shape table on one graph kind: both dtypes, p_drop in {0, 0.5}, 16-bit and f32 out, the C ABI and the
    three routes.  Returns the number of (shape, dtype, p) cases."""
    gen = torch.Generator(device=dev).manual_seed(seed + len(kind))
    index, n_src, n_dst = make_graph(kind, gen, dev)
    gp = eng.graph_plan(index, n_dst, n_src)
    n = 0
    for H, C in shapes:
        el, er, x, g = make_inputs(n_src, n_dst, H, C, gen, dev)
        for dt in dtypes:
            x16, g16 = x.to(dt), g.to(dt)
            for p in drops:
                tag = (kind, H, C, str(dt), p)
                sd = 11 + n
                rng = drawn_rng(sd, dev)
                ref = reference(eng, gp, el, er, x16, g16, p, rng)
                check_raw(eng, gp, el, er, x16, g16, p, rng, ref, tag)
                check_routes(routes, eng, index, el, er, x16, g16, n_dst, p, sd, ref, tag)
                n += 1
    return n


def check_accepts(routes, dev):
    """gat_fused takes 16-bit x on every route and returns x's dtype (on the parent commit: "expected scalar type Float")"""
    gen = torch.Generator(device=dev).manual_seed(1)
    ei = sc.make_index("uniform", 50, 400, gen, dev)
    el, er, x, _ = make_inputs(50, 50, 4, 8, gen, dev)
    for dt in DTYPES:
        for name, route in routes.items():
            out = route(ei, el, er, x.to(dt), SLOPE, 50, 0.0)
            assert out.dtype == dt and out.shape == x.shape, (name, dt)
            assert route(ei, el, er, x.to(dt), SLOPE, 50, 0.0, True).dtype == torch.float32, (name, dt)


def check_refusals(routes, eng, dev):
    """what was refused is still refused: 16-bit el / er, f64 x, an out_dtype that is neither x's nor f32"""
    gen = torch.Generator(device=dev).manual_seed(2)
    ei = sc.make_index("uniform", 50, 400, gen, dev)
    el, er, x, _ = make_inputs(50, 50, 4, 8, gen, dev)
    for name, route in routes.items():
        with pytest.raises(RuntimeError, match="Float"):
            route(ei, el, er, x.double(), SLOPE, 50, 0.0)
        for dt in DTYPES + (torch.float64,):
            for xd in (torch.float32, torch.bfloat16):
                with pytest.raises(RuntimeError, match="Float"):
                    route(ei, el.to(dt), er, x.to(xd), SLOPE, 50, 0.0)
                with pytest.raises(RuntimeError, match="Float"):
                    route(ei, el, er.to(dt), x.to(xd), SLOPE, 50, 0.0)
    for xd, od in ((torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16), (torch.bfloat16, torch.float64),
                   (torch.float32, torch.bfloat16)):
        with pytest.raises(RuntimeError, match="out_dtype"):
            eng.gat_fused(ei, el, er, x.to(xd), SLOPE, num_nodes=50, out_dtype=od)
    with pytest.raises(ValueError):
        eng.gat_fused(ei, el, er, x.bfloat16(), SLOPE, num_nodes=50, dropout_rate=1.0)


def check_long_rows(eng, dev, shapes=((3, 5), (2, 12), (8, 8)), chunk=64, n=300, e=20_000, seed=3):
    """the contract on a plan with long rows in BOTH directions (small chunk, power-law ids on both ends): the hub-chunk items,
    the f32 partials and the merges that round only at the final store"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    dst = (n * torch.rand(e, generator=gen, device=dev) ** 3).long().clamp_(max=n - 1)
    src = (n * torch.rand(e, generator=gen, device=dev) ** 3).long().clamp_(max=n - 1)
    index = torch.stack([src, dst]).contiguous()
    old = eng.chunk
    eng.chunk = chunk
    try:
        gp = eng.graph_plan(index, n)
        assert gp.fwd.n_long > 0 and gp.bwd.n_long > 0 and gp.fwd.chunk == chunk, "long rows both ways are the point"
        route = {"engine on the plan": engine_route(eng)}
        k = 0
        for H, C in shapes:
            el, er, x, g = make_inputs(n, n, H, C, gen, dev)
            for dt in DTYPES:
                for p in (0.0, 0.5):
                    x16, g16 = x.to(dt), g.to(dt)
                    tag = ("long rows", H, C, str(dt), p)
                    rng = drawn_rng(40 + k, dev)
                    ref = reference(eng, gp, el, er, x16, g16, p, rng)
                    check_raw(eng, gp, el, er, x16, g16, p, rng, ref, tag)
                    check_routes(route, eng, gp, el, er, x16, g16, n, p, 40 + k, ref, tag)
                    k += 1
        return gp
    finally:
        eng.chunk = old


def check_f32_accumulation(routes, dev):
    """4096 edges into one destination, el = er = 0, x all ones: every alpha is 1 / 4096 and the weighted sum is exactly 1.0
    with rowden exactly 4096.0 — a storage-type running sum of the 4096 equal terms stalls at 256 (bf16) or 2048 (f16)"""
    from gammagl_amd import cpp_ops

    n = 4096
    ei = torch.stack([torch.arange(n, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)])
    el, er = torch.zeros(n, 2, device=dev), torch.zeros(n, 2, device=dev)
    for dt in DTYPES:
        x = torch.ones(n, 2, 8, dtype=dt, device=dev)
        for name, route in routes.items():
            out = route(ei, el, er, x, SLOPE, n, 0.0)
            assert out.dtype == dt and torch.equal(out[0].float(), torch.ones(2, 8, device=dev)), (name, dt, out[0])
            assert torch.equal(out[1:].float(), torch.zeros(n - 1, 2, 8, device=dev)), (name, dt)
        _, rmax, rden, _, fast = cpp_ops.load().gat_fused_forward(ei, el, er, x, SLOPE, n, 0.0)
        assert not fast and torch.equal(rden[0], torch.full((2,), 4096.0, device=dev)) and \
            torch.equal(rmax[0], torch.zeros(2, device=dev)), (dt, rden[0])


def check_alignment(eng, dev, shapes=((3, 5), (2, 12), (8, 8), (4, 24))):
    """x16, g16 (and the out the backward reads) as contiguous views that start ONE element into their buffers — 2-byte
    aligned panels take the element form — give the aligned call's bits"""
    gen = torch.Generator(device=dev).manual_seed(6)
    index, n_src, n_dst = make_graph("uniform", gen, dev)
    gp = eng.graph_plan(index, n_dst, n_src)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 4 == 2
        return v

    for H, C in shapes:
        el, er, x, g = make_inputs(n_src, n_dst, H, C, gen, dev)
        for dt in DTYPES:
            for p in (0.0, 0.5):
                x16, g16 = x.to(dt), g.to(dt)
                rng = drawn_rng(70, dev)
                out, rmax, rden = raw_forward(eng, gp, el, er, x16, p, rng)
                want = raw_backward(eng, gp, el, er, x16, g16, out, rmax, rden, p, rng)
                xs, gs = shifted(x16), shifted(g16)
                out_s, rmax_s, rden_s = raw_forward(eng, gp, el, er, xs, p, rng)
                tag = (H, C, str(dt), p)
                assert same_bits(out_s, out) and same_bits(rmax_s, rmax) and same_bits(rden_s, rden), ("forward", tag)
                got = raw_backward(eng, gp, el, er, xs, gs, shifted(out), rmax, rden, p, rng)
                for a, b, what in zip(got, want, ("alpha / de", "gel", "ger", "gx")):
                    assert same_bits(a, b), (what, tag)
                # through autograd too: the engine hands the view's pointer on
                xa = xs.detach().requires_grad_(True)
                o = eng.gat_fused(gp, el, er, xa, SLOPE, num_nodes=n_dst)
                assert same_bits(o.detach(), raw_forward(eng, gp, el, er, x16, 0.0, rng)[0]), ("engine", tag)


def check_layer_parts(eng, dev):
    """FusedGATConv under autocast == its parts, bit for bit: the GEMM under autocast (a 16-bit panel), f32 el / er from it,
    the engine's 16-bit gat_fused, torch's finish — concat and head-mean layers, and a head width the layer pads"""
    from gammagl_amd import layers

    gen = torch.Generator(device=dev).manual_seed(4)
    n = 120
    ei = layers.add_self_loops(sc.make_index("uniform", n, 900, gen, dev), n)
    x = torch.randn(n, 20, generator=gen, device=dev)
    for dt in DTYPES:
        for H, C, concat in ((4, 8, True), (4, 8, False), (2, 9, True)):
            torch.manual_seed(0)
            conv = layers.FusedGATConv(20, C, heads=H, concat=concat).to(dev)
            with torch.no_grad():
                conv.bias.copy_(torch.randn(conv.bias.shape, generator=gen, device=dev))
            pad = (-C) % 4 if C >= 8 else 0
            with torch.no_grad(), torch.autocast(dev.type, dtype=dt):
                got = conv(x, ei, n)
                w = conv.w
                if pad:
                    w = torch.nn.functional.pad(w.reshape(-1, H, C), (0, pad)).reshape(-1, H * (C + pad))
                h = (x @ w).reshape(-1, H, C + pad)
                assert h.dtype == dt
                hf = h[:, :, :C].float()
                el = (hf * conv.att[:, :, :C]).sum(dim=-1)
                er = (hf * conv.att[:, :, C:]).sum(dim=-1)
                assert el.dtype == torch.float32 and er.dtype == torch.float32
                agg = eng.gat_fused(ei, el, er, h, conv.negative_slope, num_nodes=n)
                assert agg.dtype == dt
                want = conv._finish(agg[:, :, :C] if pad else agg)
            assert got.dtype == want.dtype == torch.float32            # the f32 bias promotes the sum
            assert same_bits(got, want), (dt, H, C, concat)


def check_model_autocast(dev):
    """GATModel forward + backward under autocast: finite f32 logits, f32 parameters with finite f32 gradients"""
    from gammagl_amd import layers

    gen = torch.Generator(device=dev).manual_seed(5)
    n = 400
    ei = layers.add_self_loops(sc.make_index("power", n, 6000, gen, dev), n)
    x = torch.randn(n, 32, generator=gen, device=dev)
    y = torch.randint(0, 5, (n,), generator=gen, device=dev)
    for dt in DTYPES:
        torch.manual_seed(0)
        net = layers.GATModel(32, 8, 5, heads=8, drop_rate=0.2, num_layers=2).to(dev)
        net.train()
        with torch.autocast(dev.type, dtype=dt):
            logits = net(x, ei, n)
        assert logits.dtype == torch.float32 and logits.shape == (n, 5) and bool(torch.isfinite(logits).all()), dt
        torch.nn.functional.cross_entropy(logits, y).backward()
        for prm in net.parameters():
            assert prm.dtype == torch.float32 and prm.grad is not None and prm.grad.dtype == torch.float32
            assert bool(torch.isfinite(prm.grad).all()), dt
