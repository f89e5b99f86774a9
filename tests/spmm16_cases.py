"""Shared cases of the mixed-precision aggregate (ggl_spmm_{sum,mean,mean_bwd}_x16: bf16 / f16 storage, f32 arithmetic, one
rounding at the store) for tests/test_spmm16_host.py (host library, CPU tensors), tests/test_gpu_spmm16.py (MI355X) and the
AddressSanitizer run.  Not a test module.

A *route* is a callable ``f(reduce, index, weight, x, out_f32=False) -> out`` that records autograd.  The three routes:
the ctypes engine (``Engine.c_spmm_sum / c_spmm_mean``), ``torch.ops.ggl`` (C++ registered) and ``torch.ops.gammagl_amd``.

The contract (include/ggl_mpops.h), with F = the SAME route on the upcast rows:
    route(x16)               == F(x16.float()).to(x16.dtype)         bit for bit
    route(x16, out_f32=True) == F(x16.float())                       bit for bit
    x16.grad                 == (F's gradient on g.float()).to(x16.dtype)
Every comparison is torch.equal on the integer view of the bits: no tolerance anywhere.
"""
import ctypes

import pytest
import torch

DTYPES = (torch.bfloat16, torch.float16)
WIDTHS = (1, 7, 8, 47, 64, 96, 256, 264)
KINDS = ("uniform", "power", "empty_rows", "duplicates", "no_edges", "sorted")


def bits(t):
    """the integer view of a tensor's bits"""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def engine_route(eng):
    def f(reduce, index, weight, x, out_f32=False):
        fn = {"sum": eng.c_spmm_sum, "mean": eng.c_spmm_mean}[reduce]
        return fn(index, weight, x, out_dtype=torch.float32) if out_f32 else fn(index, weight, x)
    return f


def ops_route(ns):
    """`ns` = torch.ops.ggl (cpp_ops.load()) or torch.ops.gammagl_amd (torch_ops.ops)"""
    def f(reduce, index, weight, x, out_f32=False):
        if out_f32:
            return {"sum": ns.spmm_sum_x16, "mean": ns.spmm_mean_x16}[reduce](index, weight, x, True)
        return {"sum": ns.spmm_sum, "mean": ns.spmm_mean}[reduce](index, weight, x)
    return f


def make_routes(eng):
    from gammagl_amd import cpp_ops, torch_ops

    return {"engine": engine_route(eng), "torch.ops.ggl": ops_route(cpp_ops.load()),
            "torch.ops.gammagl_amd": ops_route(torch_ops.ops)}


def make_index(kind, N, E, gen, dev):
    """edge_index [2, E] int64 of a square graph on N nodes"""
    if kind == "no_edges":
        return torch.zeros((2, 0), dtype=torch.int64, device=dev)
    src = torch.randint(0, N, (E,), generator=gen, device=dev)
    if kind == "power":         # rows of thousands of edges next to one-edge rows
        dst = (N * torch.rand(E, generator=gen, device=dev) ** 3).long().clamp_(max=N - 1)
    elif kind == "empty_rows":  # two thirds of the rows receive nothing
        dst = torch.randint(0, max(N // 3, 1), (E,), generator=gen, device=dev) * 3 % N
    else:
        dst = torch.randint(0, N, (E,), generator=gen, device=dev)
    if kind == "duplicates":    # every edge four times
        src, dst = src[: E // 4].repeat(4), dst[: E // 4].repeat(4)
    if kind == "sorted":
        dst = torch.sort(dst).values
    return torch.stack([src, dst]).contiguous()


def check_contract_case(route, index, w, x16, g16, reduce, name=""):
    """both equalities of the contract and the backward, for one (route, graph, weights, rows, reduce)"""
    dt = x16.dtype
    tag = (name, reduce, str(dt), tuple(x16.shape), w is not None)
    xf = x16.float().requires_grad_(True)
    want = route(reduce, index, w, xf)                     # F: today's f32 op on the same index and weights
    assert want.dtype == torch.float32
    want.backward(g16.float())
    xa = x16.clone().requires_grad_(True)
    out = route(reduce, index, w, xa)
    assert same_bits(out.detach(), want.detach().to(dt)), ("16-bit output", tag)
    out.backward(g16)
    assert same_bits(xa.grad, xf.grad.to(dt)), ("gradient", tag)
    xb = x16.clone().requires_grad_(True)
    out32 = route(reduce, index, w, xb, True)
    assert same_bits(out32.detach(), want.detach()), ("f32 output", tag)
    out32.backward(g16.float())
    assert same_bits(xb.grad, xf.grad.to(dt)), ("gradient of the f32 output", tag)


def check_contract(routes, dev, kinds=KINDS, widths=WIDTHS, dtypes=DTYPES, N=300, E=6000, seed=0):
    n = 0
    for kind in kinds:
        gen = torch.Generator(device=dev).manual_seed(seed + len(kind))
        index = make_index(kind, N, E, gen, dev)
        w = torch.rand(index.shape[1], generator=gen, device=dev)
        for K in widths:
            x = torch.randn(N, K, generator=gen, device=dev)
            g = torch.randn(N, K, generator=gen, device=dev)
            for dt in dtypes:
                for ww in (w, None):
                    for reduce in ("sum", "mean"):
                        for name, route in routes.items():
                            check_contract_case(route, index, ww, x.to(dt), g.to(dt), reduce, f"{name}/{kind}")
                            n += 1
    return n


def check_long_rows(eng, dev, widths=(7, 8, 64, 264), chunk=64, N=300, E=20_000, seed=3):
    """a plan whose long-row table is not empty (small chunk, power-law ids), through Engine.spmm on the explicit plan"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    index = make_index("power", N, E, gen, dev)
    w = torch.rand(E, generator=gen, device=dev)
    old = eng.chunk
    eng.chunk = chunk
    try:
        gp = eng.graph_plan(index, N)
        assert gp.fwd.n_long > 0 and gp.fwd.chunk == chunk, "the plan is meant to have rows longer than its chunk"

        def route(reduce, index_, weight, x, out_f32=False):
            return eng.spmm(gp, weight, x, reduce, out_dtype=torch.float32 if out_f32 else None)

        for K in widths:
            x = torch.randn(N, K, generator=gen, device=dev)
            g = torch.randn(N, K, generator=gen, device=dev)
            for dt in DTYPES:
                for ww in (w, None):
                    for reduce in ("sum", "mean"):
                        check_contract_case(route, index, ww, x.to(dt), g.to(dt), reduce, "explicit plan")
        return gp
    finally:
        eng.chunk = old


def check_column_blocks(eng, dev, K=256, chunk=64, N=50, E=5000, seed=11):
    """ggl_spmm_{sum,mean}_x16 in column blocks (col_block16 = 128, thresholds lowered: two blocks of a 256-wide row) on a
    plan with long rows, the hub rows walked once per aggregate (hub_one_launch = 1) and once per block (0), out in x's dtype
    and in f32: the bits of the one-launch call (col_block16 = 0)."""
    from parity_cases import option

    gen = torch.Generator(device=dev).manual_seed(seed)
    index = make_index("power", N, E, gen, dev)
    index[0, E - 1500:] = 11
    w = torch.rand(E, generator=gen, device=dev)
    x = torch.randn(N, K, generator=gen, device=dev)
    old = eng.chunk
    eng.chunk = chunk
    try:
        gp = eng.graph_plan(index, N)
        assert gp.fwd.n_long >= 2 and gp.fwd.chunk == chunk
        blocks = lambda: int(eng.lib.ggl_spmm_col_blocks_x16(ctypes.byref(gp.fwd.c_struct(None)), K))  # noqa: E731
        with option(eng, "col_block_min_edges", 0), option(eng, "col_block_min_degree", 0):
            for dt in DTYPES:
                for reduce in ("sum", "mean"):
                    for od in (None, torch.float32):
                        with option(eng, "col_block16", 0):
                            assert blocks() == 1
                            want = eng.spmm(gp, w, x.to(dt), reduce, out_dtype=od)
                        for one in (1, 0):
                            with option(eng, "col_block16", 128), option(eng, "hub_one_launch", one):
                                assert blocks() == 2
                                got = eng.spmm(gp, w, x.to(dt), reduce, out_dtype=od)
                            assert same_bits(got, want), (dt, reduce, od, one)
                assert same_bits(want, eng.spmm(gp, w, x.to(dt).float(), "mean"))   # (the last `want`: mean, f32 output)
    finally:
        eng.chunk = old


def check_accepts(dev):
    """mpops.gspmm takes 16-bit rows and returns them (on the parent commit: RuntimeError "expected scalar type Float")"""
    from gammagl_amd import mpops

    gen = torch.Generator(device=dev).manual_seed(1)
    ei = make_index("uniform", 50, 400, gen, dev)
    w = torch.rand(400, generator=gen, device=dev)
    x = torch.randn(50, 24, generator=gen, device=dev)
    for dt in DTYPES:
        for reduce in ("sum", "mean"):
            for ww in (w, None):
                out = mpops.gspmm(ei, ww, x.to(dt), reduce)
                assert out.dtype == dt and out.shape == x.shape, (dt, reduce)


def check_refusals(routes, dev):
    """what was refused is still refused, with "Float" in the message"""
    from gammagl_amd import mpops

    gen = torch.Generator(device=dev).manual_seed(2)
    ei = make_index("uniform", 50, 400, gen, dev)
    w = torch.rand(400, generator=gen, device=dev)
    x = torch.randn(50, 8, generator=gen, device=dev)
    for reduce in ("sum", "mean"):
        with pytest.raises(RuntimeError, match="Float"):
            mpops.gspmm(ei, w, x.double(), reduce)
        for name, route in routes.items():
            with pytest.raises(RuntimeError, match="Float"):
                route(reduce, ei, w, x.double())
            for wd in (torch.bfloat16, torch.float16, torch.float64):
                for xd in (torch.float32, torch.bfloat16):
                    with pytest.raises(RuntimeError, match="Float"):
                        route(reduce, ei, w.to(wd), x.to(xd))
    for dt in DTYPES:
        with pytest.raises(RuntimeError, match="Float"):
            mpops.gspmm(ei, w, x.to(dt), "max")
        with pytest.raises(RuntimeError, match="Float"):
            mpops.bspmm(ei, torch.rand(400, 2, generator=gen, device=dev), x.to(dt).reshape(50, 2, 4))


def check_f32_accumulation(routes, dev):
    """4096 edges into one row of ones: exactly 4096.0 in bf16 and f16 — a storage-type running sum stalls at 256 / 2048,
    which is what unsorted_segment_sum on the same 16-bit messages still (and on purpose) returns"""
    from gammagl_amd import mpops

    n = 4096
    ei = torch.stack([torch.arange(n, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)])
    for dt, stall in ((torch.bfloat16, 256.0), (torch.float16, 2048.0)):
        x = torch.ones(n, 8, dtype=dt, device=dev)
        for name, route in routes.items():
            for reduce, want in (("sum", 4096.0), ("mean", 1.0)):
                out = route(reduce, ei, None, x)
                assert out.dtype == dt and torch.equal(out[0].float(), torch.full((8,), want, device=dev)), (name, dt, reduce)
                assert torch.equal(out[1:].float(), torch.zeros(n - 1, 8, device=dev))
        assert torch.equal(mpops.gspmm(ei, None, x, "sum")[0].float(), torch.full((8,), 4096.0, device=dev))
        seg = mpops.unsorted_segment_sum(x[ei[0]], ei[1], n)
        assert seg.dtype == dt and torch.equal(seg[0].float(), torch.full((8,), stall, device=dev)), (dt, seg[0])


def check_gcnconv(dev):
    """GCNConv on bf16 rows == linear -> mixed-precision aggregate -> torch epilogue, written out"""
    from gammagl_amd import layers, mpops

    torch.manual_seed(0)
    gen = torch.Generator(device=dev).manual_seed(4)
    N = 120
    ei = layers.add_self_loops(make_index("uniform", N, 900, gen, dev), N)
    x = torch.randn(N, 20, generator=gen, device=dev).bfloat16()
    for n_out in (16, 7, 47):
        conv = layers.GCNConv(20, n_out).to(dev)
        with torch.no_grad():
            conv.bias.copy_(torch.randn(1, n_out, generator=gen, device=dev))
        for epi in (None, (True, 0.0, True)):
            with torch.autocast(dev.type, dtype=torch.bfloat16):
                got = conv(x, ei, None, N, _epilogue=epi)
                h = torch.nn.functional.linear(x, conv.linear.weight)
            assert h.dtype == torch.bfloat16
            w = conv._norm_weights(ei, None, N, dev)      # deg^-1/2 of both ends, f32
            agg = mpops.gspmm(ei, w, h.contiguous(), "sum")
            assert agg.dtype == torch.bfloat16
            want = agg + conv.bias.detach().to(torch.bfloat16)
            if epi is not None:
                want = torch.relu(want)
            assert got.dtype == torch.bfloat16 and same_bits(got.detach(), want), (n_out, epi)


def check_model_autocast(dev):
    """GCNModel forward + backward under autocast(bf16): f32 parameters, f32 gradients, a finite loss that moves"""
    from gammagl_amd import layers
    from gammagl_amd.trainer import GCNTrainer

    gen = torch.Generator(device=dev).manual_seed(5)
    N = 400
    ei = layers.add_self_loops(make_index("power", N, 6000, gen, dev), N)
    x = torch.randn(N, 32, generator=gen, device=dev)
    y = torch.randint(0, 5, (N,), generator=gen, device=dev)
    torch.manual_seed(0)
    net = layers.GCNModel(32, 16, 5, drop_rate=0.2, num_layers=3).to(dev)
    net.train()
    with torch.autocast(dev.type, dtype=torch.bfloat16):
        logits = net(x, ei, None, N)
    assert logits.dtype == torch.bfloat16
    torch.nn.functional.cross_entropy(logits.float(), y).backward()
    for p in net.parameters():
        assert p.dtype == torch.float32 and p.grad is not None and p.grad.dtype == torch.float32
        assert bool(torch.isfinite(p.grad).all())
    idx = torch.arange(0, N, 2, device=dev)
    for amp in (torch.bfloat16, torch.float16):
        tr = GCNTrainer(32, 16, 5, num_layers=2, drop_rate=0.0, device=dev, amp_dtype=amp)
        assert (tr.scaler is not None) == (amp == torch.float16)
        losses = [float(tr.step(x, ei, y, idx, N)) for _ in range(8)]
        assert all(l == l for l in losses) and losses[-1] < losses[0], (amp, losses)
        assert all(p.dtype == torch.float32 for p in tr.net.parameters())
        assert all(s.dtype == torch.float32 for st in tr.opt.state.values() for s in st.values()
                   if torch.is_tensor(s) and s.is_floating_point())
