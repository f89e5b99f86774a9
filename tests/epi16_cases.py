"""Shared cases of the fused epilogue on 16-bit rows (ggl_spmm_epi_x16, ggl_bias_act_{fwd,bwd}_x16: bf16 / f16 storage, f32
arithmetic, one rounding at the store) for tests/test_epi16_host.py (host library, CPU tensors) and tests/test_gpu_epi16.py
(MI355X).  Not a test module.

The contract (include/ggl_mpops.h), F = today's f32 op of the SAME route on the widened inputs, run right after
the same ``eng.reseed(seed)``:
    out16 == F(x16.float(), add16.float(), bias, relu, p).to(dtype)          out32 == F(...)        bit for bit, mask included
    ga16  == bias_act_bwd_f32(g16.float(), y16.float(), ...).ga.to(dtype)     gbias == that call's gbias (f32, same bits)
    gx16  == (transposed f32 aggregate of ga16.float()).to(dtype)             gadd == ga16     gw == spmm_grad_w(x16, ga16)
Every comparison is on the bits (spmm16_cases.same_bits): no tolerance anywhere.
"""
import ctypes

import pytest
import torch

from spmm16_cases import DTYPES, bits, make_index, same_bits  # noqa: F401

KINDS = ("uniform", "power", "empty_rows", "duplicates", "no_edges", "sorted")
WIDTHS = (1, 7, 8, 12, 44, 48, 64, 96, 256, 264)
SEED = 1234
# (add, bias, relu, p, mean)
FORMS = {
    "nothing": (False, False, False, 0.0, False),
    "bias": (False, True, False, 0.0, False),
    "bias_relu": (False, True, True, 0.0, False),
    "bias_relu_drop": (False, True, True, 0.5, False),
    "add_bias_relu_mean": (True, True, True, 0.0, True),
    "drop_no_relu": (False, False, False, 0.5, False),
}


class EngineRoute:
    """Engine.spmm_epi / Engine.bias_act and the engine's own f32 primitives as the reference's steps"""
    name = "engine"
    has_f32_out = True

    def __init__(self, eng):
        self.eng = eng

    def plan(self, index, N):
        return self.eng.graph_plan(index, N)

    def fwd(self, index, N, w, x, mean, add, bias, relu, p, out_f32=False):
        return self.eng.spmm_epi(self.plan(index, N), w, x, "mean" if mean else "sum", add, bias, relu, p, True,
                                 out_dtype=torch.float32 if out_f32 else None)

    def bias_act(self, a, bias, relu, p):
        return self.eng.bias_act(a, bias, relu, p, True)

    def used(self, dev, p):
        """the {seed, offset} the next forward reads (call right after reseed)"""
        return self.eng._rng_state(dev).clone() if p > 0 else None

    def epi_bwd(self, g, y, bias, relu, p, used):
        return self.eng._epi_bwd(g, y, relu, p, used, None if bias is None else bias.shape)

    def aggT(self, index, N, w, ga, mean):
        return self.eng._spmm_bwd_x(self.plan(index, N), w, ga, ga.dtype, mean)

    def state(self, dev):
        return self.eng._rng_state(dev).clone()


class GglRoute:
    """torch.ops.ggl.spmm_epi / bias_act and the registered forward / backward ops as the reference's steps"""
    name = "torch.ops.ggl"
    has_f32_out = False

    def __init__(self, eng):
        from gammagl_amd import cpp_ops

        self.eng, self.C = eng, cpp_ops.load()

    def fwd(self, index, N, w, x, mean, add, bias, relu, p, out_f32=False):
        return self.C.spmm_epi(index, w, x, mean, add, bias, relu, p)

    def bias_act(self, a, bias, relu, p):
        return self.C.bias_act(a, bias, relu, p)

    def used(self, dev, p):
        if not p > 0:
            return torch.empty(0, dtype=torch.int64, device=dev)
        used = self.C.bias_act_forward(torch.zeros(1, 4, device=dev), None, False, p)[1]
        self.eng.reseed(SEED)      # (that draw moved the state: back to where the forward under test starts)
        return used

    def epi_bwd(self, g, y, bias, relu, p, used):
        ga, gb = self.C.bias_act_backward(g, y, bias is not None, relu, p, used)
        return ga, (gb.reshape(bias.shape) if bias is not None else None)

    def aggT(self, index, N, w, ga, mean):
        return (self.C.spmm_mean_backward if mean else self.C.spmm_sum_backward)(index, w, ga)

    def state(self, dev):
        return None


def make_routes(eng):
    return [EngineRoute(eng), GglRoute(eng)]


def check_case(route, dev, index, N, w, x16, g16, form, name="", w_grad=False):
    """the forward and the stepwise backward contract for one (route, graph, weights, rows, epilogue form)"""
    eng = route.eng
    has_add, has_bias, relu, p, mean = FORMS[form]
    dt, K = x16.dtype, x16.shape[1]
    tag = (route.name, name, form, str(dt), K, w is not None)
    gen = torch.Generator(device=dev).manual_seed(K + len(form))
    add16 = torch.randn(N, K, generator=gen, device=dev).to(dt) if has_add else None
    bias = torch.randn(1, K, generator=gen, device=dev) if has_bias else None
    # F: today's f32 op on the widened inputs, twice (the second call reads the state the first one left)
    eng.reseed(SEED)
    with torch.no_grad():
        af = add16.float() if has_add else None
        want = route.fwd(index, N, w, x16.float(), mean, af, bias, relu, p)
        want2 = route.fwd(index, N, w, x16.float(), mean, af, bias, relu, p)
        st32 = route.state(dev) if p > 0 else None
    assert want.dtype == torch.float32
    # the 16-bit op
    eng.reseed(SEED)
    used = route.used(dev, p)
    xa = x16.clone().requires_grad_(True)
    aa = add16.clone().requires_grad_(True) if has_add else None
    ba = bias.clone().requires_grad_(True) if has_bias else None
    wa = w.clone().requires_grad_(True) if (w is not None and w_grad) else w
    out = route.fwd(index, N, wa, xa, mean, aa, ba, relu, p)
    assert out.dtype == dt and same_bits(out.detach(), want.to(dt)), ("16-bit output", tag)
    with torch.no_grad():
        out2 = route.fwd(index, N, w, x16, mean, add16, bias, relu, p)
    assert same_bits(out2, want2.to(dt)), ("second call: the state moved as the f32 op moves it", tag)
    if p > 0 and st32 is not None:
        assert torch.equal(route.state(dev), st32), ("rng state after two calls", tag)
    if route.has_f32_out:
        eng.reseed(SEED)
        with torch.no_grad():
            out32 = route.fwd(index, N, w, x16, mean, add16, bias, relu, p, out_f32=True)
        assert same_bits(out32, want), ("f32 output", tag)
    # backward, step by step on the stored values
    out.backward(g16)
    y16 = out.detach()
    ga_ref, gb_ref = route.epi_bwd(g16.float(), y16.float(), bias, relu, p, used)
    ga16 = ga_ref.to(dt)
    gx_ref = route.aggT(index, N, w, ga16.float(), mean).to(dt)
    assert xa.grad.dtype == dt and same_bits(xa.grad, gx_ref), ("gx", tag)
    if has_add:
        assert same_bits(aa.grad, ga16), ("ga (add's gradient)", tag)
    if has_bias:
        assert ba.grad.dtype == torch.float32 and same_bits(ba.grad, gb_ref), ("gbias", tag)
    if w is not None and w_grad:
        gw_ref = eng._spmm_grad_w(eng.graph_plan(index, N), x16, ga16, mean)
        assert wa.grad.dtype == torch.float32 and same_bits(wa.grad, gw_ref.view(w.shape)), ("gw", tag)


def check_contract(routes, dev, N=300, E=6000, seed=0):
    """every kind at K = 64, every width on `power`; both dtypes, sum / mean by form, weights and None, all six forms"""
    n = 0
    for kind in KINDS:
        gen = torch.Generator(device=dev).manual_seed(seed + len(kind))
        index = make_index(kind, N, E, gen, dev)
        w = torch.rand(index.shape[1], generator=gen, device=dev)
        for K in (WIDTHS if kind == "power" else (64,)):
            x = torch.randn(N, K, generator=gen, device=dev)
            g = torch.randn(N, K, generator=gen, device=dev)
            for dt in DTYPES:
                for ww in (w, None):
                    for form in FORMS:
                        for route in routes:
                            check_case(route, dev, index, N, ww, x.to(dt), g.to(dt), form, kind,
                                       w_grad=(form == "bias_relu" and route.name == "engine"))
                            n += 1
    return n


def check_mean_forms(routes, dev, N=300, E=6000):
    """the forms FORMS runs with sum, with mean as well (bias + ReLU + dropout, dropout alone) at three width classes"""
    gen = torch.Generator(device=dev).manual_seed(21)
    index = make_index("power", N, E, gen, dev)
    w = torch.rand(E, generator=gen, device=dev)
    old = dict(FORMS)
    try:
        FORMS["mean_bias_relu_drop"] = (False, True, True, 0.5, True)
        FORMS["mean_drop_no_relu"] = (True, False, False, 0.5, True)
        for K in (7, 44, 64):
            x = torch.randn(N, K, generator=gen, device=dev)
            g = torch.randn(N, K, generator=gen, device=dev)
            for dt in DTYPES:
                for route in routes:
                    for form in ("mean_bias_relu_drop", "mean_drop_no_relu"):
                        check_case(route, dev, index, N, w, x.to(dt), g.to(dt), form, "power")
    finally:
        FORMS.clear()
        FORMS.update(old)


def check_kept_share(eng, dev, N=300, K=64):
    """dropout 0.5 without ReLU on [300, 64] outputs: the kept share lies in 0.5 +- 0.02 (5.5 standard deviations of the
    binomial: a guard against an all-kept or all-dropped mask, not a measurement)"""
    gen = torch.Generator(device=dev).manual_seed(8)
    index = make_index("uniform", N, 6000, gen, dev)
    index = torch.cat([index, torch.arange(N, device=dev).repeat(2, 1)], dim=1)     # every row receives something
    x = (torch.rand(N, K, generator=gen, device=dev) + 0.5)
    for dt in DTYPES:
        eng.reseed(SEED)
        out = eng.spmm_epi(eng.graph_plan(index, N), None, x.to(dt), "sum", None, None, False, 0.5, True)
        share = float((out != 0).float().mean())
        assert abs(share - 0.5) <= 0.02, (dt, share)


def check_accepts(eng, dev):
    """Engine.spmm_epi / bias_act and torch.ops.ggl.spmm_epi / bias_act take bf16 / f16 tensors and return them (on the parent
    commit: RuntimeError "expected scalar type Float")"""
    from gammagl_amd import cpp_ops

    C = cpp_ops.load()
    gen = torch.Generator(device=dev).manual_seed(1)
    ei = make_index("uniform", 50, 400, gen, dev)
    x = torch.randn(50, 24, generator=gen, device=dev)
    bias = torch.randn(24, generator=gen, device=dev)
    gp = eng.graph_plan(ei, 50)
    for dt in DTYPES:
        x16 = x.to(dt)
        for out in (eng.spmm_epi(gp, None, x16, "mean", x16, bias, True, 0.0), eng.bias_act(x16, bias, True, 0.0),
                    C.spmm_epi(ei, None, x16, True, x16, bias, True, 0.0), C.bias_act(x16, bias, True, 0.0)):
            assert out.dtype == dt and out.shape == x.shape, dt
        assert eng.spmm_epi(gp, None, x16, "sum", None, bias, True, 0.0, out_dtype=torch.float32).dtype == torch.float32


def check_sage_accepts(dev):
    """SAGEConv (both branches) and GraphSAGEFullModel run under autocast and return 16-bit activations; the model's backward
    leaves finite f32 gradients on f32 parameters (on the parent commit: RuntimeError, or f32 activations)"""
    from gammagl_amd import layers

    gen = torch.Generator(device=dev).manual_seed(2)
    N = 120
    ei = make_index("uniform", N, 900, gen, dev)
    for dt in DTYPES:
        for fin, fout in ((8, 16), (16, 8)):
            torch.manual_seed(0)
            conv = layers.SAGEConv(fin, fout, torch.relu).to(dev)
            x = torch.randn(N, fin, generator=gen, device=dev)
            with torch.autocast(dev.type, dtype=dt):
                out = conv(x, ei)
            assert out.dtype == dt and out.shape == (N, fout), (dt, fin, fout, out.dtype)
        torch.manual_seed(0)
        net = layers.GraphSAGEFullModel(8, 16, 4, 1, torch.relu, 0.0, "mean").to(dev)
        net.train()
        x = torch.randn(N, 8, generator=gen, device=dev)
        y = torch.randint(0, 4, (N,), generator=gen, device=dev)
        with torch.autocast(dev.type, dtype=dt):
            logits = net(x, ei)
        assert logits.dtype == dt
        torch.nn.functional.cross_entropy(logits.float(), y).backward()
        for prm in net.parameters():
            assert prm.dtype == torch.float32 and prm.grad is not None and prm.grad.dtype == torch.float32
            assert bool(torch.isfinite(prm.grad).all())


def check_one_rounding(routes, dev):
    """bf16: 4111 edges from rows of ones into row 0, bias 2.0: 4113 rounds to 4128.0 (the composition rounds 4111 to 4096
    first, and 4096 + 2 back to 4096).  f16: 4097 edges: 4099 rounds to 4100.0 (the composition: 4096).  On the GPU row 0 is
    a hub row: long_final_kernel's 16-bit store."""
    from gammagl_amd import mpops

    for dt, n, fused, composed in ((torch.bfloat16, 4111, 4128.0, 4096.0), (torch.float16, 4097, 4100.0, 4096.0)):
        ei = torch.stack([torch.arange(n, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)])
        x = torch.ones(n, 8, dtype=dt, device=dev)
        bias = torch.full((8,), 2.0, device=dev)
        for route in routes:
            out = route.fwd(ei, n, None, x, False, None, bias, False, 0.0)
            assert out.dtype == dt and torch.equal(out[0].float(), torch.full((8,), fused, device=dev)), (route.name, dt, out[0])
            assert torch.equal(out[1:].float(), torch.full((n - 1, 8), 2.0, device=dev))
        comp = mpops.gspmm(ei, None, x, "sum") + bias.to(dt)        # what the parent commit's layers compute
        assert torch.equal(comp[0].float(), torch.full((8,), composed, device=dev)), (dt, comp[0])


def check_long_rows(routes, dev, widths=(8, 64, 264), chunk=64, N=300, E=20_000, seed=3):
    """a plan whose long-row table is not empty both ways (small chunk, power-law ids): bias + ReLU + dropout and add + mean"""
    eng = routes[0].eng
    gen = torch.Generator(device=dev).manual_seed(seed)
    index = make_index("power", N, E, gen, dev)
    index[0, :] = index[1, torch.randperm(E, generator=gen, device=dev)]     # power-law sources too: long transposed rows
    w = torch.rand(E, generator=gen, device=dev)
    old = eng.chunk
    eng.chunk = chunk
    eng.graph_cache.clear()
    try:
        gp = eng.graph_plan(index, N)
        assert gp.fwd.n_long > 0 and gp.bwd.n_long > 0 and gp.fwd.chunk == chunk, "long rows both ways"
        for K in widths:
            x = torch.randn(N, K, generator=gen, device=dev)
            g = torch.randn(N, K, generator=gen, device=dev)
            for dt in DTYPES:
                for form in ("bias_relu_drop", "add_bias_relu_mean"):
                    check_case(routes[0], dev, index, N, w, x.to(dt), g.to(dt), form, "long rows")
        return gp
    finally:
        eng.chunk = old
        eng.graph_cache.clear()


def check_column_blocks(eng, dev, K=256, chunk=64, N=50, E=5000, seed=11):
    """ggl_spmm_epi_x16 in column blocks (col_block16 = 128, thresholds at 0: two blocks of a 256-wide row), hub rows walked
    once per aggregate and once per block: the bits of the one-launch call, dropout mask included, and the state advances
    once — not once per block"""
    from parity_cases import option

    gen = torch.Generator(device=dev).manual_seed(seed)
    index = make_index("power", N, E, gen, dev)
    index[0, E - 1500:] = 11
    w = torch.rand(E, generator=gen, device=dev)
    x = torch.randn(N, K, generator=gen, device=dev)
    add = torch.randn(N, K, generator=gen, device=dev)
    bias = torch.randn(K, generator=gen, device=dev)
    old = eng.chunk
    eng.chunk = chunk
    eng.graph_cache.clear()
    try:
        gp = eng.graph_plan(index, N)
        assert gp.fwd.n_long >= 2 and gp.fwd.chunk == chunk
        blocks = lambda: int(eng.lib.ggl_spmm_col_blocks_x16(ctypes.byref(gp.fwd.c_struct(None)), K))  # noqa: E731

        def run(dt, mean, od):
            eng.reseed(SEED)
            s0 = eng._rng_state(dev).clone()
            out = eng.spmm_epi(gp, w, x.to(dt), "mean" if mean else "sum", add.to(dt), bias, True, 0.5, True, out_dtype=od)
            s1 = eng._rng_state(dev).clone()
            assert int(s1[0]) == int(s0[0]) and int(s1[1]) == int(s0[1]) + 1, "the state advances once per call"
            return out

        with option(eng, "col_block_min_edges", 0), option(eng, "col_block_min_degree", 0):
            for dt in DTYPES:
                for mean in (False, True):
                    for od in (None, torch.float32):
                        with option(eng, "col_block16", 0):
                            assert blocks() == 1
                            want = run(dt, mean, od)
                        for one in (1, 0):
                            with option(eng, "col_block16", 128), option(eng, "hub_one_launch", one):
                                assert blocks() == 2
                                got = run(dt, mean, od)
                            assert same_bits(got, want), (dt, mean, od, one)
                        eng.reseed(SEED)
                        f32 = eng.spmm_epi(gp, w, x.to(dt).float(), "mean" if mean else "sum", add.to(dt).float(), bias, True, 0.5)
                        assert same_bits(want, f32 if od is not None else f32.to(dt)), (dt, mean, od)
    finally:
        eng.chunk = old
        eng.graph_cache.clear()


def check_bias_act(routes, dev):
    """bias_act alone: y, ga, gbias bits against the f32 kernels on the widened inputs; N = 37 / 1000 (the unrolled body and
    its tail, more than one partial row), K = 7 / 8 / 44 / 64, the three mask forms of the backward"""
    gen = torch.Generator(device=dev).manual_seed(13)
    for N in (37, 1000):
        for K in (7, 8, 44, 64):
            a = torch.randn(N, K, generator=gen, device=dev)
            g = torch.randn(N, K, generator=gen, device=dev)
            bias = torch.randn(K, generator=gen, device=dev)
            for dt in DTYPES:
                for relu, p in ((True, 0.0), (True, 0.5), (False, 0.5), (False, 0.0)):
                    for route in routes:
                        eng = route.eng
                        tag = (route.name, N, K, str(dt), relu, p)
                        eng.reseed(SEED)
                        with torch.no_grad():
                            want = route.bias_act(a.to(dt).float(), bias, relu, p)
                        eng.reseed(SEED)
                        used = route.used(dev, p)
                        a16 = a.to(dt).requires_grad_(True)
                        b = bias.clone().requires_grad_(True)
                        y = route.bias_act(a16, b, relu, p)
                        assert y.dtype == dt and same_bits(y.detach(), want.to(dt)), ("y", tag)
                        y.backward(g.to(dt))
                        ga_ref, gb_ref = route.epi_bwd(g.to(dt).float(), y.detach().float(), bias, relu, p, used)
                        assert same_bits(a16.grad, ga_ref.to(dt)), ("ga", tag)
                        assert b.grad.dtype == torch.float32 and same_bits(b.grad, gb_ref), ("gbias", tag)
    # dropout without ReLU and without an rng state: the mask is read off y != 0 (the third form), engine primitives only
    eng = routes[0].eng
    a = torch.randn(200, 44, generator=gen, device=dev)
    g = torch.randn(200, 44, generator=gen, device=dev)
    for dt in DTYPES:
        eng.reseed(SEED)
        y = eng.bias_act(a.to(dt), None, False, 0.5).detach()
        ga, gb = eng._epi_bwd(g.to(dt), y, False, 0.5, None, (44,))
        ga_ref, gb_ref = eng._epi_bwd(g.to(dt).float(), y.float(), False, 0.5, None, (44,))
        assert same_bits(ga, ga_ref.to(dt)) and same_bits(gb, gb_ref), dt


def check_refusals(routes, dev):
    """what must keep raising, with "Float" in the message"""
    from gammagl_amd import mpops

    gen = torch.Generator(device=dev).manual_seed(2)
    N = 50
    ei = make_index("uniform", N, 400, gen, dev)
    w = torch.rand(400, generator=gen, device=dev)
    x = torch.randn(N, 8, generator=gen, device=dev)
    bias = torch.randn(8, generator=gen, device=dev)
    for route in routes:
        with pytest.raises(RuntimeError, match="Float"):
            route.fwd(ei, N, w, x.double(), False, None, bias, True, 0.0)
        with pytest.raises(RuntimeError, match="Float"):
            route.bias_act(x.double(), bias, True, 0.0)
        for bad in (torch.bfloat16, torch.float16, torch.float64):
            for xd in (torch.float32, torch.bfloat16):
                with pytest.raises(RuntimeError, match="Float"):
                    route.fwd(ei, N, w.to(bad), x.to(xd), False, None, bias, True, 0.0)
                with pytest.raises(RuntimeError, match="Float"):
                    route.fwd(ei, N, w, x.to(xd), False, None, bias.to(bad), True, 0.0)
                with pytest.raises(RuntimeError, match="Float"):
                    route.bias_act(x.to(xd), bias.to(bad), True, 0.0)
        with pytest.raises(RuntimeError, match="Float"):      # mixed 16-bit types
            route.fwd(ei, N, w, x.bfloat16(), True, x.half(), bias, True, 0.0)
        with pytest.raises(RuntimeError, match="Float"):
            route.fwd(ei, N, w, x.bfloat16(), True, x, bias, True, 0.0)
    eng = routes[0].eng
    for dt in DTYPES:
        with pytest.raises(RuntimeError, match="Float"):
            eng.segment_epi(x.to(dt)[ei[0]], ei[1], N, "mean", None, bias, True)
        with pytest.raises(RuntimeError, match="Float"):
            mpops.gspmm(ei, w, x.to(dt), "max")


def check_sage_parts(eng, dev):
    """under autocast SAGEConv (both branches) equals the GEMMs plus Engine.spmm_epi / bias_act written out"""
    from gammagl_amd import layers, mpops

    gen = torch.Generator(device=dev).manual_seed(6)
    N = 150
    ei = make_index("power", N, 1500, gen, dev)
    lin = torch.nn.functional.linear
    for dt in DTYPES:
        # transform first (input wider than output): mean(fc_neigh(x)) + fc_self(x) + bias -> relu in the aggregate's store
        torch.manual_seed(0)
        conv = layers.SAGEConv(16, 8, torch.relu).to(dev)
        with torch.no_grad():
            conv.bias.copy_(torch.randn(1, 8, generator=gen, device=dev))
        x = torch.randn(N, 16, generator=gen, device=dev)
        with torch.autocast(dev.type, dtype=dt):
            got = conv(x, ei)
            hn, hs = lin(x, conv.fc_neigh.weight), lin(x, conv.fc_self.weight)
        assert hn.dtype == dt
        want = eng.spmm_epi(eng.graph_plan(ei, N), None, hn, "mean", add=hs, bias=conv.bias, relu=True)
        assert got.dtype == dt and same_bits(got.detach(), want.detach()), ("transform first", dt)
        # aggregate first (input narrower than output): f32 mean, one GEMM under autocast, 16-bit bias_act
        torch.manual_seed(0)
        conv = layers.SAGEConv(8, 16, torch.relu).to(dev)
        with torch.no_grad():
            conv.bias.copy_(torch.randn(1, 16, generator=gen, device=dev))
        x = torch.randn(N, 8, generator=gen, device=dev)
        agg = mpops.unsorted_segment_mean(x.index_select(0, ei[0]), ei[1], N)
        with torch.autocast(dev.type, dtype=dt):
            got = conv(x, ei)
            h = lin(torch.cat([agg, x], dim=1), torch.cat([conv.fc_neigh.weight, conv.fc_self.weight], dim=1))
        assert h.dtype == dt
        want = eng.bias_act(h, conv.bias, relu=True)
        assert got.dtype == dt and same_bits(got.detach(), want.detach()), ("aggregate first", dt)


def check_gcn_model_parts(eng, dev):
    """a GCNModel hidden layer (fused form on) equals linear -> Engine.spmm_epi(..., bias, relu, p) written out; the
    keyword switches the layers' attribute, a bare GCNConv has it off"""
    from gammagl_amd import layers

    gen = torch.Generator(device=dev).manual_seed(4)
    N = 120
    ei = layers.add_self_loops(make_index("uniform", N, 900, gen, dev), N)
    x = torch.randn(N, 20, generator=gen, device=dev)
    assert layers.GCNConv(20, 16).fuse_epilogue16 is False
    off = layers.GCNModel(20, 16, 5, num_layers=2, fuse_epilogue16=False)
    assert all(c.fuse_epilogue16 is False for c in off.conv)
    torch.manual_seed(0)
    net = layers.GCNModel(20, 16, 5, drop_rate=0.5, num_layers=2).to(dev)
    assert all(c.fuse_epilogue16 is True for c in net.conv)
    net.train()
    conv = net.conv[0]
    with torch.no_grad():
        conv.bias.copy_(torch.randn(1, 16, generator=gen, device=dev))
    w = conv._norm_weights(ei, None, N, dev)
    for dt in DTYPES:
        eng.reseed(SEED)
        with torch.autocast(dev.type, dtype=dt):
            got = conv(x, ei, None, N, _epilogue=(True, 0.5, True))
            h = torch.nn.functional.linear(x, conv.linear.weight)
        eng.reseed(SEED)
        want = eng.spmm_epi(eng.graph_plan(ei, N), w, h.contiguous(), "sum", None, conv.bias, True, 0.5, True)
        assert got.dtype == dt and same_bits(got.detach(), want.detach()), dt
        with torch.autocast(dev.type, dtype=dt):
            assert net(x, ei, None, N).dtype == dt          # the output layer returns the activations' dtype


def check_trainers(dev):
    """GCNTrainer(drop_rate=0.5, amp_dtype=bf16 / f16): 8 steps, a finite loss that is lower at the end, f32 parameters and
    Adam state"""
    from gammagl_amd import layers
    from gammagl_amd.trainer import GCNTrainer

    gen = torch.Generator(device=dev).manual_seed(5)
    N = 400
    ei = layers.add_self_loops(make_index("power", N, 6000, gen, dev), N)
    y = torch.randint(0, 5, (N,), generator=gen, device=dev)
    x = torch.randn(N, 32, generator=gen, device=dev) + torch.nn.functional.one_hot(y, 32).float() * 2.0
    idx = torch.arange(0, N, 2, device=dev)
    for amp in (torch.bfloat16, torch.float16):
        tr = GCNTrainer(32, 16, 5, num_layers=2, drop_rate=0.5, device=dev, amp_dtype=amp)
        losses = [float(tr.step(x, ei, y, idx, N)) for _ in range(8)]
        assert all(l == l and l != float("inf") for l in losses) and losses[-1] < losses[0], (amp, losses)
        assert all(p.dtype == torch.float32 for p in tr.net.parameters())
        assert all(s.dtype == torch.float32 for st in tr.opt.state.values() for s in st.values()
                   if torch.is_tensor(s) and s.is_floating_point())


def check_dispatcher(eng, dev):
    """opcheck of ggl.spmm_epi / ggl.bias_act on 16-bit inputs; the *_backward op on its own equals the autograd result"""
    from gammagl_amd import cpp_ops

    C = cpp_ops.load()
    gen = torch.Generator(device=dev).manual_seed(3)
    ei = make_index("uniform", 11, 60, gen, dev)
    w = torch.rand(60, generator=gen, device=dev)
    bias = torch.randn(8, generator=gen, device=dev)
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    for dt in DTYPES:
        x = torch.randn(11, 8, generator=gen, device=dev).to(dt)
        add = torch.randn(11, 8, generator=gen, device=dev).to(dt)
        go = torch.randn(11, 8, generator=gen, device=dev).to(dt)
        for xx in (x, x.clone().requires_grad_(True)):
            torch.library.opcheck(C.spmm_epi.default, (ei, w, xx, True, add, bias, True, 0.0), test_utils=utils)
            torch.library.opcheck(C.bias_act.default, (xx, bias, True, 0.0), test_utils=utils)
        torch.library.opcheck(C.spmm_epi_forward.default, (ei, w, x, False, None, bias, True, 0.0),
                              test_utils=("test_schema", "test_faketensor"))
        xr, br = x.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        y = C.bias_act(xr, br, True, 0.0)
        y.backward(go)
        ga, gb = C.bias_act_backward(go, y.detach(), True, True, 0.0, torch.empty(0, dtype=torch.int64, device=dev))
        assert ga.dtype == dt and gb.dtype == torch.float32 and same_bits(ga, xr.grad) and same_bits(gb, br.grad), dt
        torch.library.opcheck(C.bias_act_backward.default,
                              (go, y.detach(), True, True, 0.0, torch.empty(0, dtype=torch.int64, device=dev)),
                              test_utils=("test_schema", "test_faketensor"))
        with pytest.raises(RuntimeError, match="Float"):
            C.bias_act_backward(go.double(), y.detach().double(), True, True, 0.0, torch.empty(0, dtype=torch.int64, device=dev))


def check_c_abi(eng, dev):
    """the additive entries refuse f32 rows, bf16 -> f16 and f64 with the _x16 family's code; ABI 12"""
    from gammagl_amd import _lib

    assert _lib.ABI_VERSION == 12 and eng.lib.ggl_abi_version() == 12
    gen = torch.Generator(device=dev).manual_seed(4)
    ei = make_index("uniform", 40, 300, gen, dev)
    gp = eng.graph_plan(ei, 40)
    cs = gp.fwd.c_struct(None)
    x = torch.randn(40, 16, generator=gen, device=dev).bfloat16()
    out = torch.empty(40, 16, dtype=torch.float64, device=dev)
    ws = torch.empty(max(int(eng.lib.ggl_bias_act_bwd_workspace_bytes(40, 16)), 4), dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    EDTYPE = eng.lib.ggl_spmm_sum_x16(ctypes.byref(cs), p(gp.col), None, 0, 7, p(x), 0, 16, 7, p(out), 0, None)
    assert EDTYPE == _lib.GGL_EDTYPE
    epi = eng.lib.ggl_spmm_epi_x16
    assert len(epi.argtypes) == 22           # ggl_spmm_epi_ex's 21 - accumulate + x_dtype + out_dtype: no accumulate
    for xd, od in ((7, 7), (6, 5), (5, 6), (6, 8), (8, 8)):     # f32 rows, bf16 -> f16, f16 -> bf16, bf16 -> f64, f64 rows
        assert epi(ctypes.byref(cs), p(gp.col), None, 0, xd, p(x), 0, 16, od, p(out), 0, 0, None, 0, None, 1, 0.0, None, 0, 0,
                   1, None) == EDTYPE, (xd, od)
    for d in (7, 8, 4):
        assert eng.lib.ggl_bias_act_fwd_x16(d, p(x), None, 40, 16, 1, 0.0, None, p(out), None) == EDTYPE
        assert eng.lib.ggl_bias_act_bwd_x16(d, p(x), p(x), 40, 16, 1, 0.0, None, p(out), None, p(ws), ws.numel(), None) == EDTYPE
