"""Shared cases of gspmm's gradient with respect to its edge weights (ggl_spmm_grad_w: sum and mean, f32 / bf16 / f16 rows) for
tests/test_spmm_gradw_host.py (host library, CPU tensors) and tests/test_gpu_spmm_gradw.py (MI355X).  Not a test module.

A *route* is the callable of tests/spmm16_cases.py: ``f(reduce, index, weight, x, out_f32=False) -> out``; the three routes
are the ctypes engine, ``torch.ops.ggl`` and ``torch.ops.gammagl_amd``.

The contract (include/ggl_mpops.h):
    gw[e] = sum_k x[src_e, k] * g'[dst_e, k]     f32, k ascending, rounded multiply then rounded add
    sum : g' = g          mean : g' = g / count(dst)  (the rounded f32 divide)
    16-bit x or g: widened at the load, the same f32 products and adds, gw f32 and never rounded
The bit comparisons are torch.equal on the integer view; the float64 comparison uses the dot product's own a-priori bound
|gw - gw64| <= gamma_K * sum_k |x_k g'_k|, gamma_K = K u / (1 - K u), u = 2^-24 (K rounded operations per chain: one
multiply and one add per column, the first add exact), nothing tuned.
"""
import contextlib

import torch

from spmm16_cases import DTYPES, make_index, make_routes, same_bits  # noqa: F401  (re-exported for the test modules)

KINDS = ("uniform", "power", "empty_rows", "duplicates", "no_edges", "sorted")
# every tail shape of the 32-column slab, multiples of 4 that are not multiples of 8 (the 16-bit vector path's limit), the
# plain route, 64-column blocks with a carried chain plus a tail
WIDTHS = (1, 7, 8, 12, 32, 36, 40, 47, 64, 72, 96, 256, 264)
EDGES = (0, 1, 255, 256, 257)            # the 256-item workgroup edge
N, E = 300, 5000
U = 2.0 ** -24


def gamma(K):
    return K * U / (1.0 - K * U)


@contextlib.contextmanager
def low_block_thresholds(eng):
    """small graphs never meet the column-block thresholds: lower them through the option table, restore them afterwards"""
    names = ("col_block_min_edges", "col_block_min_degree")
    old = {n: int(eng.lib.ggl_get_option(n.encode())) for n in names}
    try:
        for n in names:
            eng.set_option(n, 1)
        yield
    finally:
        for n, v in old.items():
            eng.set_option(n, v)


def grad_w(route, reduce, index, w, x, g, out_f32=False, x_grad=False):
    """w.grad of route(reduce) under the output gradient g (g's dtype is the output's)"""
    wl = w.clone().requires_grad_(True)
    xl = x.clone().requires_grad_(True) if x_grad else x
    y = route(reduce, index, wl, xl, out_f32) if out_f32 else route(reduce, index, wl, xl)
    assert y.dtype == g.dtype, (y.dtype, g.dtype)
    y.backward(g)
    return (wl.grad, xl.grad) if x_grad else wl.grad


def counts(index, n_dst):
    """the f32 edge count of every destination row (1 where a row has no edge: no edge reads it)"""
    return torch.bincount(index[1], minlength=n_dst).clamp(min=1).to(torch.float32)


def prescaled(index, g, n_dst):
    """g / cnt[:, None] in f32, divided on the CPU (IEEE division whatever the device's fast paths are)"""
    gc = g.detach().float().cpu()
    return (gc / counts(index.cpu(), n_dst)[:, None]).to(g.device)


def loop_ref(index, x, g):
    """acc = acc + x[src, k] * g[dst, k] over k, on the CPU in f32: two rounded operations per column, never fused"""
    xc, gc, ic = x.detach().float().cpu(), g.detach().float().cpu(), index.cpu()
    acc = torch.zeros(ic.shape[1], dtype=torch.float32)
    for k in range(xc.shape[1]):
        acc = acc + xc[ic[0], k] * gc[ic[1], k]
    return acc


def f64_ref(index, x, g):
    """(gw64, sum_k |x_k g_k|) in float64 on the CPU"""
    xc, gc, ic = x.detach().double().cpu(), g.detach().double().cpu(), index.cpu()
    p = xc[ic[0]] * gc[ic[1]]
    return p.sum(1), p.abs().sum(1)


def graphs(dev, seed=0):
    """(name, index, n) of the square graphs: every kind, and the workgroup-edge sizes"""
    out = []
    for kind in KINDS:
        gen = torch.Generator(device=dev).manual_seed(seed + len(kind))
        out.append((kind, make_index(kind, N, E, gen, dev), N))
    for e in EDGES:
        gen = torch.Generator(device=dev).manual_seed(seed + 100 + e)
        out.append((f"E={e}", make_index("uniform" if e else "no_edges", N, e, gen, dev), N))
    return out


def rect_index(dev, n_src=500, n_dst=200, seed=9):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return torch.stack([torch.randint(0, n_src, (E,), generator=gen, device=dev),
                        torch.randint(0, n_dst, (E,), generator=gen, device=dev)]).contiguous()


def inputs(index, n_src, n_dst, K, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return (torch.rand(index.shape[1], generator=gen, device=dev), torch.randn(n_src, K, generator=gen, device=dev),
            torch.randn(n_dst, K, generator=gen, device=dev))


# ---- check 1 ------------------------------------------------------------------------------------------------------------------
def check_exists(routes, dev):
    """gspmm(index, w, x, 'sum' | 'mean') then backward() leaves a w.grad of w's shape (on the parent commit: None)"""
    from gammagl_amd import mpops

    gen = torch.Generator(device=dev).manual_seed(1)
    ei = make_index("uniform", 50, 400, gen, dev)
    x = torch.randn(50, 24, generator=gen, device=dev)
    for reduce in ("sum", "mean"):
        for shape in ((400,), (400, 1)):
            w = torch.rand(shape, generator=gen, device=dev).requires_grad_(True)
            if len(shape) == 1:
                mpops.gspmm(ei, w, x, reduce).sum().backward()
                assert w.grad is not None and w.grad.shape == w.shape and w.grad.dtype == torch.float32, ("gspmm", reduce)
            for name, route in routes.items():
                w.grad = None
                route(reduce, ei, w, x).sum().backward()
                assert w.grad is not None and w.grad.shape == w.shape, (name, reduce, shape)
                assert bool((w.grad != 0).any())


# ---- checks 2, 3, 5 -------------------------------------------------------------------------------------------------------------
def check_f32(routes, eng, dev, widths=WIDTHS):
    """f32 sum == the bspmm_sum weight gradient with one head == the plain torch loop; mean == the sum form fed g / cnt; both
    within the float64 bound.  Returns the number of (graph, width, route, reduce) cases."""
    n = 0
    for gi, (name, index, nn) in enumerate(graphs(dev)):
        for K in widths:
            w, x, g = inputs(index, nn, nn, K, dev, 1000 * gi + K)
            gs = prescaled(index, g, nn)
            want = {"sum": loop_ref(index, x, g), "mean": loop_ref(index, x, gs)}
            wb = w[:, None].clone().requires_grad_(True)
            eng.c_bspmm_sum(index, wb, x[:, None, :].contiguous()).backward(g[:, None, :])
            assert same_bits(wb.grad[:, 0].cpu(), want["sum"]), ("bspmm vs loop", name, K)
            for rn, route in routes.items():
                for reduce in ("sum", "mean"):
                    got = grad_w(route, reduce, index, w, x, g)
                    assert got.shape == w.shape and same_bits(got.cpu(), want[reduce]), (rn, reduce, name, K)
                    n += 1
                # mean on the same route: the bits of its own sum form fed g / cnt
                assert same_bits(grad_w(route, "mean", index, w, x, g), grad_w(route, "sum", index, w, x, gs)), (rn, name, K)
            for reduce, gg in (("sum", g), ("mean", gs)):
                ref, mag = f64_ref(index, x, gg)
                err = (want[reduce].double() - ref).abs()
                assert bool((err <= gamma(K) * mag).all()), ("float64 bound", reduce, name, K, float((err - gamma(K) * mag).max()))
    return n


def grad_w_ops():
    """the spmm_grad_w dispatcher op as registered from C++ (torch.ops.ggl_grad) and from Python (torch.ops.gammagl_amd)"""
    from gammagl_amd import cpp_ops, torch_ops

    return (cpp_ops.load_grad().spmm_grad_w, torch_ops.ops.spmm_grad_w)


def check_rectangular(eng, dev, widths=(7, 8, 40, 264)):
    """N_src = 500, N_dst = 200: Engine.spmm on the explicit plan, and the spmm_grad_w op of both registrations"""
    n_src, n_dst = 500, 200
    index = rect_index(dev, n_src, n_dst)
    gp = eng.graph_plan(index, n_dst, n_src)
    for K in widths:
        w, x, g = inputs(index, n_src, n_dst, K, dev, 77 + K)
        gs = prescaled(index, g, n_dst)
        for reduce, gg in (("sum", g), ("mean", gs)):
            want = loop_ref(index, x, gg)
            wl = w.clone().requires_grad_(True)
            eng.spmm(gp, wl, x, reduce).backward(g)
            assert same_bits(wl.grad.cpu(), want), ("engine.spmm", reduce, K)
            for op in grad_w_ops():
                assert same_bits(op(index, x, g, reduce == "mean").cpu(), want), (str(op), reduce, K)
            assert same_bits(eng.spmm_grad_w(index, x, g, reduce == "mean").cpu(), want)


# ---- check 4 ------------------------------------------------------------------------------------------------------------------
def check_x16(routes, eng, dev, widths=WIDTHS, kinds=("uniform", "power", "E=257", "E=1", "E=0"), side_widths=(8, 40, 264)):
    """16-bit storage: the bits of the f32 form on the widened tensors — x bf16 / f16, g 16-bit (the op's own output dtype) and
    f32 (out_f32), sum and mean, all routes; then every (x, g) dtype pair, f32 x with 16-bit g included, through the op."""
    n = 0
    for gi, (name, index, nn) in enumerate(g for g in graphs(dev) if g[0] in kinds):
        for K in (widths if name == "uniform" else side_widths):     # every width on one graph, three on the others
            w, x, g = inputs(index, nn, nn, K, dev, 5000 + 100 * gi + K)
            for dt in DTYPES:
                x16, g16 = x.to(dt), g.to(dt)
                for reduce in ("sum", "mean"):
                    want16 = loop_ref(index, x16, prescaled(index, g16, nn) if reduce == "mean" else g16)
                    want32 = loop_ref(index, x16, prescaled(index, g, nn) if reduce == "mean" else g)
                    for rn, route in routes.items():
                        f32_form = grad_w(route, reduce, index, w, x16.float(), g16.float())
                        assert same_bits(grad_w(route, reduce, index, w, x16, g16), f32_form), (rn, reduce, dt, name, K)
                        assert same_bits(f32_form.cpu(), want16)
                        got32 = grad_w(route, reduce, index, w, x16, g, out_f32=True)
                        assert got32.dtype == torch.float32 and same_bits(got32.cpu(), want32), (rn, reduce, dt, name, K, "f32 g")
                        n += 1
            if name == "uniform":
                for xd in (torch.float32,) + DTYPES:
                    for gd in (torch.float32,) + DTYPES:
                        for mean in (False, True):
                            xx, gg = x.to(xd), g.to(gd)
                            want = loop_ref(index, xx, prescaled(index, gg, nn) if mean else gg)
                            assert same_bits(eng.spmm_grad_w(index, xx, gg, mean).cpu(), want), (xd, gd, mean, K)
    return n


def check_f32_accumulation(routes, dev):
    """x = g = ones, K = 264: exactly 264.0 (a bf16 running sum stalls at 256)"""
    gen = torch.Generator(device=dev).manual_seed(3)
    index = make_index("uniform", 40, 300, gen, dev)
    w = torch.rand(300, generator=gen, device=dev)
    for dt in DTYPES:
        ones = torch.ones(40, 264, dtype=dt, device=dev)
        for rn, route in routes.items():
            got = grad_w(route, "sum", index, w, ones, ones)
            assert got.dtype == torch.float32 and torch.equal(got, torch.full((300,), 264.0, device=dev)), (rn, dt, got[:4])


def check_carried_chain(routes, eng, dev, f32_widths=(128, 256, 264), x16_widths=(256, 264)):
    """the column-block launches with a carried chain (K >= 2 blocks: 256, and 264 = blocks + a tail; 16-bit x: 128-column
    blocks), thresholds lowered through the option table: the same bits"""
    with low_block_thresholds(eng):
        assert int(eng.lib.ggl_get_option(b"col_block_min_edges")) == 1
        n = check_f32(routes, eng, dev, widths=f32_widths)
        n += check_x16(routes, eng, dev, widths=x16_widths, kinds=("uniform", "power", "E=257"), side_widths=x16_widths[-1:])
    assert int(eng.lib.ggl_get_option(b"col_block_min_edges")) > 1
    return n


def check_block_width_not_a_multiple_of_8(eng, dev, K=264):
    """col_block = 36 (a multiple of 4, not of 8), thresholds lowered: the f32 kernels carry their chain over 36-column
    blocks, while an f32 x under a 16-bit g — the unit-of-8 kernel, whose scratch the same rule sizes — must run as ONE
    launch instead of dropping columns 32..35 of every block.  col_block16 = 36 likewise for 16-bit x.  The serial bits."""
    name, index, nn = graphs(dev)[0]
    _, x, g = inputs(index, nn, nn, K, dev, 4242)
    old = {n: int(eng.lib.ggl_get_option(n.encode())) for n in ("col_block", "col_block16")}
    try:
        with low_block_thresholds(eng):
            for n in old:
                eng.set_option(n, 36)
            for xd in (torch.float32,) + DTYPES:
                for gd in (torch.float32,) + DTYPES:
                    for mean in (False, True):
                        xx, gg = x.to(xd), g.to(gd)
                        want = loop_ref(index, xx, prescaled(index, gg, nn) if mean else gg)
                        assert same_bits(eng.spmm_grad_w(index, xx, gg, mean).cpu(), want), (xd, gd, mean)
    finally:
        for n, v in old.items():
            eng.set_option(n, v)


# ---- check 6 ------------------------------------------------------------------------------------------------------------------
# tensors each route's autograd node keeps for a CONSTANT weight (the parent commit's: the engine's node keeps none, the
# C++ node index and weight)
SAVED_CONSTANT = {"engine": 0, "torch.ops.ggl": 2, "torch.ops.gammagl_amd": 0}


def check_constant_weight_costs_nothing(routes, dev):
    """a constant weight saves no x (the node's saved tensors are the parent commit's); a learnable one saves exactly x more;
    x.grad is the same bits either way"""
    index = graphs(dev)[0][1]
    w, x, g = inputs(index, N, N, 40, dev, 11)
    for rn, route in routes.items():
        for reduce in ("sum", "mean"):
            kept = {}
            for learn in (False, True):
                packed = []
                xl = x.clone().requires_grad_(True)
                wl = w.clone().requires_grad_(learn)
                with torch.autograd.graph.saved_tensors_hooks(lambda t: packed.append(t) or t, lambda t: t):
                    y = route(reduce, index, wl, xl)
                kept[learn] = (len(packed), sum(t.data_ptr() == xl.data_ptr() for t in packed))
                y.backward(g)
                kept[learn] += (xl.grad,)
                assert (wl.grad is not None) == learn
            assert kept[False][:2] == (SAVED_CONSTANT[rn], 0), (rn, reduce, kept[False][:2])
            assert kept[True][:2] == (SAVED_CONSTANT[rn] + 1, 1), (rn, reduce, kept[True][:2])
            assert same_bits(kept[False][2], kept[True][2]), (rn, reduce)


# ---- check 7 ------------------------------------------------------------------------------------------------------------------
def check_epilogue(eng, ops_namespaces, dev, p_drop=0.0):
    """spmm_epi (bias + ReLU, dropout where p_drop > 0): w.grad against the message route in float64 under check 5's bound
    gamma_K * sum_k |x_k ga_k| on the pre-activation gradient ga.  ga is the f32 tensor the edge-dot is FED: the op hands it
    back as the gradient of `add` (zeros here), so no rounding of the epilogue's own (dropout scale) enters the bound; for
    mean the divide by the row's count is made on it in f32 (prescaled()), the contract's order.  That ga is the right one
    is asserted apart, against go * kept / (1 - p) with the kept mask (ReLU and dropout together) read off the output:
    exact without dropout; with it four named roundings (p to f32, 1 - p, the reciprocal or divide, the product)."""
    index = graphs(dev)[0][1]
    K = 40
    w, x, go = inputs(index, N, N, K, dev, 21)
    bias = torch.randn(K, generator=torch.Generator(device=dev).manual_seed(5), device=dev)
    ic, x64, go64 = index.cpu(), x.double().cpu(), go.double().cpu()

    def run_engine(reduce, wl, add):
        return eng.spmm_epi(eng.graph_plan(index, N), wl, x, reduce, add=add, bias=bias, relu=True, p_drop=p_drop, training=True)

    runs = [("engine", run_engine)]
    for ns in ops_namespaces:
        if hasattr(ns, "spmm_epi"):
            runs.append((str(ns), lambda reduce, wl, add, ns=ns: ns.spmm_epi(index, wl, x, reduce == "mean", add, bias, True, p_drop)))
    for rn, run in runs:
        for reduce in ("sum", "mean"):
            wl = w.clone().requires_grad_(True)
            add = torch.zeros(N, K, device=dev).requires_grad_(True)
            y = run(reduce, wl, add)
            y.backward(go)
            ga = add.grad.detach()                                   # f32 [N, K]: what the edge-dot was fed
            kept = (y.detach() != 0).double().cpu()
            want_ga = go64 * kept / (1.0 - p_drop)
            if p_drop == 0.0:
                assert torch.equal(ga.double().cpu(), want_ga), (rn, reduce)
            else:
                assert bool(((ga.double().cpu() - want_ga).abs() <= gamma(4) * want_ga.abs()).all()), (rn, reduce, p_drop)
            # the float64 message route under that pre-activation gradient: d/dw_e of sum_ik ga_ik (reduce_e w_e x[src_e])_ik
            w64 = w.double().cpu().requires_grad_(True)
            agg = torch.zeros(N, K, dtype=torch.float64).index_add_(0, ic[1], x64[ic[0]] * w64[:, None])
            gfed = prescaled(index, ga, N) if reduce == "mean" else ga   # f32, as the contract orders it: (g / count) * w
            (agg * gfed.double().cpu()).sum().backward()
            mag = (x64[ic[0]] * gfed.double().cpu()[ic[1]]).abs().sum(1)
            err = (wl.grad.double().cpu() - w64.grad).abs()
            assert bool((err <= gamma(K) * mag).all()), (rn, reduce, p_drop, float((err - gamma(K) * mag).max()))
            assert bool((wl.grad != 0).any())


def check_gcnconv_learnable_edge_weight(dev):
    """GCNConv(norm='both') with a learnable edge_weight, bias + ReLU: the weight takes spmm_bias_act, and ew.grad propagates
    through the normalisation — against the message route in float64 on the layer's own linear output."""
    from gammagl_amd import layers

    torch.manual_seed(0)
    gen = torch.Generator(device=dev).manual_seed(6)
    n, K = 120, 16
    ei = layers.add_self_loops(make_index("uniform", n, 900, gen, dev), n)
    x = torch.randn(n, 20, generator=gen, device=dev)
    go = torch.randn(n, K, generator=gen, device=dev)
    conv = layers.GCNConv(20, K, norm="both").to(dev)
    with torch.no_grad():
        conv.bias.copy_(torch.randn(1, K, generator=gen, device=dev))
    ew = (torch.rand(ei.shape[1], generator=gen, device=dev) + 0.5).requires_grad_(True)
    seen = {}
    eng = layers._engine(x)
    orig = eng.spmm_bias_act

    def spy(gp, weight, *a, **k):
        seen["learnable"] = weight.requires_grad
        return orig(gp, weight, *a, **k)

    hook = conv.linear.register_forward_hook(lambda m, i, o: seen.__setitem__("h", o.detach()))
    eng.spmm_bias_act = spy
    try:
        y = conv(x, ei, ew, n, _epilogue=(True, 0.0, True))
    finally:
        del eng.spmm_bias_act
        hook.remove()
    assert seen.get("learnable") is True, "a learnable edge_weight must reach spmm_bias_act"
    y.backward(go)
    assert ew.grad is not None and ew.grad.shape == ew.shape
    # float64 message route on the same h
    ic, h64 = ei.cpu(), seen["h"].double().cpu()
    ew64 = ew.detach().double().cpu().requires_grad_(True)
    ns = torch.bincount(ic[0], minlength=n).double().pow(-0.5)
    nd = torch.bincount(ic[1], minlength=n).double().pow(-0.5)
    wts = ns[ic[0]] * ew64 * nd[ic[1]]
    pre = torch.zeros(n, K, dtype=torch.float64).index_add_(0, ic[1], h64[ic[0]] * wts[:, None]) + conv.bias.detach().double().cpu()
    kept = (y.detach() != 0).double().cpu()
    (pre * kept * go.double().cpu()).sum().backward()
    ga = go.double().cpu() * kept
    mag = (h64[ic[0]] * ga[ic[1]]).abs().sum(1) * ns[ic[0]] * nd[ic[1]]
    # K roundings of the dot; the two f32 norms (pow: 2 ulp each) and the two multiplies that carry gw to ew: six more
    err = (ew.grad.double().cpu() - ew64.grad).abs()
    assert bool((err <= gamma(K + 6) * mag).all()), float((err - gamma(K + 6) * mag).max())


def check_propagate_takes_the_spmm(dev):
    """MessagePassing.propagate with a learnable 1-D f32 weight calls Engine.spmm (the fused aggregate), sum and mean"""
    from gammagl_amd import layers

    gen = torch.Generator(device=dev).manual_seed(8)
    n = 64
    ei = make_index("uniform", n, 400, gen, dev)
    x = torch.randn(n, 12, generator=gen, device=dev).bfloat16()      # 16-bit rows take the SpMM at any size
    class Plain(layers.MessagePassing):      # (no message_aggregate of its own: propagate() picks the route itself)
        pass

    mp = Plain()
    eng = layers._engine(x)
    orig, calls = eng.spmm, []

    def spy(gp, weight, *a, **k):
        calls.append(weight.requires_grad)
        return orig(gp, weight, *a, **k)

    eng.spmm = spy
    try:
        for aggr in ("sum", "mean"):
            ew = torch.rand(ei.shape[1], generator=gen, device=dev).requires_grad_(True)
            out = mp.propagate(x, ei, aggr=aggr, edge_weight=ew, num_nodes=n)
            out.float().sum().backward()
            want = loop_ref(ei, x, prescaled(ei, torch.ones(n, 12), n) if aggr == "mean" else torch.ones(n, 12))
            assert same_bits(ew.grad.cpu(), want), aggr
    finally:
        del eng.spmm
    assert calls == [True, True], calls


# ---- check 8 ------------------------------------------------------------------------------------------------------------------
def check_max_and_rows_unchanged(routes, eng, ops_namespaces, dev):
    """spmm_max gives the weight no gradient; spmm_rows refuses a weight that requires grad with the text it had"""
    import pytest
    from gammagl_amd import mpops

    index = graphs(dev)[0][1]
    w, x, g = inputs(index, N, N, 8, dev, 31)
    fns = [("gspmm", lambda wl, xl: mpops.gspmm(index, wl, xl, "max")), ("engine", lambda wl, xl: eng.c_spmm_max(index, wl, xl))]
    fns += [(str(ns), lambda wl, xl, ns=ns: ns.spmm_max(index, wl, xl)) for ns in ops_namespaces]
    for name, fn in fns:
        wl, xl = w.clone().requires_grad_(True), x.clone().requires_grad_(True)
        fn(wl, xl).backward(g)
        assert wl.grad is None and xl.grad is not None, name
    rows = torch.arange(0, N, 3, device=dev)
    wl = w.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="spmm_rows has no gradient for the edge weights: pass detached weights"):
        eng.spmm_rows(eng.graph_plan(index, N), wl, x, rows)
    for ns in ops_namespaces:
        if hasattr(ns, "spmm_rows"):
            with pytest.raises(RuntimeError, match="spmm_rows has no gradient for the edge weights: pass detached weights"):
                ns.spmm_rows(index, wl, x, rows, None)
            assert ns.spmm_rows(index, w, x, rows, None).shape == (rows.numel(), 8)
