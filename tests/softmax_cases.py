"""Shared cases of the edge-softmax op (ggl_segment_softmax_fwd / _bwd) for tests/test_softmax_host.py (host library,
CPU tensors), tests/test_gpu_softmax.py (MI355X) and the AddressSanitizer run.  Not a test module.

A *route* is any callable ``f(x, ids, N) -> y`` that records autograd: ``Engine.segment_softmax``,
``torch.ops.ggl.segment_softmax``, ``torch.ops.gammagl_amd.segment_softmax``.

Truth = the composition of gammagl/utils/softmax.py:29-35 in float64 under torch autograd on the same inputs.
Error measure = oracle.parity.report's row-scale relative error with rows = (segment, column): every element is
compared on the scale of the largest |truth| of its (segment, column), floored by `floor_min` (the tensor's mean |truth|
for gradients, which cancel to ~0 over a whole row), as parity.gat_errors_vs_truth does for the fused GAT op.
"""

import numpy as np
import torch

from gammagl_amd import layers
from oracle import parity

TOL = parity.TOL          # 1e-5: the project's bar for float reductions (BASELINE north_star)
LOWEST = -3.4028234663852886e38


def _idx(ids, x):
    return ids.view(-1, *([1] * (x.dim() - 1))).expand_as(x)


def truth_f64(x, ids, N, g):
    """(y, gx) of softmax.py:29-35 in float64 under autograd (segment max with the extension's lowest() start value)."""
    xd = x.detach().double().requires_grad_(True)
    m = torch.full((N,) + tuple(x.shape[1:]), LOWEST, dtype=torch.float64, device=x.device)
    m = m.scatter_reduce(0, _idx(ids, xd), xd.detach(), reduce="amax", include_self=True)
    ex = torch.exp(xd - m[ids])
    den = torch.zeros_like(m).index_add_(0, ids, ex)
    y = ex / (den[ids] + 1e-16)
    y.backward(g.double())
    return y.detach(), xd.grad


def seg_err(got, truth, ids, N, floor_min=0.0):
    """max row-scale relative error, rows = (segment, column): parity.report on two-column rows (value, scale) whose
    second column is the (segment, column)'s largest |truth| on both sides — report's per-row floor is then that scale."""
    E = int(truth.shape[0])
    if E == 0:
        return 0.0
    t2 = truth.reshape(E, -1)
    g2 = got.double().reshape(E, -1)
    scale = torch.zeros((N, t2.shape[1]), dtype=torch.float64, device=t2.device)
    scale = scale.scatter_reduce(0, _idx(ids, t2), t2.abs(), reduce="amax", include_self=True)[ids]
    a = torch.stack((g2.reshape(-1), scale.reshape(-1)), dim=1)
    b = torch.stack((t2.reshape(-1), scale.reshape(-1)), dim=1)
    return parity.report(a, b, tol=1.0, floor_min=floor_min)["max_rel_err"]


def run(route, x, ids, N, g):
    xx = x.detach().clone().requires_grad_(True)
    y = route(xx, ids, N)
    y.backward(g)
    return y.detach(), xx.grad


def errors(route, x, ids, N, g, truth=None):
    """(forward error, gradient error) of `route` against float64."""
    ty, tg = truth if truth is not None else truth_f64(x, ids, N, g)
    y, gx = run(route, x, ids, N, g)
    return seg_err(y, ty, ids, N), seg_err(gx, tg, ids, N, floor_min=float(tg.abs().mean()))


def composition(x, ids, N):
    return layers.segment_softmax(x, ids, N)


def make_ids(kind, N, E, gen, dev):
    if kind == "power":       # rows of tens of thousands of elements next to one-element rows
        return (N * torch.rand(E, generator=gen, device=dev) ** 3).long().clamp_(max=N - 1)
    ids = torch.randint(0, N, (E,), generator=gen, device=dev)
    return torch.sort(ids).values if kind == "sorted" else ids


def shaped(K):
    """the trailing shape a width is tested in: [E], [E, H], [E, H, 1]"""
    return {1: (), 4: (4, 1)}.get(K, (K,))


def check_kat(routes, dev, golden):
    """the reference-made fixture (tests/golden/kat.npz): the bar parity_cases.check_kat holds the composition to"""
    g = golden["kat"]
    ei = torch.from_numpy(g["mp_ei"].copy()).to(dev)
    x = torch.from_numpy(g["sm_x"].copy()).to(dev)
    for name, route in routes.items():
        y = route(x, ei[1].contiguous(), 4)
        np.testing.assert_allclose(y.cpu().numpy(), g["sm_score"], rtol=1e-6, err_msg=name)


def check_vs_float64(routes, dev, kinds=("power", "uniform", "sorted"), widths=(1, 3, 4, 8, 16, 47), N=2000, E=200_000,
                     scale=3.0, seed=0, plan_route=None, log=print):
    """forward and gradient <= 1e-5 of float64 through every route; the f32 composition's error printed beside it.
    `plan_route(x, ids, N)`: an explicit-plan form run in addition (power-law ids only)."""
    out = []
    for kind in kinds:
        for K in widths:
            gen = torch.Generator(device=dev).manual_seed(seed + 97 * K + len(kind))
            ids = make_ids(kind, N, E, gen, dev)
            x = torch.randn((E,) + shaped(K), generator=gen, device=dev) * scale
            g = torch.randn(x.shape, generator=gen, device=dev)
            truth = truth_f64(x, ids, N, g)
            ec = errors(composition, x, ids, N, g, truth)
            todo = dict(routes)
            if plan_route is not None and kind == "power":
                todo["explicit plan"] = plan_route
            for name, route in todo.items():
                ef, eg = errors(route, x, ids, N, g, truth)
                log(f"segment_softmax {kind} N={N} E={E} shape={tuple(x.shape)} x{scale:g} [{name}]: forward {ef:.2e} "
                    f"gradient {eg:.2e}   (f32 composition: {ec[0]:.2e} / {ec[1]:.2e})")
                assert ef <= TOL and eg <= TOL, (kind, K, name, ef, eg)
                out.append((kind, K, name, ef, eg, ec))
    return out


def check_peaked(routes, dev, widths=(3, 47), N=2000, E=200_000, scale=10.0, seed=5, log=print):
    """Sharply peaked rows (logits randn x 10, power-law ids): forward <= 1e-5; the gradient's row scale collapses (one y
    is 1 - 1e-6), so it is held to `never further from float64 than the composition it replaces` (and 1e-5 where that is
    larger)."""
    out = []
    for K in widths:
        gen = torch.Generator(device=dev).manual_seed(seed + K)
        ids = make_ids("power", N, E, gen, dev)
        x = torch.randn(E, K, generator=gen, device=dev) * scale
        g = torch.randn(x.shape, generator=gen, device=dev)
        truth = truth_f64(x, ids, N, g)
        ec = errors(composition, x, ids, N, g, truth)
        for name, route in routes.items():
            ef, eg = errors(route, x, ids, N, g, truth)
            log(f"segment_softmax peaked K={K} x{scale:g} [{name}]: forward {ef:.2e} gradient {eg:.2e}   "
                f"(f32 composition: {ec[0]:.2e} / {ec[1]:.2e})")
            assert ef <= TOL, (K, name, ef)
            assert eg <= max(TOL, ec[1]), (K, name, eg, ec[1])
            out.append((K, name, ef, eg, ec))
    return out


def _segment_sums(v, ids, N):
    """float64 sums per (segment, column), on the CPU: index_add_ there adds in element order, the same every run (on the GPU
    it is an atomic add whose order — and so whose last bit — changes from run to run)."""
    v2 = v.detach().double().reshape(v.shape[0], -1).cpu()
    return torch.zeros((N, v2.shape[1]), dtype=torch.float64).index_add_(0, ids.cpu(), v2).to(v.device)


def check_winner_and_invariants(routes, eng, dev, N=2000, E=200_000, K=4, scale=3.0, seed=11, kinds=("power", "uniform")):
    """The maximum is the segment op's (arg of segment_max_with_arg): y there is the largest of its (segment, column).  In the
    backward the winner — the element with the largest y, smallest element index among equals, which is the segment op's arg
    unless a runner-up's exp(x - m) rounds to 1 too — has gx = minus the float64 sum of the others, rounded to f32, bit for bit.
    Invariants, every non-empty (segment, column): |sum64(y) - 1| <= 1e-6 (the rounding of D to f32 and one correctly rounded
    division per element, weights summing to 1: <= 3 x 2^-24) and |sum64(gx)| <= 1e-6 x max |gx| (the winner is the rounded
    negative of the others' double sum: <= 2^-24 of its own magnitude)."""
    for kind in kinds:
        gen = torch.Generator(device=dev).manual_seed(seed + len(kind))
        ids = make_ids(kind, N, E, gen, dev)
        x = torch.randn(E, K, generator=gen, device=dev) * scale
        g = torch.randn(E, K, generator=gen, device=dev)
        _, arg = eng.segment_max_with_arg(x, ids, N)
        cnt = torch.bincount(ids, minlength=N)
        full = cnt > 0
        cols = torch.arange(K, device=dev).expand(int(full.sum()), K)
        elem = torch.arange(E, device=dev).view(-1, 1).expand(E, K)
        for name, route in routes.items():
            y, gx = run(route, x, ids, N, g)
            a = arg[full]                                               # [rows, K] element indices
            ymax_all = torch.zeros(N, K, device=dev).scatter_reduce(0, _idx(ids, y), y, reduce="amax", include_self=True)
            assert torch.equal(y[a, cols], ymax_all[full]), f"{name} {kind}: the segment maximum's y is not the largest of its row"
            # the kernel's winner: smallest element index among the (segment, column)'s largest y
            cand = torch.where(y == ymax_all[ids], elem, torch.full_like(elem, E))
            w = torch.full((N, K), E, dtype=torch.int64, device=dev).scatter_reduce(0, _idx(ids, cand), cand, reduce="amin")[full]
            assert float((w == a).double().mean()) >= 0.999, f"{name} {kind}: winners are not the segment op's argmax"
            others = gx.clone()
            others[w, cols] = 0.0
            want = (-_segment_sums(others, ids, N)[full]).float()
            assert torch.equal(gx[w, cols], want), f"{name} {kind}: winner gradient is not -(sum of the others)"
            sy = _segment_sums(y, ids, N)[full]
            assert float((sy - 1.0).abs().max()) <= 1e-6, (name, kind, float((sy - 1.0).abs().max()))
            sg = _segment_sums(gx, ids, N)[full].abs()
            gmax = torch.zeros(N, K, device=dev).scatter_reduce(0, _idx(ids, gx), gx.abs(), reduce="amax", include_self=True)[full]
            assert bool((sg <= 1e-6 * gmax.double()).all()), (name, kind, float((sg / gmax.double().clamp(min=1e-300)).max()))


def check_edge_cases(routes, dev):
    inf = float("inf")
    for name, route in routes.items():
        # empty segments in the middle and at the end, num_segments > max id + 1, one-element segments
        ids = torch.tensor([5, 0, 5, 2, 5, 0], device=dev)
        x = torch.tensor([[0.5, -1.0], [2.0, 0.0], [1.5, 3.0], [7.0, -7.0], [-0.5, 3.0], [2.0, 1.0]], device=dev)
        g = torch.tensor([[1.0, 2.0], [0.5, -1.0], [-2.0, 0.25], [3.0, 4.0], [1.0, 1.0], [-1.0, 2.0]], device=dev)
        y, gx = run(route, x, ids, 9, g)
        ty, tg = truth_f64(x, ids, 9, g)
        torch.testing.assert_close(y.double(), ty, rtol=1e-6, atol=1e-7, msg=name)
        torch.testing.assert_close(gx.double(), tg, rtol=1e-5, atol=1e-6, msg=name)
        assert torch.equal(y[3], torch.ones(2, device=dev)) and torch.equal(gx[3], torch.zeros(2, device=dev)), name
        # E == 0
        x0 = torch.zeros(0, 3, device=dev, requires_grad=True)
        y0 = route(x0, torch.zeros(0, dtype=torch.int64, device=dev), 4)
        assert y0.shape == (0, 3)
        y0.sum().backward()
        assert x0.grad.shape == (0, 3)
        # -inf logits mixed into a row; a row of all -inf: zeros, no NaN
        ids = torch.tensor([0, 0, 0, 1, 1, 2], device=dev)
        x = torch.tensor([1.0, -inf, 0.0, -inf, -inf, -inf], device=dev)
        y, gx = run(route, x, ids, 3, torch.ones(6, device=dev))
        assert float(y[1]) == 0.0 and bool(torch.isfinite(y).all()) and bool(torch.isfinite(gx).all()), (name, y, gx)
        assert torch.equal(y[3:], torch.zeros(3, device=dev)), (name, y)
        torch.testing.assert_close(y[[0, 2]], torch.softmax(x[[0, 2]], 0), rtol=1e-6, atol=0, msg=name)
        # an out-of-range id is an IndexError, as for the other segment ops
        for bad in (torch.tensor([0, 3], device=dev), torch.tensor([-1, 0], device=dev)):
            try:
                route(torch.zeros(2, 2, device=dev), bad, 3)
            except IndexError:
                pass
            else:
                raise AssertionError(f"{name}: out-of-range id {bad.tolist()} did not raise IndexError")
        # non-contiguous x and shapes [E], [E, H], [E, H, C]
        gen = torch.Generator(device=dev).manual_seed(2)
        ids = torch.randint(0, 7, (50,), generator=gen, device=dev)
        base = torch.randn(50, 12, generator=gen, device=dev)
        xs = base[:, ::2]
        assert not xs.is_contiguous()
        assert torch.equal(route(xs, ids, 7), route(xs.contiguous(), ids, 7)), name
        y3 = route(xs.reshape(50, 3, 2), ids, 7)
        assert y3.shape == (50, 3, 2) and torch.equal(y3.reshape(50, 6), route(xs.contiguous(), ids, 7)), name
        assert torch.equal(route(base[:, 0], ids, 7), route(base[:, :1].contiguous(), ids, 7).reshape(50)), name


def check_public_function(dev, native_route):
    """gammagl_amd.utils.segment_softmax: the reference's module path and signature; native for f32 rows the capability query
    accepts (same bits as the op), the composition (== layers.segment_softmax) for everything else."""
    import gammagl_amd.utils.softmax as sm
    from gammagl_amd.utils import segment_softmax

    assert segment_softmax is sm.segment_softmax
    gen = torch.Generator(device=dev).manual_seed(4)
    ids = torch.randint(0, 30, (400,), generator=gen, device=dev)
    x = torch.randn(400, 8, generator=gen, device=dev)
    want = native_route(x, ids, 30)
    assert torch.equal(segment_softmax(x, ids, 30), want)
    assert torch.equal(segment_softmax(x, ids.to(torch.int32), 30), want)          # ids of another integer dtype are cast
    assert torch.equal(segment_softmax(x, ids), native_route(x, ids, int(ids.max()) + 1))   # num_segments inferred
    xr = x.clone().requires_grad_(True)
    yr = segment_softmax(xr, ids, 30)
    assert "softmax" in yr.grad_fn.name().lower(), yr.grad_fn.name()   # one node, not the composition's chain
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        xd = x.to(dt)
        assert torch.equal(segment_softmax(xd, ids, 30), layers.segment_softmax(xd, ids, 30)), dt
    for one in (x[:, 0].contiguous(), x[:, :1].contiguous()):                      # one-column logits: measured slower natively
        assert torch.equal(segment_softmax(one, ids, 30), layers.segment_softmax(one, ids, 30))
    wide = torch.randn(400, 65, generator=gen, device=dev)                          # a K the capability query refuses
    xa, xb = wide.clone().requires_grad_(True), wide.clone().requires_grad_(True)
    ya, yb = segment_softmax(xa, ids, 30), layers.segment_softmax(xb, ids, 30)
    assert torch.equal(ya, yb)
    go = torch.randn(ya.shape, generator=gen, device=dev)
    ya.backward(go)
    yb.backward(go)
    assert torch.equal(xa.grad, xb.grad)


def check_routes_agree(routes, dev, seed=9):
    """the hosts are checked against each other bit for bit, forward and gradient (long rows included)"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    for K, kind in ((1, "power"), (8, "power"), (6, "uniform"), (12, "sorted")):
        ids = make_ids(kind, 500, 60_000, gen, dev)
        x = torch.randn((60_000,) + shaped(K), generator=gen, device=dev) * 3
        g = torch.randn(x.shape, generator=gen, device=dev)
        res = {name: run(route, x, ids, 500, g) for name, route in routes.items()}
        first = next(iter(res))
        for name, (y, gx) in res.items():
            assert torch.equal(y, res[first][0]) and torch.equal(gx, res[first][1]), (first, name, K, kind)
