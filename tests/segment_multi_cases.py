"""Shared cases of the fused multi-statistic segment aggregate (Engine.segment_multi, ggl_segment_multi_fwd / _bwd,
csrc/multiagg.hpp), of mpops.unsorted_segment_min, the global_*_pool functions and layers.PNAConv, for
tests/test_segment_multi_host.py (host library, CPU tensors) and tests/test_gpu_segment_multi.py (MI355X).  Not a test module.

The contract (include/ggl_mpops.h): out [N, K / C, A, C]; per row and column S, Q, min, max and the witnesses are carried in
position order, every step one rounded f32 operation; a row longer than the plan's chunk is cut into pieces that are reduced
from the start values and merged in ascending order; the backward is one walk with per-(row, column) coefficients c0, c1.
`oracle_forward` / `oracle_backward` restate that order in numpy float32, walking the plan's own rowptr / perm / chunk, and
the kernels are held to them on the bits."""
import contextlib
import ctypes
import functools

import numpy as np
import torch

from spmm16_cases import same_bits

N, E = 48, 1500
HUB, EMPTY, SINGLES = 3, (7, 31), (10, 11, 12, 13, 14, 15)   # a third of the elements; none; exactly one each
SHAPES = ((4, 4), (8, 8), (64, 64), (48, 16), (20, 5), (75, 75), (272, 68))       # (K, C)
AGG_SETS = (("mean", "min", "max", "std"), ("sum", "mean", "min", "max", "var", "std"), ("min",), ("var",), ("sum", "max"),
            ("std", "mean"))
PNA_SET = AGG_SETS[0]
CHUNKS = (8, 4096)
CODE = {"sum": 0, "mean": 1, "min": 2, "max": 3, "var": 4, "std": 5}
U = 2.0 ** -24
FMAX = np.finfo(np.float32).max
f32 = np.float32


@contextlib.contextmanager
def forced_chunk(eng, chunk):
    """the engine's long-row threshold, plans rebuilt"""
    old = eng.chunk
    eng.chunk = chunk
    eng.graph_cache.clear(); eng.seg_cache.clear()
    try:
        yield
    finally:
        eng.chunk = old
        eng.graph_cache.clear(); eng.seg_cache.clear()


@functools.lru_cache(maxsize=None)
def _ids_cpu(seed=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    others = [s for s in range(N) if s != HUB and s not in EMPTY and s not in SINGLES]
    rest = E - E // 3 - len(SINGLES)
    pick = torch.tensor(others)[torch.randint(0, len(others), (rest,), generator=g)]
    ids = torch.cat([torch.full((E // 3,), HUB), torch.tensor(SINGLES), pick])
    ids = ids[torch.randperm(E, generator=g)].contiguous()
    cnt = torch.bincount(ids, minlength=N)
    assert cnt[HUB] == E // 3 and all(cnt[s] == 0 for s in EMPTY) and all(cnt[s] == 1 for s in SINGLES)
    assert all(cnt[s] >= 2 for s in others)
    return ids


def make_ids(dev, sorted_ids=False):
    """int64 [E]: unsorted (the plan carries a perm), or the same ids sorted (no perm)"""
    ids = _ids_cpu()
    return (torch.sort(ids)[0] if sorted_ids else ids).contiguous().to(dev)


def make_x(K, dev, kind="randn", seed=5):
    """randn for the float64 checks; round(randn * 2) / 4 where ties and witnesses are tested (many equal values, +0.0 / -0.0)"""
    g = torch.Generator(device="cpu").manual_seed(seed + K)
    x = torch.randn(E, K, generator=g)
    if kind == "ties":
        x = torch.round(x * 2) / 4
    return x.to(dev)


def make_g(K, A, dev, seed=9):
    g = torch.Generator(device="cpu").manual_seed(seed + K + A)
    return torch.randn(N, A * K, generator=g).to(dev)


def stat(out, a, A, C):
    """statistic number a of out [N, K / C, A, C] as [N, K]"""
    n = out.shape[0]
    return out.reshape(n, -1, A, C)[:, :, a, :].reshape(n, -1)


def to_layout(stats, C):
    """[N, K] statistics -> out [N, A * K]"""
    n, K = stats[0].shape
    return np.concatenate([s.reshape(n, K // C, 1, C) for s in stats], 2).reshape(n, len(stats) * K)


# ---- the serial oracle -------------------------------------------------------------------------------------------------------
def _piece(x, es):
    K = x.shape[1]
    S, Q = np.zeros(K, f32), np.zeros(K, f32)
    mn, mx = np.full(K, FMAX, f32), np.full(K, -FMAX, f32)
    an, ax = np.full(K, E, np.int32), np.full(K, E, np.int32)
    for e in es:
        v = x[e]
        S = S + v
        Q = Q + v * v
        u = mx < v
        mx, ax = np.where(u, v, mx), np.where(u, np.int32(e), ax)
        u = v < mn
        mn, an = np.where(u, v, mn), np.where(u, np.int32(e), an)
    return S, Q, mn, mx, an, ax


def oracle_forward(plan, x, empty_zero=False):
    """every statistic [N, K] + mean + witnesses, in numpy float32, in the header's operation order (chunk rule included)"""
    rowptr = plan.rowptr.cpu().numpy()
    perm = None if plan.perm is None else plan.perm.cpu().numpy()
    xh = x.detach().cpu().numpy()
    K, chunk = xh.shape[1], int(plan.chunk)
    r = {k: np.empty((plan.N, K), f32) for k in ("sum", "mean", "min", "max", "var", "std")}
    r["argmin"], r["argmax"] = np.empty((plan.N, K), np.int32), np.empty((plan.N, K), np.int32)
    with np.errstate(all="ignore"):
        for i in range(plan.N):
            beg, end = int(rowptr[i]), int(rowptr[i + 1])
            n = end - beg
            es = np.arange(beg, end) if perm is None else perm[beg:end]
            if n > chunk:
                S, Q = np.zeros(K, f32), np.zeros(K, f32)
                mn, mx = np.full(K, FMAX, f32), np.full(K, -FMAX, f32)
                an, ax = np.full(K, E, np.int32), np.full(K, E, np.int32)
                for b in range(0, n, chunk):
                    pS, pQ, pmn, pmx, pan, pax = _piece(xh, es[b:b + chunk])
                    S, Q = S + pS, Q + pQ
                    u = mx < pmx
                    mx, ax = np.where(u, pmx, mx), np.where(u, pax, ax)
                    u = pmn < mn
                    mn, an = np.where(u, pmn, mn), np.where(u, pan, an)
            else:
                S, Q, mn, mx, an, ax = _piece(xh, es)
            nf = f32(n)
            mean, msq = (S / nf, Q / nf) if n > 1 else (S, Q)
            var = msq - mean * mean
            std = np.sqrt(np.fmax(var, f32(0)) + f32(1e-5))
            if n == 0 and empty_zero:
                mn, mx = np.zeros(K, f32), np.zeros(K, f32)
            for k, v in (("sum", S), ("mean", mean), ("min", mn), ("max", mx), ("var", var), ("std", std), ("argmin", an),
                         ("argmax", ax)):
                r[k][i] = v
    assert all(r[k].dtype == f32 for k in CODE)
    return r


def oracle_backward(plan, x, g, aggs, C, fw):
    """gx [E, K] in numpy float32 from the forward oracle's mean / std / witnesses, in the header's operation order"""
    rowptr = plan.rowptr.cpu().numpy()
    perm = None if plan.perm is None else plan.perm.cpu().numpy()
    xh, gh = x.detach().cpu().numpy(), g.detach().cpu().numpy()
    K, A = xh.shape[1], len(aggs)
    gs = {a: gh.reshape(plan.N, K // C, A, C)[:, :, i, :].reshape(plan.N, K) for i, a in enumerate(aggs)}
    sq = "var" in aggs or "std" in aggs
    s0 = np.sqrt(f32(1e-5))
    gx = np.full((plan.E, K), np.nan, f32)
    with np.errstate(all="ignore"):
        for i in range(plan.N):
            beg, end = int(rowptr[i]), int(rowptr[i + 1])
            if end == beg:
                continue
            nf = f32(max(end - beg, 1))
            gv = gs["var"][i] if "var" in aggs else np.zeros(K, f32)
            if "std" in aggs:
                sd = fw["std"][i]
                t = np.where(sd > s0, gs["std"][i] / (f32(2) * sd), f32(0)).astype(f32)
                gv = gv + t if "var" in aggs else t
            c1 = (f32(2) * gv) / nf if sq else np.zeros(K, f32)
            c0 = np.zeros(K, f32)
            if "sum" in aggs:
                c0 = c0 + gs["sum"][i]
            if "mean" in aggs:
                c0 = c0 + gs["mean"][i] / nf
            if sq:
                c0 = c0 - c1 * fw["mean"][i]
            for p in range(beg, end):
                e = p if perm is None else perm[p]
                t = c0 + c1 * xh[e] if sq else c0
                if "max" in aggs:
                    t = np.where(fw["argmax"][i] == e, t + gs["max"][i], t)
                if "min" in aggs:
                    t = np.where(fw["argmin"][i] == e, t + gs["min"][i], t)
                gx[e] = t
    assert gx.dtype == f32
    return gx


def run_engine(eng, x, ids, aggs, C, empty_zero=False, g=None):
    """(out, argmin, argmax, gx) of Engine.segment_multi"""
    xx = x.clone().requires_grad_(g is not None)
    out, amin, amax = eng.segment_multi(xx, ids, N, aggs, C, empty_zero, return_witnesses=True)
    if g is not None:
        out.backward(g)
    return out.detach(), amin, amax, xx.grad


def check_oracle(eng, dev, K, C, aggs, kind="ties"):
    """forward (chunk rule included) and backward on the bits of the serial oracle, unsorted and sorted ids, chunked and whole;
    two identical calls identical"""
    x, A = make_x(K, dev, kind), len(aggs)
    g = make_g(K, A, dev)
    for sorted_ids in (False, True):
        ids = make_ids(dev, sorted_ids)
        for chunk in CHUNKS:
            with forced_chunk(eng, chunk):
                plan = eng.seg_plan(ids, N)
                assert (plan.n_long > 0) == (chunk == 8) and (plan.perm is None) == sorted_ids
                for ez in (False, True):
                    out, amin, amax, gx = run_engine(eng, x, ids, aggs, C, ez, g)
                    fw = oracle_forward(plan, x, ez)
                    want = torch.from_numpy(to_layout([fw[a] for a in aggs], C)).to(dev)
                    assert same_bits(out, want), (K, C, aggs, chunk, sorted_ids, ez)
                    if "min" in aggs:
                        assert torch.equal(amin.cpu(), torch.from_numpy(fw["argmin"]))
                    if "max" in aggs:
                        assert torch.equal(amax.cpu(), torch.from_numpy(fw["argmax"]))
                    assert (amin is None) == ("min" not in aggs) and (amax is None) == ("max" not in aggs)
                    assert not torch.isnan(gx).any()          # every element of gx is written
                    assert same_bits(gx, torch.from_numpy(oracle_backward(plan, x, g, aggs, C, fw)).to(dev)), (K, C, aggs, chunk)
                out2, _, _, gx2 = run_engine(eng, x, ids, aggs, C, True, g)
                assert same_bits(out, out2) and same_bits(gx, gx2)


# ---- the composition on the existing ops -------------------------------------------------------------------------------------
def composed_stats(eng, x, ids):
    """name -> [N, K] from unsorted_segment_sum / mean / max in f32 torch: msq - mean * mean, sqrt(relu(.) + 1e-5), min = -max(-x).
    The square root is the correctly rounded one, as the contract's sqrtf: taken in float64 and rounded once (exact for f32
    operands).  torch.sqrt's vectorised CPU kernel is NOT correctly rounded — measured here: 6247 of 10^6 uniform values one
    ulp off numpy's and the float64 result — so it cannot serve as the bit reference; every other step is plain f32 torch."""
    mean = eng.c_segment_mean(x, ids, N)
    var = eng.c_segment_mean(x * x, ids, N) - mean * mean
    mx, arg = eng.segment_max_with_arg(x, ids, N)
    return {"sum": eng.c_segment_sum(x, ids, N), "mean": mean, "var": var,
            "std": torch.sqrt((torch.relu(var) + 1e-5).double()).float(), "max": mx, "argmax": arg, "min": -eng.c_segment_max(-x, ids, N)}


def check_composition(eng, dev, K, C, aggs):
    """bit equality with the composition: sums for rows of at most chunk elements, max / argmax / min on every row, hub row
    chunked or not; empty_zero == where(count > 0, ., 0)"""
    x, A = make_x(K, dev, "ties"), len(aggs)
    for sorted_ids in (False, True):
        ids = make_ids(dev, sorted_ids)
        cnt = torch.bincount(ids, minlength=N)
        for chunk in CHUNKS:
            with forced_chunk(eng, chunk):
                ref = composed_stats(eng, x, ids)
                short = (cnt <= chunk)
                out, amin, amax, _ = run_engine(eng, x, ids, aggs, C)
                outz = run_engine(eng, x, ids, aggs, C, True)[0]
                for a, name in enumerate(aggs):
                    got, gotz = stat(out, a, A, C), stat(outz, a, A, C)
                    rows = slice(None) if name in ("min", "max") else short
                    assert same_bits(got[rows], ref[name][rows]), (K, C, aggs, name, chunk)
                    wantz = torch.where((cnt > 0).unsqueeze(1), got, torch.zeros_like(got)) if name in ("min", "max") else got
                    assert same_bits(gotz, wantz), (name, "empty_zero")
                if "max" in aggs:
                    assert torch.equal(amax.long(), ref["argmax"])
                assert int(short.sum()) == (N if chunk == 4096 else int((cnt <= 8).sum())) and bool(short[list(EMPTY)].all())


# ---- float64 -----------------------------------------------------------------------------------------------------------------
def f64_stats(x64, ids):
    """name -> [N, K] in float64 torch (differentiable), empty rows 0 for min / max; also n' = max(n, 1)"""
    K = x64.shape[1]
    idx = ids.unsqueeze(1).expand(-1, K)
    cnt = torch.bincount(ids, minlength=N).double().unsqueeze(1)
    nn_ = cnt.clamp(min=1)
    s = torch.zeros(N, K, dtype=torch.float64, device=x64.device).index_add_(0, ids, x64)
    q = torch.zeros(N, K, dtype=torch.float64, device=x64.device).index_add_(0, ids, x64 * x64)
    mean, msq = s / nn_, q / nn_
    var = msq - mean * mean
    z = torch.zeros(N, K, dtype=torch.float64, device=x64.device)
    return {"sum": s, "mean": mean, "var": var, "std": torch.sqrt(torch.relu(var) + 1e-5),
            "max": z.scatter_reduce(0, idx, x64, "amax", include_self=False),
            "min": z.scatter_reduce(0, idx, x64, "amin", include_self=False)}, nn_


def gamma(m):
    return m * U / (1 - m * U)


def check_against_f64(eng, dev, K, C, aggs, worst=None):
    """sum / mean / min / max and gx within 1e-5 of the tensor's scale; var within B = gamma_{n+2} sum(x^2) / n' +
    gamma_{2n+3} (sum|x| / n')^2 per element, std within B / (std + std64) + 2 u std.  Precondition: no row with n >= 2 has
    var64 < 1e-3.  No row is left out."""
    x, A = make_x(K, dev, "randn"), len(aggs)
    g = make_g(K, A, dev)
    ids = make_ids(dev)
    cnt = torch.bincount(ids, minlength=N).double().unsqueeze(1)
    x64 = x.double().requires_grad_(True)
    ref, nn_ = f64_stats(x64, ids)
    assert float(ref["var"][(cnt >= 2).squeeze(1)].min()) >= 1e-3, "precondition: change the seed"
    assert float(ref["var"][(cnt == 1).squeeze(1)].abs().max()) == 0.0
    out64 = torch.cat([ref[a].reshape(N, K // C, 1, C) for a in aggs], 2).reshape(N, A * K)
    out64.backward(g.double())
    xa = x.double()
    sx2 = torch.zeros(N, K, dtype=torch.float64, device=dev).index_add_(0, ids, xa * xa)
    sab = torch.zeros(N, K, dtype=torch.float64, device=dev).index_add_(0, ids, xa.abs())
    B = gamma(cnt + 2) * sx2 / nn_ + gamma(2 * cnt + 3) * (sab / nn_) ** 2
    for chunk in CHUNKS:
        with forced_chunk(eng, chunk):
            out, _, _, gx = run_engine(eng, x, ids, aggs, C, True, g)
        for a, name in enumerate(aggs):
            got, want = stat(out, a, A, C).double(), ref[name].detach()
            err = (got - want).abs()
            if name == "var":
                assert bool((err <= B).all()), (name, chunk, float((err - B).max()))
            elif name == "std":
                bound = B / (got + want) + 2 * U * want
                assert bool((err <= bound).all()), (name, chunk, float((err - bound).max()))
            else:
                rel = float(err.max() / want.abs().max())
                if worst is not None:
                    worst[name] = max(worst.get(name, 0.0), rel)
                assert rel <= 1e-5, (name, chunk, rel)
            if name in ("var", "std"):
                one = (cnt == 1).squeeze(1)
                assert float(stat(out, a, A, C)[one].abs().max()) == (0.0 if name == "var" else float(np.sqrt(f32(1e-5))))
        rel = float((gx.double() - x64.grad).abs().max() / x64.grad.abs().max())
        if worst is not None:
            worst["gx"] = max(worst.get("gx", 0.0), rel)
        assert rel <= 1e-5, ("gx", aggs, chunk, rel)


# ---- ties and special values -------------------------------------------------------------------------------------------------
def check_special_values(eng, dev):
    """the witness is the smallest e among equals; NaN never wins min / max and propagates through sum; +0.0 / -0.0 keep the
    first element's sign"""
    K, aggs = 8, ("sum", "min", "max")
    ids = make_ids(dev)
    x = make_x(K, dev, "ties")
    hub = (ids == HUB).nonzero().squeeze(1)
    x[hub[5], 0] = float("nan")
    x[hub, 1] = 0.0
    x[hub[0], 1] = -0.0                 # the row's first element is -0.0, every other +0.0
    x[hub, 2] = 0.0
    x[hub[3:], 2] = -0.0                # ... and the other way round
    for chunk in CHUNKS:
        with forced_chunk(eng, chunk):
            out, amin, amax, _ = run_engine(eng, x, ids, aggs, K)
        s, mn, mx = (stat(out, a, 3, K) for a in range(3))
        assert torch.isnan(s[HUB, 0]) and not torch.isnan(mn[HUB, 0]) and not torch.isnan(mx[HUB, 0])
        assert int(amin[HUB, 0]) != int(hub[5]) and int(amax[HUB, 0]) != int(hub[5])
        for t in (mn, mx):
            assert float(t[HUB, 1]) == 0.0 and bool(torch.signbit(t[HUB, 1])) and not bool(torch.signbit(t[HUB, 2]))
        assert int(amin[HUB, 1]) == int(amax[HUB, 1]) == int(hub[0]) == int(amin[HUB, 2])
        xc, ic = x.cpu(), ids.cpu()
        for r in (HUB, 20, SINGLES[0]):
            rows = (ic == r).nonzero().squeeze(1)
            for k in range(3, K):
                col = xc[rows, k]
                assert int(amax[r, k]) == int(rows[(col == col.max()).nonzero()[0, 0]])
                assert int(amin[r, k]) == int(rows[(col == col.min()).nonzero()[0, 0]])
        assert all(int(amin[r, 0]) == E and int(amax[r, 0]) == E for r in EMPTY)
        assert all(float(mx[r, 0]) == -float(FMAX) and float(mn[r, 0]) == float(FMAX) and float(s[r, 0]) == 0.0 for r in EMPTY)


# ---- routes, refusals, memory --------------------------------------------------------------------------------------------------
def make_routes(eng):
    from gammagl_amd import cpp_ops, torch_ops

    def engine_route(x, ids, aggs, C, ez):
        return eng.segment_multi(x, ids, N, aggs, C, ez)

    def ops_route(ns):
        return lambda x, ids, aggs, C, ez: ns.segment_multi(x, ids, N, [CODE[a] for a in aggs], C, ez)

    return {"engine": engine_route, "torch.ops.ggl_agg": ops_route(cpp_ops.load_agg()),
            "torch.ops.gammagl_amd": ops_route(torch_ops.ops)}


def check_routes_agree(routes, eng, dev):
    from gammagl_amd.utils import segment_multi_aggregate

    ids = make_ids(dev)
    for (K, C), aggs in (((48, 16), PNA_SET), ((20, 5), AGG_SETS[1]), ((8, 8), ("min",)), ((64, 64), ("sum", "max"))):
        x, g = make_x(K, dev, "ties"), make_g(K, len(aggs), dev)
        res = {}
        for name, f in routes.items():
            xx = x.clone().requires_grad_(True)
            out = f(xx, ids, aggs, C, True)
            out.backward(g)
            res[name] = (out.detach(), xx.grad)
        xx = x.reshape(E, K // C, C).clone().requires_grad_(True)
        out = segment_multi_aggregate(xx, ids, N, aggs, empty_zero=True)
        assert out.shape == (N, K // C, len(aggs) * C)
        out.backward(g.reshape(out.shape))
        res["public"] = (out.detach().reshape(N, -1), xx.grad.reshape(E, K))
        first = res["engine"]
        for name, (o, gx) in res.items():
            assert same_bits(o, first[0]) and same_bits(gx, first[1]), (name, K, C, aggs)
    x2 = make_x(8, dev)
    assert segment_multi_aggregate(x2, ids, None, ("mean", "max")).shape == (N, 16)       # num_segments from the ids
    # the A/B switch: off means the composition is used
    old = eng.segment_multi_fused
    eng.segment_multi_fused = False
    try:
        xx = make_x(48, dev, "ties").requires_grad_(True)
        with forced_chunk(eng, 4096):
            o = eng.segment_multi(xx, ids, N, PNA_SET, 16, True)
            assert eng.stats["segment_multi"]["route"] == "composed"
            o.backward(make_g(48, 4, dev))
            eng.segment_multi_fused = True
            o2 = eng.segment_multi(xx.detach(), ids, N, PNA_SET, 16, True)
        assert eng.stats["segment_multi"] == {"route": "fused", "saved": ()} and same_bits(o.detach(), o2)
    finally:
        eng.segment_multi_fused = old


def check_saved_tensors(eng, dev):
    """("min",) and ("mean", "max") save no x; the PNA set saves x, mean, out and both witnesses"""
    ids, x = make_ids(dev), make_x(16, dev).requires_grad_(True)
    for aggs, want in ((("min",), ("argmin",)), (("mean", "max"), ("argmax",)), (("sum",), ()),
                       (PNA_SET, ("x", "mean", "out", "argmin", "argmax")), (("var",), ("x", "mean"))):
        seen = []
        with torch.autograd.graph.saved_tensors_hooks(lambda t: seen.append(t) or t, lambda t: t):
            out = eng.segment_multi(x, ids, N, aggs)
        assert eng.stats["segment_multi"] == {"route": "fused", "saved": want}, (aggs, eng.stats["segment_multi"])
        assert len(seen) == len(want)
        has_x = any(t.shape == x.shape and t.dtype == x.dtype and t.data_ptr() == x.data_ptr() for t in seen)
        assert has_x == ("x" in want), aggs
        out.sum().backward()
    with torch.no_grad():
        eng.segment_multi(x, ids, N, PNA_SET)
    assert eng.stats["segment_multi"]["saved"] == ()


def check_refusals(routes, eng, dev):
    import pytest
    from gammagl_amd.utils import segment_multi_aggregate

    ids, x = make_ids(dev), make_x(20, dev)
    with pytest.raises(RuntimeError, match="does not divide"):
        eng.segment_multi(x, ids, N, ("min",), C=3)
    with pytest.raises(RuntimeError, match="does not divide"):
        routes["torch.ops.ggl_agg"](x, ids, ("min",), 3, False)
    with pytest.raises(ValueError, match="given twice"):
        eng.segment_multi(x, ids, N, ("min", "min"))
    with pytest.raises(ValueError, match="unknown aggregator"):
        eng.segment_multi(x, ids, N, ("median",))
    with pytest.raises(ValueError, match="between 1 and 6"):
        eng.segment_multi(x, ids, N, ())
    ns = routes["torch.ops.ggl_agg"].__closure__[0].cell_contents
    with pytest.raises(RuntimeError, match="given twice"):
        ns.segment_multi(x, ids, N, [2, 2], 20, False)
    with pytest.raises(RuntimeError, match="unknown aggregator"):
        ns.segment_multi(x, ids, N, [9], 20, False)
    for bad in (x.double(), x.half(), x.long()):
        with pytest.raises(RuntimeError, match="expected scalar type Float"):
            segment_multi_aggregate(bad, ids, N)
        with pytest.raises(RuntimeError, match="expected scalar type Float"):
            eng.segment_multi(bad, ids, N)
    with pytest.raises(IndexError):
        eng.segment_multi(x[:-1], ids, N)
    with pytest.raises(IndexError):
        eng.segment_multi(x, ids, 5)            # an id out of range


def raw_call(eng, plan, x, aggs, C, empty_zero=False, g=None, drop=(), partial="exact"):
    """ggl_segment_multi_fwd (+ _bwd with g) through ctypes with exact-size buffers; `drop` names pointers handed as NULL.
    (rc_fwd, rc_bwd, out, mean, argmin, argmax, gx)"""
    from gammagl_amd._lib import _ptr

    dev, K, A = x.device, x.shape[1], len(aggs)
    codes = (ctypes.c_int * A)(*[CODE[a] if isinstance(a, str) else a for a in aggs])
    names = [a for a in aggs if isinstance(a, str)]
    nb = eng.lib.ggl_segment_multi_partial_bytes(plan.n_chunks, K, codes, A)
    part = torch.empty(nb, dtype=torch.uint8, device=dev) if (plan.n_long and partial == "exact") else None
    out = torch.full((plan.N, A * K), float("nan"), device=dev)
    mean = torch.full((plan.N, K), float("nan"), device=dev) if ("mean" not in drop and ("var" in names or "std" in names)) else None
    amin = torch.full((plan.N, K), -1, dtype=torch.int32, device=dev) if ("min" in names and "argmin" not in drop) else None
    amax = torch.full((plan.N, K), -1, dtype=torch.int32, device=dev) if ("max" in names and "argmax" not in drop) else None
    cs = plan.c_struct(part)
    st = eng._stream(dev)
    rc = eng.lib.ggl_segment_multi_fwd(_ptr(x), ctypes.byref(cs), K, C, codes, A, int(empty_zero), _ptr(out), _ptr(mean), _ptr(amin),
                                       _ptr(amax), st)
    rcb, gx = None, None
    if g is not None and rc == 0:
        gx = torch.full((plan.E, K), float("nan"), device=dev)
        cs = plan.c_struct(None)
        rcb = eng.lib.ggl_segment_multi_bwd(_ptr(g), None if "x" in drop else _ptr(x), None if "out" in drop else _ptr(out),
                                            _ptr(mean), _ptr(amin), _ptr(amax), ctypes.byref(cs), K, C, codes, A, _ptr(gx), st)
    return rc, rcb, out, mean, amin, amax, gx


def check_c_abi(eng, dev):
    """the C entry points with exact-size buffers against the oracle; every refusal of the header with its message"""
    from gammagl_amd import _lib

    assert _lib.ABI_VERSION == 12 and eng.lib.ggl_abi_version() == 12
    for name, n in (("ggl_segment_multi_partial_bytes", 4), ("ggl_segment_multi_fwd", 12), ("ggl_segment_multi_bwd", 13)):
        assert len(_lib.SIGNATURES[name][1]) == n
    full = (ctypes.c_int * 6)(0, 1, 2, 3, 4, 5)
    only_min = (ctypes.c_int * 1)(2)
    assert eng.lib.ggl_segment_multi_partial_bytes(0, 64, full, 6) == 0
    assert eng.lib.ggl_segment_multi_partial_bytes(5, 64, full, 6) >= 6 * 5 * 64 * 4
    assert 2 * 5 * 64 * 4 <= eng.lib.ggl_segment_multi_partial_bytes(5, 64, only_min, 1) < 3 * 5 * 64 * 4   # min pays for no sums
    ids = make_ids(dev)
    err = lambda: eng.lib.ggl_last_error().decode()
    for (K, C), aggs in (((20, 5), AGG_SETS[1]), ((48, 16), PNA_SET), ((8, 8), ("min",))):
        x, g = make_x(K, dev, "ties"), make_g(K, len(aggs), dev)
        for chunk in CHUNKS:
            with forced_chunk(eng, chunk):
                plan = eng.seg_plan(ids, N)
                rc, rcb, out, mean, amin, amax, gx = raw_call(eng, plan, x, aggs, C, True, g)
                assert rc == 0 and rcb == 0, err()
                fw = oracle_forward(plan, x, True)
                assert same_bits(out, torch.from_numpy(to_layout([fw[a] for a in aggs], C)).to(dev))
                if mean is not None:
                    assert same_bits(mean, torch.from_numpy(fw["mean"]).to(dev))
                assert same_bits(gx, torch.from_numpy(oracle_backward(plan, x, g, aggs, C, fw)).to(dev))
    # a panel one element into a buffer: the misaligned (one column per lane) path, same bits
    K, C, aggs = 48, 16, AGG_SETS[1]
    buf = torch.zeros(E * K + 1, device=dev)
    buf[1:] = make_x(K, dev, "ties").reshape(-1)
    xm = buf[1:].reshape(E, K)
    assert xm.data_ptr() % 16 == 4
    with forced_chunk(eng, 8):
        plan = eng.seg_plan(ids, N)
        g = make_g(K, 6, dev)
        a = raw_call(eng, plan, xm, aggs, C, False, g)
        b = raw_call(eng, plan, xm.clone(), aggs, C, False, g)
        assert a[0] == 0 and a[1] == 0 and same_bits(a[2], b[2]) and same_bits(a[6], b[6])
        # refusals
        x = make_x(20, dev)
        g20 = make_g(20, 1, dev)
        assert raw_call(eng, plan, x, ("min",), 3)[0] == _lib.GGL_EINVAL and "does not divide" in err()
        assert raw_call(eng, plan, x, ("min", "min"), 5)[0] == _lib.GGL_EINVAL and "duplicate" in err()
        assert raw_call(eng, plan, x, (7,), 5)[0] == _lib.GGL_EINVAL and "unknown" in err()
        assert raw_call(eng, plan, x, ("sum",), 5, partial=None)[0] == _lib.GGL_EINVAL and "plan->partial is NULL" in err()
        for aggs, drop, word in ((("std",), ("x",), "x is NULL"), (("var",), ("mean",), "mean is NULL"),
                                 (("std",), ("out",), "out is NULL"), (("min",), ("argmin",), "argmin is NULL"),
                                 (("max",), ("argmax",), "argmax is NULL")):
            r = raw_call(eng, plan, x, aggs, 5, False, g20, drop=drop)
            assert r[0] == 0 and r[1] == _lib.GGL_EINVAL and word in err(), (aggs, drop, err())


# ---- unsorted_segment_min and the pools --------------------------------------------------------------------------------------
DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, torch.float16, torch.bfloat16, torch.float32,
          torch.float64)


def check_segment_min(dev):
    """all nine dtypes against a numpy loop: empty rows hold numeric_limits<T>::max(), ties go to the first element (the f32
    gradient lands there); segment_min is the alias"""
    from gammagl_amd import mpops

    assert mpops.segment_min(torch.tensor([3.0, 1.0, 2.0], device=dev), torch.tensor([0, 0, 1], device=dev), 2).tolist() == [1.0, 2.0]
    assert "unsorted_segment_min" in mpops.__all__ and "segment_min" in mpops.__all__
    ids = make_ids(dev)
    ic = ids.cpu().numpy()
    g = torch.Generator(device="cpu").manual_seed(11)
    for dt in DTYPES:
        if dt.is_floating_point:
            x = (torch.round(torch.randn(E, 6, generator=g) * 2) / 4).to(dt)
            top = torch.finfo(dt).max
        else:
            info = torch.iinfo(dt)
            x = torch.randint(max(info.min, -100), min(info.max, 100) + 1, (E, 6), generator=g).to(dt)
            x[0, 0], x[1, 1] = info.min, info.max
            top = info.max
        got = mpops.unsorted_segment_min(x.to(dev), ids, N)
        assert got.dtype == dt and got.shape == (N, 6)
        xn = x.double().numpy()
        want = np.full((N, 6), float(top))
        for e in range(E):
            want[ic[e]] = np.minimum(want[ic[e]], xn[e])
        assert np.array_equal(got.cpu().double().numpy(), want), dt
    x = (torch.round(torch.randn(E, 6, generator=g) * 2) / 4).to(dev).requires_grad_(True)
    go = torch.randn(N, 6, generator=g).to(dev)
    mpops.unsorted_segment_min(x, ids, N).backward(go)
    want = np.zeros((E, 6), f32)
    xn, gn = x.detach().cpu().numpy(), go.cpu().numpy()
    for r in range(N):
        rows = np.nonzero(ic == r)[0]
        for k in range(6):
            if len(rows):
                want[rows[np.argmin(xn[rows, k])], k] = gn[r, k]        # np.argmin: the first of equals
    assert np.array_equal(x.grad.cpu().numpy(), want)
    x1 = torch.randn(E, generator=g).to(dev)                              # 1-d and 3-d inputs keep their trailing shape
    assert mpops.unsorted_segment_min(x1, ids, N).shape == (N,)
    assert mpops.unsorted_segment_min(torch.randn(E, 2, 3, generator=g).to(dev), ids).shape == (N, 2, 3)


def check_pools(dev):
    from gammagl_amd import layers

    g = torch.Generator(device="cpu").manual_seed(12)
    x = torch.randn(200, 7, generator=g).to(dev)
    batch = torch.sort(torch.randint(0, 9, (200,), generator=g))[0].to(dev)
    B = int(batch.max()) + 1
    idx = batch.unsqueeze(1).expand(-1, 7)
    z = torch.zeros(B, 7, device=dev)
    for fn, red, whole in ((layers.global_sum_pool, "sum", x.sum(0, keepdim=True)), (layers.global_mean_pool, "mean", x.mean(0, keepdim=True)),
                           (layers.global_max_pool, "amax", x.max(0, keepdim=True)[0]), (layers.global_min_pool, "amin", x.min(0, keepdim=True)[0])):
        want = z.scatter_reduce(0, idx, x, red, include_self=False)
        for size in (None, B):
            got = fn(x, batch, size)
            assert got.shape == (B, 7) and torch.allclose(got, want, rtol=1e-6, atol=1e-6), red
        assert torch.equal(fn(x, None), whole)
        assert fn(x, batch, B + 2).shape == (B + 2, 7)


# ---- PNAConv -------------------------------------------------------------------------------------------------------------------
SCALERS = ("identity", "amplification", "attenuation", "linear", "inverse_linear")


def pna_graph(dev, n=40, e=600, seed=21):
    g = torch.Generator(device="cpu").manual_seed(seed)
    dst = torch.randint(0, n - 2, (e,), generator=g)
    dst = dst + (dst >= 5).long() + (dst >= 17).long()          # nodes 5 and 18 receive nothing
    dst[: e // 4] = 2
    ei = torch.stack([torch.randint(0, n, (e,), generator=g), dst])[:, torch.randperm(e, generator=g)].contiguous()
    deg = torch.bincount(torch.bincount(ei[1], minlength=n))
    return ei.to(dev), deg


def _f64_aggregate(conv):
    """a float64 torch restatement of PNAConv.aggregate (no project op)"""
    def aggregate(inputs, index, num_nodes=None, aggr=None):
        dst, n = index[1], num_nodes
        T, F = inputs.shape[1], inputs.shape[2]
        st, _ = None, None
        flat = inputs.reshape(inputs.shape[0], T * F)
        idx = dst.unsqueeze(1).expand(-1, T * F)
        cnt = torch.bincount(dst, minlength=n).to(inputs.dtype).unsqueeze(1)
        nn_ = cnt.clamp(min=1)
        z = torch.zeros(n, T * F, dtype=inputs.dtype, device=inputs.device)
        s = z.index_add(0, dst, flat)
        mean = s / nn_
        var = z.index_add(0, dst, flat * flat) / nn_ - mean * mean
        st = {"sum": s, "mean": mean, "var": var, "std": torch.sqrt(torch.relu(var) + 1e-5),
              "max": z.scatter_reduce(0, idx, flat, "amax", include_self=False),
              "min": z.scatter_reduce(0, idx, flat, "amin", include_self=False)}
        out = torch.cat([st[a].reshape(n, T, F) for a in conv.aggregators], -1)
        deg = cnt.clamp(min=1).reshape(-1, 1, 1)
        outs = []
        for s_ in conv.scalers:
            if s_ == "amplification":
                out = out * (torch.log(deg + 1) / conv.avg_deg["log"])
            elif s_ == "attenuation":
                out = out * (conv.avg_deg["log"] / torch.log(deg + 1))
            elif s_ == "linear":
                out = out * (deg / conv.avg_deg["lin"])
            elif s_ == "inverse_linear":
                out = out * (conv.avg_deg["lin"] / deg)
            outs.append(out)
        return torch.cat(outs, -1)
    return aggregate


def check_pnaconv(eng, dev):
    """fused=True equals fused=False on outputs and ALL parameter gradients: on the bits with chunk 4096 (every destination's
    edges walked in one piece), within 1e-5 when chunked; both within 1e-5 of a float64 torch restatement; towers 1 and 2,
    divide_input both ways, edge_dim set and unset, all five scalers.  (fused=False is utils.segment_multi_composed: the
    statistics from the mpops segment ops, its backward the contract's formula in torch in the contract's operation order —
    autograd through the five ops adds the same terms in another order and lands 1.7e-8 .. 2.8e-7 away in the gradients in
    front of the aggregate.)"""
    import copy
    from gammagl_amd import layers

    ei, deg = pna_graph(dev)
    n = 40
    gen = torch.Generator(device="cpu").manual_seed(22)
    for towers, divide, edge_dim, pre, post in ((1, False, None, 1, 1), (2, True, 3, 2, 2), (2, False, None, 1, 2), (1, True, 3, 2, 1)):
        torch.manual_seed(23 + towers)
        fin, fout = 12, 8
        aggs = ("mean", "min", "max", "std") if towers == 1 else ("sum", "mean", "min", "max", "var", "std")
        conv = layers.PNAConv(fin, fout, aggs, SCALERS, deg, edge_dim=edge_dim, towers=towers, pre_layers=pre, post_layers=post,
                              divide_input=divide, fused=True).to(dev)
        x = torch.randn(n, fin, generator=gen).to(dev)
        ea = torch.randn(ei.shape[1], edge_dim, generator=gen).to(dev) if edge_dim else None
        go = torch.randn(n, fout, generator=gen).to(dev)

        def run(model, xin, eattr, gout):
            model.zero_grad()
            y = model(xin, ei, eattr)
            y.backward(gout)
            return y.detach(), [p.grad.clone() for p in model.parameters()]

        c64 = copy.deepcopy(conv).double()
        c64.aggregate = _f64_aggregate(c64)
        y64, g64 = run(c64, x.double(), None if ea is None else ea.double(), go.double())

        def close(a, b):
            return float((a.double() - b.double()).abs().max()) <= 1e-5 * max(float(b.double().abs().max()), 1e-30)

        for chunk in CHUNKS:
            with forced_chunk(eng, chunk):
                conv.fused = True
                yf, gf = run(conv, x, ea, go)
                conv.fused = False
                yc, gc = run(conv, x, ea, go)
            if chunk == 4096:
                names = [k for k, _ in conv.named_parameters()]
                assert same_bits(yf, yc), (towers, divide, edge_dim)
                for k, a, b in zip(names, gf, gc):
                    assert same_bits(a, b), (towers, divide, edge_dim, k, float((a - b).abs().max() / b.abs().max()))
            else:
                assert close(yf, yc) and all(close(a, b) for a, b in zip(gf, gc)), (towers, divide, edge_dim)
            for y, gs in ((yf, gf), (yc, gc)):
                assert close(y, y64) and all(close(a, b) for a, b in zip(gs, g64)), (towers, divide, edge_dim, chunk)
    import pytest
    with pytest.raises(ValueError, match="Unknown aggregator"):
        layers.PNAConv(4, 4, ("median",), ("identity",), deg)
    with pytest.raises(ValueError, match="Unknown scaler"):
        layers.PNAConv(4, 4, ("mean",), ("cube",), deg)
