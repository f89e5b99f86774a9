"""Cases shared by tests/test_spmm_rows_host.py (host + emulation libraries, CPU tensors) and tests/test_gpu_spmm_rows.py
(MI355X): the restricted aggregate ``spmm_rows`` == the full aggregate indexed, forward and backward, under torch.equal.

The graph is the smallest on which the restricted plan pair can go wrong: N = 300, ~6000 weighted edges in source-sorted
COO order; a LISTED destination with 700 in-edges (a long row of the restricted forward plan), an UNLISTED one with 700
(dropped whole), a source with 700 out-edges into listed rows (a long row of the restricted TRANSPOSED plan), a listed row
without in-edges, rows 0 and N - 1 listed.  The plans' chunk at this size is 256 (checked), so 700-element rows take the
long-row route."""
import numpy as np
import pytest
import torch

N = 300
HUB_IN, HUB_OUT = 700, 700
WIDTHS = (48, 8, 4)
ROW_LISTS = ("empty", "single", "every", "random8")
A_LISTED, B_UNLISTED, Z_EMPTY, S_SOURCE = 17, 41, 123, 77


def random8():
    """~8 % of the rows, with the special ones put in / kept out (sorted, unique)."""
    g = torch.Generator().manual_seed(11)
    keep = torch.rand(N, generator=g) < 0.08
    keep[[0, N - 1, A_LISTED, Z_EMPTY]] = True
    keep[B_UNLISTED] = False
    return torch.nonzero(keep).reshape(-1)


def graph():
    """(edge_index [2, E] int64 sorted by source, weights [E] f32)"""
    g = torch.Generator().manual_seed(5)
    listed = random8()
    targets = listed[listed != Z_EMPTY]
    src = [torch.randint(0, N, (3900,), generator=g), torch.randint(0, N, (HUB_IN,), generator=g),
           torch.randint(0, N, (HUB_IN,), generator=g), torch.full((HUB_OUT,), S_SOURCE, dtype=torch.int64)]
    dst = [torch.randint(0, N, (3900,), generator=g), torch.full((HUB_IN,), A_LISTED, dtype=torch.int64),
           torch.full((HUB_IN,), B_UNLISTED, dtype=torch.int64), targets[torch.randint(0, targets.numel(), (HUB_OUT,), generator=g)]]
    src, dst = torch.cat(src), torch.cat(dst)
    keep = dst != Z_EMPTY
    src, dst = src[keep], dst[keep]
    order = torch.argsort(src, stable=True)
    ei = torch.stack([src[order], dst[order]]).contiguous()
    w = torch.rand(ei.shape[1], generator=g) - 0.3     # both signs: a skipped term is w * (+0) = +0 or -0
    return ei, w


def row_list(name):
    if name == "empty":
        return torch.empty(0, dtype=torch.int64)
    if name == "single":
        return torch.tensor([A_LISTED])
    if name == "every":
        return torch.arange(N)
    return random8()


def check_graph(eng, ei):
    """the properties the cases rely on"""
    E = int(ei.shape[1])
    assert 5500 < E < 6300
    assert int(eng.lib.ggl_policy_chunk(E)) < min(HUB_IN, HUB_OUT)
    deg_in = torch.bincount(ei[1].cpu(), minlength=N)
    assert deg_in[A_LISTED] >= HUB_IN and deg_in[B_UNLISTED] >= HUB_IN and deg_in[Z_EMPTY] == 0
    rows = random8()
    assert {0, N - 1, A_LISTED, Z_EMPTY} <= set(rows.tolist()) and B_UNLISTED not in rows.tolist()
    assert bool((ei[0, 1:] >= ei[0, :-1]).all())


def check_restricted_plans(eng, ei, w, dev):
    """both plans of the 8 % pair have rows longer than the chunk, and the transposed one is a FILTER of the full one"""
    gp = eng.graph_plan(ei, N)
    rows = random8().to(dev)
    rp = eng.rows_plan(gp, w, rows)
    assert rp.fwd.n_long >= 1 and rp.bwd.n_long >= 1, (rp.fwd.n_long, rp.bwd.n_long)
    assert rp.fwd.N == rows.numel() and rp.bwd.N == N and rp.fwd.E == rp.bwd.E == int(rp.col.numel())
    listed = torch.zeros(N, dtype=torch.bool)
    listed[rows.cpu()] = True
    assert rp.fwd.E == int(listed[ei[1].cpu()].sum())
    # transposed: the kept destinations of every source row, in the full plan's order, renamed to their rank
    colT, rowptrT = gp.colT.cpu().long(), gp.bwd.rowptr.cpu()
    keep = listed[colT]
    rank = torch.full((N,), -1, dtype=torch.int64)
    rank[rows.cpu()] = torch.arange(rows.numel())
    assert torch.equal(rp.colT.cpu().long(), rank[colT[keep]])
    assert torch.equal(rp.bwd.rowptr.cpu(), torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(keep.long(), 0)])[rowptrT])


def check_values(route, ei, w, dev, oracle, K, rows_name, weighted):
    """`route` = (spmm_rows(ei, w, x, rows, bias), spmm_epi_full(ei, w, x, bias)) on tensors of device `dev`."""
    rows_fn, full_fn = route
    g = torch.Generator().manual_seed(100 + K)
    x = torch.randn(N, K, generator=g)
    bias = torch.randn(1, K, generator=g)
    rows = row_list(rows_name)
    go = torch.randn(rows.numel(), K, generator=g)
    wt = w if weighted else None
    want_full = oracle.spmm_sum_fwd(ei.numpy(), (w if weighted else torch.ones_like(w)).numpy(), x.numpy())
    want = torch.from_numpy(want_full)[rows] + bias
    ei_d, w_d, rows_d = ei.to(dev), (wt.to(dev) if weighted else None), rows.to(dev)
    xa, ba = x.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
    xb, bb = x.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
    y = rows_fn(ei_d, w_d, xa, rows_d, ba)
    full = full_fn(ei_d, w_d, xb, bb)
    assert y.shape == (rows.numel(), K) and y.is_contiguous()
    assert torch.equal(y, full[rows_d]), "spmm_rows differs from spmm_epi(...)[rows]"
    assert torch.equal(y.detach().cpu(), want), "spmm_rows differs from the oracle's full aggregate, indexed, plus bias"
    y.backward(go.to(dev))
    scattered = torch.zeros(N, K)
    scattered[rows] = go
    full.backward(scattered.to(dev))
    assert xa.grad.shape == (N, K)
    assert torch.equal(xa.grad, xb.grad), "gx differs from the full path fed the scattered gradient"
    assert torch.equal(ba.grad, bb.grad), "gbias differs from the full path fed the scattered gradient"
    return y.detach(), xa.grad, ba.grad


def check_errors(rows_fn, ei, w, dev):
    x = torch.randn(N, 8).to(dev)
    ei, w = ei.to(dev), w.to(dev)
    bad = {"unsorted": torch.tensor([5, 3, 9]), "duplicate": torch.tensor([3, 5, 5, 9]), "negative": torch.tensor([-1, 4]),
           "past the end": torch.tensor([4, N])}
    for what, rows in bad.items():
        with pytest.raises((RuntimeError, IndexError)):
            rows_fn(ei, w, x, rows.to(dev), None)
            pytest.fail(f"{what} row list accepted")
    with pytest.raises(RuntimeError, match="weight"):
        rows_fn(ei, w.clone().requires_grad_(True), x, torch.tensor([1, 2]).to(dev), None)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        rows_fn(ei, w, torch.randn(N, 6).to(dev), torch.tensor([1, 2]).to(dev), None)
    with pytest.raises(RuntimeError):
        rows_fn(ei, w, x, torch.tensor([1, 2], dtype=torch.int32).to(dev), None)


def check_cache(rows_fn, built, ei, w, dev):
    """`built()` = plans built so far on this route.  Same row tensor: nothing is built; a new one: a new pair."""
    x = torch.randn(N, 8).to(dev)
    ei, w = ei.to(dev), w.to(dev)
    rows = random8().to(dev)
    y0 = rows_fn(ei, w, x, rows, None)
    n0 = built()
    y1 = rows_fn(ei, w, x, rows, None)
    assert built() == n0, "a second call with the same row tensor built a plan"
    other = rows.clone()
    y2 = rows_fn(ei, w, x, other, None)
    assert built() == n0 + 2, "a new row tensor must build a new pair (forward + transposed)"
    assert torch.equal(y0, y1) and torch.equal(y0, y2)


def check_step(make_trainer, reseed, dist_module, monkeypatch, dev, steps=3):
    """Two trainers, same seed, dropout 0.5: the restricted output layer and GGL_OUT_ROWS=0 give the same losses and
    parameters, and both count six aggregations."""
    g = torch.Generator().manual_seed(3)
    F_in, n_cls = 12, 10     # (10 classes: padded to 12 columns inside the last GEMM, as 47 -> 48)
    x = torch.randn(N, F_in, generator=g).to(dev)
    y = torch.randint(0, n_cls, (N,), generator=g).to(dev)
    train = random8().to(dev)
    out = {}
    for on in (True, False):
        monkeypatch.setattr(dist_module, "OUT_ROWS", on)
        reseed()
        tr = make_trainer(F_in, n_cls)
        restricted, inner = [], tr.pg.aggregate

        def spy(*a, _inner=inner, _seen=restricted, **kw):
            _seen.append(kw.get("out_rows") is not None)
            return _inner(*a, **kw)

        monkeypatch.setattr(tr.pg, "aggregate", spy)
        losses = [tr.step(x, y, train, int(train.numel())).clone() for _ in range(steps)]
        assert tr.net.agg_per_step == 6
        assert sum(restricted) == (steps if on else 0) and len(restricted) == 3 * steps   # the output layer only
        out[on] = (losses, [p.detach().clone() for p in tr.net.parameters()])
    for la, lb in zip(out[True][0], out[False][0]):
        assert torch.equal(la, lb), (out[True][0], out[False][0])
    assert float(out[True][0][0]) != float(out[True][0][-1])
    for pa, pb in zip(out[True][1], out[False][1]):
        assert torch.equal(pa, pb)
    return out


def as_numpy(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())
