"""spmm_rows on the MI355X: the HIP library through the ctypes engine and through torch.ops.ggl, against the full aggregate
indexed by the rows (torch.equal, gradients included), the oracle, and each other; the restricted output layer of the
one-GPU training step, eager and through a captured hipGraph.  Cases: tests/spmm_rows_cases.py."""
import pytest
import torch

import spmm_rows_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def eng():
    import gammagl_amd

    return gammagl_amd.engine()


@pytest.fixture(scope="module")
def ops():
    from gammagl_amd import cpp_ops

    return cpp_ops.load()


@pytest.fixture(scope="module")
def data():
    return rc.graph()


@pytest.fixture(scope="module")
def routes(eng, ops):
    def rows_fn(ei, w, x, rows, bias):
        return eng.spmm_rows(eng.graph_plan(ei, rc.N), w, x, rows, bias)

    def full_fn(ei, w, x, bias):
        return eng.spmm_epi(eng.graph_plan(ei, rc.N), w, x, bias=bias)

    return {"ctypes": (rows_fn, full_fn),
            "cpp": (ops.spmm_rows, lambda ei, w, x, bias: ops.spmm_epi(ei, w, x, False, None, bias, False, 0.0))}


@pytest.fixture(scope="module")
def dev_data(data, dev):
    """ONE device copy of the edge list and weights for the whole module: the plan caches key on tensor identity."""
    return data[0].to(dev), data[1].to(dev)


def _on(dev_data, route):
    """the route's functions bound to the module's device tensors (so every case reuses the cached full plans)"""
    ei_d, w_d = dev_data
    rows_fn, full_fn = route
    return (lambda ei, w, x, rows, bias: rows_fn(ei_d, (w_d if w is not None else None), x, rows, bias),
            lambda ei, w, x, bias: full_fn(ei_d, (w_d if w is not None else None), x, bias))


def test_graph_has_the_shapes_the_cases_need(eng, data, dev_data, dev):
    rc.check_graph(eng, data[0])
    rc.check_restricted_plans(eng, dev_data[0], dev_data[1], dev)


@pytest.mark.parametrize("weighted", [True, False], ids=["weight", "no-weight"])
@pytest.mark.parametrize("rows_name", rc.ROW_LISTS)
@pytest.mark.parametrize("K", rc.WIDTHS)
def test_equals_full_aggregate_indexed(routes, data, dev_data, dev, oracle, K, rows_name, weighted):
    ei, w = data
    got = {name: rc.check_values(_on(dev_data, r), ei, w, dev, oracle, K, rows_name, weighted) for name, r in routes.items()}
    assert all(torch.equal(a, b) for a, b in zip(got["ctypes"], got["cpp"])), "ctypes and C++ routes differ"


@pytest.mark.parametrize("route", ["ctypes", "cpp"])
def test_bad_arguments_raise(routes, data, dev, route):
    rc.check_errors(routes[route][0], *data, dev)


def test_second_call_builds_nothing(eng, ops, routes, data, dev):
    rc.check_cache(routes["ctypes"][0], lambda: eng.stats["plans_built"], *data, dev)
    rc.check_cache(routes["cpp"][0], lambda: ops.plan_stats()[0], *data, dev)


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "hipgraph"])
def test_training_step_equals_full_row_path(eng, dev_data, dev, graphed, monkeypatch):
    from gammagl_amd import dist as D

    ei, w = dev_data
    pg = D.PartitionedGraph(ei, w + 0.35, rc.N, 0, 1, eng=eng)
    assert not pg.comm
    if not graphed:
        def make(f_in, n_cls):
            return D.DistGCNTrainer(pg, f_in, 16, n_cls, num_layers=3, drop_rate=0.5, seed=7, device=dev)

        rc.check_step(make, lambda: eng.reseed(123), D, monkeypatch, dev)
        return
    g = torch.Generator().manual_seed(3)
    x = torch.randn(rc.N, 12, generator=g).to(dev)
    y = torch.randint(0, 10, (rc.N,), generator=g).to(dev)
    train = rc.random8().to(dev)
    out = {}
    for on in (True, False):
        monkeypatch.setattr(D, "OUT_ROWS", on)
        eng.reseed(123)
        tr = D.DistGCNTrainer(pg, 12, 16, 10, num_layers=3, drop_rate=0.5, seed=7, device=dev, capturable=True)
        tr.capture(x, y, train, int(train.numel()), warmup=3)
        losses = [tr.replay().clone() for _ in range(3)]
        torch.cuda.synchronize()
        assert tr.net.agg_per_step == 6
        out[on] = (losses, [p.detach().clone() for p in tr.net.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(out[True][0], out[False][0])), (out[True][0], out[False][0])
    assert float(out[True][0][0]) != float(out[True][0][-1])
    assert all(torch.equal(a, b) for a, b in zip(out[True][1], out[False][1]))
