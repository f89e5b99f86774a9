"""spmm_rows — the aggregate restricted to a sorted list of destination rows (ggl_plan_rows_*, ggl_bias_grad_rows) — on
CPU tensors: the HOST library through both routes (ctypes Engine.spmm_rows, torch.ops.ggl.spmm_rows) and the emulation
build through the ctypes engine.  Everything is compared under torch.equal against the full aggregate indexed by the rows
(and fed the scattered gradient) and against the oracle.  Cases: tests/spmm_rows_cases.py."""
import os
import subprocess

import pytest
import torch

import spmm_rows_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DEV = torch.device("cpu")


@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "gammagl_amd", "csrc"), "host", "torch"])
    import gammagl_amd

    return gammagl_amd.host_engine()


@pytest.fixture(scope="module")
def emul():
    subprocess.check_call([os.path.join(HERE, "emul", "build.sh")])
    from gammagl_amd import _lib
    from gammagl_amd.ops import Engine

    return Engine(_lib.bind(os.path.join(HERE, "emul", "libggl_emul.so")), require_cuda=False)


@pytest.fixture(scope="module")
def data():
    return rc.graph()


def _engine_route(eng):
    def rows_fn(ei, w, x, rows, bias):
        return eng.spmm_rows(eng.graph_plan(ei, rc.N), w, x, rows, bias)

    def full_fn(ei, w, x, bias):
        return eng.spmm_epi(eng.graph_plan(ei, rc.N), w, x, bias=bias)

    return rows_fn, full_fn


def _cpp_route():
    from gammagl_amd import cpp_ops

    ops = cpp_ops.load()
    return ops.spmm_rows, (lambda ei, w, x, bias: ops.spmm_epi(ei, w, x, False, None, bias, False, 0.0))


@pytest.fixture(scope="module")
def routes(host, emul):
    return {"host-ctypes": _engine_route(host), "host-cpp": _cpp_route(), "emul-ctypes": _engine_route(emul)}


def test_graph_has_the_shapes_the_cases_need(host, emul, data):
    ei, w = data
    rc.check_graph(host, ei)
    for eng in (host, emul):
        rc.check_restricted_plans(eng, ei, w, DEV)


@pytest.mark.parametrize("weighted", [True, False], ids=["weight", "no-weight"])
@pytest.mark.parametrize("rows_name", rc.ROW_LISTS)
@pytest.mark.parametrize("K", rc.WIDTHS)
def test_equals_full_aggregate_indexed(routes, data, oracle, K, rows_name, weighted):
    ei, w = data
    got = {name: rc.check_values(r, ei, w, DEV, oracle, K, rows_name, weighted) for name, r in routes.items()}
    ref = got["host-ctypes"]
    for name, g in got.items():
        assert all(torch.equal(a, b) for a, b in zip(g, ref)), f"{name} differs from host-ctypes"


@pytest.mark.parametrize("route", ["host-ctypes", "host-cpp", "emul-ctypes"])
def test_bad_arguments_raise(routes, data, route):
    rc.check_errors(routes[route][0], *data, DEV)


def test_second_call_builds_nothing(host, emul, routes, data):
    from gammagl_amd import cpp_ops

    ops = cpp_ops.load()
    for eng, name in ((host, "host-ctypes"), (emul, "emul-ctypes")):
        rc.check_cache(routes[name][0], lambda e=eng: e.stats["plans_built"], *data, DEV)
    rc.check_cache(routes["host-cpp"][0], lambda: ops.plan_stats()[0], *data, DEV)


@pytest.mark.parametrize("which", ["host", "emul"])
def test_training_step_equals_full_row_path(host, emul, data, which, monkeypatch):
    """host: the shipped library, i.e. the C++ route of a one-rank step; emul: the ctypes route."""
    from gammagl_amd import dist as D

    eng = host if which == "host" else emul
    ei, w = data
    pg = D.PartitionedGraph(ei, w + 0.35, rc.N, 0, 1, eng=eng)
    assert pg.route == ("cpp" if which == "host" else "ctypes") and not pg.comm

    def make(f_in, n_cls):
        return D.DistGCNTrainer(pg, f_in, 16, n_cls, num_layers=3, drop_rate=0.5, seed=7, device="cpu")

    rc.check_step(make, lambda: eng.reseed(123), D, monkeypatch, DEV)


def test_forward_with_out_rows_indexes_where_it_cannot_restrict(emul, data):
    """aggregate-first association and an unsorted list: every row is computed and indexed afterwards, same values."""
    from gammagl_amd import dist as D

    ei, w = data
    pg = D.PartitionedGraph(ei, w + 0.35, rc.N, 0, 1, eng=emul)
    x = torch.randn(rc.N, 12, generator=torch.Generator().manual_seed(1))
    rows = rc.random8()
    for af in (False, True):
        torch.manual_seed(0)
        net = D.DistGCN(12, 16, 10, num_layers=3, drop_rate=0.0, aggregate_first=af)
        full = net(x, pg)
        part = net(x, pg, out_rows=rows)
        assert part.shape == (rows.numel(), 10) and part.is_contiguous() and torch.equal(part, full[rows])
    tr = D.DistGCNTrainer(pg, 12, 16, 7, num_layers=3, drop_rate=0.0, seed=7, device="cpu")
    assert tr._out_rows(rows) is rows and tr._out_rows(rows.flip(0)) is None and tr._out_rows(rows.to(torch.int32)) is None
    y = torch.randint(0, 7, (rc.N,))
    assert torch.isfinite(tr.step(x, y, rows.flip(0), int(rows.numel())))   # an unsorted train list keeps working


def test_dispatcher_contracts(host, data):
    """schema, fake-tensor (Meta) and autograd registrations of torch.ops.ggl.spmm_rows and the two ops behind it"""
    from gammagl_amd import cpp_ops

    ops = cpp_ops.load()
    ei, w = data
    rows = rc.random8()
    g = torch.Generator().manual_seed(4)
    x, b = torch.randn(rc.N, 8, generator=g), torch.randn(1, 8, generator=g)
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    torch.library.opcheck(ops.spmm_rows.default, (ei, w, x, rows, b), test_utils=utils)
    torch.library.opcheck(ops.spmm_rows.default, (ei, None, x.clone().requires_grad_(True), rows, b.clone().requires_grad_(True)),
                          test_utils=utils)
    torch.library.opcheck(ops.spmm_rows_forward.default, (ei, w, x, rows, b), test_utils=utils[:2])
    go = torch.randn(rows.numel(), 8, generator=g)
    torch.library.opcheck(ops.spmm_rows_backward.default, (ei, w, go, rows, rc.N, True), test_utils=utils[:2])
    xr = x.clone().requires_grad_(True)
    assert ops.spmm_rows(ei, w, xr, rows, b).grad_fn is not None
    with torch.no_grad():
        assert ops.spmm_rows(ei, w, xr, rows, b).grad_fn is None
    m = ops.spmm_rows(ei.to("meta"), w.to("meta"), x.to("meta"), rows.to("meta"), b.to("meta"))
    assert m.shape == (rows.numel(), 8) and m.device.type == "meta"
