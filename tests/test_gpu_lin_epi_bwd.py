"""ggl_linear_bias_act_bwd and ggl_colsum_f32 on the MI355X: the HIP library through the ctypes engine, the training step also
through torch.ops.ggl and captured into a hipGraph.  Cases: tests/lin_epi_bwd_cases.py."""
import pytest
import torch

import lin_epi_bwd_cases as lc
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


@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "J%d-K%d-ld%d" % s)
@pytest.mark.parametrize("N", lc.NS)
def test_fused_equals_bias_act_bwd_of_its_own_product(eng, dev, N, shape):
    lc.check_self_consistency(eng, dev, N, *shape)


@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "J%d-K%d-ld%d" % s)
@pytest.mark.parametrize("N", lc.NS)
def test_product_against_float64(eng, dev, N, shape):
    lc.check_against_f64(eng, dev, N, *shape)


@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "J%d-K%d-ld%d" % s)
def test_product_equals_the_host_build_on_the_bits(eng, dev, shape):
    """serial fmas in ascending j: the same number on the device and in the host build of the same source"""
    import gammagl_amd

    g, w, y = lc.operands(4099, *shape, torch.device("cpu"))
    want = lc.product(gammagl_amd.host_engine(), g, w, y)
    assert torch.equal(lc.product(eng, g.to(dev), w.to(dev), y.to(dev)).cpu(), want)


def test_bad_arguments(eng, dev):
    lc.check_bad_arguments(eng, dev)


@pytest.mark.parametrize("K", lc.COLSUM_KS)
@pytest.mark.parametrize("N", lc.COLSUM_NS)
def test_colsum_is_the_documented_sum_on_the_bits(eng, dev, N, K):
    lc.check_colsum(eng, dev, N, K)


def test_training_step_fused_on_and_off(eng, dev, monkeypatch):
    from gammagl_amd import dist as D

    lc.check_model(D, eng, dev, rc, monkeypatch, ("ctypes", "cpp"))


def test_fused_training_step_captures_into_a_hipgraph(eng, dev, monkeypatch):
    """the fused node inside one captured step: replays equal the eager steps of the same seed"""
    from gammagl_amd import dist as D

    ei, w = rc.graph()
    pg = D.PartitionedGraph(ei.to(dev), (w + 0.35).to(dev), rc.N, 0, 1, eng=eng)
    monkeypatch.setattr(D, "LIN_EPI_BWD", True)
    x, y, train = lc._step_data(rc, dev)
    eng.reseed(123)
    tr = D.DistGCNTrainer(pg, *lc.DIMS[:2], lc.DIMS[2], num_layers=3, drop_rate=lc.P_DROP, seed=7, device=dev, capturable=True)
    eager = [tr.step(x, y, train, int(train.numel())).clone() for _ in range(5)]
    eng.reseed(123)
    tr = D.DistGCNTrainer(pg, *lc.DIMS[:2], lc.DIMS[2], num_layers=3, drop_rate=lc.P_DROP, seed=7, device=dev, capturable=True)
    tr.capture(x, y, train, int(train.numel()), warmup=3)
    replayed = [tr.replay().clone() for _ in range(2)]
    torch.cuda.synchronize()
    assert tr.net.agg_per_step == 6
    assert all(torch.equal(a, b) for a, b in zip(eager[3:], replayed)), (eager, replayed)
