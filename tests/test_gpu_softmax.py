"""-m gpu: the edge-softmax op (ggl_segment_softmax_fwd / _bwd) on the MI355X, through ``torch.ops.ggl.segment_softmax``
(the route the drop-ins bind) and the ctypes engine: the host suite's cases on cuda tensors (tests/softmax_cases.py),
the Reddit-sized id vector against float64 and the reference's own compiled ops, run-to-run bits, hipGraph capture of
forward + backward, the host library on the same input, and a 3 M-element hub row."""
import time

import pytest
import torch

import softmax_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; the HIP path has no fallback")
    from gammagl_amd import engine

    return engine()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def routes(eng):
    from gammagl_amd import cpp_ops

    return {"torch.ops.ggl": cpp_ops.load().segment_softmax, "engine": eng.segment_softmax}


def test_reference_made_fixture_gpu(routes, dev, golden):
    sc.check_kat(routes, dev, golden)


def test_forward_and_gradient_within_1e5_of_float64_gpu(eng, routes, dev):
    def explicit_plan(x, ids, N):
        plan = eng.build_plan(ids, N, chunk=256)
        assert plan.n_long > 0
        return eng.segment_softmax(x, plan)

    sc.check_vs_float64(routes, dev, plan_route=explicit_plan)
    sc.check_peaked(routes, dev)


def test_winner_invariants_and_edge_cases_gpu(eng, routes, dev):
    sc.check_winner_and_invariants(routes, eng, dev)
    sc.check_edge_cases(routes, dev)


def test_hosts_agree_and_public_function_gpu(routes, dev):
    sc.check_routes_agree(routes, dev)
    sc.check_public_function(dev, routes["torch.ops.ggl"])
    g = torch.Generator(device=dev).manual_seed(3)
    ids = torch.randint(0, 11, (60,), generator=g, device=dev)
    x = torch.randn(60, 5, generator=g, device=dev)
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    from gammagl_amd import torch_ops

    for op in (routes["torch.ops.ggl"], torch_ops.ops.segment_softmax):
        torch.library.opcheck(op.default, (x.clone().requires_grad_(True), ids, 11), test_utils=utils)


def _reddit_ids(dev):
    from gammagl_amd.synth import DATASETS, rmat_graph

    n, e, _, _ = DATASETS["reddit"]
    if torch.cuda.get_device_properties(dev).total_memory < 100 * 2**30:
        e //= 8
    return rmat_graph(n, e, seed=0, device=dev)[1, ::32].contiguous(), n


def _ref_composition(ref):
    def f(x, ids, n):   # utils/softmax.py:29-35 on the reference's compiled CPU ops
        m = ref.c_segment_max(x, ids, n)
        ex = torch.exp(x - m[ids])
        return ex / (ref.c_segment_sum(ex, ids, n)[ids] + 1e-16)
    return f


@pytest.mark.parametrize("K", [8, 1])
def test_reddit_size_ids_vs_float64(routes, dev, K):
    """Destination ids of every 32nd edge of the Reddit-sized graph (3.6 M elements, hub rows of thousands), logits
    randn x 3: forward and gradient <= 1e-5 of float64 evaluated on the GPU.  The reference composition's own distance
    (its compiled c_segment_max / c_segment_sum, f32 on the CPU) is printed beside it where oracle/_ref is built."""
    from oracle import oracle as orc

    ids, n = _reddit_ids(dev)
    E = int(ids.shape[0])
    g = torch.Generator(device=dev).manual_seed(40 + K)
    x = torch.randn((E, K) if K > 1 else (E,), generator=g, device=dev) * 3
    go = torch.randn(x.shape, generator=g, device=dev)
    truth = sc.truth_f64(x, ids, n, go)
    for name, route in routes.items():
        ef, eg = sc.errors(route, x, ids, n, go, truth)
        print(f"segment_softmax Reddit-sized/32 E={E} K={K} [{name}]: forward {ef:.2e} gradient {eg:.2e}")
        assert ef <= sc.TOL and eg <= sc.TOL, (name, ef, eg)
    ref = orc.load_ref_ext()
    if ref is not None:
        torch.set_num_threads(1)
        tc = tuple(t.cpu() for t in truth)
        er = sc.errors(_ref_composition(ref), x.cpu(), ids.cpu(), n, go.cpu(), tc)
        print(f"   reference composition (compiled c_segment_max / c_segment_sum, f32): forward {er[0]:.2e} gradient {er[1]:.2e}")


def test_uniform_ids_vs_the_reference_ops(routes, dev):
    """f32 against f32 where the reference itself is inside the bar: uniform ids (E = 1 M, N = 50 000, K = 8, logits
    randn).  First the reference composition's own distance to float64 is asserted <= 1e-5 (a pass cannot come from a
    loose yardstick); then forward <= 1e-5 and gradient <= 2e-5 (floor = mean |reference gradient|), the two bars
    tests/test_gpu_refsize.py holds the fused GAT op to against the same reference ops."""
    from oracle import oracle as orc
    from oracle import parity

    ref = orc.load_ref_ext()
    if ref is None:
        pytest.fail("oracle/_ref/_torch_ext.so is missing: build it with `make -C oracle ref`")
    torch.set_num_threads(1)
    N, E, K = 50_000, 1_000_000, 8
    g = torch.Generator(device=dev).manual_seed(17)
    ids = torch.randint(0, N, (E,), generator=g, device=dev)
    x = torch.randn(E, K, generator=g, device=dev)
    go = torch.randn(E, K, generator=g, device=dev)
    truth = tuple(t.cpu() for t in sc.truth_f64(x, ids, N, go))
    ids_c = ids.cpu()
    ry, rg = sc.run(_ref_composition(ref), x.cpu(), ids_c, N, go.cpu())
    rf = sc.seg_err(ry, truth[0], ids_c, N)
    rb = sc.seg_err(rg, truth[1], ids_c, N, floor_min=float(truth[1].abs().mean()))
    print(f"reference composition vs float64 (uniform, E={E}, K={K}): forward {rf:.2e} gradient {rb:.2e}")
    assert rf <= 1e-5 and rb <= 1e-5, (rf, rb)
    for name, route in routes.items():
        y, gx = sc.run(route, x, ids, N, go)
        ef = sc.seg_err(y.cpu(), ry.double(), ids_c, N)
        eg = sc.seg_err(gx.cpu(), rg.double(), ids_c, N, floor_min=float(rg.abs().mean()))
        print(f"segment_softmax vs the reference ops [{name}]: forward {ef:.2e} gradient {eg:.2e}")
        assert ef <= 1e-5 and eg <= 2e-5, (name, ef, eg)
    assert parity.TOL == 1e-5


def test_deterministic_capturable_and_close_to_the_host_library(eng, routes, dev):
    """Two calls give the same bits; forward + backward capture into one hipGraph (plan built before the capture) and
    replay with the eager call's bits; the GPU result and the host library's result on the same input are each within
    1e-5 of float64 (their mutual distance — different exp implementations, same formulas — is printed, not asserted)."""
    import gammagl_amd

    op = routes["torch.ops.ggl"]
    N, E, K = 20_000, 1_000_000, 8
    g = torch.Generator(device=dev).manual_seed(23)
    ids = sc.make_ids("power", N, E, g, dev)
    x = torch.randn(E, K, generator=g, device=dev) * 3
    go = torch.randn(E, K, generator=g, device=dev)
    y1, g1 = sc.run(op, x, ids, N, go)
    y2, g2 = sc.run(op, x, ids, N, go)
    assert torch.equal(y1, y2) and torch.equal(g1, g2)
    ye, ge = sc.run(routes["engine"], x, ids, N, go)
    assert torch.equal(y1, ye) and torch.equal(g1, ge)
    # capture (the plan exists; a third eager call on a side stream warms the allocator as torch.cuda.graph asks)
    xs = x.clone().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        op(xs, ids, N).backward(go)
    torch.cuda.current_stream().wait_stream(s)
    xs.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys = op(xs, ids, N)
        ys.backward(go)
    ys.zero_()
    xs.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(ys.detach(), y1) and torch.equal(xs.grad, g1), "graph replay differs from the eager call"
    # the host library on the same input
    truth = sc.truth_f64(x, ids, N, go)
    yh, gh = sc.run(gammagl_amd.host_engine().segment_softmax, x.cpu(), ids.cpu(), N, go.cpu())
    tc = tuple(t.cpu() for t in truth)
    fl = float(tc[1].abs().mean())
    e_gpu = (sc.seg_err(y1, truth[0], ids, N), sc.seg_err(g1, truth[1], ids, N, floor_min=fl))
    e_host = (sc.seg_err(yh, tc[0], ids.cpu(), N), sc.seg_err(gh, tc[1], ids.cpu(), N, floor_min=fl))
    mutual = (sc.seg_err(y1.cpu(), yh.double(), ids.cpu(), N), sc.seg_err(g1.cpu(), gh.double(), ids.cpu(), N, floor_min=fl))
    print(f"segment_softmax vs float64: GPU {e_gpu[0]:.2e} / {e_gpu[1]:.2e}, host library {e_host[0]:.2e} / {e_host[1]:.2e}; "
          f"GPU vs host library {mutual[0]:.2e} / {mutual[1]:.2e} (forward / gradient)")
    assert max(e_gpu) <= sc.TOL and max(e_host) <= sc.TOL, (e_gpu, e_host)


def test_hub_row_of_three_million_elements(routes, dev):
    """One row of 3 M elements (ids shuffled) among 10^5 rows that share 1 M more, K = 8, logits randn x 3: forward and
    gradient <= 1e-5 of float64; the time is printed (a star centre has to be correct, not fast)."""
    N, K = 100_000, 8
    g = torch.Generator(device=dev).manual_seed(31)
    ids = torch.cat((torch.full((3_000_000,), 777, dtype=torch.int64, device=dev),
                     torch.randint(0, N, (1_000_000,), generator=g, device=dev)))
    ids = ids[torch.randperm(ids.shape[0], generator=g, device=dev)].contiguous()
    E = int(ids.shape[0])
    x = torch.randn(E, K, generator=g, device=dev) * 3
    go = torch.randn(E, K, generator=g, device=dev)
    truth = sc.truth_f64(x, ids, N, go)
    for name, route in routes.items():
        sc.run(route, x, ids, N, go)            # plan + allocator warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y, gx = sc.run(route, x, ids, N, go)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        ef = sc.seg_err(y, truth[0], ids, N)
        eg = sc.seg_err(gx, truth[1], ids, N, floor_min=float(truth[1].abs().mean()))
        print(f"segment_softmax hub row 3 M of E={E} K={K} [{name}]: forward {ef:.2e} gradient {eg:.2e}, "
              f"forward + backward {ms:.2f} ms")
        assert ef <= sc.TOL and eg <= sc.TOL, (name, ef, eg)


def test_every_lane_count_of_the_walks(eng, routes, dev):
    """Option softmax_sublanes (A/B): 1 ... 64 lanes per (row, column), K = 1 and 4, short and chunked rows — each within
    1e-5 of float64, rows summing to one, the winner the segment maximum; the policy's own choice is what every other test
    runs."""
    old = eng.lib.ggl_get_option(b"softmax_sublanes")
    try:
        for S in (1, 2, 4, 8, 16, 32, 64):
            eng.set_option("softmax_sublanes", S)
            for K in (1, 4):
                assert eng.lib.ggl_policy_softmax_sublanes(K, 1, 1) == min(S, 64 // K)
            out = sc.check_vs_float64({"engine": routes["engine"]}, dev, kinds=("power",), widths=(1, 4), N=500, E=60_000,
                                      log=lambda *_: None)
            print(f"softmax_sublanes = {S}: " + ", ".join(f"K={k} {ef:.1e}/{eg:.1e}" for _, k, _, ef, eg, _ in out))
            sc.check_winner_and_invariants({"engine": routes["engine"]}, eng, dev, N=500, E=60_000, K=4, kinds=("power",))
    finally:
        eng.set_option("softmax_sublanes", old)
