"""Cases shared by tests/test_lin_epi_bwd_host.py (host + emulation libraries, CPU tensors) and tests/test_gpu_lin_epi_bwd.py
(MI355X): ggl_linear_bias_act_bwd — the backward of dropout(relu(. + bias)) on a gradient that is the narrow product
g[N, J] . w[J, K], formed in registers — and the bits of ggl_colsum_f32.

Shapes: N = 1 (less than one group of rows), 67 (a ragged unroll tail), 4099 (several blocks, a ragged last one); (J, K) =
(1, 4) one lane a row, (7, 64) sixteen rows a wavefront, (47 / 48 / 64, 256) a wavefront a row (the benchmark's width; 64
fills the LDS budget), (47, 260) rows of 65 lanes that straddle wavefronts; J = 47 also in rows of 48 floats (the
benchmark's padded gradient)."""
import ctypes

import numpy as np
import torch

from oracle import parity

NS = (1, 67, 4099)
SHAPES = ((1, 4, 1), (7, 64, 7), (47, 256, 47), (47, 256, 48), (48, 256, 48), (64, 256, 64), (47, 260, 47))   # (J, K, g_ld)
P_DROP = 0.5


def operands(N, J, K, g_ld, dev, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + J + K)
    gr = torch.randn(N, g_ld, generator=g)
    w = torch.randn(J, K, generator=g) * 0.3
    y = torch.randn(N, K, generator=g)
    y[torch.rand(N, K, generator=g) < 0.4] = 0.0      # dropped / clipped; the rest of both signs: y > 0 and y != 0 differ
    return gr.to(dev), w.to(dev), y.to(dev)


def product(eng, g, w, y):
    """s = g[:, :J] @ w as the fused entry forms it: no mask, no scale, no bias"""
    s, gb = eng.linear_epi_bwd(g, w, y, False, 0.0, None, None)
    assert gb is None
    return s


def check_self_consistency(eng, dev, N, J, K, g_ld):
    """fused(g, w, y, mode) == ggl_bias_act_bwd(fused product, y, mode), torch.equal, all mask modes, with and without gbias"""
    g, w, y = operands(N, J, K, g_ld, dev)
    s = product(eng, g, w, y)
    assert s.shape == (N, K) and bool(torch.isfinite(s).all())
    used = torch.tensor([1234567, 3], dtype=torch.int64, device=dev)
    modes = {"none": (False, 0.0, None), "relu": (True, P_DROP, None), "nonzero": (False, P_DROP, None),
             "redrawn": (False, P_DROP, used)}
    for name, (relu, p, ru) in modes.items():
        for bias_shape in (None, (1, K)):
            if name == "none" and bias_shape is None:
                continue     # (that call is `product`)
            ga, gb = eng.linear_epi_bwd(g, w, y, relu, p, ru, bias_shape)
            ra, rb = eng._epi_bwd(s, y, relu, p, ru, bias_shape)
            assert torch.equal(ga, ra), (name, bias_shape, N, J, K)
            assert (gb is None) == (bias_shape is None)
            if gb is not None:
                assert gb.shape == (1, K) and torch.equal(gb, rb), (name, N, J, K)
        if name == "relu":
            assert torch.equal(ga != 0, (y > 0) & (s != 0))
        if name == "nonzero":
            assert torch.equal(ga != 0, (y != 0) & (s != 0))
    return s


def check_against_f64(eng, dev, N, J, K, g_ld):
    """Row-scale relative error of the serial-fma product against float64 <= 2 x that of torch.matmul in f32 at `highest`
    precision on the same inputs: both are J-term sums that differ in order only.  Returns (ours, matmul's)."""
    g, w, y = operands(N, J, K, g_ld, dev, seed=1)
    s = product(eng, g, w, y)
    ref = g[:, :J].double() @ w.double()
    before = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("highest")
    try:
        mm = g[:, :J].contiguous() @ w
    finally:
        torch.set_float32_matmul_precision(before)
    ours = parity.report(s.double(), ref, tol=1.0)["max_rel_err"]
    theirs = parity.report(mm.double(), ref, tol=1.0)["max_rel_err"]
    print(f"lin_epi_bwd vs f64: N={N} J={J} K={K} g_ld={g_ld} fused {ours:.3e} matmul {theirs:.3e}")
    assert ours <= 2 * theirs, (N, J, K, g_ld, ours, theirs)
    return ours, theirs


def check_bad_arguments(eng, dev):
    lib = eng.lib
    pol = lib.ggl_policy_linear_epi_bwd
    assert pol(1000, 47, 256) == 1 and pol(1000, 48, 256) == 1 and pol(1000, 64, 256) == 1 and pol(1, 1, 4) == 1
    assert pol(1000, 47, 258) == 0 and pol(1000, 47, 47) == 0            # K % 4 != 0
    assert pol(1000, 65, 64) == 0 and pol(1000, 0, 64) == 0              # J out of 1 .. 64
    assert pol(1000, 64, 260) == 0 and pol(1000, 33, 512) == 0           # J * K * 4 over 64 KiB
    assert pol(1000, 32, 512) == 1
    N, J, K = 9, 5, 8
    g, w, y = operands(N, J, K, J, dev)
    ga, gb = torch.empty_like(y), torch.empty(K, device=dev)
    wsb = lib.ggl_bias_act_bwd_workspace_bytes(N, K)
    ws = torch.empty(max(wsb, 4), dtype=torch.uint8, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    st = eng._stream(dev)

    def call(g_=g, ld=J, w_=w, y_=y, n=N, j=J, k=K, ga_=ga, gb_=gb, ws_=ws, wsb_=wsb, relu=1):
        return lib.ggl_linear_bias_act_bwd(P(g_), ld, P(w_), P(y_), n, j, k, relu, 0.0, None, P(ga_), P(gb_), P(ws_), wsb_, st)

    EINVAL, EWORKSPACE = -1, -5
    assert call() == 0, lib.ggl_last_error()
    for kw in (dict(g_=None), dict(w_=None), dict(ga_=None)):
        assert call(**kw) == EINVAL and lib.ggl_last_error() == b"NULL pointer", kw
    assert call(y_=None) == EINVAL and lib.ggl_last_error() == b"y is needed to rebuild the ReLU/dropout mask"
    for kw in (dict(n=-1), dict(j=-1), dict(k=-4), dict(ld=J - 1)):
        assert call(**kw) == EINVAL and lib.ggl_last_error() == b"bad arguments", kw
    for kw in (dict(ws_=None), dict(wsb_=wsb - 1)):
        assert call(**kw) == EWORKSPACE and lib.ggl_last_error().startswith(b"linear_bias_act_bwd workspace too small"), kw
    assert call(gb_=None, ws_=None, wsb_=0) == 0            # no bias gradient: no workspace
    assert call(k=6) == EINVAL and lib.ggl_last_error().startswith(b"linear_bias_act_bwd needs K % 4 == 0")
    assert call(j=65, ld=65) == EINVAL and lib.ggl_last_error().startswith(b"linear_bias_act_bwd needs K % 4 == 0")
    assert call(g_=g.reshape(-1)[1:]) == EINVAL and lib.ggl_last_error() == b"g, w, y and ga must be 16-byte aligned"


# ---- ggl_colsum_f32: the documented geometry restated in numpy float32 -------------------------------------------------------
COLSUM_NS = (1, 63, 64, 65, 4096, 16384, 70001)
COLSUM_KS = (1, 47, 256)


def _chains(rows):
    """[R, K] float32 rows added as the kernels add them: four chains over steps of four rows, the tail into chain 0, then
    (a0 + a1) + (a2 + a3)"""
    R, K = rows.shape
    a = np.zeros((4, K), dtype=np.float32)
    full = R // 4 * 4
    for r in range(0, full, 4):
        a += rows[r:r + 4]
    for r in range(full, R):
        a[0] += rows[r]
    return (a[0] + a[1]) + (a[2] + a[3])


def colsum_reference(x):
    """stage 1: block b owns rows [b * R, (b + 1) * R), group j of G = 256 // min(K, 256) walks rows b * R + j, + G, ...;
    more than 64 partial rows that are at most a quarter of the input are reduced the same way again; stage 2 walks the rest"""
    N, K = x.shape
    kp = min(max(K, 1), 256)
    G = 256 // kp
    blocks = min(max(-(-max(N, 1) // (G * 64)), 1), 512)
    rpb = -(-max(N, 1) // blocks)
    part = np.zeros((blocks * G, K), dtype=np.float32)
    for b in range(blocks):
        r0, r1 = b * rpb, min((b + 1) * rpb, N)
        for j in range(G):
            part[b * G + j] = _chains(x[r0 + j:r1:G]) if r0 + j < r1 else 0.0
    P = blocks * G
    if P > 64 and P * 4 <= N:
        return colsum_reference(part)
    return _chains(part)


def check_colsum(eng, dev, N, K):
    g = torch.Generator().manual_seed(N + K)
    x = torch.randn(N, K, generator=g) * torch.rand(N, 1, generator=g) * 100.0
    got = eng.colsum(x.to(dev)).cpu().numpy()
    want = colsum_reference(x.numpy())
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32)), (N, K)


# ---- the training step: fused on / off, both routes, and a float64 run of the model ------------------------------------------
DIMS = (12, 16, 10)      # features, hidden, classes (10 classes: 12 columns inside the last GEMM, as 47 -> 48)


def _step_data(rc, dev):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(rc.N, DIMS[0], generator=g)
    y = torch.randint(0, DIMS[2], (rc.N,), generator=g)
    return x.to(dev), y.to(dev), rc.random8().to(dev)


def run_f32(D, pg, eng, dev, rc, monkeypatch, fused, route, steps=3):
    """(loss of every step, parameters after `steps`, times the fused node ran) of a fresh trainer on `route`"""
    monkeypatch.setattr(D, "LIN_EPI_BWD", fused)
    monkeypatch.setattr(pg, "route", route)
    eng.reseed(123)
    tr = D.DistGCNTrainer(pg, DIMS[0], DIMS[1], DIMS[2], num_layers=3, drop_rate=P_DROP, seed=7, device=dev)
    seen, inner = [], D._AggregateThenLinear.apply

    def spy(*a):
        seen.append(1)
        return inner(*a)

    monkeypatch.setattr(D._AggregateThenLinear, "apply", spy)
    x, y, train = _step_data(rc, dev)
    losses = [tr.step(x, y, train, int(train.numel())).clone() for _ in range(steps)]
    monkeypatch.setattr(D._AggregateThenLinear, "apply", inner)
    assert tr.net.agg_per_step == 6
    assert len(seen) == (steps if fused else 0)
    return losses, [p.detach().clone() for p in tr.net.parameters()]


def run_f64(D, pg, eng, dev, rc, ei, w, steps=3):
    """The same model in float64 on a dense adjacency, with the dropout masks the f32 run draws: the engine's own draws on a
    matrix of ones, taken in the trainer's order from the same state (ctypes route: the engine's counter stream)."""
    eng.reseed(123)
    tr = D.DistGCNTrainer(pg, DIMS[0], DIMS[1], DIMS[2], num_layers=3, drop_rate=P_DROP, seed=7, device=dev)
    A = torch.zeros(rc.N, rc.N, dtype=torch.float64)
    A.index_put_((ei[1].cpu(), ei[0].cpu()), w.cpu().double(), accumulate=True)
    A = A.to(dev)
    Ws = [torch.nn.Parameter(lin.weight.detach().double().clone()) for lin in tr.net.lin]
    bs = [torch.nn.Parameter(b.detach().double().clone()) for b in tr.net.bias]
    opt = torch.optim.Adam(Ws + bs, lr=0.01, weight_decay=5e-4)
    x, y, train = _step_data(rc, dev)
    ones = torch.ones(rc.N, DIMS[1], device=dev)
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        h = x.double()
        for i in range(3):
            h = A @ (h @ Ws[i].t()) + bs[i]
            if i < 2:
                keep = eng.bias_act(ones, None, relu=False, p_drop=P_DROP, training=True).double()   # 0 or 1 / (1 - p)
                h = torch.relu(h) * keep
        loss = torch.nn.functional.cross_entropy(h[train], y[train], reduction="sum") / int(train.numel())
        loss.backward()
        opt.step()
    return [p.detach() for p in Ws + bs]


def check_model(D, eng, dev, rc, monkeypatch, routes):
    """Loss of step 1 bit-equal fused on / off; parameters after 3 steps within 2 x the two-launch form's row-scale error
    against the float64 model; the routes equal on the bits with the fused node."""
    ei, w = rc.graph()
    ei, w = ei.to(dev), (w + 0.35).to(dev)
    pg = D.PartitionedGraph(ei, w, rc.N, 0, 1, eng=eng)
    assert not pg.comm
    on = {r: run_f32(D, pg, eng, dev, rc, monkeypatch, True, r) for r in routes}
    off = run_f32(D, pg, eng, dev, rc, monkeypatch, False, "ctypes")
    first = on[routes[0]]
    assert torch.equal(first[0][0], off[0][0]), (first[0], off[0])
    assert float(first[0][0]) != float(first[0][-1])
    for r in routes[1:]:
        assert all(torch.equal(a, b) for a, b in zip(on[r][0], first[0])), "losses differ between the routes"
        assert all(torch.equal(a, b) for a, b in zip(on[r][1], first[1])), "parameters differ between the routes"
    monkeypatch.setattr(pg, "route", "ctypes")
    truth = run_f64(D, pg, eng, dev, rc, ei, w)
    names = [f"W{i + 1}" for i in range(3)] + [f"b{i + 1}" for i in range(3)]
    err = {}
    for tag, run in (("fused", on["ctypes"]), ("two launches", off)):
        got = run[1]        # (the trainer's parameter order: the three weights, then the three biases)
        err[tag] = max(parity.report(a.double(), t, tol=1.0)["max_rel_err"] for a, t in zip(got, truth))
        print(f"lin_epi_bwd model, parameters after 3 steps vs float64 ({tag}): "
              + ", ".join(f"{n} {parity.report(a.double(), t, tol=1.0)['max_rel_err']:.3e}" for n, a, t in zip(names, got, truth)))
    assert err["fused"] <= 2 * err["two launches"], err
    return err
