#!/usr/bin/env python3
"""Edge softmax: the native op (torch.ops.ggl.segment_softmax -> ggl_segment_softmax_fwd / _bwd) against the composition
it replaces (gammagl_amd.layers.segment_softmax: segment_max -> gather -> sub / exp -> segment_sum -> gather -> add / div
under autograd), on the destination ids of the Reddit-sized graph (K = 8, 1) and the products-sized graph (K = 1, 4, 8).

ONE process, warm-up, device-event timing, the two routes ALTERNATING repetition by repetition (same clocks, same cache
state), forward and forward + backward.  Bytes are counted from shapes: 2*E*K*4 + 4E per pass (x in, y out, perm) — one
pass forward, two for forward + backward counted as 2 * (...) + E*K*4 (g is read as well).  Also prints the distance
between the GPU and the host library on the same input (different exp implementations, same formulas).

    python tools/segment_softmax_bench.py [--reps 20] [--out profiles/segment_softmax.txt] [--sublanes S] [--sweep] [--small]
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import gammagl_amd  # noqa: E402
from gammagl_amd import cpp_ops, layers  # noqa: E402
from gammagl_amd.synth import DATASETS, rmat_graph  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "segment_softmax.txt"))
ap.add_argument("--sublanes", type=int, default=0, help="ggl_set_option softmax_sublanes (0 = the library's policy)")
ap.add_argument("--sweep", action="store_true", help="also time the op alone with 1, 4, 16, 64 lanes per (row, column)")
ap.add_argument("--small", action="store_true", help="every 8th edge (a quick look, not the figures of record)")
args = ap.parse_args()

dev = torch.device("cuda", 0)
eng = gammagl_amd.engine()
op = cpp_ops.load().segment_softmax
if args.sublanes:
    eng.set_option("softmax_sublanes", args.sublanes)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def alternate(fns, reps):
    """ms per call of each fn, the fns taking turns inside one loop"""
    for f in fns:
        for _ in range(3):
            f()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for _ in fns]
    for r in range(reps):
        for i, f in enumerate(fns):
            ev[i][r][0].record()
            f()
            ev[i][r][1].record()
    torch.cuda.synchronize()
    out = []
    for i in range(len(fns)):
        t = sorted(a.elapsed_time(b) for a, b in ev[i])
        out.append((t[len(t) // 2], t[0], t[-1]))
    return out


arch = torch.cuda.get_device_properties(dev).gcnArchName
say(f"# tools/segment_softmax_bench.py on {arch}: median (min .. max) ms over {args.reps} alternating repetitions")
say("# bytes from shapes: forward 2*E*K*4 + 4E; forward + backward 5*E*K*4 + 8E")
for name, widths in (("reddit", (8, 1)), ("products", (1, 4, 8))):
    n, e, _, _ = DATASETS[name]
    if args.small:
        e //= 8
    ids = rmat_graph(n, e, seed=0, device=dev)[1].contiguous()
    E = int(ids.shape[0])
    plan = eng.seg_plan(ids, n)
    say(f"\n## {name}-sized destination ids: N = {n}, E = {E}, mean row {E / n:.0f}, longest {plan.max_len}, chunk {plan.chunk}, "
        f"{plan.n_long} long rows in {plan.n_chunks} chunks")
    for K in widths:
        g = torch.Generator(device=dev).manual_seed(K)
        x = (torch.randn(E, K, generator=g, device=dev) * 3).requires_grad_(True)
        go = torch.randn(E, K, generator=g, device=dev)
        xd = x.detach()

        def fb(f):
            def run():
                x.grad = None
                f(x, ids, n).backward(go)
            return run

        with torch.no_grad():
            fwd = alternate([lambda: layers.segment_softmax(xd, ids, n), lambda: op(xd, ids, n)], args.reps)
        both = alternate([fb(layers.segment_softmax), fb(op)], args.reps)
        bf, bb = 2 * E * K * 4 + 4 * E, 5 * E * K * 4 + 8 * E
        S = int(eng.lib.ggl_policy_softmax_sublanes(K, E, n))
        for what, (c, o), nb in (("forward", fwd, bf), ("forward + backward", both, bb)):
            say(f"K = {K}  ({S} lanes)  {what:18s}: composition {c[0]:8.2f} ({c[1]:.2f} .. {c[2]:.2f}) ms   op {o[0]:8.2f} ({o[1]:.2f} .. {o[2]:.2f}) ms "
                f"= {nb / o[0] / 1e9:5.2f} TB/s of {nb / 2**30:.2f} GiB   speed-up {c[0] / o[0]:5.2f}x")
        if args.sweep:   # the policy's choice against fixed lane counts, op alone
            for S in (1, 4, 16, 64):
                if S * K > 64:
                    continue
                eng.set_option("softmax_sublanes", S)
                with torch.no_grad():
                    (f,) = alternate([lambda: op(xd, ids, n)], 5)
                (b,) = alternate([fb(op)], 5)
                say(f"K = {K}  sweep: {S:2d} lanes per (row, column): forward {f[0]:7.2f} ms   forward + backward {b[0]:7.2f} ms")
            eng.set_option("softmax_sublanes", args.sublanes)
        del x, go, xd
    del ids, plan
    eng.clear_caches()
    torch.ops.ggl.clear_caches()
    torch.cuda.empty_cache()

# GPU against the host library on one input (test_gpu_softmax.py asserts each is within 1e-5 of float64)
import softmax_cases as sc  # noqa: E402

N, E, K = 20_000, 1_000_000, 8
g = torch.Generator(device=dev).manual_seed(23)
ids = sc.make_ids("power", N, E, g, dev)
x = torch.randn(E, K, generator=g, device=dev) * 3
go = torch.randn(E, K, generator=g, device=dev)
truth = sc.truth_f64(x, ids, N, go)
fl = float(truth[1].abs().mean())
yg, gg = sc.run(op, x, ids, N, go)
yh, gh = sc.run(gammagl_amd.host_engine().segment_softmax, x.cpu(), ids.cpu(), N, go.cpu())
tc = tuple(t.cpu() for t in truth)
say(f"\n## GPU and host library on one input (power-law ids, N = {N}, E = {E}, K = {K}, logits randn x 3), forward / gradient")
say(f"GPU vs float64          : {sc.seg_err(yg, truth[0], ids, N):.2e} / {sc.seg_err(gg, truth[1], ids, N, floor_min=fl):.2e}")
say(f"host library vs float64 : {sc.seg_err(yh, tc[0], ids.cpu(), N):.2e} / {sc.seg_err(gh, tc[1], ids.cpu(), N, floor_min=fl):.2e}")
say(f"GPU vs host library     : {sc.seg_err(yg.cpu(), yh.double(), ids.cpu(), N):.2e} / "
    f"{sc.seg_err(gg.cpu(), gh.double(), ids.cpu(), N, floor_min=fl):.2e}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
