#!/usr/bin/env python3
"""Edge softmax + aggregate on per-edge logits: the fused op (torch.ops.ggl_attn.edge_softmax_aggregate ->
ggl_edge_softmax_agg_fwd / _bwd_dst / _bwd_src) against the composition it replaces (gammagl_amd.utils.segment_softmax
then gammagl_amd.mpops.bspmm under autograd), on the Reddit-sized and the products-sized graph, H x C in
{1 x 64, 8 x 8, 4 x 24}, forward and forward + backward, with the peak memory of one forward + backward.

ONE process, warm-up, device-event timing, the two routes ALTERNATING repetition by repetition (same clocks, same cache
state), as tools/segment_softmax_bench.py does.  Bytes are counted from shapes: per edge 4 H C (the gathered feature row) +
4 H (its logits) + 4 (col) + 4 (perm), forward; the composition reads and writes [E, H] four more times.  Also prints the
errors against float64 of tests/edge_softmax_agg_cases.py (tensor scale asserted there, row scale reported only).

    python tools/edge_softmax_agg_bench.py [--reps 10] [--out profiles/edge_softmax_agg.txt] [--small] [--only-forward H C]

--only-forward H C: nothing but repeated fused forwards on the Reddit-sized graph (what a kernel trace is taken of).
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import gammagl_amd  # noqa: E402
from gammagl_amd import cpp_ops, mpops  # noqa: E402
from gammagl_amd.synth import DATASETS, rmat_graph  # noqa: E402
from gammagl_amd.utils import segment_softmax  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "edge_softmax_agg.txt"))
ap.add_argument("--small", action="store_true", help="every 8th edge (a quick look, not the figures of record)")
ap.add_argument("--only-forward", type=int, nargs=2, metavar=("H", "C"))
ap.add_argument("--no-accuracy", action="store_true")
args = ap.parse_args()

dev = torch.device("cuda", 0)
eng = gammagl_amd.engine()
fused_op = cpp_ops.load_attn().edge_softmax_aggregate
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def alternate(fns, reps):
    """ms per call of each fn, the fns taking turns inside one loop"""
    for f in fns:
        for _ in range(2):
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


def peak_mib(f):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    f()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - base) / 2**20


def composed(ei, z, x, n):
    return mpops.bspmm(ei, segment_softmax(z, ei[1], n), x, "sum")


def fused(ei, z, x, n):
    return fused_op(ei, z, x, n, 0.0)


if args.only_forward:
    H, C = args.only_forward
    n, e, _, _ = DATASETS["reddit"]
    ei = rmat_graph(n, e // 8 if args.small else e, seed=0, device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    z = torch.randn(ei.shape[1], H, generator=g, device=dev) * 3
    x = torch.randn(n, H, C, generator=g, device=dev)
    with torch.no_grad():
        for _ in range(args.reps):
            fused(ei, z, x, n)
    torch.cuda.synchronize()
    sys.exit(0)

arch = torch.cuda.get_device_properties(dev).gcnArchName
say(f"# tools/edge_softmax_agg_bench.py on {arch}: median (min .. max) ms over {args.reps} alternating repetitions")
say("# composed = utils.segment_softmax + mpops.bspmm under autograd; fused = torch.ops.ggl_attn.edge_softmax_aggregate")
say("# forward bytes from shapes, fused: E * (4 H C + 4 H + 8) + 2 * 4 N H C — ALGORITHMIC bytes: a feature row is counted once per edge "
    "that gathers it and mostly comes from L2 / MALL, so the rate is not an HBM rate; peak = extra MiB allocated during one forward + backward")
for name in ("reddit", "products"):
    n, e, _, _ = DATASETS[name]
    if args.small:
        e //= 8
    ei = rmat_graph(n, e, seed=0, device=dev)
    E = int(ei.shape[1])
    gp = eng.graph_plan(ei, n)
    say(f"\n## {name}-sized graph: N = {n}, E = {E}, mean row {E / n:.0f}, longest {gp.fwd.max_len}, chunk {gp.fwd.chunk}, "
        f"{gp.fwd.n_long} long rows in {gp.fwd.n_chunks} chunks")
    for H, C in ((1, 64), (8, 8), (4, 24)):
        g = torch.Generator(device=dev).manual_seed(H * C)
        z = (torch.randn(E, H, generator=g, device=dev) * 3).requires_grad_(True)
        x = torch.randn(n, H, C, generator=g, device=dev).requires_grad_(True)
        go = torch.randn(n, H, C, generator=g, device=dev)
        zd, xd = z.detach(), x.detach()

        def fb(f):
            def run():
                z.grad = None
                x.grad = None
                f(ei, z, x, n).backward(go)
            return run

        with torch.no_grad():
            fwd = alternate([lambda: composed(ei, zd, xd, n), lambda: fused(ei, zd, xd, n)], args.reps)
        both = alternate([fb(composed), fb(fused)], args.reps)
        pk = [peak_mib(fb(composed)), peak_mib(fb(fused))]
        nb = E * (4 * H * C + 4 * H + 8) + 2 * 4 * n * H * C
        for what, (c, o) in (("forward", fwd), ("forward + backward", both)):
            tail = f" = {nb / o[0] / 1e9:5.2f} TB/s of {nb / 2**30:.2f} GiB" if what == "forward" else ""
            say(f"{H} x {C:2d}  {what:18s}: composed {c[0]:8.2f} ({c[1]:.2f} .. {c[2]:.2f}) ms   fused {o[0]:8.2f} "
                f"({o[1]:.2f} .. {o[2]:.2f}) ms   speed-up {c[0] / o[0]:5.2f}x{tail}")
        say(f"{H} x {C:2d}  peak memory, forward + backward: composed {pk[0]:9.1f} MiB   fused {pk[1]:9.1f} MiB")
        del z, x, go, zd, xd
        torch.cuda.empty_cache()
    del ei, gp
    eng.clear_caches()
    torch.ops.ggl.clear_caches()
    torch.cuda.empty_cache()

if not args.no_accuracy:
    import edge_softmax_agg_cases as ec  # noqa: E402

    say("\n## against float64 (tests/edge_softmax_agg_cases.py check_against_f64: N = 2000, E = 200 000, logits randn x 3); "
        "max|got - truth| / max|truth| per tensor (asserted <= 1e-5 for the fused op), gz also at row scale (not asserted)")
    for ln in ec.check_against_f64(lambda i, zz, xx, nd, p: fused_op(i, zz, xx, nd, p), eng, dev):
        lines.append(ln)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
