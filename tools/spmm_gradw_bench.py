#!/usr/bin/env python3
"""gspmm's gradient with respect to its edge weights (ggl_spmm_grad_w) on the Reddit-sized and the products-sized synthetic
graph: what a learnable edge weight costs on the fused route, against the message route it took before.

Per graph, ONE child process each:
  layer   learnable-weight GCNConv (K = 64, norm='none', bias) forward + backward: the layer as it is (weights through
          spmm_bias_act, gw from the edge-dot) against the MESSAGE route the layer took for such a weight before —
          linear -> message() (gather * weight: an [E, K] tensor) -> unsorted_segment_sum -> bias_act, restated here with
          the layer's own methods.  The two ALTERNATE repetition by repetition (same clocks, same cache state), device-event
          timing after a warm-up; peak memory of each from a run of its own.
  layer256  the same layer at K = 256, fused route ONLY: the message route's tensors would be E * 256 * 4 bytes each
          (products-sized: 129 GB) and were not attempted.
  dot     the edge-dot alone (Engine.spmm_grad_w's launch on a ready plan) at K = 64 / 128 / 256 for f32, bf16 and f16 rows
          (x and g in the same storage), beside the constant-weight backward of the same shape (the transposed SpMM-sum that
          makes gx), all four alternating.
The driver starts each child under its own `timeout` and stops at the first that fails.

    python tools/spmm_gradw_bench.py [--reps 7] [--out profiles/spmm_gradw.txt] [--graphs reddit,products]
"""
import argparse
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "spmm_gradw.txt"))
ap.add_argument("--graphs", default="reddit,products")
ap.add_argument("--small", action="store_true", help="every 8th edge (a quick look, not the figures of record)")
ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
ap.add_argument("--child", default="", help="(internal) layer:<graph>, layer256:<graph> or dot:<graph>")
args = ap.parse_args()


def commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def driver():
    import torch

    arch = torch.cuda.get_device_properties(0).gcnArchName if torch.cuda.is_available() else "no GPU"
    lines = [f"# tools/spmm_gradw_bench.py on {arch}, commit {commit()} (+ working tree)",
             f"# median (min .. max) ms over {args.reps} alternating repetitions"]
    graphs = [g for g in args.graphs.split(",") if g]
    jobs = [f"{kind}:{g}" for g in graphs for kind in ("layer", "dot")] + [f"layer256:{g}" for g in graphs if g == "products"]
    rc = 0
    for job in jobs:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", job,
               "--reps", str(args.reps)] + (["--small"] if args.small else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith(("##", "  ")) or not ln]
        if r.returncode != 0:
            lines.append(f"## {job}: exit status {r.returncode}; nothing after it was run")
            sys.stderr.write(r.stderr[-3000:])
            rc = r.returncode
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


def alternate(fns, reps):
    """ms per call of each fn, the fns taking turns inside one loop"""
    import torch

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


def fmt(t):
    return f"{t[0]:9.2f} ({t[1]:.2f} .. {t[2]:.2f}) ms"


def graph(name):
    import torch

    import gammagl_amd
    from gammagl_amd.synth import DATASETS, rmat_graph

    dev = torch.device("cuda", 0)
    n, e, _, _ = DATASETS[name]
    if args.small:
        e //= 8
    ei = rmat_graph(n, e, seed=0, device=dev)
    return dev, gammagl_amd.engine(), n, ei


def peak_of(fn, dev):
    import torch

    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - base) / 2**30


def child_layer(name, K, with_message):
    import torch

    from gammagl_amd import layers

    dev, eng, n, ei = graph(name)
    E = int(ei.shape[1])
    gen = torch.Generator(device=dev).manual_seed(K)
    x = torch.randn(n, K, generator=gen, device=dev)
    go = torch.randn(n, K, generator=gen, device=dev)
    torch.manual_seed(0)
    conv = layers.GCNConv(K, K, norm="none").to(dev)
    ew = torch.rand(E, generator=gen, device=dev).requires_grad_(True)
    print(f"\n## {name}-sized graph, learnable-weight GCNConv {K} -> {K}, forward + backward: N = {n}, E = {E}; one [E, K] f32 "
          f"tensor = {E * K * 4 / 2**30:.1f} GiB", flush=True)

    def fused():
        conv.zero_grad()
        ew.grad = None
        conv(x, ei, ew, n).backward(go)

    def message():
        conv.zero_grad()
        ew.grad = None
        h = conv.linear(x)
        out = conv.aggregate(conv.message(h, ei, ew), ei, n, "sum")
        layers._engine(out).bias_act(out, conv.bias, relu=False, p_drop=0.0, training=False).backward(go)

    fns = [("fused route (spmm_bias_act + edge-dot)", fused)]
    if with_message:
        fns.append(("message route ([E, K] messages)", message))
        fused()
        gf = ew.grad.clone()
        message()
        d = (ew.grad - gf).abs().max().item()
        print(f"  max |ew.grad fused - message| = {d:.3e} (max |ew.grad| {gf.abs().max().item():.3e})", flush=True)
    else:
        print(f"  message route not attempted: its message tensor and that tensor's gradient are {E * K * 4 / 1e9:.0f} GB each",
              flush=True)
    t = alternate([f for _, f in fns], args.reps)
    for (label, f), ti in zip(fns, t):
        print(f"  {label:40s} {fmt(ti)}   peak memory over the step {peak_of(f, dev):7.2f} GiB", flush=True)
    if with_message:
        print(f"  message / fused = {t[1][0] / t[0][0]:.1f}x", flush=True)


def child_dot(name):
    import torch

    dev, eng, n, ei = graph(name)
    E = int(ei.shape[1])
    gp = eng.graph_plan(ei, n)
    gp.rowidx, gp.bwd  # noqa: B018  (both sides of the plan exist before anything is timed)
    print(f"\n## {name}-sized graph, the edge-dot alone (gw[e] = sum_k x[src,k] g[dst,k]) beside the constant-weight backward "
          f"(gx: the transposed SpMM-sum, f32): N = {n}, E = {E}", flush=True)
    gen = torch.Generator(device=dev).manual_seed(1)
    w = torch.rand(E, generator=gen, device=dev)
    for K in (64, 128, 256):
        x = torch.randn(n, K, generator=gen, device=dev)
        g = torch.randn(n, K, generator=gen, device=dev)
        cont = [("edge-dot f32", x, g), ("edge-dot bf16", x.bfloat16(), g.bfloat16()), ("edge-dot f16", x.half(), g.half())]
        fns = [lambda xx=xx, gg=gg: eng._spmm_grad_w(gp, xx, gg, False) for _, xx, gg in cont]
        fns.append(lambda: eng._spmm_fwd("sum", gp.bwd, gp.colT, w, g, gp.N_src))
        t = alternate(fns, args.reps)
        for (label, xx, _), ti in zip(cont, t):
            nb = E * (K * xx.element_size() + 12)      # the gathered x strip + col, rowidx, gw (g rows are shared by a row's edges)
            print(f"  K = {K:3d}  {label:14s} {fmt(ti)}   f32 / this = {t[0][0] / ti[0]:.2f}x   {nb / ti[0] / 1e9:5.2f} TB/s algorithmic",
                  flush=True)
        print(f"  K = {K:3d}  {'gx backward f32':14s} {fmt(t[3])}", flush=True)


if __name__ == "__main__":
    if args.child:
        kind, name = args.child.split(":")
        if kind == "layer":
            child_layer(name, 64, True)
        elif kind == "layer256":
            child_layer(name, 256, False)
        else:
            child_dot(name)
    else:
        sys.exit(driver())
