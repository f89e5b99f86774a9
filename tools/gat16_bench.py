#!/usr/bin/env python3
"""Fused GAT on rows stored as bf16 / f16 (Engine.gat_fused -> ggl_gat_fused_*_x16: the general kernels, f32 softmax and sums,
one rounding) against the f32 op on the same graph, el and er: the Reddit-sized and the products-sized synthetic graph,
8 x 8 and 8 x 44 heads, forward and forward + backward.

Four contenders: the f32 fast path (gat_fast.hip, where the head shape has one), the f32 general kernels (eng.gat_fast =
False), bf16 and f16.  One (graph, head shape) is ONE child process in which the contenders ALTERNATE repetition by repetition
(same clocks, same cache state), device-event timing after a warm-up; the driver starts each child under its own `timeout` and
stops at the first that fails.  The last child times the 2-layer Reddit GAT training step (gammagl_amd.benchmarks.run_gat) in
f32 and under autocast(bf16), alternating as whole runs.  Algorithmic bytes per edge of the forward walk: H*C*element size
(feature row) + 4 (col) + 4*H (el row).

    python tools/gat16_bench.py [--reps 10] [--out profiles/gat16.txt] [--graphs reddit,products] [--heads 8x8,8x44]
"""
import argparse
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gat16.txt"))
ap.add_argument("--graphs", default="reddit,products")
ap.add_argument("--heads", default="8x8,8x44")
ap.add_argument("--small", action="store_true", help="every 8th edge (a quick look, not the figures of record)")
ap.add_argument("--no-step", action="store_true", help="skip the training step")
ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
ap.add_argument("--child", default="", help="(internal) graph:HxC, or 'step'")
args = ap.parse_args()


def commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def driver():
    import torch

    arch = torch.cuda.get_device_properties(0).gcnArchName if torch.cuda.is_available() else "no GPU"
    lines = [f"# tools/gat16_bench.py on {arch}, commit {commit()} (+ working tree)",
             f"# median (min .. max) ms over {args.reps} alternating repetitions; ratios are against the f32 GENERAL kernels"]
    jobs = [f"{g}:{h}" for g in args.graphs.split(",") if g for h in args.heads.split(",") if h]
    if not args.no_step:
        jobs.append("step")
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


def child_op(job):
    import torch

    import gammagl_amd
    from gammagl_amd.synth import DATASETS, rmat_graph

    name, hc = job.split(":")
    H, C = (int(v) for v in hc.split("x"))
    dev = torch.device("cuda", 0)
    eng = gammagl_amd.engine()
    n, e, _, _ = DATASETS[name]
    if args.small:
        e //= 8
    ei = rmat_graph(n, e, seed=0, device=dev)
    E = int(ei.shape[1])
    gp = eng.graph_plan(ei, n)
    has_fast = bool(eng.lib.ggl_gat_fast_supported(H, C))
    print(f"\n## {name}-sized graph, {H} x {C} heads: N = {n}, E = {E}, longest row {gp.fwd.max_len}, chunk {gp.fwd.chunk}, "
          f"{gp.fwd.n_long} long rows; f32 fast path {'exists' if has_fast else 'does not exist for this shape'}", flush=True)
    g = torch.Generator(device=dev).manual_seed(H * C)
    el, er = torch.randn(n, H, generator=g, device=dev), torch.randn(n, H, generator=g, device=dev)
    x32 = torch.randn(n, H, C, generator=g, device=dev)
    g32 = torch.randn(n, H, C, generator=g, device=dev)
    cont = [("f32 general", torch.float32, False), ("bf16", torch.bfloat16, False), ("f16", torch.float16, False)]
    if has_fast:
        cont.insert(0, ("f32 fast", torch.float32, True))
    xs = [x32.to(dt).requires_grad_(True) for _, dt, _ in cont]
    gs = [g32.to(dt) for _, dt, _ in cont]
    ea, ra = el.clone().requires_grad_(True), er.clone().requires_grad_(True)

    def fwd(i):
        xd = xs[i].detach()

        def run():
            eng.gat_fast = cont[i][2]
            return eng.gat_fused(gp, el, er, xd, 0.2, num_nodes=n)
        return run

    def both(i):
        def run():
            eng.gat_fast = cont[i][2]
            xs[i].grad = ea.grad = ra.grad = None
            eng.gat_fused(gp, ea, ra, xs[i], 0.2, num_nodes=n).backward(gs[i])
        return run

    with torch.no_grad():
        tf = alternate([fwd(i) for i in range(len(cont))], args.reps)
    tb = alternate([both(i) for i in range(len(cont))], args.reps)
    base = [c[0] for c in cont].index("f32 general")
    for what, t in (("forward", tf), ("forward + backward", tb)):
        for i, (cname, dt, _) in enumerate(cont):
            nb = E * (H * C * xs[i].element_size() + 4 + 4 * H)
            s = f"  {what:18s} {cname:11s} {t[i][0]:8.2f} ({t[i][1]:.2f} .. {t[i][2]:.2f}) ms   f32 general / this = {t[base][0] / t[i][0]:.2f}x"
            if what == "forward":
                s += f"   {nb / t[i][0] / 1e9:5.2f} TB/s algorithmic"
            print(s, flush=True)


def child_step():
    import argparse as ap_
    import torch

    from gammagl_amd import benchmarks

    dev = torch.device("cuda", 0)
    print("\n## 2-layer 8-head GAT training step on the Reddit-sized graph (gammagl_amd.benchmarks.run_gat: 602 -> 8 x 8 -> 41, "
          "heads averaged in the output layer, dropout 0.6; fwd + bwd + Adam), f32 and autocast(bf16) as alternating runs", flush=True)
    for rnd in range(2):
        for label, amp in (("f32", None), ("autocast(bf16)", torch.bfloat16)):
            a = ap_.Namespace(seed=0, warmup=2, steps=max(args.reps // 2, 3), no_roofline=True, dump_outputs=None, amp=amp)
            out, keep = benchmarks.run_gat(a, dev, 0, 1)
            print(f"  run {rnd + 1}  {label:15s} {out['ms_per_step']:8.2f} ms / step   loss {out['config']['loss']:.4f}", flush=True)
            del keep
            torch.cuda.empty_cache()


if __name__ == "__main__":
    if args.child == "step":
        child_step()
    elif args.child:
        child_op(args.child)
    else:
        sys.exit(driver())
