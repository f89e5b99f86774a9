#!/usr/bin/env python3
"""The fused epilogue on rows stored as bf16 / f16 (Engine.spmm_epi -> ggl_spmm_epi_x16: bias, ReLU and dropout applied to
the f32 sums in registers, one rounding at the aggregate's only store) against the composition it replaces (gspmm on 16-bit
rows, then torch `+ bias`, `relu`, `dropout`: three more read-write passes over [N, K] forward, the same again backward plus a
column reduce), with the f32 fused op beside them.

One (graph, K) is ONE child process in which the contenders ALTERNATE repetition by repetition (same clocks, same cache
state), device-event timing after a warm-up; before it times a shape the child asserts the contract's equality at that shape
(fused 16-bit == f32 fused op on the widened rows after the same reseed, rounded).  The driver starts each child under its own
`timeout` and stops at the first that fails.  Two more children time training steps, the forms alternating as whole runs:
the 3-layer GCNTrainer step (f32; autocast(bf16) with GCNModel's fuse_epilogue16 off = the composition; on = fused), step time
and peak memory, and the GraphSAGEFullModel step under autocast(bf16).

Bytes of the epilogue per hidden layer, e = 2 (16-bit): the composition writes [N, K] once and reads + writes it three more
times forward (7 N K e), the fused form writes it once (N K e); backward the composition makes the same three passes plus a
column reduce (>= 7 N K e), the fused form one read-read-write pass (3 N K e).

    python tools/epi16_bench.py [--reps 10] [--out profiles/epi16.txt] [--graphs products,reddit] [--widths 64,128,256]
"""
import argparse
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "epi16.txt"))
ap.add_argument("--graphs", default="products,reddit")
ap.add_argument("--widths", default="64,128,256")
ap.add_argument("--dtypes", default="bf16,f16")
ap.add_argument("--small", action="store_true", help="every 8th edge (a quick look, not the figures of record)")
ap.add_argument("--no-step", action="store_true", help="skip the training steps")
ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
ap.add_argument("--child", default="", help="(internal) graph:K, 'gcn' or 'sage'")
args = ap.parse_args()
P_DROP = 0.5


def commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def driver():
    import torch

    arch = torch.cuda.get_device_properties(0).gcnArchName if torch.cuda.is_available() else "no GPU"
    lines = [f"# tools/epi16_bench.py on {arch}, commit {commit()} (+ working tree)",
             f"# median (min .. max) ms over {args.reps} alternating repetitions; bias + ReLU + dropout {P_DROP}, weighted sum"]
    jobs = [f"{g}:{k}" for g in args.graphs.split(",") if g for k in args.widths.split(",") if k]
    if not args.no_step:
        jobs += ["gcn", "sage"]
    rc = 0
    for job in jobs:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", job,
               "--reps", str(args.reps), "--dtypes", args.dtypes] + (["--small"] if args.small else [])
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


def _graph(name, dev):
    from gammagl_amd.layers import add_self_loops, calc_gcn_norm
    from gammagl_amd.synth import DATASETS, rmat_graph

    n, e, _, _ = DATASETS[name]
    if args.small:
        e //= 8
    ei = add_self_loops(rmat_graph(n, e, seed=0, device=dev), n)
    return n, ei, calc_gcn_norm(ei, n).contiguous()


def child_op(job):
    import torch

    import gammagl_amd
    from gammagl_amd import mpops

    name, K = job.split(":")
    K = int(K)
    dev = torch.device("cuda", 0)
    eng = gammagl_amd.engine()
    n, ei, w = _graph(name, dev)
    gp = eng.graph_plan(ei, n)
    print(f"\n## {name}-sized graph, K = {K}: N = {n}, E = {gp.E}, longest row {gp.fwd.max_len}, {gp.fwd.n_long} long rows",
          flush=True)
    g = torch.Generator(device=dev).manual_seed(K)
    x32 = torch.randn(n, K, generator=g, device=dev)
    go32 = torch.randn(n, K, generator=g, device=dev)
    bias = torch.randn(K, generator=g, device=dev)
    dts = [{"bf16": torch.bfloat16, "f16": torch.float16}[d] for d in args.dtypes.split(",") if d]

    def fused(x):
        return eng.spmm_epi(gp, w, x, "sum", None, bias, True, P_DROP, True)

    def composed(x):       # the parent commit's GCNConv under autocast
        out = mpops.gspmm(ei, w, x, "sum") + bias.to(x.dtype)
        return torch.nn.functional.dropout(torch.relu(out), P_DROP, True)

    for dt in dts:           # the contract at this shape, before any time is taken
        with torch.no_grad():
            eng.reseed(1)
            want = fused(x32.to(dt).float()).to(dt)
            eng.reseed(1)
            got = fused(x32.to(dt))
        assert got.dtype == dt and torch.equal(got.view(torch.int16), want.view(torch.int16)), (job, dt, "contract")
    cont = [("f32 fused", torch.float32, fused)]
    for dt in dts:
        nm = str(dt).replace("torch.", "").replace("bfloat16", "bf16").replace("float16", "f16")
        cont += [(f"{nm} composed", dt, composed), (f"{nm} fused", dt, fused)]
    xs = [x32.to(dt).requires_grad_(True) for _, dt, _ in cont]
    gs = [go32.to(dt) for _, dt, _ in cont]

    def fwd(i):
        xd = xs[i].detach()
        return lambda: cont[i][2](xd)

    def both(i):
        def run():
            xs[i].grad = None
            cont[i][2](xs[i]).backward(gs[i])
        return run

    with torch.no_grad():
        tf = alternate([fwd(i) for i in range(len(cont))], args.reps)
    tb = alternate([both(i) for i in range(len(cont))], args.reps)
    for what, t in (("forward", tf), ("forward + backward", tb)):
        for i, (cname, dt, _) in enumerate(cont):
            s = f"  {what:18s} {cname:14s} {t[i][0]:8.2f} ({t[i][1]:.2f} .. {t[i][2]:.2f}) ms"
            if cname.endswith("fused") and dt != torch.float32:
                s += f"   composed / fused = {t[i - 1][0] / t[i][0]:.2f}x"
            print(s, flush=True)


def child_gcn():
    import torch

    from gammagl_amd.trainer import GCNTrainer

    dev = torch.device("cuda", 0)
    n, ei, _ = _graph("products", dev)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(n, 100, generator=g, device=dev)
    y = torch.randint(0, 47, (n,), generator=g, device=dev)
    idx = torch.arange(0, n, 10, device=dev)
    print(f"\n## 3-layer GCNTrainer step (100 -> 256 -> 256 -> 47, dropout 0.5; fwd + bwd + Adam) on the products-sized graph, "
          f"N = {n}, E = {ei.shape[1]}: whole runs alternating, median (min .. max) of {args.reps} steps after 3, peak memory",
          flush=True)
    forms = (("f32", None, True), ("autocast(bf16) composed", torch.bfloat16, False), ("autocast(bf16) fused", torch.bfloat16, True))
    for rnd in range(2):
        for label, amp, fuse in forms:
            tr = GCNTrainer(100, 256, 47, num_layers=3, drop_rate=0.5, device=dev, amp_dtype=amp)
            for c in tr.net.conv:
                c.fuse_epilogue16 = fuse
            for _ in range(3):
                loss = tr.step(x, ei, y, idx, n)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
            for a, b in ev:
                a.record()
                loss = tr.step(x, ei, y, idx, n)
                b.record()
            torch.cuda.synchronize()
            t = sorted(a.elapsed_time(b) for a, b in ev)
            print(f"  run {rnd + 1}  {label:24s} {t[len(t) // 2]:8.2f} ({t[0]:.2f} .. {t[-1]:.2f}) ms / step   "
                  f"peak {torch.cuda.max_memory_allocated() / 2**30:6.2f} GiB   loss {float(loss):.4f}", flush=True)
            del tr
            torch.cuda.empty_cache()


def child_sage():
    import torch

    from gammagl_amd import layers

    dev = torch.device("cuda", 0)
    n, ei, _ = _graph("reddit", dev)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(n, 602, generator=g, device=dev)
    y = torch.randint(0, 41, (n,), generator=g, device=dev)
    print(f"\n## GraphSAGEFullModel step (602 -> 256 -> 41, mean, dropout 0.5; fwd + bwd + Adam) on the Reddit-sized graph, N = {n}, "
          f"E = {ei.shape[1]}: f32 and autocast(bf16) (the parent commit raises under autocast: no figure to compare with)", flush=True)
    for rnd in range(2):
        for label, amp in (("f32", None), ("autocast(bf16)", torch.bfloat16)):
            torch.manual_seed(0)
            net = layers.GraphSAGEFullModel(602, 256, 41, 1, torch.relu, 0.5, "mean").to(dev)
            opt = torch.optim.Adam(net.parameters(), lr=0.01)
            net.train()

            def step():
                opt.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=amp, enabled=amp is not None):
                    logits = net(x, ei)
                loss = torch.nn.functional.cross_entropy(logits.float(), y)
                loss.backward()
                opt.step()
                return loss

            for _ in range(3):
                loss = step()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
            for a, b in ev:
                a.record()
                loss = step()
                b.record()
            torch.cuda.synchronize()
            t = sorted(a.elapsed_time(b) for a, b in ev)
            print(f"  run {rnd + 1}  {label:15s} {t[len(t) // 2]:8.2f} ({t[0]:.2f} .. {t[-1]:.2f}) ms / step   "
                  f"peak {torch.cuda.max_memory_allocated() / 2**30:6.2f} GiB   loss {float(loss):.4f}", flush=True)
            del net, opt
            torch.cuda.empty_cache()


if __name__ == "__main__":
    if args.child == "gcn":
        child_gcn()
    elif args.child == "sage":
        child_sage()
    elif args.child:
        child_op(args.child)
    else:
        sys.exit(driver())
