#!/usr/bin/env python3
"""Scaled dot-product graph attention (Engine.dot_attention) in three forms on the Reddit-sized and the products-sized
graph, H x C in {1 x 64, 8 x 8, 4 x 32}, forward and forward + backward, with the peak memory of one forward + backward:

    fused     the dot formed inside the aggregate's walk (ggl_dot_attn_fwd), backward composed from the existing walks
    composed  the edge dot along the sorted plan (ggl_bspmm_grad_w_sorted / ggl_bspmm_grad_w) + ggl_edge_softmax_agg_fwd,
              the same backward (the engine with dot_attn_fused = False)
    gather    the reference's message formula in torch: q[dst], k[src], v[src] as [E, H, C] tensors, segment softmax from
              scatter ops, index_add_ — skipped, and said so, where its [E, H, C] tensors do not fit

ONE process, warm-up, device-event timing, fused and composed ALTERNATING repetition by repetition (same clocks, same cache
state); the run-to-run spread of a form is (max - min) / median of its repetitions.  The rule for the default
(ggl_policy_dot_attn_fused): the fused forward stays on for a shape unless it is slower than the composed one by more than
that spread; the file ends with the verdict per shape.  The resource table of the new kernels is appended from
tools/kernel_resources.py (or from a file it wrote earlier: --resources-from).

    python tools/dot_attention_bench.py [--reps 9] [--out profiles/dot_attention.txt] [--small] [--resources-from FILE]
"""
import argparse
import math
import os
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import gammagl_amd  # noqa: E402
from gammagl_amd.synth import DATASETS, rmat_graph  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dot_attention.txt"))
ap.add_argument("--small", action="store_true", help="every 8th edge (a quick look, not the figures of record)")
ap.add_argument("--resources-from", default=None)
ap.add_argument("--gather-budget", type=float, default=0.7, help="share of free memory the gather route may claim")
args = ap.parse_args()

dev = torch.device("cuda", 0)
eng = gammagl_amd.engine()
lines = []
SHAPES = ((1, 64), (8, 8), (4, 32))


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def alternate(fns, reps):
    """(median, min, max) ms per call of each fn, the fns taking turns inside one loop"""
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


def engine_form(fused):
    def f(gp, q, k, v, n):
        eng.dot_attn_fused = fused
        try:
            return eng.dot_attention(gp, q, k, v, n)
        finally:
            eng.dot_attn_fused = True
    return f


def gather_form(ei):
    src, dst = ei[0], ei[1]

    def f(gp, q, k, v, n):
        H, C = q.shape[1], q.shape[2]
        z = (k[src] * q[dst]).sum(-1) / math.sqrt(C)
        m = torch.full((n, H), -torch.inf, device=dev).scatter_reduce(0, dst[:, None].expand(-1, H), z.detach(), "amax")
        e = torch.exp(z - m[dst])
        alpha = e / (torch.zeros(n, H, device=dev).index_add_(0, dst, e)[dst] + 1e-16)
        return torch.zeros(n, H, C, device=dev).index_add_(0, dst, v[src] * alpha.unsqueeze(-1))
    return f


def fmt(t):
    return f"{t[0]:8.2f} ({t[1]:.2f} .. {t[2]:.2f}) ms"


arch = torch.cuda.get_device_properties(dev).gcnArchName
say(f"# tools/dot_attention_bench.py on {arch}: median (min .. max) ms over {args.reps} repetitions, fused and composed alternating")
say("# fused = ggl_dot_attn_fwd; composed = sorted edge dot + ggl_edge_softmax_agg_fwd (Engine.dot_attn_fused = False); both run the same")
say("# backward (ggl_edge_softmax_agg_bwd_dst / _bwd_src + two ggl_bspmm_sum walks).  gather = the reference's message formula in torch.")
say("# peak = extra MiB allocated during one forward + backward; spread = (max - min) / median of a form's repetitions")
verdict = {}
for name in ("reddit", "products"):
    n, e, _, _ = DATASETS[name]
    if args.small:
        e //= 8
    ei = rmat_graph(n, e, seed=0, device=dev)
    E = int(ei.shape[1])
    gp = eng.graph_plan(ei, n)
    say(f"\n## {name}-sized graph: N = {n}, E = {E}, mean row {E / n:.0f}, longest {gp.fwd.max_len}, chunk {gp.fwd.chunk}, "
        f"{gp.fwd.n_long} long rows in {gp.fwd.n_chunks} chunks")
    for H, C in SHAPES:
        g = torch.Generator(device=dev).manual_seed(H * C)
        q, k, v = (torch.randn(n, H, C, generator=g, device=dev).requires_grad_(True) for _ in range(3))
        go = torch.randn(n, H, C, generator=g, device=dev)
        qd, kd, vd = q.detach(), k.detach(), v.detach()
        assert eng.lib.ggl_dot_attn_supported(H, C)
        fused, composed, gather = engine_form(True), engine_form(False), gather_form(ei)

        def fb(f):
            def run():
                q.grad = k.grad = v.grad = None
                f(gp, q, k, v, n).backward(go)
            return run

        with torch.no_grad():
            fwd = alternate([lambda: composed(gp, qd, kd, vd, n), lambda: fused(gp, qd, kd, vd, n)], args.reps)
        both = alternate([fb(composed), fb(fused)], args.reps)
        pk = [peak_mib(fb(composed)), peak_mib(fb(fused))]
        with torch.no_grad():
            pk_inf = [peak_mib(lambda: composed(gp, qd, kd, vd, n)), peak_mib(lambda: fused(gp, qd, kd, vd, n))]
        for what, (c, o) in (("forward", fwd), ("forward + backward", both)):
            spread = max((c[2] - c[1]) / c[0], (o[2] - o[1]) / o[0])
            say(f"{H} x {C:2d}  {what:18s}: composed {fmt(c)}   fused {fmt(o)}   composed / fused {c[0] / o[0]:5.2f}x   "
                f"spread {100 * spread:.1f} %")
            if what == "forward":
                verdict.setdefault((H, C), []).append((name, c[0], o[0], spread))
        say(f"{H} x {C:2d}  peak memory: forward + backward composed {pk[0]:9.1f} MiB  fused {pk[1]:9.1f} MiB;   "
            f"forward without grad composed {pk_inf[0]:9.1f} MiB  fused {pk_inf[1]:9.1f} MiB")
        # the torch-gather route: a forward holds about 4 [E, H, C] f32 tensors at once, a forward + backward about 8
        free = torch.cuda.mem_get_info(dev)[0]
        for what, mult, run in (("forward", 4, lambda: gather(gp, qd, kd, vd, n)), ("forward + backward", 8, fb(gather))):
            need = mult * E * H * C * 4
            if need > args.gather_budget * free:
                say(f"{H} x {C:2d}  gather {what}: SKIPPED — about {need / 2**30:.0f} GiB of [E, H, C] tensors, "
                    f"{free / 2**30:.0f} GiB free")
                continue
            try:
                with torch.set_grad_enabled(mult == 8):
                    t = alternate([run], 3)[0]
                    pk_g = peak_mib(run)
                say(f"{H} x {C:2d}  gather {what} (3 repetitions): {fmt(t)}   peak {pk_g:9.1f} MiB")
            except torch.cuda.OutOfMemoryError:
                say(f"{H} x {C:2d}  gather {what}: SKIPPED — out of memory")
            q.grad = k.grad = v.grad = None
            torch.cuda.empty_cache()
        del q, k, v, go, qd, kd, vd
        torch.cuda.empty_cache()
    del ei, gp
    eng.clear_caches()
    torch.cuda.empty_cache()

say("\n## the default (ggl_policy_dot_attn_fused): fused unless slower than composed by more than the spread, forward, any graph")
for (H, C), rows in verdict.items():
    lose = [r for r in rows if r[2] > r[1] * (1 + r[3])]
    say(f"{H} x {C:2d}: " + ("fused KEPT" if not lose else "fused LOSES on " + ", ".join(r[0] for r in lose)) + "   ("
        + "; ".join(f"{r[0]}: composed {r[1]:.2f} fused {r[2]:.2f} ms, spread {100 * r[3]:.1f} %" for r in rows) + ")"
        + f"   library answers {eng.lib.ggl_policy_dot_attn_fused(H, C, 0, 0)}")

say("\n## registers, scratch and occupancy of the dot instantiations of the shared walk (tools/kernel_resources.py")
say("## gammagl_amd/csrc/dotattn.hip gat_fwd_kernel; gat_fwd_kernel<float, float, 4, dropout, kLogitDot + 2 log2(C / 4) + z_out>,")
say("## kLogitDot = 2), beside the edge-logit instantiation of the same walk")
if args.resources_from:
    with open(args.resources_from) as f:
        res = f.read()
else:
    tool = os.path.join(REPO, "tools", "kernel_resources.py")
    res = subprocess.run([sys.executable, tool, os.path.join(REPO, "gammagl_amd", "csrc", "dotattn.hip"), "gat_fwd_kernel"],
                         capture_output=True, text=True).stdout
    res += subprocess.run([sys.executable, tool, os.path.join(REPO, "gammagl_amd", "csrc", "gat.hip"),
                           "gat_fwd_kernel<float, float, 4, false, 1>"], capture_output=True, text=True).stdout
for ln in res.splitlines():
    say(" ".join(ln.split()))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
