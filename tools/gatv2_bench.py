#!/usr/bin/env python3
"""GATv2's additive graph attention (Engine.gatv2_attention) in three forms on the Reddit-sized and the products-sized graph,
H x C in {8 x 8, 1 x 64, 4 x 32}: forward, forward + backward, memory of a forward without grad and peak memory of a
forward + backward:

    fused     the logit formed inside the aggregate's walk (ggl_gatv2_fwd); backward = ggl_edge_softmax_agg_bwd_dst / _bwd_src +
              ggl_gatv2_logit_bwd on the plan and on its transpose
    composed  z formed by torch under no_grad in edge blocks of at most 256 MiB of [E_block, H, C], then
              ggl_edge_softmax_agg_fwd; the same backward (the engine with gatv2_fused = False).  This is the baseline.
    gather    the message formula in torch, unblocked: xl[src] + xr[dst] as an [E, H, C] tensor, segment softmax from scatter
              ops, index_add_ — run only where its [E, H, C] tensors fit, and the table says where they do not

ONE process, warm-up, device-event timing, fused and composed ALTERNATING repetition by repetition (same clocks, same cache
state); the run-to-run spread of a form is (max - min) / median of its repetitions.  The rule for the default
(ggl_policy_gatv2_fused): the fused forward stays on for a shape unless it is slower than the composed one by more than that
spread; the file ends with the verdict per shape.  The resource table of the new kernels is appended from
tools/kernel_resources.py (or from a file it wrote earlier: --resources-from).

    python tools/gatv2_bench.py [--reps 9] [--out profiles/gatv2_attention.txt] [--small] [--resources-from FILE]
"""
import argparse
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
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gatv2_attention.txt"))
ap.add_argument("--small", action="store_true", help="every 8th edge (a quick look, not the figures of record)")
ap.add_argument("--resources-from", default=None)
ap.add_argument("--gather-budget", type=float, default=0.7, help="share of free memory the gather route may claim")
args = ap.parse_args()

dev = torch.device("cuda", 0)
eng = gammagl_amd.engine()
lines = []
SHAPES = ((8, 8), (1, 64), (4, 32))
SLOPE = 0.2


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
    def f(gp, xl, xr, att, n):
        eng.gatv2_fused = fused
        try:
            return eng.gatv2_attention(gp, xl, xr, att, n, SLOPE)
        finally:
            eng.gatv2_fused = True
    return f


def gather_form(ei):
    src, dst = ei[0], ei[1]

    def f(gp, xl, xr, att, n):
        H, C = xl.shape[1], xl.shape[2]
        z = (att * torch.nn.functional.leaky_relu(xl[src] + xr[dst], SLOPE)).sum(-1)
        m = torch.full((n, H), -torch.inf, device=dev).scatter_reduce(0, dst[:, None].expand(-1, H), z.detach(), "amax")
        e = torch.exp(z - m[dst])
        alpha = e / (torch.zeros(n, H, device=dev).index_add_(0, dst, e)[dst] + 1e-16)
        return torch.zeros(n, H, C, device=dev).index_add_(0, dst, xl[src] * alpha.unsqueeze(-1))
    return f


def fmt(t):
    return f"{t[0]:8.2f} ({t[1]:.2f} .. {t[2]:.2f}) ms"


arch = torch.cuda.get_device_properties(dev).gcnArchName
say(f"# tools/gatv2_bench.py on {arch}: median (min .. max) ms over {args.reps} repetitions, fused and composed alternating")
say("# fused = ggl_gatv2_fwd; composed = z by torch in edge blocks of <= 256 MiB + ggl_edge_softmax_agg_fwd (Engine.gatv2_fused = False);")
say("# both run the same backward (ggl_edge_softmax_agg_bwd_dst / _bwd_src + ggl_gatv2_logit_bwd on the plan and its transpose).")
say("# gather = the unblocked message formula in torch.  peak = extra MiB allocated during the call;")
say("# spread = (max - min) / median of a form's repetitions")
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
        xl, xr = (torch.randn(n, H, C, generator=g, device=dev).requires_grad_(True) for _ in range(2))
        att = (torch.randn(H, C, generator=g, device=dev) / C ** 0.5).requires_grad_(True)
        go = torch.randn(n, H, C, generator=g, device=dev)
        ld, rd, ad = xl.detach(), xr.detach(), att.detach()
        assert eng.lib.ggl_gatv2_supported(H, C)
        fused, composed, gather = engine_form(True), engine_form(False), gather_form(ei)

        def fb(f):
            def run():
                xl.grad = xr.grad = att.grad = None
                f(gp, xl, xr, att, n).backward(go)
            return run

        with torch.no_grad():
            fwd = alternate([lambda: composed(gp, ld, rd, ad, n), lambda: fused(gp, ld, rd, ad, n)], args.reps)
        both = alternate([fb(composed), fb(fused)], args.reps)
        pk = [peak_mib(fb(composed)), peak_mib(fb(fused))]
        with torch.no_grad():
            pk_inf = [peak_mib(lambda: composed(gp, ld, rd, ad, n)), peak_mib(lambda: fused(gp, ld, rd, ad, n))]
        for what, (c, o) in (("forward", fwd), ("forward + backward", both)):
            spread = max((c[2] - c[1]) / c[0], (o[2] - o[1]) / o[0])
            say(f"{H} x {C:2d}  {what:18s}: composed {fmt(c)}   fused {fmt(o)}   composed / fused {c[0] / o[0]:5.2f}x   "
                f"spread {100 * spread:.1f} %")
            if what == "forward":
                verdict.setdefault((H, C), []).append((name, c[0], o[0], spread))
        say(f"{H} x {C:2d}  peak memory: forward + backward composed {pk[0]:9.1f} MiB  fused {pk[1]:9.1f} MiB;   "
            f"forward without grad composed {pk_inf[0]:9.1f} MiB  fused {pk_inf[1]:9.1f} MiB   "
            f"(one [E, H] array {E * H * 4 / 2**20:.1f} MiB, one [E, H, C] array {E * H * C * 4 / 2**20:.1f} MiB)")
        # the unblocked torch route: a forward holds about 4 [E, H, C] f32 tensors at once, a forward + backward about 8
        free = torch.cuda.mem_get_info(dev)[0]
        for what, mult, run in (("forward", 4, lambda: gather(gp, ld, rd, ad, n)), ("forward + backward", 8, fb(gather))):
            need = mult * E * H * C * 4
            if need > args.gather_budget * free:
                say(f"{H} x {C:2d}  gather {what}: not measured — about {need / 2**30:.0f} GiB of [E, H, C] tensors do not fit, "
                    f"{free / 2**30:.0f} GiB free")
                continue
            try:
                with torch.set_grad_enabled(mult == 8):
                    t = alternate([run], 3)[0]
                    pk_g = peak_mib(run)
                say(f"{H} x {C:2d}  gather {what} (3 repetitions): {fmt(t)}   peak {pk_g:9.1f} MiB")
            except torch.cuda.OutOfMemoryError:
                say(f"{H} x {C:2d}  gather {what}: not measured — out of memory")
            xl.grad = xr.grad = att.grad = None
            torch.cuda.empty_cache()
        del xl, xr, att, go, ld, rd, ad
        torch.cuda.empty_cache()
    del ei, gp
    eng.clear_caches()
    torch.cuda.empty_cache()

say("\n## the default (ggl_policy_gatv2_fused): fused unless slower than composed by more than the spread, forward, any graph")
for (H, C), rows in verdict.items():
    lose = [r for r in rows if r[2] > r[1] * (1 + r[3])]
    say(f"{H} x {C:2d}: " + ("fused KEPT" if not lose else "fused LOSES on " + ", ".join(r[0] for r in lose)) + "   ("
        + "; ".join(f"{r[0]}: composed {r[1]:.2f} fused {r[2]:.2f} ms, spread {100 * r[3]:.1f} %" for r in rows) + ")"
        + f"   library answers {eng.lib.ggl_policy_gatv2_fused(H, C, 0, 0)}")

say("\n## registers, scratch and occupancy (tools/kernel_resources.py): the GATv2 instantiations of the shared walk,")
say("## gat_fwd_kernel<float, float, 4, dropout, kLogitGatv2 + 2 log2(C / 4) + z_out>, kLogitGatv2 = 12 (gatv2.hip); the backward walk")
say("## gatv2_logit_bwd_kernel<VEC, att_rows> and its merge (gatv2_bwd.hpp in gat.hip); and the gat_fwd_kernel instantiations of")
say("## gat.hip and dotattn.hip")
if args.resources_from:
    with open(args.resources_from) as f:
        res = f.read()
else:
    tool = os.path.join(REPO, "tools", "kernel_resources.py")
    res = ""
    for src, flt in (("gatv2.hip", "gat_fwd_kernel"), ("gat.hip", "gatv2_logit"), ("gat.hip", "gat_fwd_kernel"),
                     ("dotattn.hip", "gat_fwd_kernel")):
        res += subprocess.run([sys.executable, tool, os.path.join(REPO, "gammagl_amd", "csrc", src), flt],
                              capture_output=True, text=True).stdout
for ln in res.splitlines():
    say(" ".join(ln.split()))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
