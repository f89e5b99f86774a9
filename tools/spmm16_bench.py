#!/usr/bin/env python3
"""Mixed-precision aggregate: gspmm(sum) on rows stored as bf16 / f16 (torch.ops.ggl.spmm_sum -> ggl_spmm_sum_x16: f32 sums,
one rounding) against the f32 op on the same graph and weights, on the products-sized and the Reddit-sized synthetic graph
with GCN-norm weights, K = 64 / 128 / 256.

ONE process, warm-up, device-event timing, the f32, bf16 and f16 ops ALTERNATING repetition by repetition (same clocks, same
cache state), forward and forward + backward; then the column-block width sweep of the 16-bit launches (option col_block16:
64, 128, 256, 0 = one launch) at K = 256, forward.  Gathered bytes from shapes: E * K * element size per direction.

    python tools/spmm16_bench.py [--reps 10] [--out profiles/spmm16.txt] [--graphs products,reddit] [--small] [--no-sweep]
"""
import argparse
import ctypes
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import gammagl_amd  # noqa: E402
from gammagl_amd import cpp_ops  # noqa: E402
from gammagl_amd.layers import calc_gcn_norm  # noqa: E402
from gammagl_amd.synth import DATASETS, rmat_graph  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "spmm16.txt"))
ap.add_argument("--graphs", default="products,reddit")
ap.add_argument("--widths", default="64,128,256")
ap.add_argument("--small", action="store_true", help="every 8th edge (a quick look, not the figures of record)")
ap.add_argument("--no-sweep", action="store_true")
args = ap.parse_args()

dev = torch.device("cuda", 0)
eng = gammagl_amd.engine()
op = cpp_ops.load().spmm_sum
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
say(f"# tools/spmm16_bench.py on {arch}: median (min .. max) ms over {args.reps} alternating repetitions; ratio = f32 / 16-bit")
say(f"# gspmm(sum), GCN-norm weights (second sight: streamed in sorted order); col_block = {eng.lib.ggl_get_option(b'col_block')}, "
    f"col_block16 = {eng.lib.ggl_get_option(b'col_block16')}")
names = ("f32", "bf16", "f16")
dts = (torch.float32, torch.bfloat16, torch.float16)
for name in args.graphs.split(","):
    n, e, _, _ = DATASETS[name]
    if args.small:
        e //= 8
    ei = rmat_graph(n, e, seed=0, device=dev)
    w = calc_gcn_norm(ei, n).contiguous()
    E = int(ei.shape[1])
    gp = eng.graph_plan(ei, n)
    say(f"\n## {name}-sized graph: N = {n}, E = {E}, mean row {E / n:.0f}, longest {gp.fwd.max_len}, chunk {gp.fwd.chunk}, "
        f"{gp.fwd.n_long} long rows")
    for K in (int(k) for k in args.widths.split(",")):
        g = torch.Generator(device=dev).manual_seed(K)
        x32 = torch.randn(n, K, generator=g, device=dev)
        g32 = torch.randn(n, K, generator=g, device=dev)
        xs = [x32.to(dt).requires_grad_(True) for dt in dts]
        gs = [g32.to(dt) for dt in dts]

        def fwd(i):
            xd = xs[i].detach()
            return lambda: op(ei, w, xd)

        def both(i):
            def run():
                xs[i].grad = None
                op(ei, w, xs[i]).backward(gs[i])
            return run

        with torch.no_grad():
            tf = alternate([fwd(i) for i in range(3)], args.reps)
        tb = alternate([both(i) for i in range(3)], args.reps)
        cs = gp.fwd.c_struct(None)
        blocks = (int(eng.lib.ggl_spmm_col_blocks_plan(ctypes.byref(cs), K)), int(eng.lib.ggl_spmm_col_blocks_x16(ctypes.byref(cs), K)))
        for what, t, passes in (("forward", tf, 1), ("forward + backward", tb, 2)):
            s = f"K = {K:3d}  {what:18s} (launches f32 {blocks[0]}, 16-bit {blocks[1]}):"
            for i in range(3):
                nb = passes * E * K * xs[i].element_size()
                s += f"  {names[i]} {t[i][0]:7.2f} ({t[i][1]:.2f} .. {t[i][2]:.2f}) ms = {nb / t[i][0] / 1e9:5.2f} TB/s gathered"
            s += f"   ratio bf16 {t[0][0] / t[1][0]:.2f}x  f16 {t[0][0] / t[2][0]:.2f}x"
            say(s)
        if K == 256 and not args.no_sweep:
            old = int(eng.lib.ggl_get_option(b"col_block16"))
            xd = xs[1].detach()
            x0 = xs[0].detach()
            for bw in (64, 128, 256, 0):
                eng.set_option("col_block16", bw)
                with torch.no_grad():
                    t = alternate([lambda: op(ei, w, x0), lambda: op(ei, w, xd)], max(args.reps // 2, 3))
                say(f"K = 256  sweep col_block16 = {bw:3d} ({int(eng.lib.ggl_spmm_col_blocks_x16(ctypes.byref(cs), K))} launches): "
                    f"bf16 forward {t[1][0]:7.2f} ({t[1][1]:.2f} .. {t[1][2]:.2f}) ms   (f32 beside it {t[0][0]:7.2f} ms)")
            eng.set_option("col_block16", old)
        del xs, gs, x32, g32
    del ei, w, gp
    eng.clear_caches()
    torch.ops.ggl.clear_caches()
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
