#!/usr/bin/env python3
"""The output-layer aggregate restricted to the rows the loss reads: torch.ops.ggl.spmm_rows (restricted plan pair,
ggl_plan_rows_* + ggl_bias_grad_rows) against what it replaces — the full K = 48 aggregate torch.ops.ggl.spmm_epi followed
by indexing the rows — on the products-sized graph with an 8 % row list (benchmarks._gcn_data: rand < 0.08).

ONE process, warm-up, device-event timing, the two routes ALTERNATING repetition by repetition, forward and
forward + backward.  Bytes are counted from shapes (no-reuse model: 4K + 8 bytes per edge and per output row, forward;
the backward of the full route also writes and re-reads the zero-filled [N, K] gradient).  Also reports the time to build
the restricted pair (first call, synchronous) and the HBM it holds.

    python tools/spmm_rows_bench.py [--reps 20] [--out profiles/spmm_rows.txt] [--small]
"""
import argparse
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import gammagl_amd  # noqa: E402
from gammagl_amd import cpp_ops  # noqa: E402
from gammagl_amd.synth import DATASETS, rmat_graph  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "spmm_rows.txt"))
ap.add_argument("--small", action="store_true", help="every 8th edge (a quick look, not the figures of record)")
ap.add_argument("--K", type=int, default=48)
ap.add_argument("--share", type=float, default=0.08)
args = ap.parse_args()

dev = torch.device("cuda", 0)
eng = gammagl_amd.engine()
ops = cpp_ops.load()
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
n, e, _, _ = DATASETS["products"]
if args.small:
    e //= 8
K = args.K
ei = rmat_graph(n, e, seed=0, device=dev)
E = int(ei.shape[1])
gen = torch.Generator(device=dev).manual_seed(0)
w = torch.rand(E, generator=gen, device=dev)
x = torch.randn(n, K, generator=gen, device=dev).requires_grad_(True)
bias = torch.randn(1, K, generator=gen, device=dev).requires_grad_(True)
rows = torch.nonzero(torch.rand(n, generator=gen, device=dev) < args.share).reshape(-1)
R = int(rows.numel())
go = torch.randn(R, K, generator=gen, device=dev)
say(f"# tools/spmm_rows_bench.py on {arch}: median (min .. max) ms over {args.reps} alternating repetitions")
say(f"## products-sized graph: N = {n}, E = {E}, K = {K}; row list: {R} rows ({R / n:.3f} of N)")


def full(xx, bb):
    return ops.spmm_epi(ei, w, xx, False, None, bb, False, 0.0)[rows]


def part(xx, bb):
    return ops.spmm_rows(ei, w, xx, rows, bb)


with torch.no_grad():
    for _ in range(2):       # full plans (forward side), sorted weights
        full(x, bias)
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated(dev)
    t0 = time.perf_counter()
    y = part(x, bias)        # builds the restricted pair (the transposed full plan with it, if this is its first use)
    torch.cuda.synchronize()
    t_first = (time.perf_counter() - t0) * 1e3
    m1 = torch.cuda.memory_allocated(dev) - y.numel() * 4
    assert torch.equal(y, full(x, bias)), "spmm_rows differs from the full aggregate indexed"
    del y
# build time of the pair alone: a second row tensor (same values) once every full plan exists
full(x, bias).backward(go)
x.grad = bias.grad = None
torch.cuda.synchronize()
rows2 = rows.clone()
m2 = torch.cuda.memory_allocated(dev)
t0 = time.perf_counter()
with torch.no_grad():
    y = ops.spmm_rows(ei, w, x, rows2, bias)
torch.cuda.synchronize()
t_pair = (time.perf_counter() - t0) * 1e3
pair_bytes = torch.cuda.memory_allocated(dev) - m2 - y.numel() * 4
del y
deg = torch.bincount(ei[1], minlength=n)
E_r = int(deg[rows].sum())
say(f"edges whose destination is listed: E' = {E_r} ({E_r / E:.3f} of E)")
say(f"restricted pair: built in {t_pair:.1f} ms (first call, with the full transposed plan: {t_first:.1f} ms); holds "
    f"{pair_bytes / 2**20:.0f} MiB (16 E' + 8 (N + R) = {(16 * E_r + 8 * (n + R)) / 2**20:.0f} MiB + long-row tables and row orders; "
    f"memory after the first call grew by {(m1 - m0) / 2**20:.0f} MiB)")


def fb(f):
    def run():
        x.grad = bias.grad = None
        f(x, bias).backward(go)
    return run


with torch.no_grad():
    fwd = alternate([lambda: full(x, bias), lambda: part(x, bias)], args.reps)
both = alternate([fb(full), fb(part)], args.reps)
fb(full)()
gx_f, gb_f = x.grad.clone(), bias.grad.clone()
fb(part)()
assert torch.equal(gx_f, x.grad) and torch.equal(gb_f, bias.grad), "gradients differ from the full path"
row_b = 4 * K + 8
bytes_full_f = E * row_b + n * row_b + R * 2 * 4 * K
bytes_part_f = E_r * row_b + R * row_b
bytes_full_b = bytes_full_f + 3 * n * 4 * K + E * row_b + n * row_b        # zero fill + index_put, bias_act_bwd copy, transposed walk
bytes_part_b = bytes_part_f + E_r * row_b + n * (4 * K + 8) + R * 4 * K     # bias gradient over R rows, transposed walk, full gx written
for what, (c, o), (nc, no) in (("forward", fwd, (bytes_full_f, bytes_part_f)), ("forward + backward", both, (bytes_full_b, bytes_part_b))):
    say(f"K = {K}  {what:18s}: full + index {c[0]:7.3f} ({c[1]:.3f} .. {c[2]:.3f}) ms [{nc / 2**30:.2f} GiB]   "
        f"spmm_rows {o[0]:7.3f} ({o[1]:.3f} .. {o[2]:.3f}) ms [{no / 2**30:.2f} GiB = {no / o[0] / 1e9:.2f} TB/s]   "
        f"saves {c[0] - o[0]:.3f} ms ({c[0] / o[0]:.1f}x)")
say("results: forward, gx and gbias equal the full route's under torch.equal")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
