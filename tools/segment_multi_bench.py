#!/usr/bin/env python3
"""The fused multi-statistic segment aggregate (Engine.segment_multi, ggl_segment_multi_fwd / _bwd) against the composition on
the existing segment ops (the engine with segment_multi_fused = False: one walk per statistic, an [E, K] tensor of squares),
on the destination ids of the Reddit-sized and the products-sized graph: K = 16, 64, 128 and 4 x 16 towers (K = 64, C = 16);
the PNA set (mean, min, max, std) and ("min",): forward, forward + backward, peak memory; and a PNAConv forward + backward
with fused on and off.

ONE process, warm-up, device-event timing, fused and composed ALTERNATING repetition by repetition; the spread of a form is
(max - min) / median of its repetitions.  An [E, K] f32 message tensor of the full graphs is 7 GB at K = 16 and 59 GB at
K = 128, and the composition holds seven of them: where 8 arrays do not fit in 70 % of the free memory the ids are cut to
their first E / 2^s elements, and the line says so.  Byte model, forward: the composition moves about 7 E K 4 bytes (x read by
mean, max, min and the square; -x and x * x written and read back), the fused walk 1 E K 4.  The rule for the defaults
(Engine.segment_multi_fused, PNAConv.fused): on, unless fused is slower than the composition by more than the spread for a
shape class; the file ends with the verdict.  The resource table and the ISA comparison are appended from --resources-from.

    python tools/segment_multi_bench.py [--reps 7] [--out profiles/segment_multi.txt] [--small] [--resources-from FILE]
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import gammagl_amd  # noqa: E402
from gammagl_amd import layers  # noqa: E402
from gammagl_amd.synth import DATASETS, rmat_graph  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "segment_multi.txt"))
ap.add_argument("--small", action="store_true", help="every 8th edge (a quick look, not the figures of record)")
ap.add_argument("--resources-from", default=None)
args = ap.parse_args()

dev = torch.device("cuda", 0)
eng = gammagl_amd.engine()
lines = []
SHAPES = ((16, 16), (64, 64), (128, 128), (64, 16))     # (K, C); the last is 4 towers of 16
SETS = (("mean", "min", "max", "std"), ("min",))


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def alternate(fns, reps):
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


def form(fused):
    def f(x, ids, n, aggs, C):
        eng.segment_multi_fused = fused
        try:
            return eng.segment_multi(x, ids, n, aggs, C, True)
        finally:
            eng.segment_multi_fused = True
    return f


def fmt(t):
    return f"{t[0]:8.2f} ({t[1]:.2f} .. {t[2]:.2f}) ms"


arch = torch.cuda.get_device_properties(dev).gcnArchName
say(f"# tools/segment_multi_bench.py on {arch}: median (min .. max) ms over {args.reps} repetitions, fused and composed alternating")
say("# fused = ggl_segment_multi_fwd / _bwd (one walk each way); composed = Engine.segment_multi_fused = False: segment mean / max,")
say("# -max(-x), mean(x * x) - mean^2, sqrt(relu + 1e-5) and torch's autograd through them.  peak = extra MiB allocated during a")
say("# forward + backward.  Byte model, forward, PNA set: composed ~ 7 E K 4 bytes against 1 E K 4 fused -> expected ratio ~ 7x")
say("# (\"min\" alone: composed reads x, writes -x, reads -x: 3 against 1).  spread = (max - min) / median of a form's repetitions")
say("# (peak memory: x.grad of the call before, one [E, K] array, is released at the start of the measured call — a first call peaks")
say("#  one array higher on both routes: tests/test_gpu_segment_multi.py measures 1.47 against 4.26 arrays that way)")
verdict = {}
fused, composed = form(True), form(False)
for name in ("reddit", "products"):
    n, e, _, _ = DATASETS[name]
    if args.small:
        e //= 8
    ids_full = rmat_graph(n, e, seed=0, device=dev)[1].contiguous()
    for K, C in SHAPES:
        free = torch.cuda.mem_get_info(dev)[0]
        s = 0
        while 8 * (ids_full.shape[0] >> s) * K * 4 > 0.7 * free:
            s += 1
        ids = ids_full[: ids_full.shape[0] >> s].contiguous()
        E = int(ids.shape[0])
        plan = eng.seg_plan(ids, n)
        say(f"\n## {name}-sized ids{'' if s == 0 else f' (first E / {1 << s}: 8 [E, K] arrays of the full list do not fit)'}: "
            f"N = {n}, E = {E}, K = {K}, C = {C}, longest row {plan.max_len}, chunk {plan.chunk}, {plan.n_long} long rows; "
            f"one [E, K] array {E * K * 4 / 2**20:.0f} MiB")
        g = torch.Generator(device=dev).manual_seed(K + C)
        x = torch.randn(E, K, generator=g, device=dev).requires_grad_(True)
        xd = x.detach()
        for aggs in SETS:
            go = torch.randn(n, len(aggs) * K, generator=g, device=dev)
            tag = f"K {K:3d} C {C:3d} {'+'.join(aggs):16s}"

            def fb(f):
                def run():
                    x.grad = None
                    f(x, ids, n, aggs, C).backward(go)
                return run

            try:
                with torch.no_grad():
                    fwd = alternate([lambda: composed(xd, ids, n, aggs, C), lambda: fused(xd, ids, n, aggs, C)], args.reps)
                both = alternate([fb(composed), fb(fused)], args.reps)
                pk = [peak_mib(fb(composed)), peak_mib(fb(fused))]
            except torch.cuda.OutOfMemoryError:
                say(f"{tag}: not measured — out of memory")
                x.grad = None
                torch.cuda.empty_cache()
                continue
            x.grad = None
            model = 7.0 if len(aggs) > 1 else 3.0
            for what, (c, o) in (("forward", fwd), ("forward + backward", both)):
                spread = max((c[2] - c[1]) / c[0], (o[2] - o[1]) / o[0])
                say(f"{tag} {what:18s}: composed {fmt(c)}   fused {fmt(o)}   composed / fused {c[0] / o[0]:5.2f}x"
                    + (f" (byte model {model:.0f}x)" if what == "forward" else "") + f"   spread {100 * spread:.1f} %"
                    + (f"   fused forward {E * K * 4 / o[0] / 1e9:.2f} TB/s of x" if what == "forward" else ""))
                verdict.setdefault((K, C, aggs), []).append((name, what, c[0], o[0], spread))
            say(f"{tag} peak memory forward + backward: composed {pk[0]:9.1f} MiB ({pk[0] * 2**20 / (E * K * 4):.2f} arrays)   "
                f"fused {pk[1]:9.1f} MiB ({pk[1] * 2**20 / (E * K * 4):.2f} arrays)")
        del x, xd, ids, plan
        eng.clear_caches()
        torch.cuda.empty_cache()
    # PNAConv, 4 towers of 16 channels, forward + backward, on at most 8 M edges of the graph (the edge MLP's [E, T, 2 F] and
    # [E, T, F] tensors and their gradients are the layer's memory, whatever the aggregate)
    ei = rmat_graph(n, min(e, 8_000_000), seed=1, device=dev)
    deg = torch.bincount(torch.bincount(ei[1], minlength=n))
    torch.manual_seed(0)
    conv = layers.PNAConv(64, 64, ("mean", "min", "max", "std"), ("identity", "amplification", "attenuation"), deg, towers=4,
                          divide_input=True).to(dev)
    xn = torch.randn(n, 64, device=dev)
    gn = torch.randn(n, 64, device=dev)

    def layer(flag):
        def run():
            conv.fused = flag
            conv.zero_grad()
            conv(xn, ei).backward(gn)
        return run

    try:
        c, o = alternate([layer(False), layer(True)], args.reps)
        pk = [peak_mib(layer(False)), peak_mib(layer(True))]
        spread = max((c[2] - c[1]) / c[0], (o[2] - o[1]) / o[0])
        say(f"\n## PNAConv(64 -> 64, 4 towers, divide_input, PNA set, 3 scalers) on {name}-sized nodes, E = {ei.shape[1]}, forward + backward:")
        say(f"fused=False {fmt(c)}   fused=True {fmt(o)}   ratio {c[0] / o[0]:5.2f}x   spread {100 * spread:.1f} %   "
            f"peak {pk[0]:.0f} -> {pk[1]:.0f} MiB")
        verdict.setdefault(("PNAConv", 4, 16), []).append((name, "forward + backward", c[0], o[0], spread))
    except torch.cuda.OutOfMemoryError:
        say(f"\n## PNAConv on {name}-sized nodes: not measured — out of memory")
    del ei, conv, xn, gn, ids_full
    eng.clear_caches()
    torch.cuda.empty_cache()

say("\n## the defaults (Engine.segment_multi_fused, PNAConv.fused): on unless fused is slower than composed by more than the spread")
for key, rows in verdict.items():
    lose = [r for r in rows if r[3] > r[2] * (1 + r[4])]
    say(f"{key}: " + ("fused KEPT" if not lose else "fused LOSES on " + ", ".join(f"{r[0]} {r[1]}" for r in lose)) + "   ("
        + "; ".join(f"{r[0]} {r[1]}: {r[2]:.2f} vs {r[3]:.2f} ms" for r in rows) + ")")
if args.resources_from:
    say()
    with open(args.resources_from) as f:
        for ln in f.read().splitlines():
            say(ln)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
