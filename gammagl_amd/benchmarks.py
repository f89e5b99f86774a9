"""The benchmark bodies behind bench.py: one function per workload family, each
returning the JSON line's dict.  Harness code only — graphs are synthetic (`synth`), the work runs through the
same Engine / layers / trainers a user gets; nothing here touches `oracle/` (bench.py's cpu_baseline leg does).

  gcn   : full-graph 3-layer GCN training step (BASELINE metric) on `products` | `arxiv` | `tiny` (R-MAT),
          `products-planted` (hierarchical planted communities: a graph WITH locality, beside R-MAT which has none)
          and `papers-share` (config 5: rank 3's share of the 8-way papers100M-sized partition, dry, on one GPU);
  gat   : `reddit-gat` — config 3, the 2-layer 8-head GAT training step on the Reddit-sized graph;
  sage  : `sage-minibatch` — config 4, neighbour-sampled GraphSAGE mini-batches on the products-sized graph.
"""
import os
import time

import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import engine as _default_engine
from .dist import DistGCNTrainer, _HaloAggregate, build_partition
from .synth import DATASETS

PEAK_GBPS = 8000.0     # HBM3E peak of one MI355X (MI355X_MICROARCH.md)

WORKLOADS = {
    # name: family, dataset sizes, generator, (dry partition: parts / rank played), second node order reported beside the main one
    "products": dict(kind="gcn", dataset="products", gen="rmat", also="degree"),
    "arxiv": dict(kind="gcn", dataset="arxiv", gen="rmat", also="degree"),
    "tiny": dict(kind="gcn", dataset=None, gen="rmat", also=None),
    "tiny-planted": dict(kind="gcn", dataset=None, gen="planted", also=("cluster", "none")),
    "products-planted": dict(kind="gcn", dataset="products", gen="planted", also=("cluster", "none")),
    "papers-share": dict(kind="gcn", dataset="papers100M", gen="rmat", parts=8, play=3, also=None),
    "reddit-gat": dict(kind="gat", dataset="reddit"),
    "sage-minibatch": dict(kind="sage", dataset="products"),
}


def sizes_of(workload):
    spec = WORKLOADS[workload]
    if spec["dataset"] is None:
        return 20000, 400000, 100, 47
    return DATASETS[spec["dataset"]]


def _sync(dev, world):
    if world > 1:
        dist.barrier()
    if dev.type == "cuda":
        torch.cuda.synchronize()


def step_outputs(net, loss):
    """What a caller of the timed step holds after its last step, on the host (bench.py --dump-outputs): the loss, every
    parameter as the optimizer left it and the gradient that step computed for it."""
    out = {"loss": torch.tensor([float(loss)], dtype=torch.float64)}
    for name, p in net.named_parameters():
        out[name] = p.detach().float().cpu()
        if p.grad is not None:
            out[name + ".grad"] = p.grad.detach().float().cpu()
    return out


# ---------------------------------------------------------------------------------------------------------------
# PMC calibration: two launches of KNOWN byte counts in the access patterns of the aggregate, so that the counter
# corrections applied to the dominant kernel are measured on this part, in this run (MI355X_MICROARCH.md, HBM section:
# "calibrate on a known byte count in your own access pattern")
# ---------------------------------------------------------------------------------------------------------------
CALIB = {"reps": 3,
         # kernel-name fragments of the calibration launches in a rocprofv3 counter file, bytes each moves
         # a 16 B / lane streaming READ (16 x the 256 MB Infinity Cache): what the aggregate mostly does
         "stream_read": {"kernel": "calib_stream_kernel<0>", "vec4": 1 << 28},      # 4 GiB: the ramp of a 0.7 ms launch is small
         # 2 GiB read + 2 GiB written
         "stream_copy": {"kernel": "calib_stream_kernel<1>", "vec4": 1 << 27},
         # a gather of 256-byte rows (what a 64-column block of the aggregate reads per edge): a random PERMUTATION of
         # 2^22 rows, so every source line is needed exactly once — known bytes with no cache-reuse term
         "gather256": {"kernel": "gather_rows_ex_kernel", "rows": 1 << 22, "K": 64}}
CALIB_ORDER = ("stream_read", "stream_copy", "gather256")


def calib_known_bytes(which):
    """(bytes read, bytes written) of one calibration launch"""
    c = CALIB[which]
    if which == "stream_read":
        return c["vec4"] * 16, 0
    if which == "stream_copy":
        return c["vec4"] * 16, c["vec4"] * 16
    return c["rows"] * c["K"] * 4 + c["rows"] * 8, c["rows"] * c["K"] * 4     # the rows + their int64 row ids


def calibration_launches(eng, dev, time_it=False):
    """Launch the calibration patterns CALIB["reps"] times each (`ggl_calib_stream` read / copy, then the library's
    row-gather kernel over a random permutation).  With `time_it`: ms per launch of each (hipEvents on the launch
    stream, median) -> the rates this part ACHIEVES, the yardstick for `frac_of_achievable`."""
    import ctypes

    out = {}
    g = torch.Generator(device=dev).manual_seed(99)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for which in CALIB_ORDER:
        if which == "gather256":
            n, K = CALIB[which]["rows"], CALIB[which]["K"]
            src = torch.randn(n, K, generator=g, device=dev)
            dst = torch.empty(n, K, device=dev)
            idx = torch.randperm(n, generator=g, device=dev)
            run = lambda: eng.gather_rows_into(src, idx, dst)      # noqa: E731
        else:
            n4 = CALIB[which]["vec4"]
            src = torch.randn(n4 * 4, generator=g, device=dev)
            dst = torch.empty(n4 * 4 if which == "stream_copy" else 65536, device=dev)
            mode = 1 if which == "stream_copy" else 0
            run = lambda: eng._check(eng.lib.ggl_calib_stream(ctypes.c_void_p(src.data_ptr()),   # noqa: E731
                                                              ctypes.c_void_p(dst.data_ptr()), n4, mode, st))
        ts = []
        for _ in range(CALIB["reps"]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            if time_it:
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b))
        torch.cuda.synchronize()
        if time_it:
            rd, wr = calib_known_bytes(which)
            ms = min(ts)
            out[which] = {"ms": ms, "GBps": (rd + wr) / (ms * 1e-3) / 1e9, "bytes": rd + wr}
        del src, dst, run
    torch.cuda.empty_cache()
    return out


def roofline_block(kernel, launches, ms_per_aggregate, alg_bytes_aggregate, compulsory_bytes, edges,
                   traffic_per_launch=None, traffic_source=None, extra=None):
    """The `roofline` object of the line.  `frac` is a fraction of the HBM peak that cannot exceed 1: measured
    HBM-side bytes per launch (PMC) / launch duration / peak.  The algorithmic rate (SURVEY.md §8d's no-reuse
    byte count per AGGREGATE, ids and weights counted once, / the aggregate's duration) is `eff_GBps`: it may
    exceed the peak when L2 serves part of the gathers, so it is reported as a rate, never as a fraction."""
    ms_launch = max(ms_per_aggregate / max(launches, 1), 1e-9)
    eff = alg_bytes_aggregate / (max(ms_per_aggregate, 1e-9) * 1e-3) / 1e9
    rf = {"bound": "hbm", "kernel": kernel, "launches_per_aggregate": launches, "ms_per_aggregate": ms_per_aggregate,
          "ms_per_launch": ms_launch, "peak": PEAK_GBPS, "unit": "GB/s",
          "eff_GBps": eff, "alg_bytes_per_aggregate": alg_bytes_aggregate,
          "compulsory_bytes": compulsory_bytes, "edges_per_s_aggregate": edges / (max(ms_per_aggregate, 1e-9) * 1e-3)}
    set_traffic(rf, traffic_per_launch, traffic_source)
    if extra:
        rf.update(extra)
    return rf


def set_traffic(rf, traffic_per_launch, source, achievable=None):
    """Fill the rate fields of a roofline block so that every fraction can be recomputed from fields of the block:

      traffic              bytes per launch the counters saw on the L2's FABRIC side (FETCH_SIZE / WRITE_SIZE with the
                           corrections `pmc_calibration` measured in this run) — Infinity-Cache hits INCLUDED: the
                           counters sit between L2 and the fabric and cannot tell MALL from DRAM
      achieved             = traffic / ms_per_launch                      [GB/s]
      frac_of_peak         = achieved / peak (8 TB/s HBM3E)               — can exceed what DRAM alone delivers when the
                                                                            Infinity Cache serves part of the misses
      frac_of_achievable   = achieved / achievable_GBps                   — achievable = the rate a 16 B/lane streaming
                                                                            copy reaches on this part, timed in this run
      alg_frac             = alg_bytes_per_aggregate / ms_per_aggregate / peak  (SURVEY.md §8d's no-reuse byte model;
                             ABOVE 1 when L2 / MALL serve gathers the model counts as DRAM reads — it is a rate of
                             useful work, not a traffic fraction)
      frac                 = min(frac_of_peak, 1): the contract's field."""
    rf["traffic"], rf["traffic_source"] = traffic_per_launch, source
    rf["traffic_side"] = "L2-fabric side (FETCH_SIZE / WRITE_SIZE): Infinity-Cache hits included, not DRAM-only"
    if traffic_per_launch:
        rf["achieved"] = traffic_per_launch / (rf["ms_per_launch"] * 1e-3) / 1e9
        rf["achieved_basis"] = "measured fabric-side bytes per launch (rocprofv3 --pmc, corrections calibrated in-run) / launch duration"
        rf["traffic_per_aggregate"] = traffic_per_launch * rf["launches_per_aggregate"]
        rf["traffic_over_compulsory"] = rf["traffic_per_aggregate"] / max(rf["compulsory_bytes"], 1)
        rf["traffic_over_algorithmic"] = rf["traffic_per_aggregate"] / max(rf["alg_bytes_per_aggregate"], 1)
    else:
        rf["achieved"] = min(rf["eff_GBps"], PEAK_GBPS)
        rf["achieved_basis"] = "no counter data for this workload: algorithmic bytes / duration, capped at the peak"
    raw = rf["achieved"] / PEAK_GBPS
    rf["frac_of_peak"] = raw
    rf["alg_frac"] = rf["eff_GBps"] / PEAK_GBPS
    if achievable is not None:
        rf["achievable_GBps"] = achievable
    if rf.get("achievable_GBps"):
        rf["frac_of_achievable"] = rf["achieved"] / rf["achievable_GBps"]
    rf["frac"] = min(raw, 1.0)
    if raw > 1.0:
        rf["beyond_hbm_peak"] = {"achieved_over_peak": raw,
                                 "note": "fabric-side traffic above the HBM peak: part of it is served by the Infinity Cache"}
    return rf


# ---------------------------------------------------------------------------------------------------------------
# gcn: the BASELINE metric
# ---------------------------------------------------------------------------------------------------------------
def _gcn_data(pg, f_in, n_cls, seed, rank, dev, world):
    """features / labels / train mask of the local rows only (no [N, F] tensor on any rank)"""
    gen = torch.Generator(device=dev).manual_seed(seed + 7919 * (rank + 1))
    x = torch.randn(pg.n_local, f_in, generator=gen, device=dev)
    y = torch.randint(0, n_cls, (pg.n_local,), generator=gen, device=dev)
    train_local = torch.nonzero(torch.rand(pg.n_local, generator=gen, device=dev) < 0.08).reshape(-1)
    nt = torch.tensor([train_local.numel()], device=dev, dtype=torch.int64)
    if world > 1:
        dist.all_reduce(nt)  # the global train-set size every rank normalises its loss by
    return x, y, train_local, max(int(nt), 1), gen


def _norm_both_steps(pg, data, args, f_in, n_cls, dev, steps=4):
    """Side figure (round-4 verdict, missing #5): the step as the reference's example runs it BY DEFAULT —
    GCNModel(norm='both') with edge_weight=None, every GCNConv.forward computing its own symmetric normalisation from the
    edge list (gcn_conv.py:88-102: two `degree` scatters, two pows, two [E] gathers, two [E] products per layer; the
    `calc_gcn_norm` line of examples/gcn/gcn_trainer.py:58-59 is commented out there) — through layers.GCNModel, (a) as
    shipped here: the weights computed once per edge_index and kept on the graph's plan, (b) recomputed in every
    forward like the reference (layers.CACHE_GCN_NORM = False).  The headline step (norm='none' + precomputed weights) is
    (a) minus the layer-side bookkeeping."""
    from . import layers
    from .trainer import GCNTrainer

    x, y, train_local, _, _ = data
    ei = pg.ei_loc                      # one rank: the whole graph, local ids = global ids
    n = pg.n_local
    res = {}
    for label, cached in (("ms_per_step_cached", True), ("ms_per_step_uncached", False)):
        layers.CACHE_GCN_NORM = cached
        try:
            tr = GCNTrainer(f_in, args.hidden, n_cls, num_layers=args.layers, norm="both", seed=args.seed, device=dev)
            for _ in range(2):
                tr.step(x, ei, y, train_local, n)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step(x, ei, y, train_local, n)
            torch.cuda.synchronize()
            res[label] = (time.perf_counter() - t0) / steps * 1e3
        finally:
            layers.CACHE_GCN_NORM = True
        del tr
    res["note"] = ("GCNModel(norm='both'), edge_weight=None (the reference example's default, gcn_conv.py:88-102): cached = the "
                   "normalised weights kept on the graph's plan; uncached = recomputed in every GCNConv.forward as the reference does")
    torch.cuda.empty_cache()
    return res


def _wants_graph(args, pg, dev, world):
    """Record the step into a hipGraph?  One rank on a GPU only; `auto`: launch-bound sizes (bench.py --hipgraph)."""
    mode = getattr(args, "hipgraph", "off")
    if mode == "off" or world > 1 or dev.type != "cuda" or (pg.comm and not pg.dry):
        return False
    return mode == "on" or pg.e_local < (1 << 25)


def _time_steps(trainer, data, args, dev, world):
    x, y, train_local, n_train, _ = data
    step = lambda: trainer.step(x, y, train_local, n_train)   # noqa: E731
    trainer.graphed = _wants_graph(args, trainer.pg, dev, world)
    trainer.halo_tune = None
    tune = os.environ.get("GGL_HALO_TUNE", "auto")
    if trainer.pg.comm and tune != "0" and (tune == "1" or trainer.pg.e_local < (1 << 27)):
        # untimed, before warm-up: how many column chunks the exchange runs in is measured here, not assumed.  (auto: not
        # for shares of 2^27 edges and more — a papers100M-sized share holds 24 GB per exchange buffer and 0.56 s per
        # pass; its defaults are the measured ones, and GGL_HALO_TUNE=1 asks for the measurement all the same)
        trainer.halo_tune = trainer.tune_halo_chunks(x, y, train_local, n_train)
    if trainer.graphed:
        trainer.capture(x, y, train_local, n_train, warmup=max(int(args.warmup), 3))
        step = trainer.replay
    for _ in range(args.warmup):
        step()
    _sync(dev, world)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    _sync(dev, world)
    dt = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
    lsum = loss.detach().double().reshape(1).clone()
    if world > 1:
        dist.all_reduce(dt, op=dist.ReduceOp.MAX)
        dist.all_reduce(lsum)
    return float(dt), float(lsum)


def _exchange_report(pg, trainer, data, args, dev, world, widths):
    """What the N > 1 step does on the wire, measured AFTER the timed region (events around every work.wait() would
    perturb it): per-step exchange volume, the time the compute stream stalled waiting for all-to-alls
    (`halo_exposed_ms`), each distinct exchange timed on its own (no compute beside it) and the overlap they imply."""
    x, y, train_local, n_train, _ = data
    k = max(1, min(int(args.steps), 5))
    pg.profile = {}
    for _ in range(k):
        trainer.step(x, y, train_local, n_train)
    _sync(dev, world)
    rep = pg.profile_summary(k)
    pg.profile = None
    iso, iso_total = [], 0.0
    P = max(pg.world, len(pg.send_splits)) if pg.dry else pg.world
    for K, per_step in widths:
        chunks = _HaloAggregate._chunks(K, pg)
        ms = {}
        for direction, (n_out, n_in, osp, isp) in (("fwd", (pg.n_halo, pg.n_send, pg.recv_splits, pg.send_splits)),
                                                   ("bwd", (pg.n_send, pg.n_halo, pg.send_splits, pg.recv_splits))):
            bufs = [torch.zeros((n_in, c1 - c0), dtype=torch.float32, device=dev) for c0, c1 in chunks]
            for rep_i in range(3):
                if rep_i == 1:
                    _sync(dev, world)
                    t0 = time.perf_counter()
                for ci, b in enumerate(bufs):
                    _, w = pg._a2a(n_out, b, osp, isp, tag=("probe", direction, ci))
                    w.wait()
            _sync(dev, world)
            ms[direction] = (time.perf_counter() - t0) / 2 * 1e3
            del bufs
        gb_in = pg.n_halo * K * 4 / 1e9
        e = {"K": K, "exchanges_per_step": per_step, "chunks": len(chunks), "fwd_ms": ms["fwd"], "bwd_ms": ms["bwd"],
             "GB_in_fwd": gb_in, "GBps_in_fwd": gb_in / max(ms["fwd"], 1e-9) * 1e3,
             "GBps_per_link_fwd": gb_in / max(ms["fwd"], 1e-9) * 1e3 / max(P - 1, 1)}
        iso.append(e)
        iso_total += per_step * (ms["fwd"] + ms["bwd"]) / 2
    for key in [k_ for k_ in pg._bufs if k_[0] == "probe"]:
        del pg._bufs[key]
    rep["halo_chunks"] = getattr(trainer, "halo_tune", None)   # measured before warm-up (DistGCNTrainer.tune_halo_chunks)
    rep["a2a_isolated"] = iso
    rep["a2a_isolated_ms_per_step"] = iso_total
    rep["overlap_frac"] = (1.0 - rep["halo_exposed_ms"] / iso_total) if iso_total > 0 and not pg.dry else None
    rep["note"] = ("rank 0's figures; exposed = compute-stream stalls at work.wait(); isolated = the same all-to-all-v "
                   "shapes with nothing beside them" + ("; DRY partition: nothing travels, times are buffer handling only"
                                                        if pg.dry else ""))
    return rep


def dominant_spmm(pg, eng, K, gen, dev, reps=10):
    """(ms per K-wide aggregate, launches, plan, weights, source rows, edges) of the step's dominant kernel on this
    rank: the CSR SpMM-sum over its largest edge block (local-source edges on one GPU, halo-source edges in a
    partition where most edges have a remote source)."""
    use_halo = pg.gp_halo is not None and pg.gp_halo.E > pg.gp_loc.E
    gp, w, rows = (pg.gp_halo, pg.w_halo, pg.n_halo) if use_halo else (pg.gp_loc, pg.w_loc, pg.n_local)
    h = torch.randn(rows, K, generator=gen, device=dev)
    ms = eng.time_spmm_sum(gp, w, h, reps=reps)
    import ctypes

    cs = gp.fwd.c_struct(None)    # (the plan decides: 128-column blocks where its node order carries locality)
    launches = int(eng.lib.ggl_spmm_col_blocks_plan(ctypes.byref(cs), K))
    del h
    return ms, launches, gp, rows, use_halo


def _dry(args, spec):
    """(parts, rank played) of a dry partition: built into the workload (papers-share) or asked for with --dry-parts."""
    parts = int(getattr(args, "dry_parts", 0) or 0) or spec.get("parts")
    if not parts:
        return None, 0
    play = int(getattr(args, "dry_rank", -1))
    return parts, (play if play >= 0 else spec.get("play", parts // 2))


def pmc_probe_gcn(args, dev, eng):
    """`bench.py --pmc-probe` for the gcn family: rebuild this run's graph and launch the dominant kernel a few
    times (rocprofv3 --pmc wraps this process; FETCH_SIZE / WRITE_SIZE / TCC_* go in separate passes)."""
    spec = WORKLOADS[args.workload]
    n_nodes, n_edges, _, _ = sizes_of(args.workload)
    parts, play = _dry(args, spec)
    calibration_launches(eng, dev)
    pg = build_partition(n_nodes, n_edges, args.seed, play, 1, None, dev, eng, relabel=args.relabel,
                         order=args.order, parts=parts, kind=spec["gen"])
    gen = torch.Generator(device=dev).manual_seed(1)
    ms, launches, gp, rows, _ = dominant_spmm(pg, eng, args.hidden, gen, dev, reps=4)
    torch.cuda.synchronize()
    # (reps + 1 warm-up) aggregates of `launches` dispatches each were the LAST dispatches of the dominant kernel: the
    # parent averages the counters over exactly those (a clustered order runs the same kernel while it is computed)
    # ... and the hub walk beside them runs once per launch — or ONCE per aggregate where the plan's long rows lead the id
    # range (a degree-sorted order; option hub_one_launch, round 5)
    ohl = int(eng.lib.ggl_get_option(b"hub_one_launch"))
    one_hub = launches > 1 and (ohl == 1 or (ohl == 2 and gp.fwd.hub_first))
    hub = 5 * (1 if one_hub else launches)
    print(f"pmc-probe: E={gp.E} rows_in={rows} K={args.hidden} launches/aggregate={launches} ms/aggregate={ms:.3f} "
          f"aggregates=5 dispatches={5 * launches},{hub}", flush=True)


def run_gcn(args, dev, rank, world, eng=None):
    """bench.py body for the gcn family, any world size (world == 1 degenerates to no exchange).  Top-level
    `value` / `ms_per_step` belong to the step with every layer associated as GammaGL's GCNConv writes it,
    A (X W) (gcn_conv.py:79): 2 aggregations per layer."""
    eng = eng if eng is not None else _default_engine()
    spec = WORKLOADS[args.workload]
    n_nodes, n_edges, f_in, n_cls = sizes_of(args.workload)
    parts, play = _dry(args, spec)
    if parts and world != 1:
        raise SystemExit(f"bench.py: --workload {args.workload} plays rank {play} of a {parts}-way partition on ONE GPU "
                         f"(dry partition); run it with --gpus 1")
    emul = dev.type != "cuda"

    def build(relabel):
        t0 = time.perf_counter()
        stats = {}
        pg = build_partition(n_nodes, n_edges, args.seed, play if parts else rank, world, None, dev, eng, relabel=relabel,
                             order=args.order, parts=parts, stats=stats, kind=spec["gen"])
        if dev.type == "cuda":
            torch.cuda.empty_cache()
            torch.cuda.synchronize()
        return pg, stats, time.perf_counter() - t0

    pg, stats, t_gen = build(args.relabel)
    E = pg.e_global
    # edges this process aggregates per aggregation: the whole graph over all ranks — or, for a dry share, its own
    e_unit = pg.e_local if parts else E
    data = _gcn_data(pg, f_in, n_cls, args.seed, rank, dev, world)
    gen = data[4]
    af_main = bool(getattr(args, "aggregate_first", False))

    def trainer(aggregate_first):
        return DistGCNTrainer(pg, f_in, args.hidden, n_cls, num_layers=args.layers, seed=args.seed, device=dev,
                              aggregate_first=aggregate_first, capturable=_wants_graph(args, pg, dev, world))

    tr = trainer(af_main)
    dt, lsum = _time_steps(tr, data, args, dev, world)
    outputs = step_outputs(tr.net, lsum) if getattr(args, "dump_outputs", None) else None
    n_agg = tr.net.agg_per_step     # aggregations the step actually executed (counted by the model's forward)
    graphed = bool(getattr(tr, "graphed", False))
    value = n_agg * e_unit * args.steps / dt
    exchange = None
    if pg.comm and not getattr(args, "no_exchange_report", False):
        kc = n_cls + (-n_cls) % 4
        widths = [(args.hidden, 2 * (args.layers - 2)), (kc, 2)] if args.layers >= 2 else [(kc, 2)]
        if not tr.net.const_input_halo:
            widths[0] = (args.hidden, widths[0][1] + 2)
        exchange = _exchange_report(pg, tr, data, args, dev, world, [w for w in widths if w[1] > 0])
    side = None
    if not getattr(args, "no_comparison", False):
        tr2 = trainer(not af_main)
        dt2, _ = _time_steps(tr2, data, args, dev, world)
        if tr2.net.agg_per_step != n_agg:
            side = {"ms_per_step": dt2 / args.steps * 1e3, "aggregations_per_step": tr2.net.agg_per_step,
                    "value": tr2.net.agg_per_step * e_unit * args.steps / dt2, "unit": "edges/s",
                    "note": ("the same model with a layer whose input is narrower than its output computing (A X) W "
                             "(layer 1 aggregates its 100-wide input: one aggregate forward, none backward) — NOT the "
                             "reference's association, reported beside the headline only") if not af_main else
                            "every layer A (X W) as gcn_conv.py:79 writes it"}
        del tr2
    routes = None
    if not pg.comm and getattr(pg, "route", None) == "cpp" and not getattr(args, "no_comparison", False) and not emul:
        # the same step through the other host implementation (the ctypes engine's autograd Functions), so that the line says
        # what the choice of route costs: both end in the same C ABI calls
        pg.route = "ctypes"
        try:
            tr3 = trainer(af_main)
            dt3, _ = _time_steps(tr3, data, args, dev, world)
            del tr3
        finally:
            pg.route = "cpp"
        routes = {"torch.ops.ggl (headline)": round(dt / args.steps * 1e3, 4), "ctypes engine": round(dt3 / args.steps * 1e3, 4),
                  "unit": "ms_per_step"}
    del tr

    # dominant kernel (K = hidden), hipEvents on the launch stream
    K = args.hidden
    rf = ms_op = gp_t = None
    if not getattr(args, "no_roofline", False):
        ms_op, launches, gp_t, rows_t, use_halo = dominant_spmm(pg, eng, K, gen, dev)
        alg = gp_t.E * (4 * K + 8) + pg.n_local * (4 * K + 8)             # SURVEY §8d, per aggregate
        b_min = 4 * K * (rows_t + pg.n_local) + 8 * gp_t.E + 8 * pg.n_local   # every row once + ids + rowptr
        rf = roofline_block(
            f"row_reduce_kernel<float,4,SUM,SPMM> (CSR SpMM-sum, rank 0's {'halo-source' if use_halo else 'local-source'} "
            f"edge block: {gp_t.E} edges into {pg.n_local} rows from {rows_t} source rows; the K={K} aggregate runs as "
            f"{launches} launch(es) over {K // max(launches, 1)}-column blocks"
            + (f"; the {gp_t.fwd.n_long} rows longer than {gp_t.fwd.chunk} elements are summed in the reference's serial "
               f"order by hub_rows_f32_kernel on a side stream BESIDE each launch: a launch's duration is the later of the "
               f"two, its traffic the sum of both" if gp_t.fwd.n_long > 0 else "") + ")",
            launches, ms_op, alg, b_min, gp_t.E)

    kc = n_cls + (-n_cls) % 4
    per_row = 2 * (args.hidden * max(args.layers - 2, 0) + kc)
    cfg = {
        "workload": f"{args.workload}: {spec['dataset'] or 'tiny'}-sized {'R-MAT' if spec['gen'] == 'rmat' else 'hierarchical planted-community graph'}"
                    f", N={n_nodes}, E={E} directed incl. self-loops, features {f_in}->{args.hidden}x{args.layers - 1}->{n_cls}, "
                    f"edge order={args.order}, relabel={args.relabel}, full-graph GCN train step (fwd+bwd+Adam), "
                    f"{n_agg} aggregations/step ({'A (X W) in every layer, as gcn_conv.py:79' if not af_main else '(A X) W where the input is narrower'}), "
                    f"symmetric-norm edge weights precomputed (GCNConv norm='none' + calc_gcn_norm edge_weight)"
                    + (f"; DRY partition: this GPU plays rank {play} of {parts} (its {pg.n_local} rows, {pg.e_local} in-edges, "
                       f"{pg.n_halo} halo rows; send lists and buffers as in the {parts}-rank run, nothing on the wire); value "
                       f"counts the edges THIS rank aggregates" if parts else ""),
        "association": "A (X W)" if not af_main else "(A X) W where narrower",
        "hipgraph": ("the whole step (fwd + bwd + Adam) recorded once into a hipGraph, the timed steps are its replays"
                     if graphed else "no: eager launches"),
        "aggregations_per_step": n_agg,
        "route": getattr(pg, "route", None) if not pg.comm else "ctypes engine (partitioned: in-place / accumulating forms)",
        "routes": routes,
        "aggregate_first" if not af_main else "transform_first": side,
        "parallelism": (f"node-partition x{world}, 1-hop halo all-to-all-v, per-rank graph construction" if world > 1 else
                        (f"1 GPU playing rank {play} of {parts}" if parts else "1 GPU")),
        "rank0_local_edges": pg.e_local, "rank0_local_source_edges": pg.gp_loc.E, "rank0_halo_rows": pg.n_halo,
        "rank0_send_rows": pg.n_send, "rank0_owned_rows": pg.n_local,
        "rank0_peak_edges_during_build": stats.get("peak_edges"),
        # floats a halo row costs per step: layers 2.. exchange their K-wide rows forward and backward; layer 1
        # exchanges nothing (the input features' halo rows were fetched once at setup)
        "halo_floats_per_row_per_step": per_row,
        "rank0_halo_GB_per_step": round((pg.n_halo + pg.n_send) * 4 * per_row / 1e9, 3),
        "exchange": exchange, "setup_s": round(t_gen, 2), "loss": lsum}
    if parts:
        cfg["if_links_were_free_edges_per_s_all_ranks"] = n_agg * E * args.steps / dt
    out = {
        "metric": ("edges aggregated/sec, 3-layer GCN hidden=256 training step, ogbn-products-sized graph"
                   if args.workload == "products" else
                   f"edges aggregated/sec, {args.layers}-layer GCN hidden={args.hidden} training step, {args.workload}"),
        "value": value, "unit": "edges/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "strong",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "rccl_ranks": dist.get_world_size() if (world > 1 and dist.is_initialized()) else 1,
        "config": cfg, "roofline": None if emul else rf}

    # the other node orders ("report both"), same association, same step count: degree-sorted for the R-MAT
    # workloads; for the planted graph the order partition.cluster_order recovers from the random ids, and the
    # generator's own ("none": a dataset whose native order already carries its locality)
    also = getattr(args, "also_relabel", None)
    also = spec.get("also") if also in (None, "auto") else (None if also == "none" else also)
    also = [also] if isinstance(also, str) else list(also or [])
    also = [a for a in also if a != args.relabel]
    if (world == 1 and not parts and dev.type == "cuda" and args.workload == "products"
            and not getattr(args, "no_comparison", False)):
        out["config"]["norm_both"] = _norm_both_steps(pg, data, args, f_in, n_cls, dev)
    ctx = {"pg": pg, "data": data}
    if also and world == 1 and not parts and not getattr(args, "no_comparison", False):
        host_graph = None
        if getattr(args, "keep_host_graph", False):   # bench.py's cpu_baseline leg wants the main graph on the host
            host_graph = (torch.stack([pg.ei_loc[0] + pg.lo, pg.ei_loc[1] + pg.lo]).cpu().contiguous(), pg.w_loc.cpu())
        orderings = [{"relabel": args.relabel, "ms_per_step": out["ms_per_step"], "value": value,
                      "ms_per_aggregate_K%d" % K: ms_op}]
        del pg, data, gp_t
        ctx = {"host_graph": host_graph}
        for other in also:
            eng.clear_caches()
            if dev.type == "cuda":
                torch.cuda.empty_cache()
            pg, stats2, t2 = build(other)
            data = _gcn_data(pg, f_in, n_cls, args.seed, rank, dev, world)
            tr = trainer(af_main)
            dt_b, _ = _time_steps(tr, data, args, dev, world)
            ms_b, _, gp_b, _, _ = dominant_spmm(pg, eng, K, data[4], dev)
            entry = {"relabel": other, "ms_per_step": dt_b / args.steps * 1e3,
                     "value": tr.net.agg_per_step * pg.e_global * args.steps / dt_b,
                     "ms_per_aggregate_K%d" % K: ms_b, "setup_s": round(t2, 2), "E": pg.e_global,
                     "xcd_run_rows": gp_b.fwd.xcd_run}
            if "clusters" in stats2:
                entry["clusters"] = stats2["clusters"]
            orderings.append(entry)
            del tr, gp_b, pg, data
        out["config"]["orderings"] = orderings
    ctx["outputs"] = outputs
    return out, ctx


# ---------------------------------------------------------------------------------------------------------------
# gat: config 3
# ---------------------------------------------------------------------------------------------------------------
def _event_ms(fn, reps=9, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def pmc_probe_gat(args, dev, eng):
    from .synth import rmat_graph

    calibration_launches(eng, dev)
    n, e, _, _ = DATASETS["reddit"]
    ei = rmat_graph(n, e, seed=args.seed, device=dev)
    H, C = 8, 8
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(n, H, C, generator=g, device=dev)
    el, er = torch.randn(n, H, generator=g, device=dev), torch.randn(n, H, generator=g, device=dev)
    with torch.no_grad():
        for _ in range(4):
            eng.gat_fused(ei, el, er, x, 0.2)
    torch.cuda.synchronize()
    print("pmc-probe: gat forward 8x8 on the Reddit-sized graph aggregates=4 dispatches=4", flush=True)


def run_gat(args, dev, rank, world, eng=None):
    """Config 3: 2-layer, 8-head GAT (602 -> 8 x 8 -> 41 classes, the last layer averages its heads; feature and
    attention dropout 0.6 — examples/gat/gat_trainer.py defaults) on the Reddit-sized graph, one full-graph
    training step (fwd + bwd + Adam) through FusedGATConv = the fused edge-softmax + aggregate kernels.
    args.amp (torch.bfloat16 / torch.float16; bench.py has no such flag: f32) runs the forward under torch.autocast — the
    8 x 8 layer's panel is then stored in 16 bits (tools/gat16_bench.py)."""
    from .layers import GATModel
    from .synth import rmat_graph

    if world != 1:
        raise SystemExit("bench.py: --workload reddit-gat is BASELINE config 3, a single-GPU configuration (--gpus 1)")
    eng = eng if eng is not None else _default_engine()
    n, e, f_in, n_cls = DATASETS["reddit"]
    t0 = time.perf_counter()
    ei = rmat_graph(n, e, seed=args.seed, device=dev)
    torch.cuda.synchronize()
    t_gen = time.perf_counter() - t0
    E = int(ei.shape[1])
    g = torch.Generator(device=dev).manual_seed(args.seed)
    x = torch.randn(n, f_in, generator=g, device=dev)
    y = torch.randint(0, n_cls, (n,), generator=g, device=dev)
    tidx = torch.arange(0, n, 3, device=dev)
    torch.manual_seed(args.seed)
    H, C = 8, 8
    net = GATModel(f_in, C, n_cls, H, 0.6, 2, fused=True).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=0.005, weight_decay=5e-4)

    amp = getattr(args, "amp", None)
    scaler = torch.amp.GradScaler("cuda") if amp == torch.float16 else None

    def step():
        net.train()
        opt.zero_grad(set_to_none=True)
        if amp is None:
            loss = F.cross_entropy(net(x, ei, n)[tidx], y[tidx])
        else:
            with torch.autocast("cuda", dtype=amp):
                out = net(x, ei, n)
            loss = F.cross_entropy(out[tidx].float(), y[tidx])
        if scaler is not None:
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        else:
            loss.backward()
            opt.step()
        return loss

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    outputs = step_outputs(net, loss) if getattr(args, "dump_outputs", None) else None
    walks = 4     # 2 layers x (forward + backward) walks over every edge (the backward of a layer is two walks — by
    #               destination and by source — counted as one aggregation like a GCN layer's transposed SpMM)
    rf = ms_k = None
    if not getattr(args, "no_roofline", False):
        # dominant kernel: the forward walk of the 8 x 8 layer
        xg = torch.randn(n, H, C, generator=g, device=dev)
        el, er = torch.randn(n, H, generator=g, device=dev), torch.randn(n, H, generator=g, device=dev)
        with torch.no_grad():
            ms_k = _event_ms(lambda: eng.gat_fused(ei, el, er, xg, 0.2))
        alg = E * (4 * H * C + 4 * H + 4) + n * (4 * H * C + 8 * H + 8)
        b_min = n * (4 * H * C + 4 * H) + n * (4 * H * C + 4 * H) + 4 * E + 8 * n
        rf = roofline_block("gat_fwd2_kernel (fused edge-softmax + weighted aggregate, forward walk of the 8 x 8 layer; "
                            "one launch + the hub-chunk combine)", 1, ms_k, alg, b_min, E)
    out = {"metric": "edges aggregated/sec, 2-layer 8-head GAT training step, Reddit-sized graph (fused edge-softmax + aggregate)",
           "value": walks * E * args.steps / dt, "unit": "edges/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
           "dtype": "f32" if amp is None else f"autocast({str(amp).replace('torch.', '')})", "data": "synthetic", "rccl_ranks": 1,
           "config": {"workload": f"reddit-gat: Reddit-sized R-MAT N={n}, E={E} directed incl. self-loops, GATModel({f_in} -> "
                                  f"{H}x{C} -> {n_cls}, heads averaged in the output layer), feature + attention dropout 0.6, "
                                  f"full-graph train step (fwd+bwd+Adam), {walks} edge walks/step",
                      "walks_per_step": walks, "fused_gat_forward_ms": ms_k, "setup_s": round(t_gen, 2),
                      "loss": float(loss), "parallelism": "1 GPU"},
           "roofline": rf}
    return out, {"ei": ei, "n": n, "outputs": outputs}


# ---------------------------------------------------------------------------------------------------------------
# sage: config 4
# ---------------------------------------------------------------------------------------------------------------
def run_sage(args, dev, rank, world, eng=None):
    """Config 4: GraphSAGE mini-batches (2048 seeds, fan-out [25, 10], hidden 256) on the products-sized graph:
    static-shape device sampler + SAGEConv(mean) with the fused epilogue, the whole step replayed as one hipGraph
    (world == 1); with world > 1 every rank is a replica sampling its own seeds, gradients averaged by one flat
    all-reduce per step ("replicas only") — scaling = weak."""
    from .sampler import BlockSampler
    from .synth import rmat_graph
    from .trainer import SAGEBlockTrainer

    eng = eng if eng is not None else _default_engine()
    n, e, f_in, n_cls = DATASETS["products"]
    t0 = time.perf_counter()
    ei = rmat_graph(n, e, seed=args.seed, device=dev)
    g = torch.Generator(device=dev).manual_seed(args.seed + 31 * rank)
    x = torch.randn(n, f_in, generator=g, device=dev)
    y = torch.randint(0, n_cls, (n,), generator=g, device=dev)
    B = 2048
    bs = BlockSampler(ei, [25, 10], num_nodes=n, eng=eng)
    caps = bs.calibrate(B, trials=8, slack=1.25)
    tr = SAGEBlockTrainer(bs, f_in, args.hidden, n_cls, device=dev, caps=caps, world=world)
    torch.cuda.synchronize()
    t_gen = time.perf_counter() - t0
    batches = [torch.randperm(n, generator=g, device=dev)[:B].contiguous() for _ in range(max(args.steps, 1))]
    seeds = batches[0].clone()
    # world == 1: the whole step is one hipGraph; replicas: two graphs around the eager gradient all-reduce
    # (SAGEBlockTrainer.capture); --hipgraph off: everything eager (the offline GEMM selection pass)
    graphed = getattr(args, "hipgraph", "auto") != "off" and dev.type == "cuda"
    if graphed:
        tr.capture(x, y, seeds)

        def run(b):
            seeds.copy_(b)
            return tr.replay()
    else:
        def run(b):
            return tr.step(x, y, b)
    for i in range(args.warmup):
        run(batches[i % len(batches)])
    _sync(dev, world)
    t0 = time.perf_counter()
    for b in batches[: args.steps]:
        loss = run(b)
    _sync(dev, world)
    dtt = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(dtt, op=dist.ReduceOp.MAX)
    dt = float(dtt)
    outputs = step_outputs(tr.net, loss) if getattr(args, "dump_outputs", None) else None
    # what one batch aggregates: valid edges of its two blocks (outermost first)
    _, blocks, _ = bs.sample(batches[0], caps=caps)
    valid = [(int(b.counts[0]), int(b.counts[1])) for b in blocks]   # (source rows, edges) per block
    e_batch = sum(v[1] for v in valid)
    rf = None
    if not getattr(args, "no_roofline", False):
        # dominant aggregate: the outer block's mean over 100-wide input rows (layer 1 aggregates before it transforms)
        blk = blocks[0]
        xin = torch.randn(blk.n_src_cap, f_in, generator=g, device=dev)
        yout = torch.empty(blk.n_dst_cap, f_in, device=dev)
        ms_k = _event_ms(lambda: eng.spmm_epi_into(blk.plan, blk.col, None, xin, yout, mean=True), reps=21)
        alg = valid[0][1] * (4 * f_in + 4) + blk.n_dst_cap * (4 * f_in + 8)
        b_min = 4 * f_in * (valid[0][0] + blk.n_dst_cap) + 4 * valid[0][1] + 8 * blk.n_dst_cap
        rf = roofline_block(f"row_reduce_kernel<float,4,MEAN,SPMM_EPI> (the outer block's mean aggregate: {valid[0][1]} sampled "
                            f"edges, {f_in}-wide rows; a {ms_k * 1e3:.0f} us kernel — the replayed step is bound by its ~110 small "
                            f"kernels, not by HBM)", 1, ms_k, alg, b_min, valid[0][1])
    out = {"metric": "sampled-block edges aggregated/sec, GraphSAGE mini-batch training (2048 seeds, fan-out [25,10]), "
                     "products-sized graph",
           "value": world * e_batch * args.steps / dt, "unit": "edges/s", "n_gpus": world, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "rccl_ranks": dist.get_world_size() if (world > 1 and dist.is_initialized()) else 1,
           "config": {"workload": f"sage-minibatch: products-sized R-MAT N={n}, E={int(ei.shape[1])}, GraphSAGE {f_in}->"
                                  f"{args.hidden}->{n_cls}, SAGEConv(mean), {B} seeds/batch/GPU, fan-out [25,10]; a step = "
                                  f"sample 2 hops on the device + gather + fwd + bwd + Adam"
                                  + (" as ONE replayed hipGraph" if graphed and world == 1 else
                                     (", two replayed hipGraphs around the replicas' eager gradient all-reduce" if graphed else
                                      (", eager launches" if world == 1 else ", eager replicas + gradient all-reduce"))),
                      "seeds_per_s": world * B * args.steps / dt, "block_valid_src_rows_edges": valid,
                      "block_capacities": [list(c) for c in caps], "overflowed_hops": bs.overflow_count(),
                      "parallelism": f"{world} replica(s)", "setup_s": round(t_gen, 2), "loss": float(loss)},
           "roofline": rf}
    return out, {"blocks": blocks, "valid": valid, "outputs": outputs}


RUNNERS = {"gcn": run_gcn, "gat": run_gat, "sage": run_sage}
PROBES = {"gcn": pmc_probe_gcn, "gat": pmc_probe_gat}
