"""The autograd formulas of the ctypes route, defined once: every Function takes the Engine it runs on as the first argument of
``forward`` (``SpMMSum.apply(eng, gp, w, x)``), keeps it on ``ctx`` for ``backward`` and returns None for it there.  All state — plan
caches, the dropout RNG, stats, the A/B switches — stays on the Engine; nothing here is per engine.

This is the part of the reference that lives in ``gammagl/mpops/torch_ext/src/*.cpp`` — the seven ``torch::autograd::Function``s
(src/segment_sum.cpp:35-54, src/segment_mean.cpp:36-63, src/segment_max.cpp:37-61, src/gspmm.cpp:26-260) — plus the fused
ops of this backend.  The class names are what ``grad_fn`` and profiler traces show.
"""
import ctypes
import math

import torch
from torch.autograd.function import once_differentiable

from ._lib import _DTYPE_CODE, _X16_DTYPES, _ptr


def _flat(bias, add=None):
    """(bias as one contiguous row, add contiguous) for an epilogue launch; None stays None."""
    return (bias.contiguous().reshape(-1) if bias is not None else None), (add.contiguous() if add is not None else None)


def segment_function(op):
    """SegmentSum / SegmentMean (src/segment_sum.cpp:35-54, src/segment_mean.cpp:36-63): one body, the reduce as its
    parameter.  The mean also keeps the plan's rowptr: its backward divides by the segment's length."""

    class Segment(torch.autograd.Function):
        @staticmethod
        def forward(ctx, eng, x, ids, N):
            ctx.eng = eng
            plan = eng.seg_plan(ids, N)
            out, _ = eng._segment_fwd(op, x, plan)
            ctx.save_for_backward(ids, *((plan.rowptr,) if op == "mean" else ()))
            ctx.x_shape = x.shape
            return out

        @staticmethod
        def backward(ctx, g):
            ids, *rowptr = ctx.saved_tensors
            return None, ctx.eng._segment_bwd(g, ids, ctx.x_shape, *rowptr), None, None

    Segment.__name__ = Segment.__qualname__ = "Segment" + op.capitalize()
    return Segment


SegmentSum, SegmentMean = segment_function("sum"), segment_function("mean")


class SegmentMax(torch.autograd.Function):  # src/segment_max.cpp:37-61
    @staticmethod
    def forward(ctx, eng, x, ids, N):
        ctx.eng = eng
        plan = eng.seg_plan(ids, N)
        out, arg = eng._segment_fwd("max", x, plan)
        ctx.save_for_backward(arg)
        ctx.x_shape = x.shape
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, g, _garg):
        eng = ctx.eng
        (arg,) = ctx.saved_tensors
        g = g.contiguous()
        E = ctx.x_shape[0]
        K = int(math.prod(ctx.x_shape[1:]))
        gin = torch.empty(ctx.x_shape, dtype=g.dtype, device=g.device)
        eng._check(eng.lib.ggl_segment_max_bwd(eng._code(g), _ptr(g), _ptr(arg), E,
                                               int(arg.shape[0]), K, _ptr(gin),
                                               eng._stream(g.device)))
        return None, gin, None, None


class SegmentMulti(torch.autograd.Function):  # pna_conv.py:159-181: several statistics of the same rows, one walk each way
    @staticmethod
    def forward(ctx, eng, x, plan, codes, C, empty_zero, need_grad):
        ctx.eng = eng   # (need_grad: x requires grad and grad mode is on — the caller's grad mode, which forward() cannot see)
        sq = 4 in codes or 5 in codes
        out, mean, amin, amax = eng._segment_multi_fwd(x, plan, codes, C, empty_zero, want_mean=need_grad and sq)
        ctx.plan, ctx.codes, ctx.C, ctx.K = plan, codes, C, int(x.shape[1])
        # only what the requested statistics' backward reads: x and mean for var / std, out for std, the witnesses for min / max
        ctx.names = ()
        if need_grad:
            saved = {"x": x if sq else None, "mean": mean, "out": out if 5 in codes else None, "argmin": amin, "argmax": amax}
            ctx.names = tuple(k for k, v in saved.items() if v is not None)
            ctx.save_for_backward(*(saved[k] for k in ctx.names))
        eng.stats["segment_multi"] = {"route": "fused", "saved": ctx.names}
        ctx.mark_non_differentiable(*(t for t in (amin, amax) if t is not None))
        return out, amin, amax

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gmin, _gmax):
        t = dict(zip(ctx.names, ctx.saved_tensors))
        gx = ctx.eng._segment_multi_bwd(g, t.get("x"), t.get("out"), t.get("mean"), t.get("argmin"), t.get("argmax"),
                                        ctx.plan, ctx.K, ctx.C, ctx.codes)
        return None, gx, None, None, None, None, None


class SegmentSoftmax(torch.autograd.Function):  # utils/softmax.py:29-35 as one op each way
    @staticmethod
    def forward(ctx, eng, x, plan):
        ctx.eng = eng
        y = eng._softmax_fwd(x, plan)
        ctx.save_for_backward(y)
        ctx.plan = plan
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        eng = ctx.eng
        (y,) = ctx.saved_tensors
        return None, eng._softmax_bwd(y, g, ctx.plan), None


def spmm_function(op):
    """SpMMSum / SpMMMean (src/gspmm.cpp:26-80, 82-141): one body, the reduce as its parameter.  An extension
    over the reference (gspmm.cpp:30 marks the weight non-differentiable): a weight that requires grad gets its
    gradient (Engine._spmm_grad_w); only then is x saved, a constant weight costs what it did."""

    class SpMM(torch.autograd.Function):
        @staticmethod
        def forward(ctx, eng, gp, w, x, out_dtype=None):
            ctx.eng = eng
            out, _ = eng._spmm_fwd(op, gp.fwd, gp.col, w, x, gp.N_dst, out_dtype=out_dtype)
            ctx.gp, ctx.w, ctx.x_dtype = gp, w, x.dtype
            if w is not None and ctx.needs_input_grad[2]:
                ctx.save_for_backward(x)
            return out

        @staticmethod
        def backward(ctx, g):
            eng = ctx.eng
            gx = gw = None
            if ctx.needs_input_grad[3]:
                gx = eng._spmm_bwd_x(ctx.gp, ctx.w, g, ctx.x_dtype, op == "mean")
            if ctx.w is not None and ctx.needs_input_grad[2]:
                gw = eng._spmm_grad_w(ctx.gp, ctx.saved_tensors[0], g, op == "mean").view(ctx.w.shape)
            return None, None, gw, gx, None

    SpMM.__name__ = SpMM.__qualname__ = "SpMM" + op.capitalize()
    return SpMM


SpMMSum, SpMMMean = spmm_function("sum"), spmm_function("mean")


class SpMMMax(torch.autograd.Function):  # src/gspmm.cpp:143-202
    @staticmethod
    def forward(ctx, eng, gp, w, x):
        ctx.eng = eng
        out, arg = eng._spmm_fwd("max", gp.fwd, gp.col, w, x, gp.N_dst)
        ctx.gp, ctx.w = gp, w
        ctx.save_for_backward(arg)
        return out

    @staticmethod
    def backward(ctx, g):
        eng = ctx.eng
        gp = ctx.gp
        (arg,) = ctx.saved_tensors
        gx, _ = eng._spmm_fwd("max_bwd", gp.bwd, gp.colT, ctx.w, g.contiguous(), gp.N_src,
                              aux=arg, gp=gp)
        return None, None, None, gx


def _edge_dot(eng, gp, x, g, out):
    """out[e, h] = <x[src(e), h, :], g[dst(e), h, :]> in f32, channels ascending, e the CALLER's edge number: bspmm's weight
    gradient, and the logits of dot-product attention (x = k, g = q)."""
    H, C = int(x.shape[1]), int(x.shape[2])
    # a plan built from the caller's CSR has no COO edge list to walk (gp.index is None): it always takes the
    # sorted route, whose plain kernel covers any channel count
    if gp.index is None or (eng.gradw_sorted and eng.lib.ggl_policy_gradw_sorted(H, C)):
        # along the destination-sorted forward plan, strips staged through LDS (edgedot.hip): the g rows
        # of a batch are a handful of rows, only x[src] is a random gather — and a coalesced one
        sb = eng.lib.ggl_bspmm_grad_w_sorted_scratch_bytes(gp.E, gp.N_dst, H, C)
        scratch = torch.empty(sb // 4, dtype=torch.float32, device=g.device) if sb else None
        cs = gp.fwd.c_struct(None)
        eng._check(eng.lib.ggl_bspmm_grad_w_sorted(ctypes.byref(cs), _ptr(gp.col), _ptr(gp.rowidx), _ptr(x),
                                                   _ptr(g), H, C, _ptr(out), _ptr(scratch),
                                                   eng._stream(g.device)))
    else:
        eng._check(eng.lib.ggl_bspmm_grad_w(_ptr(gp.index), _ptr(x), _ptr(g), gp.E, H, C,
                                            _ptr(out), eng._stream(g.device)))
    return out


class BSpMMSum(torch.autograd.Function):  # src/gspmm.cpp:204-260
    @staticmethod
    def forward(ctx, eng, gp, w, x):
        ctx.eng = eng
        out = eng._bspmm_fwd(gp.fwd, gp.col, w, x, gp.N_dst)
        ctx.gp = gp
        ctx.save_for_backward(w, x)
        return out

    @staticmethod
    def backward(ctx, g):
        eng = ctx.eng
        gp = ctx.gp
        w, x = ctx.saved_tensors
        g = g.contiguous()
        gx = eng._bspmm_fwd(gp.bwd, gp.colT, w, g, gp.N_src)
        gw = _edge_dot(eng, gp, x, g, torch.empty_like(w))
        # the reference returns grad_weight although it marked weight non-differentiable
        # (gspmm.cpp:208,259): w.grad is populated there, and here.
        return None, None, gw, gx


class GATFused(torch.autograd.Function):
    """edge-softmax + aggregate in one kernel (gat_conv.py:103-112 + softmax.py:29-35).  bf16 / f16 x (an
    extension, ggl_gat_fused_*_x16): the general kernels on 16-bit rows, f32 softmax and sums, out in x's dtype
    (or f32 with out_dtype); the backward reads x16 and the out RETURNED here, no f32 copy of either is kept."""

    @staticmethod
    def forward(ctx, eng, gp, el, er, x, slope, p_drop=0.0, out_dtype=None):
        ctx.eng = eng
        dev = x.device
        N, H, C = gp.N_dst, int(x.shape[1]), int(x.shape[2])
        x16 = x.dtype in _X16_DTYPES
        out = torch.empty((N, H, C), dtype=(out_dtype or x.dtype) if x16 else torch.float32, device=dev)
        rmax = torch.empty((N, H), dtype=torch.float32, device=dev)
        rden = torch.empty((N, H), dtype=torch.float32, device=dev)
        part = eng._gat_partial(gp.fwd, H, C, dev)
        cs = gp.fwd.c_struct(part)
        rng, rng_used = eng._draw(dev, p_drop)
        fast = bool(not x16 and eng.gat_fast and eng.lib.ggl_gat_fast_supported(H, C))
        if x16:
            eng._check(eng.lib.ggl_gat_fused_fwd_x16(
                ctypes.byref(cs), _ptr(gp.col), _ptr(el), _ptr(er), _DTYPE_CODE[x.dtype], _ptr(x), float(slope),
                H, C, float(p_drop), _ptr(rng), _DTYPE_CODE[out.dtype], _ptr(out), _ptr(rmax), _ptr(rden),
                eng._stream(dev)))
        elif fast:
            eng._check(eng.lib.ggl_gat_fast_fwd(ctypes.byref(cs), _ptr(gp.col), _ptr(el), _ptr(er), _ptr(x),
                                                int(x.shape[0]), float(slope), H, C, float(p_drop), _ptr(rng),
                                                _ptr(out), _ptr(rmax), _ptr(rden), eng._stream(dev)))
        else:
            eng._check(eng.lib.ggl_gat_fused_fwd(ctypes.byref(cs), _ptr(gp.col), _ptr(el), _ptr(er),
                                                 _ptr(x), float(slope), H, C, float(p_drop), _ptr(rng),
                                                 _ptr(out), _ptr(rmax), _ptr(rden), eng._stream(dev)))
        ctx.fast = fast
        ctx.gp, ctx.slope, ctx.p_drop, ctx.rng_used = gp, float(slope), float(p_drop), rng_used
        ctx.save_for_backward(el, er, x, out, rmax, rden)
        return out

    @staticmethod
    def backward(ctx, g):
        eng = ctx.eng
        gp = ctx.gp
        el, er, x, out, rmax, rden = ctx.saved_tensors
        g = g.contiguous()
        dev = g.device
        H, C = int(x.shape[1]), int(x.shape[2])
        st = eng._stream(dev)
        x16 = x.dtype in _X16_DTYPES
        if x16 and g.dtype != out.dtype:
            g = g.to(out.dtype)
        if ctx.fast:  # both walks recompute alpha / de from per-row constants: no [E, H, 2] buffer
            bwd = gp.bwd
            stats = torch.empty((gp.N_dst, H, 4), dtype=torch.float32, device=dev)
            ger = torch.empty_like(er)
            gx = torch.empty((gp.N_src, H, C), dtype=torch.float32, device=dev)
            gel = torch.empty((gp.N_src, H), dtype=torch.float32, device=dev)
            part_f = eng._gat_fast_bwd_dst_partial(gp.fwd, H, dev)
            part_t = eng._gat_bwd_src_partial(bwd, H, C, dev)
            cs, csT = gp.fwd.c_struct(part_f), bwd.c_struct(part_t)
            posT = gp.posT if ctx.p_drop > 0 else None
            eng._check(eng.lib.ggl_gat_fast_bwd(
                ctypes.byref(cs), _ptr(gp.col), ctypes.byref(csT), _ptr(gp.colT), _ptr(posT), _ptr(el),
                _ptr(er), _ptr(x), _ptr(g), _ptr(out), _ptr(rmax), _ptr(rden), ctx.slope, H, C, ctx.p_drop,
                _ptr(ctx.rng_used), _ptr(stats), _ptr(gx), _ptr(gel), _ptr(ger), st))
            return None, None, gel, ger, gx, None, None, None
        # alpha and de interleaved [E, H, 2]: the source-side walk fetches both with one 64-byte line
        ad = torch.empty((max(gp.E, 1), H, 2), dtype=torch.float32, device=dev)
        alpha, de = ad.data_ptr(), ad.data_ptr() + 4
        ger = torch.empty_like(er)
        part_f = eng._gat_bwd_dst_partial(gp.fwd, H, dev)  # must outlive the launch
        cs = gp.fwd.c_struct(part_f)
        xc, gc = _DTYPE_CODE.get(x.dtype), _DTYPE_CODE.get(g.dtype)
        if x16:
            eng._check(eng.lib.ggl_gat_fused_bwd_dst_x16(
                ctypes.byref(cs), _ptr(gp.col), _ptr(el), _ptr(er), xc, _ptr(x), gc, _ptr(g), gc, _ptr(out),
                _ptr(rmax), _ptr(rden), ctx.slope, H, C, ctx.p_drop, _ptr(ctx.rng_used), alpha, de, _ptr(ger),
                st))
        else:
            eng._check(eng.lib.ggl_gat_fused_bwd_dst(
                ctypes.byref(cs), _ptr(gp.col), None, _ptr(el), _ptr(er), _ptr(x),
                _ptr(g), _ptr(out), _ptr(rmax), _ptr(rden), ctx.slope, H, C, ctx.p_drop,
                _ptr(ctx.rng_used), alpha, de, _ptr(ger), None, st))
        bwd = gp.bwd
        gx = torch.empty((gp.N_src, H, C), dtype=x.dtype, device=dev)
        gel = torch.empty((gp.N_src, H), dtype=torch.float32, device=dev)
        part = eng._gat_bwd_src_partial(bwd, H, C, dev)
        csT = bwd.c_struct(part)
        if x16:
            eng._check(eng.lib.ggl_gat_fused_bwd_src_x16(ctypes.byref(csT), _ptr(gp.colT), _ptr(gp.posT),
                                                         alpha, de, gc, _ptr(g), H, C, xc, _ptr(gx), _ptr(gel),
                                                         st))
        else:
            eng._check(eng.lib.ggl_gat_fused_bwd_src(ctypes.byref(csT), _ptr(gp.colT), _ptr(gp.posT),
                                                     alpha, de, _ptr(g), H, C,
                                                     _ptr(gx), _ptr(gel), st))
        return None, None, gel, ger, gx, None, None, None


def _esa_forward(eng, gp, v, p_drop, z=None, launch=None):
    """The forward every logit attention op shares: out [N_dst, H, C], rowmax and rowden, the hub partial, the plan struct and
    the rng draw, then ggl_edge_softmax_agg_fwd on the given logits z — or launch(cs, rng, out, rmax, rden), a fused kernel
    of the same walk that forms its logits itself.  The launch happens here: cs points into the partial and the plan's
    tensors, which this frame keeps alive until the kernel is enqueued.  (out, rowmax, rowden, rng_used)."""
    dev = v.device
    N, H, C = gp.N_dst, int(v.shape[1]), int(v.shape[2])
    out = torch.empty((N, H, C), dtype=torch.float32, device=dev)
    rmax = torch.empty((N, H), dtype=torch.float32, device=dev)
    rden = torch.empty((N, H), dtype=torch.float32, device=dev)
    part = eng._gat_partial(gp.fwd, H, C, dev)
    cs = gp.fwd.c_struct(part)
    rng, rng_used = eng._draw(dev, p_drop)
    if launch is not None:
        launch(cs, rng, out, rmax, rden)
    else:
        eng._check(eng.lib.ggl_edge_softmax_agg_fwd(ctypes.byref(cs), _ptr(gp.col), _ptr(z), _ptr(v), H, C, float(p_drop),
                                                    _ptr(rng), _ptr(out), _ptr(rmax), _ptr(rden), eng._stream(dev)))
    return out, rmax, rden, rng_used


def _esa_backward(eng, gp, z, v, g, out, rmax, rden, p_drop, rng_used, need_gz, need_gv):
    """The backward every logit attention op shares, on the logits z the forward used: the destination walk (alpha, and gz
    in the caller's edge order only with need_gz), then — only with need_gv — the source walk.  (gz, gv), None where not
    needed."""
    g = g.contiguous()
    dev = g.device
    H, C = int(v.shape[1]), int(v.shape[2])
    st = eng._stream(dev)
    alpha = torch.empty((max(gp.E, 1), H), dtype=torch.float32, device=dev) if need_gv else None   # sorted positions
    gz = torch.empty_like(z) if need_gz else None                                                  # caller's order
    part_f = eng._gat_bwd_dst_partial(gp.fwd, H, dev)  # must outlive the launch
    cs = gp.fwd.c_struct(part_f)
    eng._check(eng.lib.ggl_edge_softmax_agg_bwd_dst(
        ctypes.byref(cs), _ptr(gp.col), _ptr(z), _ptr(v), _ptr(g), _ptr(out), _ptr(rmax), _ptr(rden), H, C,
        p_drop, _ptr(rng_used), _ptr(alpha), _ptr(gz), st))
    gv = None
    if need_gv:
        bwd = gp.bwd
        gv = torch.empty((gp.N_src, H, C), dtype=torch.float32, device=dev)
        part = eng._gat_bwd_src_partial(bwd, H, C, dev)
        csT = bwd.c_struct(part)
        eng._check(eng.lib.ggl_edge_softmax_agg_bwd_src(ctypes.byref(csT), _ptr(gp.colT), _ptr(gp.posT), _ptr(alpha),
                                                        _ptr(g), H, C, _ptr(gv), st))
    return gz, gv


def _logit_attention_forward(ctx, name, eng, gp, inputs, v, p_drop, keep_z, fused, compose, launch):
    """The forward of an op whose logits come from its `inputs` (DotAttention, GATv2Attention), values v.  fused: the op's
    kernel forms the logits inside the aggregate's walk, launch(z, cs, rng, out, rmax, rden), and stores them to z unless z is
    None; otherwise compose(z) fills z and ggl_edge_softmax_agg_fwd reads it.  z [E, H] exists only if a backward will read
    it, the caller asked for it, or the composed route needs it.  Returns (out, z or an empty tensor), z not differentiable."""
    need = any(ctx.needs_input_grad[2:5])
    z = None
    if need or keep_z or not fused:
        z = torch.empty((gp.E, int(v.shape[1])), dtype=torch.float32, device=v.device)
    if fused:
        out, rmax, rden, rng_used = _esa_forward(eng, gp, v, p_drop, launch=lambda *a: launch(z, *a))
    else:
        compose(z)
        out, rmax, rden, rng_used = _esa_forward(eng, gp, v, p_drop, z=z)
    eng.stats[name] = {"fused": fused, "logits_bytes": 0 if z is None else z.numel() * 4, "logits_saved": bool(need)}
    ctx.eng, ctx.gp, ctx.p_drop, ctx.rng_used = eng, gp, float(p_drop), rng_used
    if need:
        ctx.save_for_backward(z, *inputs, out, rmax, rden)
    zr = z if (keep_z and z is not None) else out.new_empty(0)
    ctx.mark_non_differentiable(zr)
    return out, zr


class EdgeSoftmaxAgg(torch.autograd.Function):
    """edge-softmax + aggregate on per-edge logits z [E, H] (ggl_edge_softmax_agg_*): GATFused's general f32 kernels with
    the logit read from z through the plan's perm.  The source walk runs only when x needs a gradient, gz is stored — by
    the destination walk itself, in the caller's edge order — only when z does."""

    @staticmethod
    def forward(ctx, eng, gp, z, x, p_drop=0.0):
        out, rmax, rden, rng_used = _esa_forward(eng, gp, x, p_drop, z=z)
        ctx.eng, ctx.gp, ctx.p_drop, ctx.rng_used = eng, gp, float(p_drop), rng_used
        ctx.save_for_backward(z, x, out, rmax, rden)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        z, x, out, rmax, rden = ctx.saved_tensors
        need_z, need_x = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        if not (need_z or need_x):
            return None, None, None, None, None
        gz, gx = _esa_backward(ctx.eng, ctx.gp, z, x, g, out, rmax, rden, ctx.p_drop, ctx.rng_used, need_z, need_x)
        return None, None, gz, gx, None


def _bspmm_by_perm(eng, plan, col, w, x, n_out):
    """bspmm_sum over `plan` with the weights read through its permutation in the kernel (w_by_pos = 0): for weights that
    live for one launch, which the sorted-weight cache should neither remember nor gather."""
    return eng._bspmm_fwd(plan, col, w, x, n_out, perm_override=plan.perm if plan.perm is not None else plan.wperm)


class DotAttention(torch.autograd.Function):
    """Scaled dot-product graph attention: z[e, h] = scale * <q[dst(e), h], k[src(e), h]>, then EdgeSoftmaxAgg on (z, v).
    Forward, fused route (ggl_dot_attn_fwd, GPU build, where ggl_dot_attn_supported and the policy say so): the dot is formed
    inside the aggregate's walk; z is stored — by that walk, in the caller's edge order — only when a backward will read it
    (or the caller asked for it), so a forward without grad touches no [E, H] array.  Composed route (any other shape, CPU
    tensors): z = scale * edge dot, chosen as BSpMMSum.backward chooses, then ggl_edge_softmax_agg_fwd.  Both routes run the
    same backward on the saved z: ggl_edge_softmax_agg_bwd_dst (alpha, gz), _bwd_src (gv), gs = gz * scale, gq = bspmm_sum
    (plan, gs, k), gk = bspmm_sum(planT, gs, q); a walk whose gradient nobody needs is skipped.
    Returns (out, z); z is not differentiable and is an empty tensor when it was not formed."""

    @staticmethod
    def forward(ctx, eng, gp, q, k, v, scale, p_drop=0.0, keep_z=False):
        H, C = int(v.shape[1]), int(v.shape[2])
        fused = bool(eng.dot_attn_fused and v.is_cuda and eng.lib.ggl_dot_attn_supported(H, C)
                     and eng.lib.ggl_policy_dot_attn_fused(H, C, gp.E, gp.N_src))

        def compose(z):
            _edge_dot(eng, gp, k, q, z).mul_(scale)   # one rounded f32 multiply per element

        def launch(z, cs, rng, out, rmax, rden):
            eng._check(eng.lib.ggl_dot_attn_fwd(ctypes.byref(cs), _ptr(gp.col), _ptr(q), _ptr(k), _ptr(v), float(scale), H, C,
                                                float(p_drop), _ptr(rng), _ptr(out), _ptr(rmax), _ptr(rden), _ptr(z),
                                                eng._stream(v.device)))

        ctx.scale = float(scale)
        return _logit_attention_forward(ctx, "dot_attention", eng, gp, (q, k, v), v, p_drop, keep_z, fused, compose, launch)

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gz_unused):
        eng = ctx.eng
        gp = ctx.gp
        need_q, need_k, need_v = ctx.needs_input_grad[2:5]
        if not (need_q or need_k or need_v):
            return (None,) * 8
        z, q, k, v, out, rmax, rden = ctx.saved_tensors
        need_z = need_q or need_k
        gs, gv = _esa_backward(eng, gp, z, v, g, out, rmax, rden, ctx.p_drop, ctx.rng_used, need_z, need_v)
        gq = gk = None
        if need_z:
            gs.mul_(ctx.scale)   # d z / d <q, k>
        if need_q:
            gq = _bspmm_by_perm(eng, gp.fwd, gp.col, gs, k, gp.N_dst)
        if need_k:
            gk = _bspmm_by_perm(eng, gp.bwd, gp.colT, gs, q, gp.N_src)
        return None, None, gq, gk, gv, None, None, None


GATV2_BLOCK_BYTES = 256 << 20   # the composed route's [E_block, H, C] f32 scratch is at most this large


def _gatv2_logits(gp, xl, xr, att, slope, z):
    """z[e, h] = sum_c att[h, c] * leaky_relu(xl[src(e), h, c] + xr[dst(e), h, c]) in the caller's edge order, formed by torch
    under no_grad in edge blocks of at most GATV2_BLOCK_BYTES of [E_block, H, C]: the composed route's logits."""
    H, C = int(xl.shape[1]), int(xl.shape[2])
    if gp.index is not None:
        src, dst = gp.index[0], gp.index[1]
    else:   # a plan built from the caller's CSR: its edge order is the CSR's
        src = gp.col.long()
        dst = torch.repeat_interleave(torch.arange(gp.N_dst, device=xl.device), gp.fwd.counts())
    block = max(1, GATV2_BLOCK_BYTES // (4 * H * C))
    with torch.no_grad():
        for b in range(0, gp.E, block):
            s = xl[src[b:b + block]] + xr[dst[b:b + block]]
            z[b:b + block] = (att * torch.nn.functional.leaky_relu(s, slope)).sum(-1)
    return z


def _gatv2_logit_bwd(eng, plan, col, other, self_, gz, att, slope, add=None, want_rows=False):
    """ggl_gatv2_logit_bwd over `plan` (include/ggl_mpops.h): (g_self, att_rows or None).  gz is read through the plan's
    permutation in the kernel, as _bspmm_by_perm reads a weight."""
    dev = self_.device
    H, C = int(self_.shape[1]), int(self_.shape[2])
    perm = plan.perm if plan.perm is not None else plan.wperm
    part = eng._hub_partial(plan, lambda n: eng.lib.ggl_gatv2_logit_bwd_partial_bytes(n, H, C, 1 if want_rows else 0), dev)
    cs = plan.c_struct(part, perm)
    g_self = torch.empty_like(self_)
    rows = torch.empty_like(self_) if want_rows else None
    eng._check(eng.lib.ggl_gatv2_logit_bwd(ctypes.byref(cs), _ptr(col), _ptr(other), _ptr(self_), _ptr(gz), _ptr(att),
                                           float(slope), H, C, _ptr(add), _ptr(g_self), _ptr(rows), eng._stream(dev)))
    return g_self, rows


class GATv2Attention(torch.autograd.Function):
    """GATv2's additive attention: z[e, h] = sum_c att[h, c] * LeakyReLU(xl[src(e), h, c] + xr[dst(e), h, c]), then
    EdgeSoftmaxAgg on (z, xl).  Forward, fused route (ggl_gatv2_fwd, GPU build, where ggl_gatv2_supported and the policy say
    so): the logit is formed inside the aggregate's walk from the value row it gathers; z is stored — by that walk, in the
    caller's edge order — only when a backward will read it (or the caller asked for it), so a forward without grad touches
    no [E, H] array.  Composed route (any other shape, CPU tensors): _gatv2_logits in edge blocks, then
    ggl_edge_softmax_agg_fwd.  Both routes run the same backward on the saved z: ggl_edge_softmax_agg_bwd_dst (alpha, gz),
    _bwd_src (gv), then ggl_gatv2_logit_bwd on the forward plan (g_xr and R, g_att = colsum(R)) and on the transposed plan
    with add = gv (the whole g_xl); a walk whose gradient nobody needs is skipped.  No [E, H, C] array in either.
    Returns (out, z); z is not differentiable and is an empty tensor when it was not formed."""

    @staticmethod
    def forward(ctx, eng, gp, xl, xr, att, slope, p_drop=0.0, keep_z=False):
        H, C = int(xl.shape[1]), int(xl.shape[2])
        fused = bool(eng.gatv2_fused and xl.is_cuda and eng.lib.ggl_gatv2_supported(H, C)
                     and eng.lib.ggl_policy_gatv2_fused(H, C, gp.E, gp.N_src))

        def compose(z):
            _gatv2_logits(gp, xl, xr, att, slope, z)

        def launch(z, cs, rng, out, rmax, rden):
            eng._check(eng.lib.ggl_gatv2_fwd(ctypes.byref(cs), _ptr(gp.col), _ptr(xl), _ptr(xr), _ptr(att), float(slope), H, C,
                                             float(p_drop), _ptr(rng), _ptr(out), _ptr(rmax), _ptr(rden), _ptr(z),
                                             eng._stream(xl.device)))

        ctx.slope = float(slope)
        return _logit_attention_forward(ctx, "gatv2_attention", eng, gp, (xl, xr, att), xl, p_drop, keep_z, fused, compose,
                                        launch)

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gz_unused):
        eng = ctx.eng
        gp = ctx.gp
        need_l, need_r, need_a = ctx.needs_input_grad[2:5]
        if not (need_l or need_r or need_a):
            return (None,) * 8
        z, xl, xr, att, out, rmax, rden = ctx.saved_tensors
        H, C = int(xl.shape[1]), int(xl.shape[2])
        gz, gv = _esa_backward(eng, gp, z, xl, g, out, rmax, rden, ctx.p_drop, ctx.rng_used, True, need_l)
        gl = gr = ga = None
        if need_r or need_a:
            gr, rows = _gatv2_logit_bwd(eng, gp.fwd, gp.col, xl, xr, gz, att, ctx.slope, None, need_a)
            if need_a:
                ga = eng.colsum(rows.reshape(gp.N_dst, H * C)).reshape(H, C)
            if not need_r:
                gr = None
        if need_l:
            gl, _ = _gatv2_logit_bwd(eng, gp.bwd, gp.colT, xr, xl, gz, att, ctx.slope, gv, False)
        return None, None, gl, gr, ga, None, None, None


class BiasAdd(torch.autograd.Function):
    """out = x + bias (bias broadcast over rows); d bias = column sums of the gradient."""

    @staticmethod
    def forward(ctx, eng, x, bias):
        ctx.eng = eng
        ctx.bias_shape = bias.shape
        return x + bias

    @staticmethod
    def backward(ctx, g):
        eng = ctx.eng
        gb = eng.colsum(g.reshape(g.shape[0], -1)).reshape(ctx.bias_shape)
        return None, g, gb


class BiasAct(torch.autograd.Function):
    """y = dropout(relu(a + bias)) in one kernel; backward rebuilds the mask from y and reduces
    the bias gradient in the same pass (csrc/epilogue.hip)."""

    @staticmethod
    def forward(ctx, eng, a, bias, relu, p_drop):
        ctx.eng = eng
        a = a.contiguous()
        rng, rng_used = eng._draw(a.device, p_drop)
        y = eng._epi_fwd(a, bias, relu, p_drop, rng)
        ctx.epi = (relu, p_drop, rng_used, None if bias is None else bias.shape)   # _epi_bwd's arguments after (g, y)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        eng = ctx.eng
        (y,) = ctx.saved_tensors
        ga, gb = eng._epi_bwd(g, y, *ctx.epi)
        return None, ga, gb, None, None


class SpMMEpi(torch.autograd.Function):
    """y = dropout(relu(reduce(A x) + add + bias)), reduce = sum | mean, in ONE kernel (ggl_spmm_epi_ex):
    GCNConv's "+ bias" (gcn_conv.py:105-106) and SAGEConv's "mean + fc_self(x_dst) + bias -> act"
    (sage_conv.py:100-108) applied to each finished row in registers.  bf16 / f16 x and add (ggl_spmm_epi_x16): the same f32
    operations, y rounded once to x's dtype (or f32 with out_dtype); the backward is the f32 one step by step on the stored
    values — ga and gx in x's dtype, gbias and gw f32."""

    @staticmethod
    def forward(ctx, eng, gp, w, x, mean, add, bias, relu, p_drop, out_dtype=None):
        ctx.eng = eng
        dev = x.device
        K = int(x.shape[1])
        y = torch.empty((gp.N_dst, K), dtype=out_dtype or x.dtype, device=dev)
        ctx.x_dtype = x.dtype
        rng, rng_used = eng._draw(dev, p_drop)
        b, a = _flat(bias, add)
        eng.spmm_epi_into(gp.fwd, gp.col, w, x, y, mean=mean, add=a, bias=b, relu=relu, p_drop=p_drop, rng=rng)
        ctx.gp, ctx.w, ctx.mean, ctx.has_add = gp, w, bool(mean), add is not None
        ctx.epi = (relu, p_drop, rng_used, None if bias is None else bias.shape)
        # a learnable weight's gradient is the edge-dot of x with the pre-activation gradient: x is kept for it alone
        ctx.want_gw = w is not None and ctx.needs_input_grad[2]
        ctx.save_for_backward(y, *((x,) if ctx.want_gw else ()))
        return y

    @staticmethod
    def backward(ctx, g):
        eng = ctx.eng
        y = ctx.saved_tensors[0]
        ga, gb = eng._epi_bwd(g, y, *ctx.epi)
        gp = ctx.gp
        gx = gw = None
        if ctx.needs_input_grad[3]:
            gx = eng._spmm_bwd_x(gp, ctx.w, ga, ctx.x_dtype, ctx.mean)
        if ctx.want_gw:
            gw = eng._spmm_grad_w(gp, ctx.saved_tensors[1], ga, ctx.mean).view(ctx.w.shape)
        gadd = (ga if ga.dtype == ctx.x_dtype else ga.to(ctx.x_dtype)) if ctx.has_add else None
        return None, None, gw, gx, None, gadd, gb, None, None, None


class SegmentEpi(torch.autograd.Function):
    """The same epilogue on segment_sum / segment_mean of f32 messages x[E, K] (ggl_segment_epi): the
    message() + aggregate() route of a sampled SAGEConv block."""

    @staticmethod
    def forward(ctx, eng, x, ids, N, mean, add, bias, relu):
        ctx.eng = eng
        dev = x.device
        plan = eng.seg_plan(ids, N)
        K = int(x.shape[1])
        if int(x.shape[0]) != plan.E:
            raise IndexError("fisrt dimension of x and index should be same")
        y = torch.empty((plan.N, K), dtype=torch.float32, device=dev)
        part = eng._partial(plan, torch.float32, K, False, dev)
        cs = plan.c_struct(part)
        b, a = _flat(bias, add)
        eng._check(eng.lib.ggl_segment_epi(_ptr(x), ctypes.byref(cs), K, int(bool(mean)), _ptr(a), 0, _ptr(b),
                                           int(bool(relu)), 0.0, None, _ptr(y), eng._stream(dev)))
        ctx.mean, ctx.has_add, ctx.x_shape = bool(mean), add is not None, x.shape
        ctx.epi = (relu, 0.0, None, None if bias is None else bias.shape)
        ctx.save_for_backward(y, ids, plan.rowptr)
        return y

    @staticmethod
    def backward(ctx, g):
        eng = ctx.eng
        y, ids, rowptr = ctx.saved_tensors
        ga, gb = eng._epi_bwd(g, y, *ctx.epi)
        gx = None
        if ctx.needs_input_grad[1]:
            gx = eng._segment_bwd(ga, ids, ctx.x_shape, rowptr if ctx.mean else None)
        return None, gx, None, None, None, (ga if ctx.has_add else None), gb, None


class GATHeadMean(torch.autograd.Function):
    """y_i = 1/H sum_h sum_j alpha_ijh (x_j W_h) for a head-averaging GAT layer (gat_conv.py:98-122 with
    concat=False), aggregated BEFORE it is transformed: y_i = 1/H (sum_j alpha_ijh x_j) W_h, logits from
    el = x (W a_src), er = x (W a_dst).  The three walks gather the F-float input row / the C-float output
    gradient instead of the H x C transformed row (gat.hip, ggl_gat_sh_*); everything dense runs as GEMMs."""

    @staticmethod
    def forward(ctx, eng, gp, x, W, att, slope, p_drop):
        ctx.eng = eng
        dev = x.device
        N, F = int(x.shape[0]), int(x.shape[1])
        H = 8
        C = int(W.shape[1]) // H
        Wr = W.view(F, H, C)
        a_src, a_dst = att[0, :, :C], att[0, :, C:]
        U, V = (Wr * a_src).sum(-1), (Wr * a_dst).sum(-1)           # [F, H]
        el, er = (x @ U).contiguous(), (x @ V).contiguous()         # [N, H]
        rowmax = torch.empty((N, H), dtype=torch.float32, device=dev)
        den = torch.empty((N, H), dtype=torch.float32, device=dev)
        A = torch.empty((N, H, F), dtype=torch.float32, device=dev)
        part = eng._gat_sh_partial(gp.fwd, F, dev)
        cs = gp.fwd.c_struct(part)
        rng, rng_used = eng._draw(dev, p_drop)
        eng._check(eng.lib.ggl_gat_sh_fwd(ctypes.byref(cs), _ptr(gp.col), _ptr(el), _ptr(er), _ptr(x), F,
                                          float(slope), float(p_drop), _ptr(rng), _ptr(rowmax), _ptr(A),
                                          _ptr(den), eng._stream(dev)))
        Wst = Wr.permute(1, 0, 2).reshape(H * F, C)
        y = (A.view(N, H * F) @ Wst) / H
        ctx.gp, ctx.slope, ctx.p_drop, ctx.rng_used = gp, float(slope), float(p_drop), rng_used
        ctx.save_for_backward(x, W, att, el, er, rowmax, den, A)
        return y

    @staticmethod
    def backward(ctx, gy):
        eng = ctx.eng
        gp = ctx.gp
        x, W, att, el, er, rowmax, den, A = ctx.saved_tensors
        dev = gy.device
        N, F = int(x.shape[0]), int(x.shape[1])
        H = 8
        C = int(W.shape[1]) // H
        Cp = C + (-C) % 4
        Wr = W.view(F, H, C)
        a_src, a_dst = att[0, :, :C], att[0, :, C:]
        U, V = (Wr * a_src).sum(-1), (Wr * a_dst).sum(-1)
        Wst = Wr.permute(1, 0, 2).reshape(H * F, C)
        gyh = gy.contiguous() / H
        gyp = torch.nn.functional.pad(gyh, (0, Cp - C)).contiguous()
        G = (gyh @ Wst.t()).view(N, H, F).contiguous()               # dL/dA
        # {er, m, 1 / (den + 1e-16), <G, A>} per (row, head) in one pass (was: product + reduce + reciprocal + stack)
        stats = torch.empty((N, H, 4), dtype=torch.float32, device=dev)
        eng._check(eng.lib.ggl_gat_sh_stats(_ptr(er), _ptr(rowmax), _ptr(den), _ptr(G), _ptr(A), N, F, _ptr(stats),
                                            eng._stream(dev)))
        z = torch.nn.functional.pad((x @ W).view(N, H, C), (0, Cp - C)).contiguous()
        ger = torch.empty((N, H), dtype=torch.float32, device=dev)
        gel = torch.empty((N, H), dtype=torch.float32, device=dev)
        T = torch.empty((N, H, Cp), dtype=torch.float32, device=dev)
        bwd = gp.bwd
        # forward plan's partial: four doubles per hub chunk and head (the destination walk's row sums, round 6)
        part_f, part_t = eng._gat_sh_bwd_dst_partial(gp.fwd, dev), eng._gat_sh_bwd_src_partial(bwd, Cp, dev)
        cs, csT = gp.fwd.c_struct(part_f), bwd.c_struct(part_t)
        posT = gp.posT if ctx.p_drop > 0 else None
        eng._check(eng.lib.ggl_gat_sh_bwd(ctypes.byref(cs), _ptr(gp.col), ctypes.byref(csT), _ptr(gp.colT),
                                          _ptr(posT), _ptr(el), _ptr(x), F, _ptr(G), _ptr(stats), _ptr(z),
                                          _ptr(gyp), Cp, ctx.slope, ctx.p_drop, _ptr(ctx.rng_used), _ptr(ger),
                                          _ptr(T), _ptr(gel), eng._stream(dev)))
        gx = torch.einsum("nhc,fhc->nf", T[:, :, :C], Wr) + gel @ U.t() + ger @ V.t()
        # reductions over the N nodes: slab-split two-level sums (dense.wgrad), not one GEMM with an N-long accumulation per
        # element (round 6: a tuned kernel choice for the latter left these 1e-3 from a float64 evaluation)
        from .dense import wgrad

        gU, gV = wgrad(x, gel), wgrad(x, ger)                       # x^T gel, x^T ger: [F, H]
        gW = wgrad(A.view(N, H * F), gyh).view(H, F, C).permute(1, 0, 2) \
            + gU.unsqueeze(-1) * a_src + gV.unsqueeze(-1) * a_dst
        gatt = torch.cat([torch.einsum("fh,fhc->hc", gU, Wr), torch.einsum("fh,fhc->hc", gV, Wr)], dim=-1)
        return None, None, gx, gW.reshape(F, H * C), gatt.unsqueeze(0), None, None


class BlockMeanEpi(torch.autograd.Function):
    """relu(mean_{j in block row i} x[j] + add_i + bias) over a sampler Block (static capacities,
    device-side sizes): forward = the rectangular SpMM-mean with the epilogue in its store; backward
    = the MEANBWD walk of the block's CSC, which is built on the device without a host read."""

    @staticmethod
    def forward(ctx, eng, x, blk, add, bias, relu):
        ctx.eng = eng
        dev = x.device
        K = int(x.shape[1])
        if int(x.shape[0]) != blk.n_src_cap:
            raise RuntimeError(f"block expects {blk.n_src_cap} source rows, got {x.shape[0]}")
        y = torch.empty((blk.n_dst_cap, K), dtype=torch.float32, device=dev)
        b, a = _flat(bias, add)
        eng.spmm_epi_into(blk.plan, blk.col, None, x, y, mean=True, add=a, bias=b, relu=relu)
        ctx.blk, ctx.has_add = blk, add is not None
        ctx.epi = (relu, 0.0, None, None if bias is None else bias.shape)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        eng = ctx.eng
        (y,) = ctx.saved_tensors
        ga, gb = eng._epi_bwd(g, y, *ctx.epi)
        gx = None
        if ctx.needs_input_grad[1]:
            blk = ctx.blk
            planT, dstT = blk.transposed()
            gx, _ = eng._spmm_fwd("mean_bwd", planT, dstT, None, ga, blk.n_src_cap, aux=blk.rowptr)
        return None, gx, None, (ga if ctx.has_add else None), gb, None


class SpMMRows(torch.autograd.Function):
    """y[r] = sum_{j -> rows[r]} w x_j + bias for a sorted list of destination rows: the aggregate of a layer whose
    consumer reads only those rows (the loss over the training nodes), on the restricted plan pair
    (Engine.rows_plan).  Backward: gx = the transposed restricted walk over the compact [R, K] gradient, written
    into a full [N_src, K] result; gbias = ggl_bias_grad_rows.  Same bits as spmm_epi(...)[rows] and its backward."""

    @staticmethod
    def forward(ctx, eng, gp, w, x, rows, bias):
        ctx.eng = eng
        dev = x.device
        K = int(x.shape[1])
        rp = eng.rows_plan(gp, w, rows)
        y = torch.empty((rp.R, K), dtype=torch.float32, device=dev)
        b, _ = _flat(bias)
        eng.spmm_epi_into(rp.fwd, rp.col, rp.w_fwd, x, y, bias=b)
        ctx.rp, ctx.bshape, ctx.K = rp, (None if bias is None else bias.shape), K
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        eng = ctx.eng
        rp, K = ctx.rp, ctx.K
        g = g.contiguous()
        dev = g.device
        gb = None
        if ctx.bshape is not None and ctx.needs_input_grad[5]:
            gb = torch.empty(K, dtype=torch.float32, device=dev)
            wsb = eng.lib.ggl_bias_act_bwd_workspace_bytes(rp.N_dst, K)
            ws = torch.empty(max(wsb, 4), dtype=torch.uint8, device=dev)
            eng._check(eng.lib.ggl_bias_grad_rows(_ptr(g), _ptr(rp.rows), rp.R, rp.N_dst, K, _ptr(gb), _ptr(ws), wsb,
                                                  eng._stream(dev)))
            gb = gb.reshape(ctx.bshape)
        gx = None
        if ctx.needs_input_grad[3]:
            gx = torch.empty((rp.N_src, K), dtype=torch.float32, device=dev)
            eng.spmm_sum_into(rp.bwd, rp.colT, rp.w_bwd, g, gx)
        return None, None, None, gx, None, gb
