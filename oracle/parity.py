"""How a HIP result is compared with the reference's at full size.

TEST INFRASTRUCTURE ONLY (like everything under oracle/): used by tests/ and by bench.py's cpu_baseline leg, never by
the product package.  One function, so that the GPU tests and the bench line's `parity` object state the same thing.

Criterion (BASELINE.json north_star: "bit-exact for segment_max argmax indices and within 1e-5 relative for float
reductions"):

* rows the HIP kernels reduce in ONE piece follow the reference's serial order (spmm_sum_cpu.cpp:29-39: for e in edge
  order: out[dst] += w * x[src]) add for add — they must be BIT-IDENTICAL, and `rows_bit_exact_frac` says how many are;
* rows longer than the plan's chunk are combined from in-order partial sums, a different association of the same adds:
  `max_rel_err` = max |got - ref| / max(|ref|, floor_i), floor_i = the largest |ref| of row i (an element that cancels to
  ~0 inside a row whose other elements are O(1) has no meaningful relative error of its own; the row's magnitude is the
  scale its rounding errors live on).  Pass = max_rel_err <= tol.
"""
import numpy as np
import torch

TOL = 1e-5
# what `max_rel_err` / `tol` of a report mean — stated in every bench line's `parity.criterion` (round-5 verdict, weak #11)
CRITERION = ("row-scale relative: |got - ref| / max(|ref|, largest |ref| of the element's row) <= tol; rows reduced in one piece must be "
             "bit-identical (rows_bit_exact_frac)")


def _bits(t):
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    if t.dtype == torch.float64:
        return t.contiguous().view(torch.int64)
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.contiguous().view(torch.int16)
    return t


def report(got, ref, tol=TOL, rows_in_one_piece=None, floor_min=0.0):
    """`got`, `ref`: tensors of the same shape [rows, ...] (any device; compared where `got` lives).
    `rows_in_one_piece`: optional bool [rows] — rows that MUST be bit-identical (reduced without chunk partials).
    `floor_min`: lower bound of the per-row scale, for quantities that cancel to ~0 over a whole row by construction
    (the logit gradients of an edge softmax: exactly 0 for a one-edge row) — callers pass the tensor's mean |ref|."""
    ref = ref.to(got.device)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    n = int(got.shape[0])
    g2, r2 = got.reshape(n, -1), ref.reshape(n, -1)
    same = _bits(g2) == _bits(r2)
    if g2.dtype.is_floating_point:      # NaN payloads / signed zeros are compared as bits above; as values for the error
        both_nan = torch.isnan(g2) & torch.isnan(r2)
        same = same | both_nan
    row_same = same.all(dim=1)
    out = {"rows": n, "rows_bit_exact_frac": float(row_same.double().mean()) if n else 1.0,
           "elems_bit_exact_frac": float(same.double().mean()) if same.numel() else 1.0, "tol": tol}
    if g2.dtype.is_floating_point and same.numel():
        d = (g2.double() - r2.double()).abs()
        d = torch.where(same, torch.zeros_like(d), d)
        floor = r2.double().abs().amax(dim=1, keepdim=True).clamp(min=max(float(floor_min), 1e-30))
        rel = d / torch.maximum(r2.double().abs(), floor)
        out["max_abs_err"] = float(d.max())
        out["max_rel_err"] = float(torch.nan_to_num(rel, nan=float("inf")).max())
    else:
        out["max_abs_err"] = 0.0 if bool(same.all()) else float("inf")
        out["max_rel_err"] = out["max_abs_err"]
    out["ok"] = out["max_rel_err"] <= tol
    if rows_in_one_piece is not None:
        m = rows_in_one_piece.to(got.device)
        out["one_piece_rows"] = int(m.sum())
        out["one_piece_rows_bit_exact"] = bool(row_same[m].all()) if int(m.sum()) else True
        out["ok"] = bool(out["ok"] and out["one_piece_rows_bit_exact"])
    return out


def check(got, ref, what, tol=TOL, rows_in_one_piece=None, floor_min=0.0):
    r = report(got, ref, tol, rows_in_one_piece, floor_min)
    assert r["ok"], f"{what}: {r}"
    return r


def gat_truth_f64(ei, el, er, x, go, n, slope=0.2, attn_keep=None):
    """gat_conv.py:103-112 + softmax.py:29-35 in float64 with torch on the tensors' device, under autograd: the ground truth
    both f32 evaluations of a GAT layer (the fused HIP kernels, the reference ops composed) are measured against.
    `attn_keep`: optional [E, H] attention-dropout factor (gat_keep_mask) applied to alpha after the softmax.
    Returns (out, gx, g_el, g_er) as float64."""
    src, dst = ei[0], ei[1]
    xd, eld, erd = (t.detach().double().requires_grad_(True) for t in (x, el, er))
    s = torch.nn.functional.leaky_relu(eld[src] + erd[dst], slope)
    m = torch.full((n, s.shape[1]), -float("inf"), dtype=torch.float64, device=s.device)
    m = m.scatter_reduce(0, dst.view(-1, 1).expand_as(s), s, reduce="amax", include_self=True)
    ex = torch.exp(s - m[dst])
    den = torch.zeros_like(m).index_add_(0, dst, ex)
    alpha = ex / (den[dst] + 1e-16)
    if attn_keep is not None:
        alpha = alpha * attn_keep.to(device=alpha.device, dtype=alpha.dtype)
    out = torch.zeros(n, *x.shape[1:], dtype=torch.float64, device=x.device).index_add_(0, dst, xd[src] * alpha.unsqueeze(-1))
    out.backward(go.double())
    return out.detach(), xd.grad, eld.grad, erd.grad


def gat_errors_vs_truth(truth, got):
    """{name: max row-scale relative error} of an (out, gx, g_el, g_er) tuple against gat_truth_f64's (logit gradients
    cancel to ~0 over whole rows: their scale floor is the tensor's mean magnitude, as in the f32-vs-f32 checks)."""
    out = {}
    for name, t64, a in zip(("out", "gx", "g_el", "g_er"), truth, got):
        floor = float(t64.abs().mean()) if name in ("g_el", "g_er") else 0.0
        out[name] = report(a.double().to(t64.device), t64, tol=1.0, floor_min=floor)["max_rel_err"]
    return out


def gat_drop_word(index, offset, seed):
    """numpy restatement of gat_common.hpp drop_word: the attention-dropout word of counter index = p * H + h."""
    m64 = (1 << 64) - 1
    z = (int(seed) + int(offset) * 0x9E3779B97F4A7C15) & m64        # drop_key: splitmix64 of the launch's (seed, offset)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m64
    z ^= z >> 31
    k0, k1 = np.uint64(z & 0xFFFFFFFF), np.uint64(z >> 32)
    idx = np.asarray(index, dtype=np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    lo, hi = idx & m32, idx >> np.uint64(32)
    x = ((lo ^ k0) * np.uint64(0x9E3779B1)) & m32
    x ^= x >> np.uint64(15)
    x = ((x ^ hi ^ k1) * np.uint64(0x85EBCA77)) & m32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE3D)) & m32
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def gat_keep_mask(perm, E, H, seed, offset, p):
    """The [E, H] attention-dropout factor one fused GAT launch applied, in ORIGINAL edge order (float32, on the host):
    keep / (1 - p), 0 where dropped.  The kernels draw the word of counter p_s * H + h for sorted position p_s (the
    destination-sorted plan) and head h, and keep when it is >= the threshold set_dropout derives from the f32 rate;
    `perm` (the plan's perm, sorted position -> original edge; None = identity) maps the positions back to edges."""
    p32 = np.float32(p)
    thresh = np.uint32(int(float(p32) * 4294967296.0))              # (uint32_t)((double)p_drop * 2^32), p_drop a float
    scale = np.float32(1.0) / (np.float32(1.0) - p32)                # drop_scale = 1.0f / (1.0f - p_drop)
    keep = np.zeros((E, H), dtype=np.float32)
    for a in range(0, E, 1 << 22):                                   # (bounded host temporaries at millions of edges)
        b = min(E, a + (1 << 22))
        cnt = (np.arange(a, b, dtype=np.int64)[:, None] * H + np.arange(H)[None, :]).reshape(-1)
        keep[a:b] = (gat_drop_word(cnt, offset, seed).reshape(b - a, H) >= thresh) * scale
    if perm is None:
        return torch.from_numpy(keep)
    pm = perm.cpu().numpy().astype(np.int64) if isinstance(perm, torch.Tensor) else np.asarray(perm, dtype=np.int64)
    out = np.empty_like(keep)
    out[pm] = keep
    return torch.from_numpy(out)


def gat_fused_composed(ei, el, er, x, n, slope=0.2, seg=None, attn_keep=None):
    """The fused layer's op (gat_conv.py:103-112 + softmax.py:29-35) from its logit terms el [N_src, H], er [N_dst, H] and
    x [N_src, H, C], composed in the tensors' dtype: `seg` = (segment_max, segment_sum) as in gat_conv_composed (None = torch
    scatters), `attn_keep` = the [E, H] attention-dropout factor.  Differentiable in el, er, x."""
    seg_max, seg_sum = seg if seg is not None else _torch_segment_ops(x.dtype)
    src, dst = ei[0], ei[1]
    s = torch.nn.functional.leaky_relu(el[src] + er[dst], slope)
    m = seg_max(s, dst, n)
    ex = torch.exp(s - m[dst])
    den = seg_sum(ex, dst, n)
    alpha = ex / (den[dst] + 1e-16)
    if attn_keep is not None:
        alpha = alpha * attn_keep.to(device=alpha.device, dtype=alpha.dtype)
    return seg_sum(x[src] * alpha.unsqueeze(-1), dst, n)


# ---------------------------------------------------------------------------------------------------------------
# The whole GATConv layer / GATModel restated (round 6): what the head-averaging output layer (concat=False) of
# config 3 is checked against — the path FusedGATConv dispatches to ggl_gat_sh_* had only met the builder's own kernels.
# ---------------------------------------------------------------------------------------------------------------
def _torch_segment_ops(dtype):
    """(segment_max, segment_sum) as torch scatters in `dtype` on the tensors' device: the float64 ground truth's ops."""

    def seg_max(s, ids, n):
        m = torch.full((n, *s.shape[1:]), -float("inf"), dtype=dtype, device=s.device)
        return m.scatter_reduce(0, ids.view(-1, *([1] * (s.dim() - 1))).expand_as(s), s, reduce="amax", include_self=True)

    def seg_sum(v, ids, n):
        return torch.zeros((n, *v.shape[1:]), dtype=dtype, device=v.device).index_add_(0, ids, v)

    return seg_max, seg_sum


def gat_conv_composed(x, W, att, bias, ei, n, heads, out_channels, concat, slope=0.2, seg=None, attn_keep=None):
    """GATConv.forward exactly as gat_conv.py:98-122 writes it (attention dropout off): matmul, reshape [N, H, C], gather
    source and destination rows, concat, `(feat * att).sum(-1)`, LeakyReLU, segment_softmax (softmax.py:29-35: segment max,
    exp, segment sum, / (den + 1e-16)), message = x[src] * alpha, segment sum into the destinations, then concat heads
    (:112-113) or `reduce_mean` over them (:115-118) and `+ bias` (:120-121).  `seg` = (segment_max, segment_sum): the
    reference's compiled c_segment_max / c_segment_sum for the f32 composition; None = torch scatters in x's dtype (the
    float64 truth).  `attn_keep`: optional [E, H] attention-dropout factor (gat_keep_mask), multiplied into alpha after the
    softmax as gat_conv.py:104 applies dropout.  Differentiable in x, W, att, bias."""
    seg_max, seg_sum = seg if seg is not None else _torch_segment_ops(x.dtype)
    src, dst = ei[0], ei[1]
    z = (x @ W).reshape(-1, heads, out_channels)
    feat = torch.cat((z[src], z[dst]), dim=-1)
    e = torch.nn.functional.leaky_relu((feat * att).sum(dim=-1), slope)
    m = seg_max(e, dst, n)
    ex = torch.exp(e - m[dst])
    den = seg_sum(ex, dst, n)
    alpha = ex / (den[dst] + 1e-16)
    if attn_keep is not None:
        alpha = alpha * attn_keep.to(device=alpha.device, dtype=alpha.dtype)
    out = seg_sum(z[src] * alpha.unsqueeze(-1), dst, n)
    out = out.reshape(-1, heads * out_channels) if concat else out.mean(dim=1)
    return out + bias if bias is not None else out


def gat_conv_lean(x, W, att, bias, ei, n, heads, out_channels, concat, slope=0.2, attn_keep=None):
    """gat_conv_composed's math without the [E, H, 2C] concatenation: (cat(z_src, z_dst) * att).sum(-1) = z_src . a_src +
    z_dst . a_dst, taken per NODE before the gather (algebraically identical; in float64 the two differ by ~1e-16) — the largest
    per-edge tensor is then [E, H, C], which lets a float64 evaluation reach 14 M edges (rows of 19 k edges) in 288 GB.  Torch
    scatters in x's dtype; `attn_keep` as in gat_conv_composed; differentiable in x, W, att, bias."""
    seg_max, seg_sum = _torch_segment_ops(x.dtype)
    src, dst = ei[0], ei[1]
    C = out_channels
    z = (x @ W).reshape(-1, heads, C)
    el, er = (z * att[:, :, :C]).sum(-1), (z * att[:, :, C:]).sum(-1)
    e = torch.nn.functional.leaky_relu(el[src] + er[dst], slope)
    m = seg_max(e, dst, n)
    ex = torch.exp(e - m[dst])
    den = seg_sum(ex, dst, n)
    alpha = ex / (den[dst] + 1e-16)
    if attn_keep is not None:
        alpha = alpha * attn_keep.to(device=alpha.device, dtype=alpha.dtype)
    out = seg_sum(z[src] * alpha.unsqueeze(-1), dst, n)
    out = out.reshape(-1, heads * C) if concat else out.mean(dim=1)
    return out + bias if bias is not None else out


def kink_free_edges(ei, x, W, att, heads, out_channels, margin=1e-4):
    """`ei` without the edges whose logit el[src] + er[dst] lies within `margin` of 0 in any head (evaluated in float64).
    LeakyReLU is not differentiable at 0: an edge whose f32 logit rounds to the other side of 0 than its float64 value gets the
    OTHER slope (1 vs 0.2) in an f32 evaluation — a jump of 0.8 alpha (da - s) in the logit gradient that no precision removes, and
    at 10^7 edges x 8 heads a few dozen logits lie within 1e-6 of 0 (round 6: at 14 M edges BOTH f32 evaluations, the HIP kernels and
    plain torch ops, were 6.9e-2 from the float64 "truth" by the SAME amount).  A comparison against float64 is meaningful only
    where the function is differentiable at the evaluation point to f32 precision; dropping ~0.03 % of the edges changes no code path."""
    C = out_channels
    z = (x.double() @ W.double()).reshape(-1, heads, C)
    a = att.double()
    el, er = (z * a[:, :, :C]).sum(-1), (z * a[:, :, C:]).sum(-1)
    keep = ((el[ei[0]] + er[ei[1]]).abs() >= margin).all(dim=1)
    return ei[:, keep].contiguous(), int((~keep).sum())


def near_kink_rows(ei, x, W, att, heads, out_channels, n, margin=1e-4):
    """bool [n]: the rows touched (as source or destination) by an edge whose float64 logit lies within `margin` of 0 in any
    head — where an f32 evaluation that forms the logit differently (x @ (W a) against (x W) . a) may take the other slope.
    Returns (rows, number of such edges)."""
    C = out_channels
    z = (x.double() @ W.double()).reshape(-1, heads, C)
    a = att.double()
    el, er = (z * a[:, :, :C]).sum(-1), (z * a[:, :, C:]).sum(-1)
    near = ((el[ei[0]] + er[ei[1]]).abs() < margin).any(dim=1)
    rows = torch.zeros(n, dtype=torch.bool, device=ei.device)
    rows[ei[0][near]] = True
    rows[ei[1][near]] = True
    return rows, int(near.sum())


def kink_free_edges_logits(ei, el, er, margin=1e-4):
    """kink_free_edges for a layer given by its logit terms el [N_src, H], er [N_dst, H] directly."""
    keep = ((el.double()[ei[0]] + er.double()[ei[1]]).abs() >= margin).all(dim=1)
    return ei[:, keep].contiguous(), int((~keep).sum())


def kink_free_edges_model(ei, x, params, n, heads, slope=0.2, margin=1e-4):
    """kink_free_edges for every layer of a GATModel (params = [(W, att, bias), ...]): layer i's logits are evaluated in float64 on
    the output of the layers before it (computed on the edges kept so far).  Edges dropped for a later layer change the earlier
    layers' outputs on a few rows only; the handful of logits that could re-enter the band that way is left alone."""
    h = x.double()
    dropped = 0
    L = len(params)
    for i, (W, att, bias) in enumerate(params):
        C = int(att.shape[-1]) // 2
        ei, d = kink_free_edges(ei, h, W, att, heads, C, margin)
        dropped += d
        if i < L - 1:
            with torch.no_grad():
                h = torch.nn.functional.elu(gat_conv_lean(h, W.double(), att.double(), None if bias is None else bias.double(), ei, n,
                                                          heads, C, concat=True, slope=slope))
    return ei, dropped


def gat_model_composed(x, params, ei, n, heads, slope=0.2, seg=None, attn_keep=None, feat_keep=None):
    """GATModel.forward (models/gat.py:65-72): `params` = [(W, att, bias), ...] per layer; every layer but the last concatenates
    its heads and is followed by ELU, the last one averages them (:49-53; a one-layer model's only layer is built by the
    `i == 0` branch: concat).  Eval mode (dropout = identity) by default; training mode with recorded masks: `feat_keep` = one
    factor per layer multiplied into the layer's input (the model's nn.Dropout, keep / (1 - p)), `attn_keep` = one [E, H]
    attention-dropout factor per layer (gat_keep_mask)."""
    L = len(params)
    for i, (W, att, bias) in enumerate(params):
        C = int(att.shape[-1]) // 2
        if feat_keep is not None:
            x = x * feat_keep[i].to(device=x.device, dtype=x.dtype)
        x = gat_conv_composed(x, W, att, bias, ei, n, heads, C, concat=(i == 0 or i < L - 1), slope=slope, seg=seg,
                              attn_keep=None if attn_keep is None else attn_keep[i])
        if i < L - 1:
            x = torch.nn.functional.elu(x)
    return x


def layer_errors_vs_truth(truth, got, names, zero_mean_rows=(), abs_floor=0.0):
    """{name: max row-scale relative error} of a tuple of tensors against float64 truths; `zero_mean_rows` names tensors whose
    rows can cancel to ~0 as a whole (scale floor = the tensor's mean magnitude, at least `abs_floor`: a one-edge graph's logit
    gradients are exactly 0 everywhere, and rounding noise of the cancelling terms is all there is to compare)."""
    out = {}
    for name, t64, a in zip(names, truth, got):
        t2 = t64.reshape(t64.shape[0], -1) if t64.dim() > 1 else t64.reshape(1, -1)
        a2 = a.double().to(t64.device).reshape(t2.shape)
        floor = max(float(t64.abs().mean()), float(abs_floor)) if name in zero_mean_rows else 0.0
        out[name] = report(a2, t2, tol=1.0, floor_min=floor)["max_rel_err"]
    return out
