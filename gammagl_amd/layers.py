"""Harness-side callers of the hot path: torch restatements of the
reference layers that sit directly on ``gammagl.mpops`` — just enough of them to drive the ops the
way GammaGL does.  The reference classes are TensorLayerX modules (``tlx`` is not installable
here); every tlx call they make on this path maps 1:1 onto torch (``tlx.gather`` = index_select,
``tlx.pow``, ``tlx.reshape`` ...), so these are line-for-line the same computations:

* ``MessagePassing``  — layers/conv/message_passing.py:35-156 (message / aggregate /
  message_aggregate / propagate, including the "fused route only if the class defines
  message_aggregate itself" rule at :144)
* ``GCNConv``         — layers/conv/gcn_conv.py:78-115, with the reference's own (commented-out)
  ``message_aggregate`` -> ``gspmm`` override at :110-115 enabled, which is what makes
  ogbn-products-sized graphs fit one GPU (the unfused route materialises an [E,K] = 129 GB message)
* ``SAGEConv``        — layers/conv/sage_conv.py:56-108 ('mean', 'gcn' and 'pool' aggregators)
* ``GATConv``         — layers/conv/gat_conv.py:98-122 (unfused: segment_softmax + propagate)
* ``FusedGATConv``    — layers/conv/fusedgat_conv.py:89-130 with our single-kernel op in place of
  the external dgNN GATConvFuse
* ``HGTConv``         — layers/conv/hgt_conv.py:41-153 (fused: utils.dot_attention per edge type)
* ``GATv2Conv``       — the GATv2 paper's layer (fused: utils.gatv2_attention); variant="reference" is
  layers/conv/gatv2_conv.py:94-119, whose logit is separable
* ``PNAConv``         — layers/conv/pna_conv.py:82-201 (fused: utils.segment_multi_aggregate, all statistics in one walk),
  with the ``global_{sum,mean,max,min}_pool`` functions of layers/pool/glob.py:5-114
* ``GCNModel``        — models/gcn.py:30-64
"""
import math

import torch
from torch import nn

from . import engine as _engine
from .dense import Linear, _LinearFn, node_matmul
from .sampler import Block
from .utils.attention import dot_attention, edge_softmax_aggregate, gatv2_attention
from .utils.aggregate import segment_multi_aggregate, segment_multi_composed
from .mpops import (bspmm, gspmm, unsorted_segment_max, unsorted_segment_mean,  # noqa: F401
                    unsorted_segment_min, unsorted_segment_sum, use_ext)


def degree(index, num_nodes, dtype=torch.float32):
    """utils/degree.py:10-40: unsorted_segment_sum(ones[E], index, N) (K = 1).

    The sum of ones per segment is the segment's element count, which the cached plan of ``index`` already
    holds as rowptr differences — no kernel, no pass over E.  Float dtypes clamp at
    the value where the reference's ``+= 1`` accumulation in that dtype stops growing (2^24 for f32)."""
    if not index.is_cuda or index.dim() != 1 or index.dtype != torch.int64:
        one = torch.ones((index.shape[0],), dtype=dtype, device=index.device)
        return unsorted_segment_sum(one, index, num_nodes)
    cnt = _engine(index).seg_plan(index, num_nodes).counts()
    sat = {torch.float32: 1 << 24, torch.float16: 2048, torch.bfloat16: 256}.get(dtype)
    if sat is not None:
        cnt = cnt.clamp(max=sat)
    return cnt.to(dtype)


def calc_gcn_norm(edge_index, num_nodes, edge_weight=None):
    """utils/norm.py:5-30."""
    src, dst = edge_index[0], edge_index[1]
    if edge_weight is None:
        edge_weight = torch.ones((edge_index.shape[1], 1), device=edge_index.device)
    deg = unsorted_segment_sum(edge_weight, src, num_segments=num_nodes).reshape(-1)
    deg_inv_sqrt = deg.pow(-0.5)
    return deg_inv_sqrt[src] * edge_weight.reshape(-1) * deg_inv_sqrt[dst]


def segment_softmax(data, segment_ids, num_segments):
    """utils/softmax.py:10-36."""
    max_values = unsorted_segment_max(data, segment_ids, num_segments=num_segments)
    exp = torch.exp(data - max_values[segment_ids])
    denominator = unsorted_segment_sum(exp, segment_ids, num_segments=num_segments)
    return exp / (denominator[segment_ids] + 1e-16)


def add_self_loops(edge_index, num_nodes):
    """utils/loop.py:57-142 with n_loops=1, no edge attributes: loops are appended at the end."""
    loops = torch.arange(num_nodes, device=edge_index.device, dtype=edge_index.dtype)
    return torch.cat([edge_index, torch.stack([loops, loops])], dim=1)


FUSED_MIN_EDGES = 2_000_000  # default message()+aggregate() pairs take the fused SpMM from this many edges up
SAGE_FUSE_EPILOGUE = True    # SAGEConv(mean): "+ fc_self(x_dst) + bias -> act" in the aggregate's store (A/B switch)


class MessagePassing(nn.Module):
    def message(self, x, edge_index, edge_weight=None):
        msg = x.index_select(0, edge_index[0, :])
        if edge_weight is not None:
            return msg * edge_weight.unsqueeze(-1)
        return msg

    _REDUCERS = {'sum': unsorted_segment_sum, 'mean': unsorted_segment_mean, 'max': unsorted_segment_max}

    def aggregate(self, msg, edge_index, num_nodes=None, aggr='sum'):
        """Reduce the messages onto their destination nodes (message_passing.py:63-92: same signature, same three
        reducers over edge_index[1])."""
        reduce = self._REDUCERS.get(aggr)
        if reduce is None:
            raise NotImplementedError(f'aggr={aggr!r}: this layer aggregates with sum, mean or max')
        return reduce(msg, edge_index[1, :], num_nodes)

    def message_aggregate(self, x, edge_index, edge_weight=None, aggr='sum'):
        if use_ext:
            if edge_weight is None:
                edge_weight = torch.ones(edge_index.shape[1], device=x.device, dtype=x.dtype)
            return gspmm(edge_index, edge_weight, x, aggr)
        msg = self.message(x, edge_index, edge_weight)
        return self.aggregate(msg, edge_index)

    def update(self, x):
        return x

    def propagate(self, x, edge_index, aggr='sum', **kwargs):
        if kwargs.get('num_nodes') is None:
            kwargs['num_nodes'] = x.shape[0]
        if 'message_aggregate' in self.__class__.__dict__:  # message_passing.py:144
            x = self.message_aggregate(x, edge_index, edge_weight=kwargs.get('edge_weight'), aggr=aggr)
        elif (aggr in ('sum', 'mean') and x.dim() == 2
              # (bf16 / f16 rows take the SpMM whatever the size: it sums in f32, the segment route in the storage type)
              and ((x.dtype == torch.float32 and edge_index.shape[1] >= FUSED_MIN_EDGES)
                   or x.dtype in (torch.bfloat16, torch.float16))
              and type(self).message is MessagePassing.message
              and type(self).aggregate is MessagePassing.aggregate
              # a weight that is not one f32 value per edge stays on the message() route, which promotes /
              # broadcasts it (a learnable one takes the SpMM: sum and mean differentiate with respect to it)
              and not (kwargs.get('edge_weight') is not None and
                       (kwargs['edge_weight'].dtype != torch.float32
                        or kwargs['edge_weight'].numel() != edge_index.shape[1]))):
            # The default message() (gather * weight) + aggregate() pair IS an SpMM.  A big (full-graph) edge
            # list takes the fused rectangular kernel: no [E, K] message tensor (Reddit-sized SAGEConv layer:
            # 155 -> 14.7 ms forward+backward, 59 GB less HBM), same sums in the same order.  Sampled blocks stay
            # below the threshold on purpose: they are NEW edge lists every batch and the fused backward would
            # need a transposed plan (a sort + host syncs) each time — measured 4.5 vs 3.1 ms per batch.
            eng = _engine(x)
            gp = eng.graph_plan(edge_index, int(kwargs['num_nodes']), int(x.shape[0]))
            ew = kwargs.get('edge_weight')
            x = eng.spmm(gp, None if ew is None else ew.reshape(-1).contiguous(), x, aggr)
        elif (aggr == 'sum' and edge_index.shape[1] >= FUSED_MIN_EDGES and x.dim() == 3 and x.dtype == torch.float32
              and kwargs.get('edge_weight') is not None and kwargs['edge_weight'].dim() == 2
              and kwargs['edge_weight'].dtype == torch.float32
              and kwargs['edge_weight'].shape == (edge_index.shape[1], x.shape[1])
              and int(kwargs['num_nodes']) == x.shape[0] and type(self).message is MessagePassing.message
              and type(self).aggregate is MessagePassing.aggregate):
            # multi-head messages x[src,h,:] * w[e,h] summed per destination == bspmm (what GATConv's own
            # commented-out message_aggregate would call, gat_conv.py:124-129): no [E, H, C] message tensor
            x = bspmm(edge_index, kwargs['edge_weight'], x, 'sum')
        else:
            msg = self.message(x, edge_index, edge_weight=kwargs.get('edge_weight'))
            x = self.aggregate(msg, edge_index, num_nodes=kwargs['num_nodes'], aggr=aggr)
        return self.update(x)


CACHE_GCN_NORM = True    # False: every GCNConv.forward recomputes its normalisation, as the reference does (bench.py's side figure)


_X16 = (torch.bfloat16, torch.float16)


class GCNConv(MessagePassing):
    # bf16 / f16 activations (torch.autocast): True = "+ bias", ReLU and dropout ride on the mixed-precision aggregate's
    # store (Engine.spmm_epi on 16-bit rows: every step in f32, ONE rounding, the library's Philox dropout).  Off for a
    # bare layer, which keeps the composition "aggregate, round, + bias.to(dtype), relu, dropout" in torch; GCNModel
    # switches it on for its layers.
    fuse_epilogue16 = False

    def __init__(self, in_channels, out_channels, norm='both', add_bias=True):
        super().__init__()
        if norm not in ['left', 'right', 'none', 'both']:
            raise ValueError('Invalid norm value. Must be either "none", "both", "right" or "left".'
                             ' But got "{}".'.format(norm))
        self._norm = norm
        self.linear = Linear(in_channels, out_channels, bias=False)
        nn.init.xavier_uniform_(self.linear.weight)
        self.bias = nn.Parameter(torch.zeros(1, out_channels)) if add_bias else None

    def _norm_weights(self, edge_index, edge_weight, num_nodes, device):
        """gcn_conv.py:84-102: deg^-1/2 (or 1/deg) of the source and/or destination end of every edge, degrees
        counted on the edge list as given.  The reference recomputes this in every layer of every step; with
        edge_weight=None it depends on the graph alone, so it is computed once per edge_index and kept on the
        cached GraphPlan (the same tensor every call also lets the SpMM stream its sorted copy)."""
        gp = None
        if edge_weight is None and CACHE_GCN_NORM:
            gp = _engine(edge_index).graph_plan(edge_index, num_nodes)
            hit = gp.aux.get(("gcn_norm", self._norm))
            if hit is not None:
                return hit
        src, dst = edge_index[0], edge_index[1]
        ew = torch.ones((edge_index.shape[1],), device=device) if edge_weight is None else edge_weight.reshape(-1)
        weights = ew
        if self._norm in ['left', 'both']:
            deg = degree(src, num_nodes=num_nodes, dtype=torch.float32)
            norm = deg.pow(-0.5) if self._norm == 'both' else 1.0 / deg
            weights = norm[src] * ew
        if self._norm in ['right', 'both']:
            deg = degree(dst, num_nodes=num_nodes, dtype=torch.float32)
            norm = deg.pow(-0.5) if self._norm == 'both' else 1.0 / deg
            weights = weights * norm[dst]
        if gp is not None:
            gp.aux[("gcn_norm", self._norm)] = weights
        return weights

    def forward(self, x, edge_index, edge_weight=None, num_nodes=None, _epilogue=None):
        """`_epilogue=(relu, p_drop, training)` (used by GCNModel): the ReLU and dropout the model applies right
        after this layer, fused with the bias into the aggregate's store (or one pass after it)."""
        n_out = self.linear.weight.shape[0]
        pad = (-n_out) % 4 if n_out >= 8 else 0
        if pad and x.dim() == 2:  # class-count widths: 47 -> 48 columns inside the GEMM, dropped at the end
            wp = torch.nn.functional.pad(self.linear.weight, (0, 0, 0, pad))
            if torch.is_autocast_enabled(x.device.type):   # the built-in linear casts its operands (dense.Linear does the same)
                x = torch.nn.functional.linear(x, wp)
            else:
                x = _LinearFn.apply(x.contiguous(), wp)
        else:
            x = self.linear(x)
        num_nodes = x.shape[0]
        weights = self._norm_weights(edge_index, edge_weight, num_nodes, x.device)
        relu, p_drop, training = _epilogue if _epilogue is not None else (False, 0.0, False)
        bias = self.bias
        if pad and bias is not None:
            bias = torch.nn.functional.pad(bias, (0, pad))
        if weights.dtype != torch.float32 or weights.dim() != 1 or weights.numel() != edge_index.shape[1]:
            # weights that are not one f32 value per edge take the message() * weight -> unsorted_segment_sum route
            # (a float64 edge_weight promotes the messages exactly as the reference's message() does, a mis-shaped
            # one raises there as it does here); a learnable f32 one takes the aggregate below, which differentiates
            # with respect to it
            out = self.aggregate(self.message(x, edge_index, weights), edge_index, num_nodes, 'sum')
            if out.dtype != torch.float32:   # promoted messages: the epilogue in torch, as the reference runs it
                out = out + bias if bias is not None else out
                out = torch.relu(out) if relu else out
                out = torch.nn.functional.dropout(out, p_drop, training) if p_drop > 0 else out
            elif bias is not None or relu or p_drop > 0:
                out = _engine(out).bias_act(out, bias, relu=relu, p_drop=p_drop, training=training)
        elif (x.dim() == 2 and x.dtype == torch.float32 and x.shape[1] % 4 == 0
              and weights.dtype == torch.float32 and weights.numel() == edge_index.shape[1]):
            eng = _engine(x)
            out = eng.spmm_bias_act(eng.graph_plan(edge_index, num_nodes), weights, x, bias, relu=relu,
                                    p_drop=p_drop, training=training)
        elif (self.fuse_epilogue16 and x.dim() == 2 and x.dtype in _X16
              and (bias is None or bias.dtype == torch.float32)):
            # bf16 / f16 activations (torch.autocast) with the fused form on: the f32 bias, ReLU and dropout applied to the
            # f32 sums in registers, one rounding at the aggregate's only store
            eng = _engine(x)
            out = eng.spmm_epi(eng.graph_plan(edge_index, num_nodes), weights, x, "sum", None, bias, relu=relu,
                               p_drop=p_drop, training=training)
        else:
            out = self.propagate(x, edge_index, edge_weight=weights, num_nodes=num_nodes)
            if out.dtype != torch.float32:
                # bf16 / f16 activations (torch.autocast), the bare layer: the mixed-precision aggregate (f32 sums, rounded
                # once), then the epilogue in torch, each step rounding again (fuse_epilogue16 = True fuses it)
                out = out + bias.to(out.dtype) if bias is not None else out
                out = torch.relu(out) if relu else out
                out = torch.nn.functional.dropout(out, p_drop, training) if p_drop > 0 else out
            elif bias is not None or relu or p_drop > 0:
                out = _engine(out).bias_act(out, bias, relu=relu, p_drop=p_drop, training=training)
        return out[:, :n_out] if pad else out

    def message_aggregate(self, x, edge_index, edge_weight=None, aggr="sum"):  # gcn_conv.py:110-115
        if edge_weight is None:
            edge_weight = torch.ones((edge_index.shape[1],), dtype=torch.float32, device=x.device)
        return gspmm(edge_index, edge_weight, x, aggr)


class SAGEConv(MessagePassing):
    """layers/conv/sage_conv.py.  ASSOCIATION: the reference always transforms first, mean(fc_neigh(x_src))
    (sage_conv.py:100).  With aggr='mean', f32 features and a layer whose input is NARROWER than its output this
    class computes fc_neigh(mean(x_src)) instead — the same product associated the cheap way round (the rule DGL's
    SAGEConv applies): results then agree with the reference to f32 rounding (1e-5 relative), not bit for bit.
    Set `gammagl_amd.layers.SAGE_FUSE_EPILOGUE = False` for the reference's order of operations throughout."""

    def __init__(self, in_channels, out_channels, activation=None, aggr="mean", add_bias=True):
        super().__init__()
        self.aggr = aggr
        self.act = activation
        self.fc_neigh = Linear(in_channels, out_channels, bias=False)
        if aggr != 'gcn':
            self.fc_self = Linear(in_channels, out_channels, bias=False)
        if aggr == 'pool':
            self.pool = Linear(in_channels, in_channels, bias=False)
        if aggr == 'lstm':   # sage_conv.py:46-47
            self.in_feat = in_channels
            self.lstm = nn.LSTM(input_size=in_channels, hidden_size=in_channels, batch_first=True)
        self.bias = nn.Parameter(torch.zeros(1, out_channels)) if add_bias else None

    def forward(self, feat, edge):
        src_feat, dst_feat = feat if isinstance(feat, tuple) else (feat, feat)
        num_nodes = int(dst_feat.shape[0])
        if isinstance(edge, Block):   # a static-shape block of the BlockSampler (graph-capturable step)
            if self.aggr != 'mean':
                raise NotImplementedError("sampler Blocks carry the mean aggregator")
            fused_act = self.act is None or self.act is torch.relu or self.act is torch.nn.functional.relu
            w_n, w_s = self.fc_neigh.weight, self.fc_self.weight
            if w_n.shape[1] < w_n.shape[0] and src_feat.shape[1] % 4 == 0:
                # input narrower than output: aggregate first (the rule DGL's SAGEConv applies; sage_conv.py:100 always
                # transforms first).  In a sampled block this also shrinks the GEMM from the block's SOURCE rows to its
                # destination rows (100 608 -> 18 432 on the products-sized graph) and, for the first layer, whose
                # input rows carry no gradient, removes the backward aggregate together with the block's CSC build.
                agg = edge.eng.block_mean_epi(src_feat, edge)
                out = torch.nn.functional.linear(torch.cat([agg, dst_feat], dim=1), torch.cat([w_n, w_s], dim=1))
                if self.bias is not None or self.act is not None:
                    out = edge.eng.bias_act(out, self.bias, relu=fused_act and self.act is not None)
                return out if fused_act else self.act(out)
            out = edge.eng.block_mean_epi(self.fc_neigh(src_feat), edge, add=self.fc_self(dst_feat), bias=self.bias,
                                           relu=fused_act and self.act is not None)
            return out if fused_act else self.act(out)
        if self.aggr == 'mean':
            fused_act = self.act is None or self.act is torch.relu or self.act is torch.nn.functional.relu
            w_n = self.fc_neigh.weight
            if (SAGE_FUSE_EPILOGUE and w_n.shape[1] < w_n.shape[0] and src_feat.dim() == 2 and src_feat.shape[1] % 4 == 0
                    and src_feat.dtype == torch.float32 and fused_act):
                # input narrower than output: aggregate first, transform the (fewer, in a sampled block) destination
                # rows afterwards — see the Block branch above
                eng = _engine(src_feat)
                if edge.shape[1] >= FUSED_MIN_EDGES:
                    gp = eng.graph_plan(edge, num_nodes, int(src_feat.shape[0]))
                    agg = eng.spmm(gp, None, src_feat, "mean")
                else:
                    agg = unsorted_segment_mean(src_feat.index_select(0, edge[0]), edge[1], num_nodes)
                out = torch.nn.functional.linear(torch.cat([agg, dst_feat], dim=1), torch.cat([w_n, self.fc_self.weight], dim=1))
                if self.bias is not None or self.act is not None:
                    out = eng.bias_act(out, self.bias, relu=self.act is not None)
                return out
            src_feat = self.fc_neigh(src_feat)
            big = edge.shape[1] >= FUSED_MIN_EDGES
            # bf16 / f16 rows (torch.autocast) take the fused SpMM-mean whatever the edge count and width: it sums in f32
            # and rounds once, where the segment route would sum in the storage type (the rule of propagate())
            x16 = src_feat.dtype in _X16 and (self.bias is None or self.bias.dtype == torch.float32)
            # (a small block whose width is not a multiple of 4 — e.g. the 47-class output layer — has no fused form:
            # it goes straight to propagate() below without computing fc_self / the gather here first and again there)
            if (SAGE_FUSE_EPILOGUE and src_feat.dim() == 2 and fused_act
                    and ((src_feat.dtype == torch.float32 and (big or src_feat.shape[1] % 4 == 0)) or x16)):
                # "mean + fc_self(x_dst) + bias -> act" (sage_conv.py:100-108) rides on the aggregate's store:
                # the fused rectangular SpMM-mean for big edge lists, the segment route for sampled blocks
                eng = _engine(src_feat)
                self_term = self.fc_self(dst_feat)
                if x16 and self_term.dtype != src_feat.dtype:
                    self_term = self_term.to(src_feat.dtype)
                if big or x16:
                    gp = eng.graph_plan(edge, num_nodes, int(src_feat.shape[0]))
                    return eng.spmm_epi(gp, None, src_feat, "mean", add=self_term, bias=self.bias,
                                        relu=self.act is not None)
                return eng.segment_epi(src_feat.index_select(0, edge[0]), edge[1], num_nodes, "mean", add=self_term,
                                       bias=self.bias, relu=self.act is not None)
            # (propagate picks the fused SpMM-mean for big edge lists, the segment route for sampled blocks)
            out = self.propagate(src_feat, edge, edge_weight=None, num_nodes=num_nodes, aggr='mean')
        elif self.aggr == 'gcn':
            src_feat = self.fc_neigh(src_feat)
            n = int(1 + edge[0].max())
            edge = add_self_loops(edge, n)
            weight = calc_gcn_norm(edge, n)
            out = self.propagate(src_feat, edge, edge_weight=weight, num_nodes=n, aggr='sum')
            out = out[:num_nodes]
        elif self.aggr == 'pool':
            src_feat = torch.relu(self.pool(src_feat))
            out = self.propagate(src_feat, edge, edge_weight=None, num_nodes=num_nodes, aggr='max')
            out = self.fc_neigh(out)
        elif self.aggr == 'lstm':
            # sage_conv.py:93-98: no graph op at all — the source rows are taken as [N_dst, fan-out, D] sequences in
            # the order they arrive (the edge list is not consulted) and the LSTM's last hidden state is the aggregate
            size = dst_feat.shape[0]
            seq = src_feat.reshape(size, -1, src_feat.shape[1])
            h0 = (torch.zeros((1, size, self.in_feat), dtype=seq.dtype, device=seq.device),
                  torch.zeros((1, size, self.in_feat), dtype=seq.dtype, device=seq.device))
            _, (rst, _) = self.lstm(seq, h0)
            out = self.fc_neigh(rst[0])
        else:
            raise NotImplementedError(self.aggr)
        if self.aggr != 'gcn':
            out = out + self.fc_self(dst_feat)
        if self.bias is not None:
            out = out + self.bias
        return self.act(out) if self.act is not None else out


class GATConv(MessagePassing):
    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout_rate=0.,
                 add_bias=True):
        super().__init__()
        self.heads, self.out_channels, self.concat = heads, out_channels, concat
        self.negative_slope = negative_slope
        self.dropout_rate = dropout_rate
        self.dropout = nn.Dropout(dropout_rate)   # on the attention coefficients (gat_conv.py:90,104)
        self.w = nn.Parameter(torch.empty(in_channels, out_channels * heads))
        self.att = nn.Parameter(torch.empty(1, heads, out_channels * 2))
        nn.init.trunc_normal_(self.w, std=0.05)
        nn.init.trunc_normal_(self.att, std=0.05)
        nb = heads * out_channels if concat else out_channels
        self.bias = nn.Parameter(torch.zeros(nb)) if add_bias else None

    def _finish(self, x):
        if self.concat:
            x = x.reshape(-1, self.heads * self.out_channels)
        else:
            x = x.mean(dim=1)
        return x + self.bias if self.bias is not None else x

    def forward(self, x, edge_index, num_nodes=None):
        x = node_matmul(x, self.w).reshape(-1, self.heads, self.out_channels)
        node_src, node_dst = edge_index[0, :], edge_index[1, :]
        feat = torch.cat((x[node_src], x[node_dst]), dim=-1)
        e = (feat * self.att).sum(dim=-1)
        e = torch.nn.functional.leaky_relu(e, self.negative_slope)
        alpha = self.dropout(segment_softmax(e, node_dst, num_nodes))
        x = self.propagate(x, edge_index, num_nodes=num_nodes, edge_weight=alpha)
        return self._finish(x)


class FusedGATConv(GATConv):
    """Same parameters and math as GATConv; logits, softmax, attention dropout and aggregate run in one HIP
    kernel per direction.  The reference layer (fusedgat_conv.py:89-130) optionally takes a prebuilt
    CSR/CSC (`row_ptr`, `col_ind`, `col_ptr`, `row_ind`, `permute`) to skip its numpy preprocessing; here
    the destination-sorted plan is built on the device once per edge_index and cached, so those keywords are
    accepted and not needed.  Aggregates into edge_index[1] like GATConv (the reference's fused layer builds
    its CSR on edge_index[0], which only coincides on symmetric graphs — SURVEY.md §8a row G).

    Under torch.autocast the transformed [N, H, C] panel leaves the GEMM as bf16 / f16 and goes to the kernels as it is
    (Engine.gat_fused on 16-bit rows: f32 softmax and sums, one rounding at the store); el / er are computed from it in f32
    and the finish (reshape / head mean, bias) is torch's.  A head-averaging layer that takes the aggregate-first route
    keeps it in f32: its input, the previous layer's bias + ELU, is f32."""

    def forward(self, x, edge_index, num_nodes=None, **kwargs):
        H, C = self.heads, self.out_channels
        eng = _engine(x)
        if 'row_ptr' in kwargs:
            # fusedgat_conv.py:95-100: the caller's own CSR (rows = the aggregating nodes, col_ind = the nodes they
            # gather from), its transpose and the CSC -> CSR position map: taken as they are, no sort, no host trip
            edge_index = eng.graph_plan_from_csr(kwargs['row_ptr'], kwargs['col_ind'], kwargs['col_ptr'],
                                                 kwargs['row_ind'], kwargs['permute'])
        if (not self.concat and x.dim() == 2 and x.dtype == torch.float32 and (num_nodes is None or num_nodes == x.shape[0])
                and eng.gat_headmean_supported(H, x.shape[1], C)):
            # a head-averaging layer whose input row (F floats) is narrower than its H x C transformed row: aggregate
            # the input per head, transform afterwards (same math, 1408 B -> 256 B gathered per edge on the Reddit GAT)
            with torch.autocast(x.device.type, enabled=False):   # f32 in, f32 GEMMs inside, f32 logits out
                y = eng.gat_headmean(edge_index, x, self.w, self.att, self.negative_slope, num_nodes=x.shape[0],
                                     dropout_rate=self.dropout_rate, training=self.training)
            # (bias_add: the bias gradient as the library's two-stage column sum instead of a torch reduce over [N, C])
            return eng.bias_add(y, self.bias) if self.bias is not None else y
        w = self.w
        pad = (-C) % 4 if C >= 8 else 0
        if pad:  # e.g. 41 classes per head: 44 channels inside the GEMM keep the kernels on 16-byte slices
            w = torch.nn.functional.pad(w.reshape(-1, H, C), (0, pad)).reshape(-1, H * (C + pad))
        x = node_matmul(x, w).reshape(-1, H, C + pad)
        xf = x[:, :, :C].float()                      # (x itself when it is f32) the logit terms are f32 whatever x is stored as
        el = (xf * self.att[:, :, :C]).sum(dim=-1)    # source term  a_src . x_j
        er = (xf * self.att[:, :, C:]).sum(dim=-1)    # destination term a_dst . x_i
        x = _engine(x).gat_fused(edge_index, el, er, x, self.negative_slope, num_nodes=num_nodes,
                                dropout_rate=self.dropout_rate, training=self.training)
        return self._finish(x[:, :, :C] if pad else x)


class AGNNConv(MessagePassing):
    """agnn_conv.py:40-69: X' = P X with P_ij = softmax_j(beta * cos(x_i, x_j)) over the edges j -> i; `beta` is the only
    parameter (uniform in [0, 1), or a constant 0 with require_grad=False).  fused=False is the reference's composition
    (segment_softmax on the [E] logits, then the weighted message sum); fused=True hands the logits and x to
    utils.edge_softmax_aggregate: one kernel per direction, no [E, K] message tensor."""

    def __init__(self, in_channels, require_grad=True, fused=True):
        super().__init__()
        self.in_channels, self.fused = in_channels, fused
        if require_grad:
            self.beta = nn.Parameter(torch.rand(1))
        else:
            self.beta = nn.Parameter(torch.zeros(1), requires_grad=False)

    def _logits(self, x, edge_index):
        xn = torch.nn.functional.normalize(x, p=2.0, dim=-1, eps=1e-12)   # tlx.l2_normalize
        cos = (xn[edge_index[0, :]] * xn[edge_index[1, :]]).sum(dim=-1)
        return cos * self.beta

    def forward(self, x, edge_index, num_nodes=None):
        num_nodes = x.shape[0] if num_nodes is None else num_nodes
        z = self._logits(x, edge_index)
        if self.fused:
            return edge_softmax_aggregate(edge_index, z, x, num_nodes)
        alpha = segment_softmax(z, edge_index[1, :], num_nodes)
        return self.propagate(x, edge_index, num_nodes=num_nodes, edge_weight=alpha)


class GATv2Conv(MessagePassing):
    """GATv2 ("How Attentive are Graph Attention Networks?").  variant="paper": xl = lin_l(x), xr = lin_r(x) (one Linear with
    share_weights), att [H, C], and
        z_ij = sum_c att[h, c] * LeakyReLU(xl_j + xr_i)[h, c],  alpha = softmax_i(z),  out_i = sum_j dropout(alpha_ij) xl_j,
    then concat or head mean, then the bias.  The LeakyReLU sits inside the channel sum: the logit does not separate.
    fused=True hands xl, xr and att to utils.gatv2_attention — no [E, H, C] tensor, attention dropout from the library's
    draw; fused=False is the message formula in torch: two [E, H, C] gathers, segment_softmax, torch dropout on alpha.

    variant="reference" reproduces layers/conv/gatv2_conv.py:94-119, which carries the name but scores an edge with
    mean_c(LeakyReLU(x_j) * att_src + LeakyReLU(x_i) * att_dst): a separable, static logit el[src] + er[dst] with
    el = mean_c(LeakyReLU(x) * att_src).  Parameters `linear` (no bias), `att_src`, `att_dst` [1, H, C], `bias`.  fused=True
    forms el and er on the nodes and goes through utils.edge_softmax_aggregate; fused=False is the reference's composition."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout_rate=0., add_bias=True,
                 share_weights=False, fused=True, variant="paper"):
        super().__init__()
        if variant not in ("paper", "reference"):
            raise ValueError(f"variant={variant!r}: paper or reference")
        self.in_channels, self.out_channels, self.heads, self.concat = in_channels, out_channels, heads, concat
        self.negative_slope, self.dropout_rate, self.fused, self.variant = negative_slope, dropout_rate, fused, variant
        self.share_weights = share_weights
        self.dropout = nn.Dropout(dropout_rate)   # on the attention coefficients
        if variant == "paper":
            self.lin_l = Linear(in_channels, heads * out_channels)
            self.lin_r = self.lin_l if share_weights else Linear(in_channels, heads * out_channels)
            self.att = nn.Parameter(nn.init.xavier_uniform_(torch.empty(heads, out_channels)))
        else:
            self.linear = Linear(in_channels, heads * out_channels, bias=False)
            self.att_src = nn.Parameter(nn.init.trunc_normal_(torch.empty(1, heads, out_channels), std=0.05, a=-0.1, b=0.1))
            self.att_dst = nn.Parameter(nn.init.trunc_normal_(torch.empty(1, heads, out_channels), std=0.05, a=-0.1, b=0.1))
        nb = heads * out_channels if concat else out_channels
        self.bias = nn.Parameter(torch.zeros(nb)) if add_bias else None

    def _finish(self, x):
        x = x.reshape(-1, self.heads * self.out_channels) if self.concat else x.mean(dim=1)
        return x + self.bias if self.bias is not None else x

    def forward(self, x, edge_index, num_nodes=None):
        H, C = self.heads, self.out_channels
        n = x.shape[0] if num_nodes is None else num_nodes
        src, dst = edge_index[0, :], edge_index[1, :]
        lrelu = torch.nn.functional.leaky_relu
        if self.variant == "paper":
            xl = self.lin_l(x).reshape(-1, H, C)
            xr = xl if self.share_weights else self.lin_r(x).reshape(-1, H, C)
            if self.fused:
                return self._finish(gatv2_attention(edge_index, xl, xr[:n], self.att, n, self.negative_slope,
                                                    self.dropout_rate, self.training))
            z = (self.att * lrelu(xl[src] + xr[dst], self.negative_slope)).sum(dim=-1)
        else:
            xl = self.linear(x).reshape(-1, H, C)
            act = lrelu(xl, self.negative_slope)
            if self.fused:   # the logit separates: its two terms are formed on the nodes
                el, er = (act * self.att_src).mean(dim=-1), (act * self.att_dst).mean(dim=-1)
                return self._finish(edge_softmax_aggregate(edge_index, el[src] + er[dst], xl, n, self.dropout_rate,
                                                           self.training))
            z = (act[src] * self.att_src + act[dst] * self.att_dst).mean(dim=-1)   # gatv2_conv.py:97-99
        alpha = self.dropout(segment_softmax(z, dst, n))
        return self._finish(self.aggregate(xl[src] * alpha.unsqueeze(-1), edge_index, num_nodes=n, aggr='sum'))


class HGTConv(MessagePassing):
    """hgt_conv.py:41-153, the Heterogeneous Graph Transformer layer: per node type k / q / v / a linears (relu6, as the
    reference's Linear(act='relu6')) and a sigmoid skip gate; per edge type (src, rel, dst) the head-wise maps a_rel, m_rel
    [H, D, D] and the prior p_rel [H].  For an edge type, with k' = k[src_type] a_rel and v' = v[src_type] m_rel on the nodes,
        alpha = softmax_dst(<k'_j, q_i> * p_rel / sqrt(D)),   out_i = sum_j dropout(alpha) v'_j;
    the outputs of the edge types that end in a node type are grouped (`group`: sum as the reference, mean, min, max), sent
    through a_lin and mixed with the input by the gate (in_channels of that type must equal out_channels, as there).
    fused=False is the reference's message(): three [E, H, D] gathers, segment_softmax, torch dropout on alpha.  fused=True
    hands q * (p_rel / sqrt(D)) — the prior applied on the nodes, where torch differentiates it — k' and v' to
    utils.dot_attention with scale = 1: no [E, H, D] tensor, attention dropout from the library's draw."""

    def __init__(self, in_channels, out_channels, metadata, heads=1, group='sum', dropout_rate=0., fused=True):
        super().__init__()
        if not isinstance(in_channels, dict):
            in_channels = {node_type: in_channels for node_type in metadata[0]}
        if out_channels % heads != 0:
            raise ValueError("out_channels must be a multiple of heads")
        if group not in ('sum', 'mean', 'min', 'max'):
            raise ValueError(f"group={group!r}: sum, mean, min or max")
        self.in_channels, self.out_channels, self.heads, self.group = in_channels, out_channels, heads, group
        self.dropout_rate, self.fused = dropout_rate, fused
        self.dropout = nn.Dropout(dropout_rate)
        self.k_lin, self.q_lin, self.v_lin, self.a_lin = nn.ModuleDict(), nn.ModuleDict(), nn.ModuleDict(), nn.ModuleDict()
        self.skip = nn.ParameterDict()
        for node_type, c in in_channels.items():
            self.k_lin[node_type] = Linear(c, out_channels)
            self.q_lin[node_type] = Linear(c, out_channels)
            self.v_lin[node_type] = Linear(c, out_channels)
            self.a_lin[node_type] = Linear(out_channels, out_channels)
            self.skip[node_type] = nn.Parameter(torch.tensor(1.0))
        self.a_rel, self.m_rel, self.p_rel = nn.ParameterDict(), nn.ParameterDict(), nn.ParameterDict()
        dim = out_channels // heads
        for edge_type in metadata[1]:
            name = '__'.join(edge_type)
            for table in (self.a_rel, self.m_rel):   # tlx.initializers.TruncatedNormal(): mean 0, stddev 0.05, cut at 2 sigma
                table[name] = nn.Parameter(nn.init.trunc_normal_(torch.empty(heads, dim, dim), std=0.05, a=-0.1, b=0.1))
            self.p_rel[name] = nn.Parameter(torch.ones(heads))

    def forward(self, x_dict, edge_index_dict):
        H, D = self.heads, self.out_channels // self.heads
        act = torch.nn.functional.relu6
        k_dict, q_dict, v_dict, out_dict = {}, {}, {}, {}
        for node_type, x in x_dict.items():
            k_dict[node_type] = act(self.k_lin[node_type](x)).reshape(-1, H, D)
            q_dict[node_type] = act(self.q_lin[node_type](x)).reshape(-1, H, D)
            v_dict[node_type] = act(self.v_lin[node_type](x)).reshape(-1, H, D)
            out_dict[node_type] = []
        for edge_type, edge_index in edge_index_dict.items():
            src_type, _, dst_type = edge_type
            name = '__'.join(edge_type)
            k = (k_dict[src_type].transpose(0, 1) @ self.a_rel[name]).transpose(0, 1)
            v = (v_dict[src_type].transpose(0, 1) @ self.m_rel[name]).transpose(0, 1)
            q, rel = q_dict[dst_type], self.p_rel[name]
            n_dst = x_dict[dst_type].shape[0]
            if self.fused:
                out = dot_attention(edge_index, q * (rel / math.sqrt(D))[None, :, None], k, v, num_nodes=n_dst, scale=1.0,
                                    dropout_rate=self.dropout_rate, training=self.training)
            else:
                src, dst = edge_index[0, :], edge_index[1, :]
                alpha = (k[src] * q[dst]).sum(dim=-1) * rel / math.sqrt(D)
                alpha = self.dropout(segment_softmax(alpha, dst, n_dst))
                out = self.aggregate(v[src] * alpha.unsqueeze(-1), edge_index, num_nodes=n_dst, aggr='sum')
            out_dict[dst_type].append(out.reshape(-1, self.out_channels))
        for node_type, outs in out_dict.items():
            if not outs:    # no edge type ends here (the reference's tlx.stack([]) raises)
                out_dict[node_type] = None
                continue
            outs = torch.stack(outs)
            out = {'sum': lambda t: t.sum(0), 'mean': lambda t: t.mean(0), 'min': lambda t: t.min(0)[0],
                   'max': lambda t: t.max(0)[0]}[self.group](outs)
            out = act(self.a_lin[node_type](out))
            gate = torch.sigmoid(self.skip[node_type])
            out_dict[node_type] = gate * out + (1 - gate) * x_dict[node_type]
        return out_dict


def _pool_size(batch, size):
    return int(batch.max()) + 1 if size is None else int(size)


def global_sum_pool(x, batch, size=None):
    """layers/pool/glob.py:5-30; batch=None reduces dimension 0."""
    if batch is None:
        return x.sum(dim=0, keepdim=True)
    return unsorted_segment_sum(x, batch, _pool_size(batch, size))


def global_mean_pool(x, batch, size=None):
    """layers/pool/glob.py:33-58."""
    if batch is None:
        return x.mean(dim=0, keepdim=True)
    return unsorted_segment_mean(x, batch, _pool_size(batch, size))


def global_max_pool(x, batch, size=None):
    """layers/pool/glob.py:61-86."""
    if batch is None:
        return x.max(dim=0, keepdim=True)[0]
    return unsorted_segment_max(x, batch, _pool_size(batch, size))


def global_min_pool(x, batch, size=None):
    """layers/pool/glob.py:89-114."""
    if batch is None:
        return x.min(dim=0, keepdim=True)[0]
    return unsorted_segment_min(x, batch, _pool_size(batch, size))


class PNAConv(MessagePassing):
    """pna_conv.py:82-201, Principal Neighbourhood Aggregation: per tower an edge MLP h(x_i, x_j[, edge_attr]) (pre_nns), the
    statistics named in `aggregators` (sum, mean, min, max, var, std) of the messages per destination, each degree scaler of
    `scalers` (identity, amplification, attenuation, linear, inverse_linear) applied to their concatenation, a node MLP
    (post_nns) on [x, scaled statistics] and one output Linear.  `deg` is the in-degree histogram the scalers normalise by.
    The edge MLP and the scalers (node-sized) stay in torch.  As in the reference (lines 186-200) a scaler multiplies the
    result of the scalers before it, and the destination degree is clamped at 1.
    fused=True aggregates through utils.segment_multi_aggregate (C = F_in, empty_zero): one walk of the [E, T, F_in] messages
    instead of one per statistic plus a tensor of squares.  fused=False is the reference's composition on the mpops ops
    (utils.segment_multi_composed), with min / max of destinations without edges zeroed the same way; its backward is the
    fused walk's formula written in torch in the same operation order, so the two routes agree on the bits, gradients
    included, wherever every destination's edges are walked in one piece."""

    AGGREGATORS = ("sum", "mean", "min", "max", "var", "std")
    SCALERS = ("identity", "amplification", "attenuation", "linear", "inverse_linear")

    def __init__(self, in_channels, out_channels, aggregators, scalers, deg, edge_dim=None, towers=1, pre_layers=1,
                 post_layers=1, divide_input=False, fused=True):
        super().__init__()
        if divide_input and in_channels % towers != 0:
            raise ValueError("divide_input: in_channels must be a multiple of towers")
        if out_channels % towers != 0:
            raise ValueError("out_channels must be a multiple of towers")
        for a in aggregators:
            if a not in self.AGGREGATORS:
                raise ValueError(f'Unknown aggregator "{a}".')
        for s in scalers:
            if s not in self.SCALERS:
                raise ValueError(f'Unknown scaler "{s}".')
        if len(set(aggregators)) != len(aggregators):
            raise ValueError("aggregators must be distinct")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.aggregators, self.scalers = tuple(aggregators), tuple(scalers)
        self.edge_dim, self.towers, self.divide_input, self.fused = edge_dim, towers, divide_input, fused
        self.F_in = in_channels // towers if divide_input else in_channels
        self.F_out = out_channels // towers
        deg = torch.as_tensor(deg).to(torch.float32).cpu()
        num_nodes = int(deg.sum())
        bins = torch.arange(deg.numel(), dtype=torch.float32)
        self.avg_deg = {'lin': float((bins * deg).sum()) / num_nodes,
                        'log': float((torch.log(bins + 1) * deg).sum()) / num_nodes,
                        'exp': float((torch.exp(bins) * deg).sum()) / num_nodes}
        if edge_dim is not None:
            self.edge_encoder = Linear(edge_dim, self.F_in)
        self.pre_nns, self.post_nns = nn.ModuleList(), nn.ModuleList()
        for _ in range(towers):
            mods = [Linear((3 if edge_dim else 2) * self.F_in, self.F_in)]
            for _ in range(pre_layers - 1):
                mods += [nn.ReLU(), Linear(self.F_in, self.F_in)]
            self.pre_nns.append(nn.Sequential(*mods))
            mods = [Linear((len(aggregators) * len(scalers) + 1) * self.F_in, self.F_out)]
            for _ in range(post_layers - 1):
                mods += [nn.ReLU(), Linear(self.F_out, self.F_out)]
            self.post_nns.append(nn.Sequential(*mods))
        self.lin = Linear(out_channels, out_channels)

    def forward(self, x, edge_index, edge_attr=None):
        if self.divide_input:
            x = x.reshape(-1, self.towers, self.F_in)
        else:
            x = torch.stack([x for _ in range(self.towers)], dim=1)
        n = x.shape[0]
        out = self.aggregate(self.message(x, edge_index, edge_attr), edge_index, num_nodes=n)
        out = torch.cat([x, out], dim=-1)
        out = torch.cat([net(out[:, i]) for i, net in enumerate(self.post_nns)], dim=1)
        return self.lin(out)

    def message(self, x, edge_index, edge_attr=None):
        x_j, x_i = x[edge_index[0]], x[edge_index[1]]
        if edge_attr is not None:
            e = self.edge_encoder(edge_attr)
            h = torch.cat([x_i, x_j, torch.stack([e for _ in range(self.towers)], dim=1)], dim=-1)
        else:
            h = torch.cat([x_i, x_j], dim=-1)
        return torch.stack([net(h[:, i]) for i, net in enumerate(self.pre_nns)], dim=1)

    def aggregate(self, inputs, index, num_nodes=None, aggr=None):
        dst = index[1]
        dst = dst if dst.is_contiguous() else dst.contiguous()
        n = int(dst.max()) + 1 if num_nodes is None else int(num_nodes)
        deg = degree(dst, n, dtype=inputs.dtype)
        if self.fused:
            out = segment_multi_aggregate(inputs, dst, n, self.aggregators, empty_zero=True)
        else:
            out = segment_multi_composed(inputs, dst, n, self.aggregators, empty_zero=True)
        deg = torch.where(deg > 1, deg, torch.ones_like(deg)).reshape(-1, 1, 1)
        outs = []
        for s in self.scalers:
            if s == 'amplification':
                out = out * (torch.log(deg + 1) / self.avg_deg['log'])
            elif s == 'attenuation':
                out = out * (self.avg_deg['log'] / torch.log(deg + 1))
            elif s == 'linear':
                out = out * (deg / self.avg_deg['lin'])
            elif s == 'inverse_linear':
                out = out * (self.avg_deg['lin'] / deg)
            outs.append(out)
        return torch.cat(outs, dim=-1)


class GCNModel(nn.Module):
    """models/gcn.py:30-64."""

    def __init__(self, feature_dim, hidden_dim, num_class, drop_rate=0.2, num_layers=2, norm='both', fuse_epilogue16=True):
        """`fuse_epilogue16`: under torch.autocast the layers apply bias, ReLU and dropout in the 16-bit aggregate's store
        (GCNConv.fuse_epilogue16); False keeps the torch composition after the aggregate.  No effect on f32 activations."""
        super().__init__()
        self.num_layers = num_layers
        if num_layers == 1:
            self.conv = nn.ModuleList([GCNConv(feature_dim, num_class, norm=norm)])
        else:
            self.conv = nn.ModuleList([GCNConv(feature_dim, hidden_dim, norm=norm)])
            for _ in range(1, num_layers - 1):
                self.conv.append(GCNConv(hidden_dim, hidden_dim, norm=norm))
            self.conv.append(GCNConv(hidden_dim, num_class, norm=norm))
        self.dropout = nn.Dropout(drop_rate)
        for conv in self.conv:
            conv.fuse_epilogue16 = bool(fuse_epilogue16)

    def forward(self, x, edge_index, edge_weight, num_nodes):
        if self.num_layers == 1:
            return self.conv[0](x, edge_index, edge_weight, num_nodes)
        for i in range(self.num_layers - 1):
            # relu(conv(x)) then dropout (models/gcn.py:55-59), handed to the layer so that bias, ReLU and
            # dropout ride on the aggregate's store instead of three more passes over [N, hidden]
            x = self.conv[i](x, edge_index, edge_weight, num_nodes,
                             _epilogue=(True, self.dropout.p, self.training))
        return self.conv[-1](x, edge_index, edge_weight, num_nodes)


class GATModel(nn.Module):
    """models/gat.py:4-73: dropout -> GATConv (-> ELU) per layer, attention dropout inside the conv, the
    last layer averages its heads.  `fused=True` uses FusedGATConv (one kernel per direction)."""

    def __init__(self, feature_dim, hidden_dim, num_class, heads, drop_rate, num_layers, fused=True):
        super().__init__()
        conv = FusedGATConv if fused else GATConv
        if num_layers == 1:
            hidden_dim = num_class
        self.gat_list = nn.ModuleList()
        for i in range(num_layers):
            if i == 0:
                self.gat_list.append(conv(feature_dim, hidden_dim, heads=heads, dropout_rate=drop_rate, concat=True))
            elif i == num_layers - 1:
                self.gat_list.append(conv(hidden_dim * heads, num_class, heads=heads, dropout_rate=drop_rate,
                                          concat=False))
            else:
                self.gat_list.append(conv(hidden_dim * heads, hidden_dim, heads=heads, dropout_rate=drop_rate,
                                          concat=True))
        self.dropout = nn.Dropout(drop_rate)

    def forward(self, x, edge_index, num_nodes):
        for i, gat in enumerate(self.gat_list):
            x = gat(self.dropout(x), edge_index, num_nodes)
            if i < len(self.gat_list) - 1:
                x = torch.nn.functional.elu(x)
        return x


class GraphSAGEFullModel(nn.Module):
    """models/graphsage.py:7-32 (GraphSAGE_Full_Model): full-graph GraphSAGE — dropout on the input, n_layers
    hidden SAGEConv layers with `activation`, an output SAGEConv without, dropout between layers.  On a big edge
    list every mean / gcn aggregate takes the fused SpMM route (MessagePassing.propagate)."""

    def __init__(self, in_feats, n_hidden, n_classes, n_layers, activation, dropout, aggregator_type):
        super().__init__()
        self.dropout = nn.Dropout(dropout)
        convs = [SAGEConv(in_feats, n_hidden, activation, aggregator_type)]
        convs += [SAGEConv(n_hidden, n_hidden, activation, aggregator_type) for _ in range(n_layers - 1)]
        convs += [SAGEConv(n_hidden, n_classes, None, aggregator_type)]
        self.convs = nn.ModuleList(convs)

    def forward(self, feat, edge):
        h = self.dropout(feat)
        for i, layer in enumerate(self.convs):
            h = layer(h, edge)
            if i != len(self.convs) - 1:
                h = self.dropout(h)
        return h


class GraphSAGESampleModel(nn.Module):
    """models/graphsage.py:35-83 (GraphSAGE_Sample_Model): SAGEConv(mean) per sampled hop; the target
    nodes of a block are the first size[1] rows of its input ("target nodes are always placed first")."""

    def __init__(self, in_feat, hid_feat, out_feat, drop_rate=0.0, num_layers=2):
        super().__init__()
        self.dropout = nn.Dropout(drop_rate)
        if num_layers == 1:
            self.convs = nn.ModuleList([SAGEConv(in_feat, out_feat)])
        else:
            convs = [SAGEConv(in_feat, hid_feat, torch.relu)]
            convs += [SAGEConv(hid_feat, hid_feat, torch.relu) for _ in range(num_layers - 2)]
            convs += [SAGEConv(hid_feat, out_feat)]
            self.convs = nn.ModuleList(convs)

    def forward(self, x, adjs):
        adjs = adjs if isinstance(adjs, (list, tuple)) else [adjs]
        for i, (conv, adj) in enumerate(zip(self.convs, adjs)):
            x = conv((x, x[: adj.size[1]]), adj if isinstance(adj, Block) else adj.edge_index)
            if i != len(self.convs) - 1:
                x = self.dropout(x)
        return x

    @torch.no_grad()
    def inference(self, feat, sampler, batch_size=4096):
        """models/graphsage.py:85-103: layer by layer over ALL nodes with one full-neighbourhood hop per batch
        (a NeighborSampler built with sample_lists=[-1]); returns the logits of every node."""
        n = feat.shape[0]
        for i, layer in enumerate(self.convs):
            out = None
            for b in range(0, n, batch_size):
                dst = torch.arange(b, min(n, b + batch_size), device=feat.device)
                _, n_id, adj = sampler.sample(dst)
                adj = adj[0] if isinstance(adj, (list, tuple)) else adj
                h = feat[n_id]
                h = layer((h, h[: adj.size[1]]), adj.edge_index)
                if out is None:
                    out = torch.empty((n, h.shape[1]), dtype=h.dtype, device=h.device)
                out[dst] = h
            feat = out
        return feat


__all__ = ["MessagePassing", "GCNConv", "SAGEConv", "GATConv", "FusedGATConv", "HGTConv", "GATv2Conv", "GCNModel", "GATModel", "GraphSAGEFullModel", "GraphSAGESampleModel", "degree",
           "calc_gcn_norm", "segment_softmax", "add_self_loops"]
