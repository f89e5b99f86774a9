#!/usr/bin/env python3
"""A GATv2 node classifier on the MI355X backend: examples/gat_trainer_amd.py's flow with layers.GATv2Conv, whose attention
logit is the paper's att . LeakyReLU(W_l x_j + W_r x_i), fused into the edge-softmax aggregate (utils.gatv2_attention).

Two layers (heads x hidden_dim concatenated, ELU, then one head-averaged output layer), dropout on the features and on the
attention coefficients, self-loops added once, Adam with weight decay, cross-entropy on the train nodes.  Trains on a seeded
Cora-sized homophilous synthetic graph (datasets cannot be downloaded here).

    python examples/gatv2_trainer_amd.py --n_epoch 100 [--no-fused] [--variant reference] [--share_weights]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gammagl_amd.layers import GATv2Conv, add_self_loops  # noqa: E402
from gammagl_amd.synth import homophilous_graph  # noqa: E402


class GATv2Model(torch.nn.Module):
    def __init__(self, feature_dim, hidden_dim, num_class, heads, drop_rate, num_layers, **conv):
        super().__init__()
        dims = [feature_dim] + [hidden_dim * heads] * (num_layers - 1)
        self.convs = torch.nn.ModuleList(
            [GATv2Conv(d, hidden_dim, heads=heads, dropout_rate=drop_rate, **conv) for d in dims[:-1]]
            + [GATv2Conv(dims[-1], num_class, heads=heads, concat=False, dropout_rate=drop_rate, **conv)])
        self.dropout = torch.nn.Dropout(drop_rate)

    def forward(self, x, edge_index, num_nodes):
        for conv in self.convs[:-1]:
            x = F.elu(conv(self.dropout(x), edge_index, num_nodes))
        return self.convs[-1](self.dropout(x), edge_index, num_nodes)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--lr", type=float, default=0.005)
    p.add_argument("--n_epoch", type=int, default=200)
    p.add_argument("--hidden_dim", type=int, default=8)
    p.add_argument("--heads", type=int, default=8)
    p.add_argument("--drop_rate", type=float, default=0.6)
    p.add_argument("--num_layers", type=int, default=2)
    p.add_argument("--l2_coef", type=float, default=5e-4)
    p.add_argument("--no-fused", dest="fused", action="store_false", help="the message formula in torch instead of the fused op")
    p.add_argument("--variant", choices=["paper", "reference"], default="paper")
    p.add_argument("--share_weights", action="store_true")
    p.add_argument("--gpu", type=int, default=0)
    args = p.parse_args()
    dev = torch.device("cuda", args.gpu) if args.gpu >= 0 else torch.device("cpu")
    n, f, c = 2708, 1433, 7
    x, y, edge_index = homophilous_graph(n, f, c, deg=2, seed=0, device=dev)
    edge_index = add_self_loops(edge_index, n)
    perm = torch.randperm(n, generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    train_idx, val_idx, test_idx = perm[:140], perm[140:640], perm[640:1640]
    torch.manual_seed(0)
    conv = dict(fused=args.fused, variant=args.variant)
    if args.variant == "paper":
        conv["share_weights"] = args.share_weights
    net = GATv2Model(f, args.hidden_dim, c, args.heads, args.drop_rate, args.num_layers, **conv).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=args.lr, weight_decay=args.l2_coef)
    best_val, best_state = 0.0, None
    for epoch in range(args.n_epoch):
        net.train()
        opt.zero_grad(set_to_none=True)
        out = net(x, edge_index, n)
        loss = F.cross_entropy(out[train_idx], y[train_idx])
        loss.backward()
        opt.step()
        net.eval()
        with torch.no_grad():
            logits = net(x, edge_index, n)
        val_acc = float((logits[val_idx].argmax(1) == y[val_idx]).float().mean())
        if epoch % 10 == 0 or epoch == args.n_epoch - 1:
            print("Epoch [{:0>3d}]   train loss: {:.4f}  val acc: {:.4f}".format(epoch + 1, float(loss.detach()), val_acc))
        if val_acc > best_val or best_state is None:
            best_val, best_state = val_acc, {k: v.clone() for k, v in net.state_dict().items()}
    net.load_state_dict(best_state)
    net.eval()
    with torch.no_grad():
        logits = net(x, edge_index, n)
    print("Test acc:  {:.4f}".format(float((logits[test_idx].argmax(1) == y[test_idx]).float().mean())))


if __name__ == "__main__":
    main()
