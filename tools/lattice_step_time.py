#!/usr/bin/env python3
"""ms/step of the LATTICE training step at the sports shape (35,598 users, 18,357 items, raw
features 4096 / 384 wide, d = 64, B = 2048, cf_model lightgcn with two UI layers, one item
layer, knn_k 10) on rsx.synth data, and ms of the once-per-epoch item-graph build.

Measured, each as `--repeats` windows of `--steps` iterations between two device events after
a warm-up on the timed shape (median, and minimum / maximum as the spread):
  * the steady step (zero_grad, forward, loss, backward, RsxAdam) replayed from the Trainer's
    captured graph and launched eagerly, the HIP variant ALTERNATED window by window with
    the same step whose loss (lattice.py:199-227) and item propagation (gather, scale and
    sum on the same edge table) are composed from torch ops;
  * the build, forward (projections, rsx_knn_graph on both projected tables,
    rsx_lattice_graph, the transpose index) and backward (rsx_lattice_graph_bwd alone, and
    the build batch's whole backward), each window a number of builds;
  * the dense matrices the reference would hold (bytes), for scale.
Prints one JSON line.  Needs a GPU: there is no CPU fallback for the measured path.

Usage:  python tools/lattice_step_time.py [--steps 100] [--repeats 5] [--warmup 20] [--scale 1.0]
"""
from __future__ import annotations

import json

import torch
import torch.nn.functional as F

from _step_time import alternated, parser, require_gpu, synth_model, trainer_runs


class TorchLoss:
    """rsx.lattice._LatticeLoss's call shape with lattice.py:199-227's torch ops."""

    @staticmethod
    def apply(cfg, triplets, E, H):
        n_users, reg, batch_size, _, keep = cfg
        ia = E[n_users:] + F.normalize(H, p=2, dim=1)
        eu, ep, en = E[:n_users][triplets[0]], ia[triplets[1]], ia[triplets[2]]
        x = (eu * ep).sum(1) - (eu * en).sum(1)
        l2 = 0.5 * ((eu * eu).sum() + (ep * ep).sum() + (en * en).sum())
        total = -F.logsigmoid(x).mean() + reg * l2 / batch_size
        if keep is not None:
            keep["terms"] = total.detach()
        return total


class TorchProp:
    """rsx.lattice._ItemProp's call shape composed from torch ops on the same edge table (the
    steady batch: the graph is a constant): gather the K neighbour rows, scale, sum.  (A torch
    sparse product did not capture in a HIP graph, and the reference's dense torch.mm needs the
    n x n matrix.)"""

    cache = {}

    @classmethod
    def apply(cls, h0, g, n_layers, build, mw, *Fs):
        col = cls.cache.get(id(g))
        if col is None:
            col = g.col.long()
            cls.cache = {id(g): col}
        h = h0
        for _ in range(n_layers):
            h = (g.val.unsqueeze(-1) * h[col]).sum(1)
        return h


def main():
    ap = parser(steps=100, warmup=20)
    ap.add_argument("--builds", type=int, default=5, help="builds per timed window")
    args = ap.parse_args()
    require_gpu("lattice_step_time", args)
    from rsx import lattice

    m, c, batches, n_edges = synth_model(
        "LATTICE", "sports", args, dict(reg_weight=0.001, learning_rate=0.001, is_multimodal_model=True),
        (("image_feat.npy", 4096, 5), ("text_feat.npy", 384, 6)))
    m.train()
    d, B, nu, ni = m.embedding_dim, 2048, m.n_users, m.n_items
    res = {"n_users": nu, "n_items": ni, "train_edges": n_edges, "d": d, "F": [4096, 384], "batch": B,
           "n_ui_layers": m.n_ui_layers, "n_layers": m.n_layers, "knn_k": m.knn_k, "steps_per_window": args.steps,
           "windows": args.repeats, "format": "[median, min, max] ms",
           "reference_dense_matrix_bytes": 4 * ni * ni, "edge_table_bytes": 8 * ni * 4 * m.knn_k}

    fused = (lattice._LatticeLoss, lattice._ItemProp)
    # ---- the build: forward, the graph's backward alone, the build batch's whole backward
    def build_fwd():
        with torch.no_grad():
            return m.build_graph()

    g = build_fwd()
    h0 = m.item_id_embedding.weight.detach()
    G = torch.randn_like(h0)

    def build_batch_bwd():
        m.build_item_graph = True
        m.calculate_loss(batches[0]).backward()
        m.zero_grad(set_to_none=True)

    res.update(alternated(args, {"build_fwd": build_fwd, "graph_bwd": lambda: g.backward([G], [h0]),
                                 "build_batch_fwd_bwd": build_batch_bwd}, steps=args.builds))

    # ---- the steady step through the Trainer, HIP and torch-composed alternated
    m.pre_epoch_processing()
    m.calculate_loss(batches[0]).backward()  # the epoch's build: every later batch is steady
    m.zero_grad(set_to_none=True)
    def use(pair):
        def select():
            lattice._LatticeLoss, lattice._ItemProp = pair
        return select

    res.update(trainer_runs(args, c, m, batches, {"hip": use(fused), "torch_ops": use((TorchLoss, TorchProp))}))
    lattice._LatticeLoss, lattice._ItemProp = fused

    print(json.dumps(res))


if __name__ == "__main__":
    main()
