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

import argparse
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "recommendar-systems_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


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


def build(args, root):
    from scipy.sparse import coo_matrix

    from rsx import synth
    from rsx.config import Config
    from rsx.lattice import LATTICE
    from rsx.utils import init_seed

    df = synth.shaped("sports", seed=0, scale=args.scale)
    df = df[df.x_label == 0]
    nu, ni = int(df.userID.max()) + 1, int(df.itemID.max()) + 1
    os.makedirs(os.path.join(root, "sports"))
    np.save(os.path.join(root, "sports", "image_feat.npy"), synth.features(ni, 4096, seed=5))
    np.save(os.path.join(root, "sports", "text_feat.npy"), synth.features(ni, 384, seed=6))
    c = Config("LATTICE", "sports", dict(data_path=root + "/", train_batch_size=2048, reg_weight=0.001,
                                         learning_rate=0.001, seed=999, is_multimodal_model=True))
    ds = types.SimpleNamespace(get_user_num=lambda: nu, get_item_num=lambda: ni)
    loader = types.SimpleNamespace(dataset=ds, inter_matrix=lambda form="coo": coo_matrix(
        (np.ones(len(df)), (df.userID.values, df.itemID.values)), shape=(nu, ni)))
    init_seed(999)
    m = LATTICE(c, loader)
    rng = np.random.default_rng(1)
    sel = rng.permutation(len(df))[: 4 * 2048].reshape(4, 2048)
    batches = [torch.from_numpy(np.stack([df.userID.values[s], df.itemID.values[s],
                                          rng.integers(0, ni, 2048)]).astype(np.int64)).cuda() for s in sel]
    return m, c, batches, len(df)


def alternated(args, runs: dict, steps=None) -> dict:
    """ms per iteration of each run in `runs`, their windows alternated: name -> [median, min, max]."""
    steps = steps or args.steps
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for run in runs.values():
        for _ in range(min(args.warmup, steps)):
            run()
    torch.cuda.synchronize()
    out = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, run in runs.items():
            e0.record()
            for _ in range(steps):
                run()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) / steps)
    return {k: [round(sorted(v)[len(v) // 2], 4), round(min(v), 4), round(max(v), 4)] for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100, help="iterations per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per variant (median, min, max reported)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--builds", type=int, default=5, help="builds per timed window")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graph (a rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lattice_step_time: needs a GPU (step times are device measurements)")
    if args.repeats < 5:
        raise SystemExit("lattice_step_time: at least 5 windows")
    from rsx import lattice
    from rsx.trainer import Trainer

    with tempfile.TemporaryDirectory() as root:
        m, c, batches, n_edges = build(args, root)
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
    for graph in (False, True):  # the captures last: a failed capture leaves the stream unusable
        c["rsx_graph_step"] = graph
        runs = {}
        for name, pair in (("hip", fused), ("torch_ops", (TorchLoss, TorchProp))):
            t = Trainer(c, m)
            k = [0]

            def step(t=t, k=k, pair=pair):
                lattice._LatticeLoss, lattice._ItemProp = pair
                t.train_step(batches[k[0] % len(batches)], k[0])
                k[0] += 1

            runs[f"step_{name}_{'graph' if graph else 'eager'}"] = step
        try:
            res.update(alternated(args, runs))
        except RuntimeError as e:
            if not graph:
                raise
            res["step_graph"] = "not measured: " + str(e).splitlines()[0][:160]
    lattice._LatticeLoss, lattice._ItemProp = fused

    print(json.dumps(res))


if __name__ == "__main__":
    main()
