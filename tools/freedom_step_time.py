#!/usr/bin/env python3
"""ms/step of the FREEDOM training step at the sports shape (35,598 users, 18,357 items, raw
features 4096 / 384 wide, d = 64, B = 2048, dropout 0.8, n_ui_layers 2, n_mm_layers 1,
knn_k 10) on rsx.synth data, against the same step with the loss composed from torch ops as
reference src/models/freedom.py:182-212 writes it.

Measured, each as `--repeats` windows of `--steps` iterations between two device events after
a warm-up on the timed shape (median, and minimum / maximum as the spread), the fused and
the torch variant ALTERNATED window by window in one process:
  * the whole step (zero_grad, forward, loss, backward, RsxAdam) replayed from the Trainer's
    captured graph, and launched eagerly;
  * the loss alone, forward plus backward on fixed tables, eager and graph-replayed;
  * the whole step split by phase (eager, device events between the phases), with the share
    of the whole-table projections and of Adam over the two raw feature tables;
  * kernel launches per eager step and the per-kernel device time (torch.profiler).
Prints one JSON line.  Needs a GPU: there is no CPU fallback for the measured path.

Usage:  python tools/freedom_step_time.py [--steps 100] [--repeats 5] [--warmup 20] [--scale 1.0]
"""
from __future__ import annotations

import json

import torch
import torch.nn.functional as F

from _step_time import (alternated, captured, not_measured, parser, require_gpu, stage_times, synth_model,
                        trainer_runs)


# ------------------------------------------------------------ the comparator loss
def _bpr_loss(users, pos_items, neg_items):
    """freedom.py:182-189 as written."""
    pos_scores = torch.sum(torch.mul(users, pos_items), dim=1)
    neg_scores = torch.sum(torch.mul(users, neg_items), dim=1)
    return -torch.mean(F.logsigmoid(pos_scores - neg_scores))


class TorchLoss:
    """rsx.freedom._FreedomLoss's call shape with freedom.py:191-212's torch ops."""

    @staticmethod
    def apply(cfg, triplets, E, H, T, V, bias_t, bias_v):
        n_users, reg, _, keep = cfg
        users, pos_items, neg_items = triplets[0], triplets[1], triplets[2]
        ua_embeddings, ia_embeddings = E[:n_users], E[n_users:] + H
        u_g = ua_embeddings[users]
        mf = _bpr_loss(u_g, ia_embeddings[pos_items], ia_embeddings[neg_items])
        mf_t = mf_v = 0.0
        if T is not None:
            mf_t = _bpr_loss(ua_embeddings[users], T[pos_items], T[neg_items])
        if V is not None:
            mf_v = _bpr_loss(ua_embeddings[users], V[pos_items], V[neg_items])
        total = mf + reg * (mf_t + mf_v)
        for b in (bias_t, bias_v):  # the model hands the biases to the loss for their (zero) gradient
            if b is not None:
                total = total + 0.0 * b.sum()
        if keep is not None:
            keep["terms"] = total.detach()
        return total


def loss_bytes(n_users: int, n_items: int, d: int, B: int) -> dict:
    """Bytes the fused loss has to move (f32 rows of 4 d bytes).  Forward: 9 rows a triplet
    read (the user row; positive and negative of E, H, T, V).  Backward: the same 9 rows read
    again, one contribution row a triplet written and read back, the zero fill of every row of
    gE, gT, gV, one user row read per item occurrence (2 B; one read serves gE, gT and gV), and
    at most B + 3 * 2 B summed rows written."""
    row = 4 * d
    return {"fwd_bytes": 9 * B * row,
            "bwd_bytes": (9 * B + 2 * B + (n_users + 3 * n_items) + 2 * B + 7 * B) * row,
            "bwd_zero_fill_bytes": (n_users + 3 * n_items) * row}


def main():
    args = parser(steps=100, warmup=20).parse_args()
    require_gpu("freedom_step_time", args)
    from rsx import freedom
    from rsx.blocks import _ego, ui_backbone
    from rsx.dense import _Project
    from rsx.optim import RsxAdam

    fused = freedom._FreedomLoss
    m, c, batches, n_edges = synth_model(
        "FREEDOM", "sports", args, dict(dropout=0.8, reg_weight=0.001, is_multimodal_model=True),
        (("image_feat.npy", 4096, 5), ("text_feat.npy", 384, 6)))
    m.train()
    m.pre_epoch_processing()  # one epoch graph (device edge dropout) for every measurement
    d, B, nu, ni = m.embedding_dim, 2048, m.n_users, m.n_items
    res = {"n_users": nu, "n_items": ni, "train_edges": n_edges, "epoch_graph_nnz": m.train_adj.nnz, "d": d,
           "F": [4096, 384], "batch": B, "dropout": m.dropout, "n_ui_layers": m.n_ui_layers, "n_mm_layers": m.n_layers,
           "knn_k": m.knn_k, "steps_per_window": args.steps, "windows": args.repeats,
           "format": "[median, min, max] ms", "loss_bytes": loss_bytes(nu, ni, d, B)}

    # ---- whole steps through the Trainer, fused and torch loss alternated
    def use(cls):
        def select():
            freedom._FreedomLoss = cls
        return select

    # (this tool times the captured steps first, as it always has: its JSON lists them first)
    res.update(trainer_runs(args, c, m, batches, {"fused": use(fused), "torch_loss": use(TorchLoss)},
                            order=(True, False)))
    freedom._FreedomLoss = fused

    # ---- the loss alone, forward + backward on fixed tables
    g = torch.Generator(device="cuda").manual_seed(3)
    rnd = lambda *s: (torch.randn(*s, device="cuda", generator=g) * 0.1).requires_grad_()  # noqa: E731
    E, H, T, V = rnd(nu + ni, d), rnd(ni, d), rnd(ni, d), rnd(ni, d)
    ws = freedom.workspace(B, d, m.device)
    cfg = (nu, m.reg_weight, ws, None)
    alone = {name: (lambda cls=cls: torch.autograd.grad(cls.apply(cfg, batches[0], E, H, T, V, None, None),
                                                        [E, H, T, V]))
             for name, cls in (("loss_fused", fused), ("loss_torch", TorchLoss))}
    res.update({k + "_eager": v for k, v in alternated(args, alone).items()})
    graphs = {}
    for name, run in alone.items():
        try:
            graphs[name + "_graph"] = captured(run)
        except RuntimeError as e:
            res[name + "_graph"] = not_measured(e)
    if graphs:
        res.update(alternated(args, graphs))

    # ---- the whole-step split (eager): device events between the phases
    feat = [m.image_embedding.weight, m.text_embedding.weight]
    rest = [p for p in m.parameters() if all(p is not f for f in feat)]
    opt_feat, opt_rest = RsxAdam(feat, lr=1e-3), RsxAdam(rest, lr=1e-3)
    names = ("ui_prop_fwd", "item_prop_fwd", "proj_fwd", "loss_fwd", "loss_bwd", "proj_bwd", "item_prop_bwd",
             "ui_prop_bwd", "adam_feature_tables", "adam_rest")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
    leaf = lambda *xs: [None if x is None else x.detach().requires_grad_() for x in xs]  # noqa: E731
    off = torch.cat([torch.zeros(B, dtype=torch.int64), torch.full((2 * B,), nu)]).cuda()

    def one_step(it):
        opt_feat.zero_grad(set_to_none=True)
        opt_rest.zero_grad(set_to_none=True)
        trip = batches[it % len(batches)]
        rows = trip.reshape(-1) + off
        ev[0].record()
        Et = ui_backbone(m, _ego(m.user_embedding.weight, m.item_id_embedding.weight), m.train_adj, m.n_ui_layers, rows)
        ev[1].record()
        Ht = m._item_prop()
        ev[2].record()
        Tt = _Project.apply(m.text_embedding.weight, m.text_trs.weight, m.text_trs.bias.detach())
        Vt = _Project.apply(m.image_embedding.weight, m.image_trs.weight, m.image_trs.bias.detach())
        ev[3].record()
        lf = leaf(Et, Ht, Tt, Vt)
        loss = fused.apply((nu, m.reg_weight, m._ws, None), trip, *lf, m.text_trs.bias, m.image_trs.bias)
        ev[4].record()
        loss.backward()
        ev[5].record()
        torch.autograd.backward([Tt, Vt], [lf[2].grad, lf[3].grad])
        ev[6].record()
        Ht.backward(lf[1].grad)
        ev[7].record()
        Et.backward(lf[0].grad)
        ev[8].record()
        opt_feat.step()
        ev[9].record()
        opt_rest.step()
        ev[10].record()
        return loss

    split, acc, loss = stage_times(args, names, ev, one_step)
    split["share_projections"] = round(float(acc[2] + acc[5]) / float(acc.sum()), 4)
    split["share_adam_feature_tables"] = round(float(acc[8]) / float(acc.sum()), 4)
    split["share_loss"] = round(float(acc[3] + acc[4]) / float(acc.sum()), 4)
    res["split_eager_ms"] = split
    assert bool(torch.isfinite(loss))

    # ---- launches per step and the per-kernel device time (eager steps under torch.profiler)
    try:
        from torch.profiler import ProfilerActivity, profile

        n_prof = 10
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for it in range(n_prof):
                one_step(it)
                torch.cuda.synchronize()
        rows = [(e.key, e.count, getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0))
                for e in prof.key_averages()]
        rows = [r for r in rows if r[2] > 0]
        rows.sort(key=lambda r: -r[2])
        res["launches_per_step"] = round(sum(r[1] for r in rows) / n_prof, 1)
        res["kernels_us_per_step"] = [[r[0][:90], round(r[1] / n_prof, 1), round(r[2] / n_prof, 2)] for r in rows[:24]]
    except Exception as e:  # noqa: BLE001 - a profiler that cannot run here is reported, not hidden
        res["launches_per_step"] = "not measured: " + str(e).splitlines()[0][:160]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
