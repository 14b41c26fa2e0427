#!/usr/bin/env python3
"""ms/step of the SELFCFED_LGN training step at the sports shape (35,598 users, 18,357 items, d = 64,
B = 2048, 2 layers, dropout 0.3) on rsx.synth data, against the same step with the per-step edge
dropout and the loss written as torch ops.

Measured, each as `--repeats` windows of `--steps` iterations between two device events after a
warm-up on the timed shape (median, and minimum / maximum as the spread):
  * the whole step (zero_grad, edge drop, propagation, loss, backward, RsxAdam) launched eagerly,
    and replayed from the Trainer's captured graph;
  * the same with the comparator: the edge dropout as a torch.rand mask, torch.where and an
    index_select of the values into the same two value buffers, and the loss as F.linear, F.dropout
    and cosine_similarity on the gathered rows (reference src/models/selfcfed_lgn.py:41-69 as
    written), around the same propagation and optimizer;
  * the loss part alone, forward plus backward on a fixed table: the fused kernels
    (rsx_selfcf_loss_fwd / _bwd) and the torch composition, eager and graph-replayed;
  * the edge drop alone: the one launch (rsx_selfcf_edge_drop) and the torch composition, replayed;
  * the whole-step split by phase (eager, device events between the phases): edge drop, propagation
    forward, loss forward + backward, propagation backward, Adam; and the edge drop's share.
Prints one JSON line.  Needs a GPU: there is no CPU fallback for the measured path.

Usage:  python tools/selfcf_step_time.py [--steps 200] [--repeats 5] [--warmup 30] [--scale 1.0]
"""
from __future__ import annotations

import json

import torch
import torch.nn.functional as F

from _step_time import alternated, captured, not_measured, parser, require_gpu, stage_times, synth_model, trainer_step


def step_bytes(n: int, nnz: int, d: int, B: int, K: int) -> dict:
    """Bytes the new launches must move (f32 / int32 / int64), from the shapes.  Edge drop: val0 and
    rev read, val and valT written.  Loss forward: the 2 B online rows read by the predictor and
    again by the cosines, the predicted rows written and read, the index lists.  Loss backward: gE
    cleared, the online and predicted rows read, the gradient rows written and read twice (G P,
    G^T x), the online rows read by the weight gradient, dX written and read by the walk, the
    batch's rows of gE written."""
    row = 4 * d
    drop = 16 * nnz
    fwd = 2 * (2 * B) * row + 2 * (2 * B) * row + 2 * B * (8 + 8 + 4 + 4)
    bwd = n * row + 2 * (2 * B) * row + 3 * (2 * B) * row + (2 * B) * row + 2 * (2 * B) * row + (2 * B) * row
    return {"edge_drop": drop, "loss_fwd": fwd, "loss_bwd": bwd, "dense_layer_products": 2 * K}


def torch_drop(g, rev64, zero):
    """The per-step dropped graph as torch ops (encoders.py:80-96 on a fixed structure): a rate, a
    mask, the scaled values, and their transpose through an index_select."""
    rate = torch.rand((), device=g.val0.device)
    keep = torch.rand(g.nnz, device=g.val0.device) >= rate
    val = torch.where(keep, g.val0 / (1 - rate), zero)
    g.val.copy_(val)
    g.valT.copy_(val.index_select(0, rev64))


def torch_loss(m, E, P, pb, users, items):
    """The loss part as the reference writes it (selfcfed_lgn.py:41-69) on the given table."""
    xu, xi = E[users], E[m.n_users + items]
    with torch.no_grad():
        tu, ti = F.dropout(xu.clone(), m.dropout), F.dropout(xi.clone(), m.dropout)
    qu, qi = F.linear(xu, P, pb), F.linear(xi, P, pb)
    cos = lambda a, b: -F.cosine_similarity(a, b, dim=-1).mean() / 2  # noqa: E731
    return cos(qu, ti) + cos(qi, tu) + m.reg_weight * 0.5 * ((xu ** 2).sum() + (xi ** 2).sum())


def main():
    args = parser(steps=200, warmup=30).parse_args()
    require_gpu("selfcf_step_time", args)
    from rsx import selfcf
    from rsx.trainer import Trainer

    # the batches are [user, item] pairs: the model draws no negatives and reads no feature file
    m, c, batches, _ = synth_model("SELFCFED_LGN", "sports", args, dict(n_layers=2, dropout=0.3, reg_weight=0.1), (),
                                   negatives=False)
    m.train()
    g = m.graph
    res = {"n_users": m.n_users, "n_items": m.n_items, "nnz": g.nnz, "d": 64, "batch": 2048, "n_layers": 2,
           "dropout": 0.3, "steps_per_window": args.steps, "windows": args.repeats, "format": "[median, min, max] ms"}
    rev64, zero = g.rev.to(torch.int64), torch.zeros((), device=g.val0.device)

    # ---- whole steps through the Trainer: eager and the captured graph, fused and torch comparator
    def torch_calc(inter):
        pairs = inter[:2].contiguous()
        torch_drop(g, rev64, zero)
        E = m._propagate(m._rows.rows(pairs))
        return torch_loss(m, E, m.predictor.weight, m.predictor.bias, pairs[0], pairs[1])

    fused_calc = m.calculate_loss
    for name, calc in (("fused", fused_calc), ("torch", torch_calc)):
        for graph in (False, True):
            m.calculate_loss = calc
            t, step = trainer_step(c, m, batches, graph)
            key = f"step_{name}_{'graph' if graph else 'eager'}"
            try:
                res.update(alternated(args, {key: step}))
            except RuntimeError as e:  # a torch op that cannot be captured: reported, not hidden
                if name == "fused":
                    raise
                res[key] = not_measured(e, 120)
                continue
            if graph:
                assert t._graph is not None and t._graph.replays >= args.steps
    m.calculate_loss = fused_calc

    # ---- the edge drop alone
    res.update(alternated(args, {"edge_drop_fused_graph": captured(g.drop),
                                 "edge_drop_torch_graph": captured(lambda: torch_drop(g, rev64, zero))}))

    # ---- the loss part alone on a fixed table
    with torch.no_grad():
        m.eval()
        E = m._propagate().detach().clone().contiguous()
        m.train()
    P, pb = m.predictor.weight.detach().clone(), m.predictor.bias.detach().clone()
    users, items = batches[0][0].contiguous(), batches[0][1].contiguous()
    a = selfcf.selfcf_args(E, P, pb, users, items, m.n_users, m.reg_weight, m.dropout, g.seed, None, m._ws)
    go = torch.ones(1, device="cuda")

    def fused_loss():
        selfcf.loss_fwd(a, E.device)
        selfcf.loss_bwd(a, go, E, P)

    leaves = [x.requires_grad_() for x in (E, P, pb)]

    def torch_loss_part():
        torch.autograd.grad(torch_loss(m, *leaves, users, items), leaves)

    res.update(alternated(args, {"loss_fused_eager": fused_loss, "loss_torch_eager": torch_loss_part}))
    res.update(alternated(args, {"loss_fused_graph": captured(fused_loss)}))
    try:
        res.update(alternated(args, {"loss_torch_graph": captured(torch_loss_part)}))
    except RuntimeError as e:
        res["loss_torch_graph"] = not_measured(e, 120)
    res["algorithmic_bytes"] = step_bytes(m.n_users + m.n_items, g.nnz, 64, 2048, m.n_layers)

    # ---- the whole-step split (eager): device events between the phases
    opt = Trainer(c, m).optimizer
    names = ("edge_drop", "prop_fwd", "loss_fwd_bwd", "prop_bwd", "adam")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]

    def one_step(it):
        opt.zero_grad(set_to_none=True)
        pairs = batches[it % len(batches)][:2].contiguous()
        ev[0].record()
        g.seed.add_(1)
        g.drop()
        ev[1].record()
        Eo = m._propagate(m._rows.rows(pairs))
        ev[2].record()
        lv = Eo.detach().requires_grad_()
        cfg = (m.n_users, m.reg_weight, m.dropout, g.seed, None, m._ws, None)
        loss = selfcf._SelfcfLoss.apply(cfg, pairs[0], pairs[1], lv, m.predictor.weight, m.predictor.bias)
        loss.backward()
        ev[3].record()
        Eo.backward(lv.grad)
        ev[4].record()
        opt.step()
        ev[5].record()
        return loss

    res["split_eager_ms"], _, loss = stage_times(args, names, ev, one_step)
    res["edge_drop_share_of_eager_split"] = round(res["split_eager_ms"]["edge_drop"] / res["split_eager_ms"]["sum"], 4)
    if isinstance(res.get("step_fused_graph"), list):
        res["edge_drop_share_of_graph_step"] = round(res["edge_drop_fused_graph"][0] / res["step_fused_graph"][0], 4)
    assert bool(torch.isfinite(loss))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
