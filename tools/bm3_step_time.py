#!/usr/bin/env python3
"""ms/step of the BM3 training step at the sports shape (35,598 users, 18,357 items, raw
features 4096 / 384 wide, d = 64, B = 2048, 2 layers, dropout 0.3) on rsx.synth data, against
the same step with the loss written as torch ops.

Measured, each as `--repeats` windows of `--steps` iterations between two device events after
a warm-up on the timed shape (median, and minimum / maximum as the spread):
  * the whole step (zero_grad, forward, loss, backward, RsxAdam) launched eagerly, and
    replayed from the Trainer's captured graph;
  * the same with the comparator loss: F.linear, F.dropout, cosine_similarity, torch.norm
    (reference src/models/bm3.py:108-149 as written) around the same propagation, projections
    and optimizer;
  * the loss part alone, forward plus backward on fixed tables: the fused kernels
    (rsx_bm3_loss_fwd / _bwd) and the torch composition, eager and graph-replayed;
  * the whole-step split by phase (eager, device events between the phases): propagation
    forward, projections forward, loss forward + backward, projections backward, propagation
    backward, Adam.
Prints one JSON line.  Needs a GPU: there is no CPU fallback for the measured path.

Usage:  python tools/bm3_step_time.py [--steps 200] [--repeats 5] [--warmup 30] [--scale 1.0]
"""
from __future__ import annotations

import json

import torch
import torch.nn.functional as F

from _step_time import alternated, captured, not_measured, parser, require_gpu, stage_times, synth_model, trainer_step


def loss_bytes(nu: int, ni: int, d: int, B: int, S: int = 4) -> dict:
    """Bytes the fused loss must move (f32), from the shapes.  Forward: the S B gathered rows
    read (the item row twice: E and H) and written stacked, read by the predictor with its
    output written, both read by the cosines; the two whole tables read for the norms.
    Backward: the whole tables read and gE written (regulariser), gT / gV cleared, the stacked
    online and predicted rows read, the gradient rows written, read twice (g P, g^T x), the
    online rows' gradients written, read and added (read + write)."""
    row = 4 * d
    fwd = (S + 1) * B * row + S * B * row + 2 * S * B * row + 2 * S * B * row + (nu + 2 * ni) * row
    bwd = (nu + 2 * ni) * row + (nu + ni) * row + (S - 2) * ni * row + 2 * S * B * row + S * B * row + \
        3 * S * B * row + S * B * row + 3 * S * B * row
    return {"fwd": fwd, "bwd": bwd, "total": fwd + bwd}


def torch_loss(m, E, H, T, V, P, pb, users, items):
    """The loss part as the reference writes it (bm3.py:108-149) on the given tables."""
    nu = m.n_users
    u_on, i_on = E[:nu], E[nu:] + H
    with torch.no_grad():
        u_t, i_t = F.dropout(u_on.clone(), m.dropout), F.dropout(i_on.clone(), m.dropout)
        t_t, v_t = F.dropout(T.clone(), m.dropout), F.dropout(V.clone(), m.dropout)
    u_p, i_p = F.linear(u_on, P, pb)[users], F.linear(i_on, P, pb)[items]
    t_p, v_p = F.linear(T, P, pb)[items], F.linear(V, P, pb)[items]
    u_t, i_t, t_t, v_t = u_t[users], i_t[items], t_t[items], v_t[items]
    cos = lambda a, b: 1 - F.cosine_similarity(a, b, dim=-1).mean()  # noqa: E731
    reg = (torch.norm(u_on) + torch.norm(i_on)) / i_on.shape[0]
    return (cos(u_p, i_t) + cos(i_p, u_t)) + m.reg_weight * reg + \
        m.cl_weight * (cos(t_p, i_t) + cos(v_p, i_t) + cos(t_p, t_t) + cos(v_p, v_t))


def main():
    args = parser(steps=200, warmup=30).parse_args()
    require_gpu("bm3_step_time")
    from rsx import bm3
    from rsx.trainer import Trainer

    # the batches are [user, item] pairs: BM3 draws no negatives
    m, c, batches, _ = synth_model("BM3", "sports", args, dict(n_layers=2, dropout=0.3, reg_weight=0.1),
                                   (("image_feat.npy", 4096, 5), ("text_feat.npy", 384, 6)), negatives=False)
    m.train()
    res = {"n_users": m.n_users, "n_items": m.n_items, "d": 64, "F": [4096, 384], "batch": 2048, "n_layers": 2,
           "dropout": 0.3, "steps_per_window": args.steps, "windows": args.repeats, "format": "[median, min, max] ms"}

    # ---- whole steps through the Trainer: eager and the captured graph, fused and torch loss
    def torch_calc(inter):
        E, H, T, V = m._tables()
        return torch_loss(m, E, H, T, V, m.predictor.weight, m.predictor.bias, inter[0], inter[1])

    fused_calc = m.calculate_loss
    for name, calc in (("fused", fused_calc), ("torch_loss", torch_calc)):
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

    # ---- the loss part alone on fixed tables
    with torch.no_grad():
        E, H, T, V = (x.detach().clone() for x in m._tables())
    P, pb = m.predictor.weight.detach().clone(), m.predictor.bias.detach().clone()
    users, items = batches[0][0].contiguous(), batches[0][1].contiguous()
    a = bm3.bm3_args(E, H, T, V, P, pb, users, items, m.n_users, m.reg_weight, m.cl_weight, m.dropout, m._drop_seed,
                     None, m._ws)
    go = torch.ones(1, device="cuda")

    def fused_loss():
        bm3.loss_fwd(a, E.device)
        bm3.loss_bwd(a, go, E, T, V, P)

    leaves = [x.requires_grad_() for x in (E, H, T, V, P, pb)]

    def torch_loss_part():
        torch.autograd.grad(torch_loss(m, *leaves, users, items), leaves)

    res.update(alternated(args, {"loss_fused_eager": fused_loss}))
    res.update(alternated(args, {"loss_fused_graph": captured(fused_loss)}))
    res.update(alternated(args, {"loss_torch_eager": torch_loss_part}))
    try:
        res.update(alternated(args, {"loss_torch_graph": captured(torch_loss_part)}))
    except RuntimeError as e:
        res["loss_torch_graph"] = not_measured(e, 120)
    by = loss_bytes(m.n_users, m.n_items, 64, 2048)
    res["loss_algorithmic_bytes"] = by
    res["loss_fused_graph_bytes_per_s_over_8TBps"] = round(by["total"] / (res["loss_fused_graph"][0] * 1e-3) / 8e12, 4)

    # ---- the whole-step split (eager): device events between the phases
    opt = Trainer(c, m).optimizer
    names = ("prop_fwd", "proj_fwd", "loss_fwd_bwd", "proj_bwd", "prop_bwd", "adam")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
    from rsx.blocks import _ego, _PropMean
    from rsx.dense import _Project

    def one_step(it):
        opt.zero_grad(set_to_none=True)
        inter = batches[it % len(batches)]
        ev[0].record()
        Eo = _PropMean.apply(_ego(m.user_embedding.weight, m.item_id_embedding.weight), m.norm_adj_csr, m.n_layers)
        ev[1].record()
        To = _Project.apply(m.text_embedding.weight, m.text_trs.weight, m.text_trs.bias)
        Vo = _Project.apply(m.image_embedding.weight, m.image_trs.weight, m.image_trs.bias)
        ev[2].record()
        lv = [x.detach().requires_grad_() for x in (Eo, To, Vo)]
        m._drop_seed.add_(1)
        cfg = (m.n_users, m.reg_weight, m.cl_weight, m.dropout, m._drop_seed, None, m._ws, None)
        loss = bm3._Bm3Loss.apply(cfg, inter[0], inter[1], lv[0], m.item_id_embedding.weight, m.predictor.weight,
                                  m.predictor.bias, lv[1], lv[2])
        loss.backward()
        ev[3].record()
        torch.autograd.backward([To, Vo], [lv[1].grad, lv[2].grad])
        ev[4].record()
        Eo.backward(lv[0].grad)
        ev[5].record()
        opt.step()
        ev[6].record()
        return loss

    res["split_eager_ms"], _, loss = stage_times(args, names, ev, one_step)
    assert bool(torch.isfinite(loss))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
