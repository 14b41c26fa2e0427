#!/usr/bin/env python3
"""ms/step of the MGCN training step at the sports shape (35,598 users, 18,357 items, raw
features 4096 / 384 wide, d = 64, B = 2048, n_ui_layers 2, n_layers 1, knn_k 10) on rsx.synth
data, against the same step with the purifier and the fuser written as torch ops.

Measured, each as `--repeats` windows of `--steps` iterations between two device events after
a warm-up on the timed shape (median, and minimum / maximum as the spread):
  * the whole step (zero_grad, forward, loss, backward, RsxAdam) launched eagerly, and
    replayed from the Trainer's captured graph;
  * the same with the comparator blocks: the torch ops of reference src/models/mgcn.py:152-154
    and :187-201 as written (on the batch's gathered rows, as the fused fuser runs) around the
    same propagation, projections, loss and optimizer;
  * the two blocks alone, forward plus backward on fixed inputs: the purifier over the item
    table, the fuser on the batch rows (n = 3 B) and over all rows, fused and torch, eager and
    graph-replayed;
  * the whole step split by phase (eager, device events between the phases).
Prints one JSON line.  Needs a GPU: there is no CPU fallback for the measured path.

Usage:  python tools/mgcn_step_time.py [--steps 100] [--repeats 5] [--warmup 20] [--scale 1.0]
"""
from __future__ import annotations

import json
import types

import torch
import torch.nn.functional as F

from _step_time import alternated, captured, not_measured, parser, require_gpu, stage_times, synth_model, trainer_step


# ------------------------------------------------------------ the comparator blocks
def _seq(mod, x):
    """An nn.Sequential of the model's applied with torch's own ops (F.linear and the
    activations; the modules' rsx weight-gradient path is not used)."""
    for layer in mod:
        x = F.linear(x, layer.weight, layer.bias) if isinstance(layer, torch.nn.Linear) else layer(x)
    return x


def torch_purify(image_feats, text_feats, item, gate_v, gate_t):
    """mgcn.py:152-154 as written."""
    return torch.multiply(item, _seq(gate_v, image_feats)), torch.multiply(item, _seq(gate_t, text_feats))


def _torch_fuse(m, content_embeds, image_embeds, text_embeds):
    """mgcn.py:187-201 as written."""
    att_common = torch.cat([_seq(m.query_common, image_embeds), _seq(m.query_common, text_embeds)], dim=-1)
    weight_common = m.softmax(att_common)
    common_embeds = weight_common[:, 0].unsqueeze(dim=1) * image_embeds + weight_common[:, 1].unsqueeze(
        dim=1) * text_embeds
    sep_image_embeds = image_embeds - common_embeds
    sep_text_embeds = text_embeds - common_embeds
    image_prefer = _seq(m.gate_image_prefer, content_embeds)
    text_prefer = _seq(m.gate_text_prefer, content_embeds)
    sep_image_embeds = torch.multiply(image_prefer, sep_image_embeds)
    sep_text_embeds = torch.multiply(text_prefer, sep_text_embeds)
    side_embeds = (sep_image_embeds + sep_text_embeds + common_embeds) / 3
    return content_embeds + side_embeds, side_embeds


def torch_fuse(m, content, image_embeds, text_embeds):
    return _torch_fuse(m, content, image_embeds, text_embeds)


def torch_fuse_rows(m, content, image_embeds, text_embeds, rows):
    c = content.index_select(0, rows)
    all_, side = _torch_fuse(m, c, image_embeds.index_select(0, rows), text_embeds.index_select(0, rows))
    return all_, side, c


def block_counts(d: int) -> dict:
    """Per logical row of the fuser (f32): bytes moved and d x d products."""
    row = 4 * d
    return {"fuse_fwd_bytes": (3 + 4) * row, "fuse_fwd_products": 4,
            "fuse_bwd_bytes": (3 + 3 + 3 + 5 + 2) * row, "fuse_bwd_products": 8,
            "purify_fwd_bytes_per_gate": 3 * row, "purify_bwd_bytes_per_gate": 5 * row}


def main():
    args = parser(steps=100, warmup=20).parse_args()
    require_gpu("mgcn_step_time")
    from rsx import mgcn
    from rsx import mgcn_fuse as MF
    from rsx import smore_fuse as SF
    from rsx.blocks import _ego, ui_backbone
    from rsx.dense import _Project
    from rsx.trainer import Trainer

    m, c, batches, _ = synth_model("MGCN", "sports", args, dict(cl_loss=0.01, is_multimodal_model=True),
                                   (("image_feat.npy", 4096, 5), ("text_feat.npy", 384, 6)))

    m.train()
    d, B = m.embedding_dim, 2048
    res = {"n_users": m.n_users, "n_items": m.n_items, "d": d, "F": [4096, 384], "batch": B,
           "n_ui_layers": m.n_ui_layers, "n_layers": m.n_layers, "knn_k": m.knn_k, "steps_per_window": args.steps,
           "windows": args.repeats, "format": "[median, min, max] ms", "per_row": block_counts(d)}

    # ---- whole steps through the Trainer: eager and the captured graph, fused and torch blocks
    torch_blocks = types.SimpleNamespace(purify=torch_purify, fuse=torch_fuse, fuse_rows=torch_fuse_rows,
                                         supported=MF.supported)
    for name, blocks in (("fused", MF), ("torch_blocks", torch_blocks)):
        for graph in (False, True):
            mgcn.MF = blocks
            t, step = trainer_step(c, m, batches, graph)
            key = f"step_{name}_{'graph' if graph else 'eager'}"
            try:
                res.update(alternated(args, {key: step}))
            except RuntimeError as e:
                if name == "fused":
                    raise
                res[key] = not_measured(e, 120)
                continue
            if graph:
                assert t._graph is not None and t._graph.replays >= args.steps
    mgcn.MF = MF

    # ---- the two blocks alone, forward + backward on fixed inputs
    def both(key, run):
        """`run` launched eagerly and replayed from a graph of its own."""
        res.update(alternated(args, {key + "_eager": run}))
        try:
            res.update(alternated(args, {key + "_graph": captured(run)}))
        except RuntimeError as e:  # a torch op that cannot be captured: reported, not hidden
            res[key + "_graph"] = not_measured(e, 120)

    g = torch.Generator(device="cuda").manual_seed(3)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g) * 0.1  # noqa: E731
    ni, N = m.n_items, m.n_users + m.n_items
    item, fi, ft = (rnd(ni, d).requires_grad_() for _ in range(3))
    go2 = (rnd(ni, d), rnd(ni, d))
    pw = [p for gate in (m.gate_v, m.gate_t) for p in gate.parameters()]
    for name, fn in (("fused", MF.purify), ("torch", torch_purify)):
        both(f"purify_{name}", lambda fn=fn: torch.autograd.grad(fn(fi, ft, item, m.gate_v, m.gate_t),
                                                                 [item, fi, ft] + pw, go2))
    C_, I_, T_ = (rnd(N, d).requires_grad_() for _ in range(3))
    rows = (batches[0].reshape(-1) + torch.cat([torch.zeros(B, dtype=torch.int64), torch.full((2 * B,), m.n_users)]
                                               ).cuda()).contiguous()
    fw = list(m.query_common.parameters()) + list(m.gate_image_prefer.parameters()) + \
        list(m.gate_text_prefer.parameters())
    gr, gf = [rnd(3 * B, d) for _ in range(3)], [rnd(N, d) for _ in range(2)]
    for name, fr, ff in (("fused", MF.fuse_rows, MF.fuse), ("torch", torch_fuse_rows, torch_fuse)):
        both(f"fuse_rows_{name}", lambda fr=fr: torch.autograd.grad(fr(m, C_, I_, T_, rows), [C_, I_, T_] + fw, gr))
        both(f"fuse_full_{name}", lambda ff=ff: torch.autograd.grad(ff(m, C_, I_, T_), [C_, I_, T_] + fw, gf))

    # ---- the whole-step split (eager): device events between the phases
    opt = Trainer(c, m).optimizer
    names = ("proj_fwd", "purify_fwd", "prop_views_fwd", "fuse_fwd", "loss_fwd_bwd", "fuse_bwd", "prop_views_bwd",
             "purify_bwd", "proj_bwd", "adam")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
    leaf = lambda *xs: [x.detach().requires_grad_() for x in xs]  # noqa: E731

    def one_step(it):
        opt.zero_grad(set_to_none=True)
        inter = batches[it % len(batches)]
        ar, trip = m._bidx[B]
        rws = inter[:3].reshape(-1) + m._rows_off[B]
        ev[0].record()
        Fi = _Project.apply(m.image_embedding.weight, m.image_trs.weight, m.image_trs.bias)
        Ft = _Project.apply(m.text_embedding.weight, m.text_trs.weight, m.text_trs.bias)
        ev[1].record()
        lf = leaf(Fi, Ft)
        item_l = m.item_id_embedding.weight
        xi, xt = MF.purify(lf[0], lf[1], item_l, m.gate_v, m.gate_t)
        ev[2].record()
        lx = leaf(xi, xt)
        content = ui_backbone(m, _ego(m.user_embedding.weight, item_l), m.norm_adj_csr, m.n_ui_layers, rws)
        ie = SF.view_prop(lx[0], m.image_graph, m.R, m.n_layers, m.n_users)
        te = SF.view_prop(lx[1], m.text_graph, m.R, m.n_layers, m.n_users)
        ev[3].record()
        lt = leaf(content, ie, te)
        all_c, side_c, content_c = MF.fuse_rows(m, *lt, rws)
        ev[4].record()
        lo = leaf(all_c, side_c, content_c)
        total, _ = SF.smore_loss_rows(*lo, trip, ar, B, m.reg_weight, m.batch_size, m.cl_loss, mgcn.CL_TEMPERATURE)
        total.backward()
        ev[5].record()
        torch.autograd.backward([all_c, side_c, content_c], [x.grad for x in lo])
        ev[6].record()
        torch.autograd.backward([content, ie, te], [x.grad for x in lt])
        ev[7].record()
        torch.autograd.backward([xi, xt], [x.grad for x in lx])
        ev[8].record()
        torch.autograd.backward([Fi, Ft], [x.grad for x in lf])
        ev[9].record()
        opt.step()
        ev[10].record()
        return total

    res["split_eager_ms"], _, total = stage_times(args, names, ev, one_step)
    assert bool(torch.isfinite(total))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
