#!/usr/bin/env python3
"""ms/step of the GRCN training step at a baby-like synthetic shape (19,445 users, 7,050 items,
raw features 4096 / 384 wide, embedding_size = latent_embedding = 64, B = 2048) on rsx.synth data.

Measured, each as `--repeats` windows of `--steps` iterations between two device events after
a warm-up on the timed shape (median, and minimum / maximum as the spread):
  * the step (zero_grad, forward, loss, backward, RsxAdam) launched eagerly through the Trainer;
  * the step replayed from the Trainer's captured graph, alternated window by window with the
    same step composed from torch ops (tests/grcn_ref.py in float32 on the GPU, zero_grad and
    RsxAdam included): once with the preferences normalised once (n_layers = 0: the arithmetic of
    the HIP path) and once with the reference's literal routing loop (n_layers = 3);
    `bar`: whether the captured median is below the torch median (normalised once) by more than
    the larger of the two min-max spreads;
  * each new kernel on the step's own tensors, forward and backward, the four SpMMs of the id
    GCN, the two MLPs with their normalisations, RsxAdam's update, and each one's share of the
    eager forward + backward.
The hub degree (rsx_grcn_hub_degree) is a compile-time constant: reported, not swept.
Prints one JSON line.  Needs a GPU: there is no CPU fallback for the measured path.

Usage:  python tools/grcn_step_time.py [--steps 20] [--repeats 5] [--warmup 5] [--scale 1.0]
"""
from __future__ import annotations

import json

import torch

from _step_time import alternated, parser, require_gpu, synth_model, trainer_runs, trainer_step


def main():
    args = parser(steps=20, warmup=5).parse_args()
    require_gpu("grcn_step_time", args)
    import grcn_ref as R
    from rsx import _lib as L
    from rsx import grcn as G
    from rsx import ops
    from rsx.optim import RsxAdam

    m, c, batches, n_edges = synth_model("GRCN", "baby", args, dict(learning_rate=0.001, reg_weight=0.001,
                                                                     is_multimodal_model=True),
                                         (("image_feat_raw.npy", 4096, 5), ("text_feat_raw.npy", 384, 6)))
    m.train()
    nu, ni, g = m.n_users, m.n_items, m.graph
    dev = m.device
    deg = (g.rowptr[1:] - g.rowptr[:-1])
    H = int(L.lib().rsx_grcn_hub_degree())
    res = {"n_users": nu, "n_items": ni, "train_edges": n_edges, "slots": g.nnz, "dx": m.dim_x, "dc": m.dim_C,
           "F": [4096, 384], "batch": 2048, "hub_degree": H, "hub_rows": int((deg > H).sum()), "max_degree": int(deg.max()),
           "steps_per_window": args.steps, "windows": args.repeats, "warmup": args.warmup, "format": "[median, min, max] ms"}
    trip = batches[0]
    one = torch.ones((), device=dev)

    def whole():
        return m.calculate_loss(trip)

    def fwd_bwd(make):
        def run():
            m.zero_grad(set_to_none=True)
            make().backward(one)
        return run

    # ---- the step's own tensors
    with torch.no_grad():
        x_v, x_t, xn = m._inputs()
        conf, E = m.model_specific_conf.detach(), m.id_gcn.id_embedding.detach()
        pv, pt = (p.detach() for p in m._prefs())
        reps, h1, id_rep = G.step_forward(g, [x_v, x_t], conf, xn)
        a = G.loss_args(id_rep, reps[0], reps[1], E, pv, pt, trip, nu, m.reg_weight)
        out = torch.empty(3, device=dev)
        Gi, g_v, g_t, gE, gpv, gpt = G.loss_bwd(a, one, id_rep, reps[0], reps[1], pv, m._ws)
        D = torch.empty_like(Gi)
        g.AT.spmm_epi(Gi, ops.epi(L.RSX_EPI_ADD, y=D, s_in=Gi), m.dim_x)
        dw = G.edge_dots(g, Gi, h1, D, xn)
        das, _ = G.refine_bwd(g, g.alpha, conf, dw)
    tmp = torch.empty_like(xn)

    def spmms():  # the id GCN's four products: A_w x, A_w h1, A_w^T G, A_w^T D
        g.A.spmm(xn, out=tmp)
        g.A.spmm_epi(h1, ops.epi(L.RSX_EPI_ADD, y=tmp, s_in=xn, r_add=h1), m.dim_x)
        g.AT.spmm_epi(Gi, ops.epi(L.RSX_EPI_ADD, y=tmp, s_in=Gi), m.dim_x)
        g.AT.spmm_epi(D, ops.epi(L.RSX_EPI_ADD, y=tmp, s_in=Gi), m.dim_x)

    def mlps():
        x = m._inputs()
        return x[0].sum() + x[1].sum() + x[2].sum()

    res.update(alternated(args, {"model_fwd_bwd_eager": fwd_bwd(whole)}))
    res.update(alternated(args, {
        "attn_fwd_v": lambda: G.attn_fwd(g, x_v, g.alpha[0]), "attn_bwd_v": lambda: G.attn_bwd(g, g_v, das[0], x_v, g.alpha[0]),
        "refine_fwd": lambda: G.refine_fwd(g, g.alpha, conf), "refine_bwd": lambda: G.refine_bwd(g, g.alpha, conf, dw),
        "edge_dots": lambda: G.edge_dots(g, Gi, h1, D, xn), "spmm_x4": spmms,
        "loss_fwd": lambda: G.loss_fwd(a, out, m._result, m._ws),
        "loss_bwd": lambda: G.loss_bwd(a, one, id_rep, reps[0], reps[1], pv, m._ws),
        "mlp_normalize_fwd_bwd": fwd_bwd(mlps)}))
    opt = RsxAdam(m.parameters(), lr=1e-3)
    fwd_bwd(whole)()  # gradients for the update to read
    res.update(alternated(args, {"adam": opt.step}))
    total = res["model_fwd_bwd_eager"][0]
    res["share_of_fwd_bwd"] = {k: round(res[k][0] * mult / total, 3) for k, mult in (
        ("attn_fwd_v", 2), ("attn_bwd_v", 2), ("refine_fwd", 1), ("refine_bwd", 1), ("edge_dots", 1), ("spmm_x4", 1),
        ("loss_fwd", 1), ("loss_bwd", 1), ("mlp_normalize_fwd_bwd", 1))}  # (x2: the text branch's launch of the same shape)
    m.zero_grad(set_to_none=True)

    # ---- the step composed from torch ops on the same parameters
    P = dict(m.named_parameters())
    feats = {"v": m.v_feat, "t": m.t_feat}
    ei_rows = torch.repeat_interleave(torch.arange(g.n, device=dev), deg)  # target of a slot
    user_to_item = ei_rows >= nu  # slots whose target is an item: source a user
    ei = torch.stack([g.col.long()[user_to_item], ei_rows[user_to_item]])  # [2, E]: users, items (offset)

    def torch_step(n_layers):
        def run():
            m.zero_grad(set_to_none=True)
            fw = R.forward(P, feats, ei, nu, n_layers)
            R.loss(P, feats, fw["representation"], trip, nu, m.reg_weight)[0].backward(one)
            opt.step()
        return run

    with torch.no_grad():
        fw = R.forward(P, feats, ei, nu, 0)
        ref = R.loss(P, feats, fw["representation"], trip, nu, m.reg_weight)[0]
        res["hip_vs_torch_loss_rel_diff"] = float(abs(whole() - ref) / abs(ref))

    # ---- the step through the Trainer: eager; then captured, alternated with the torch steps
    res.update(trainer_runs(args, c, m, batches, order=(False,)))
    _, graph_step = trainer_step(c, m, batches, True)
    try:
        res.update(alternated(args, {"step_graph": graph_step, "step_torch_ops": torch_step(0),
                                     "step_torch_ops_routing": torch_step(3)}))
        hip, tor = res["step_graph"], res["step_torch_ops"]
        spread = max(hip[2] - hip[1], tor[2] - tor[1])
        res["bar"] = {"hip_below_torch_by_ms": round(tor[0] - hip[0], 4), "larger_spread_ms": round(spread, 4),
                      "cleared": bool(tor[0] - hip[0] > spread)}
    except RuntimeError as e:
        res["step_graph"] = "not measured: " + str(e).splitlines()[0][:160]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
