#!/usr/bin/env python3
"""ms/step of the LGMRec training step at a baby-like synthetic shape (19,445 users, 7,050 items,
raw features 4096 / 384 wide, d = 64, 4 hyperedges, one hypergraph layer, B = 2048, cf_model
lightgcn with two UI and two modality layers) on rsx.synth data.

Measured, each as `--repeats` windows of `--steps` iterations between two device events after
a warm-up on the timed shape (median, and minimum / maximum as the spread):
  * the step (zero_grad, forward, loss, backward, RsxAdam) replayed from the Trainer's captured
    graph and launched eagerly;
  * each kernel family of a step on the step's own tensors, forward and backward, and its share
    of the eager forward + backward: the two table-wide InfoNCE terms (rsx_lgm_ssl_*), the four
    assignments (rsx_lgm_assign_*), the two hypergraph layers (rsx_lgm_hgnn_*), the loss
    (rsx_lgm_loss_*), the four feature projections, and the rest (SpMMs, propagation);
  * beside the InfoNCE kernels, the same two terms composed from torch ops as the reference
    writes them (lgmrec.py:159-166), which materialise B x N, forward and backward, on the same
    inputs, alternated window by window with the kernels.
Prints one JSON line.  Needs a GPU: there is no CPU fallback for the measured path.

Usage:  python tools/lgmrec_step_time.py [--steps 50] [--repeats 5] [--warmup 10] [--scale 1.0]
"""
from __future__ import annotations

import json

import torch
import torch.nn.functional as F

from _step_time import alternated, parser, require_gpu, synth_model, trainer_runs


def torch_ssl(T1, T2, idx, tau):
    """lgmrec.py:159-166 on whole tables: the B x N matrix is formed."""
    n1, n2, na = F.normalize(T1[idx]), F.normalize(T2[idx]), F.normalize(T2)
    pos = torch.exp((n1 * n2).sum(1) / tau)
    ttl = torch.exp(n1 @ na.t() / tau).sum(1)
    return -torch.log(pos / ttl).sum()


def main():
    args = parser(steps=50, warmup=10).parse_args()
    require_gpu("lgmrec_step_time", args)
    from rsx import lgmrec as LG

    m, c, batches, n_edges = synth_model("LGMRec", "baby", args, dict(learning_rate=0.001, is_multimodal_model=True),
                                         (("image_feat_raw.npy", 4096, 5), ("text_feat_raw.npy", 384, 6)))
    m.train()
    d, B, nu, ni, H = m.embedding_dim, 2048, m.n_users, m.n_items, m.hyper_num
    res = {"n_users": nu, "n_items": ni, "train_edges": n_edges, "d": d, "F": [4096, 384], "batch": B,
           "hyper_num": H, "n_hyper_layer": m.n_hyper_layer, "n_ui_layers": m.n_ui_layers,
           "n_mm_layers": m.n_mm_layer, "steps_per_window": args.steps, "windows": args.repeats,
           "warmup": args.warmup, "format": "[median, min, max] ms",
           "reference_ssl_matrix_bytes": 4 * B * (nu + ni),
           "ssl_workspace_bytes": int(m._ssl_ws[0].numel() + m._ssl_ws[1].numel())}

    # ---- the kernel families on a step's own tensors
    with torch.no_grad():
        tabs = [t.detach().clone() for t in m._tables()]
    Gv, Gt = tabs[3], tabs[4]
    trip = batches[0]
    one = torch.ones((), device=trip.device)

    def fwd_bwd(make):
        def run():
            make().backward(one)
        return run

    def ssl(fn_u, fn_i):
        def make():
            a, b = Gv.requires_grad_(True), Gt.requires_grad_(True)
            a.grad = b.grad = None
            return fn_u(a[:nu], b[:nu]) + fn_i(a[nu:], b[nu:])
        return make

    hip = ssl(lambda a, b: LG._Ssl.apply((m.tau, m._ssl_ws[0]), trip[0], a, b),
              lambda a, b: LG._Ssl.apply((m.tau, m._ssl_ws[1]), trip[1], a, b))
    tor = ssl(lambda a, b: torch_ssl(a, b, trip[0], m.tau), lambda a, b: torch_ssl(a, b, trip[1], m.tau))
    with torch.no_grad():
        res["ssl_hip_vs_torch_rel_diff"] = float(abs(hip() - tor()) / abs(tor()))

    def loss():
        ts = [t.requires_grad_(True) for t in tabs]
        for t in ts:
            t.grad = None
        return LG._LgmLoss.apply((nu, m.alpha, m.reg_weight, m._ws, None), trip, *ts)

    li = torch.randn(ni, m.ld, device=trip.device)
    lu = torch.randn(nu, m.ld, device=trip.device)

    def assign():
        out = 0
        for s, x in enumerate((li, lu, li, lu)):
            x = x.requires_grad_(True)
            x.grad = None
            out = out + LG._Assign.apply((H, m.tau, m.keep_rate, None, None, m._seed, s), x).sum()
        return out

    with torch.no_grad():
        Pi = LG.assign_fwd(li, H, m.tau, 1.0, seed=m._seed)[1]
        Pu = LG.assign_fwd(lu, H, m.tau, 1.0, seed=m._seed)[1]
    X = tabs[0][nu:].clone()

    def hgnn():
        out = 0
        for _ in range(2):
            a, b, x = Pi.requires_grad_(True), Pu.requires_grad_(True), X.requires_grad_(True)
            a.grad = b.grad = x.grad = None
            out = out + LG._Hgnn.apply(a, b, x, H, m.n_hyper_layer).sum()
        return out

    def project():
        out = 0
        for Xf, W, ld in ((m.image_embedding.weight, m.item_image_trs, d), (m.image_embedding.weight, m.v_hyper, m.ld),
                          (m.text_embedding.weight, m.item_text_trs, d), (m.text_embedding.weight, m.t_hyper, m.ld)):
            W.grad = None
            out = out + LG._ProjectT.apply(Xf, W, ld).sum()
        return out

    def whole():
        m.zero_grad(set_to_none=True)
        return m.calculate_loss(trip)

    res.update(alternated(args, {"ssl_hip_fwd_bwd": fwd_bwd(hip), "ssl_torch_ops_fwd_bwd": fwd_bwd(tor)}))
    res.update(alternated(args, {"loss_fwd_bwd": fwd_bwd(loss), "assign_fwd_bwd": fwd_bwd(assign),
                                 "hgnn_fwd_bwd": fwd_bwd(hgnn), "project_fwd_bwd": fwd_bwd(project),
                                 "model_fwd_bwd_eager": fwd_bwd(whole)}))
    total = res["model_fwd_bwd_eager"][0]
    res["share_of_fwd_bwd"] = {k: round(res[k + "_fwd_bwd"][0] / total, 3)
                               for k in ("ssl_hip", "loss", "assign", "hgnn", "project")}
    m.zero_grad(set_to_none=True)

    # ---- the step through the Trainer, eager and captured
    res.update(trainer_runs(args, c, m, batches))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
