#!/usr/bin/env python3
"""ms/step of the MMGCN training step at a baby-like synthetic shape (19,445 users, 7,050 items,
raw features 4096 / 384 wide, d = 64, B = 2048) on rsx.synth data.

Measured, each as `--repeats` windows of `--steps` iterations between two device events after
a warm-up on the timed shape (median, and minimum / maximum as the spread):
  * the step (zero_grad, forward, loss, backward, RsxAdam) replayed from the Trainer's captured
    graph and launched eagerly;
  * each stage of a step on the step's own tensors, forward and backward, and its share of the
    eager forward + backward: the image MLP with the normalisation of its rows, layer 1 of the
    image branch (width 256) and of the text branch (width 384, constant input), the four fused
    layers 2 and 3, the SpMMs those stages contain (timed again on their own), the loss with
    `result`, and RsxAdam's update;
  * the same forward, loss and backward composed from torch ops as the reference writes them
    (tests/mmgcn_ref.py in float32 on the GPU, the mean operator a torch sparse tensor),
    alternated window by window with the HIP path.
Prints one JSON line.  Needs a GPU: there is no CPU fallback for the measured path.

Usage:  python tools/mmgcn_step_time.py [--steps 20] [--repeats 5] [--warmup 5] [--scale 1.0]
"""
from __future__ import annotations

import json

import torch

from _step_time import alternated, parser, require_gpu, synth_model, trainer_runs


def main():
    args = parser(steps=20, warmup=5).parse_args()
    require_gpu("mmgcn_step_time", args)
    import mmgcn_ref as R
    from rsx import mmgcn as M
    from rsx.dense import _Gemm
    from rsx.optim import RsxAdam

    m, c, batches, n_edges = synth_model("MMGCN", "baby", args, dict(learning_rate=0.001, reg_weight=0.001,
                                                                      is_multimodal_model=True),
                                         (("image_feat_raw.npy", 4096, 5), ("text_feat_raw.npy", 384, 6)))
    m.train()
    d, B, nu, ni, n = m.dim_x, 2048, m.n_users, m.n_items, m.n_nodes
    dev = m.device
    res = {"n_users": nu, "n_items": ni, "train_edges": n_edges, "d": d, "F": [4096, 384], "batch": B,
           "steps_per_window": args.steps, "windows": args.repeats, "warmup": args.warmup,
           "format": "[median, min, max] ms"}
    trip, E, G = batches[0], m.id_embedding, m.graph
    v, t = m.v_gcn, m.t_gcn
    one = torch.ones((), device=dev)

    def leaf(x):
        x = x.detach().requires_grad_(True)
        x.grad = None
        return x

    def fwd_bwd(make):
        def run():
            m.zero_grad(set_to_none=True)
            make().backward(one)
        return run

    with torch.no_grad():
        x0v = M._ImageRows.apply(_Gemm.apply(m.v_feat, None, v.MLP.weight, v.MLP.bias, False, False), m._x0["v"][0])
        x1 = M._Layer1.apply(G, None, x0v, E, *v.layer(1))
    x0t, a0t = m._x0["t"]

    def mlp():
        temp = _Gemm.apply(m.v_feat, None, v.MLP.weight, v.MLP.bias, False, False)
        return M._ImageRows.apply(temp, m._x0["v"][0]).sum()

    def layers23():
        out = 0
        for g in (v, t):
            x = leaf(x1)
            for k in (2, 3):
                x = M._Layer.apply(G, None, x, E, *g.layer(k))
            out = out + x.sum()
        return out

    def spmms():  # what the stages above contain: A and A^T at 256 once, at d four times each
        G.AT.spmm(G.A.spmm(x0v))
        for _ in range(4):
            G.AT.spmm(G.A.spmm(x1))

    def loss():
        return M._Loss.apply((nu, m.reg_weight, m._pref_term, E, m.result, m._ws, None), trip, leaf(x1), leaf(x1))

    def whole():
        return m.calculate_loss(trip)

    opt = RsxAdam(m.parameters(), lr=1e-3)
    fwd_bwd(whole)()  # gradients for the update to read

    # the reference's ops in float32 torch on the same tensors
    P = {name: p for name, p in m.named_parameters()}
    C = {"id_embedding": E, "v_gcn.preference": v.preference, "t_gcn.preference": t.preference}
    rows =torch.repeat_interleave(torch.arange(n, device=dev), G.A.rowptr[1:] - G.A.rowptr[:-1])
    A = torch.sparse_coo_tensor(torch.stack([rows, G.A.col.long()]), G.A.val, (n, n)).coalesce()
    feats = {"v": m.v_feat, "t": m.t_feat}

    def torch_whole():
        rep, _ = R.forward(P, C, feats, A)
        return R.loss(C, feats, rep, trip, nu, m.reg_weight)[0]

    with torch.no_grad():
        res["hip_vs_torch_loss_rel_diff"] = float(abs(whole() - torch_whole()) / abs(torch_whole()))
    res.update(alternated(args, {"model_fwd_bwd_eager": fwd_bwd(whole), "model_fwd_bwd_torch_ops": fwd_bwd(torch_whole)}))
    res.update(alternated(args, {
        "mlp_fwd_bwd": fwd_bwd(mlp),
        "layer1_v_fwd_bwd": fwd_bwd(lambda: M._Layer1.apply(G, None, leaf(x0v), E, *v.layer(1)).sum()),
        "layer1_t_fwd_bwd": fwd_bwd(lambda: M._Layer1.apply(G, a0t, x0t, E, *t.layer(1)).sum()),
        "layers23_fwd_bwd": fwd_bwd(layers23), "loss_fwd_bwd": fwd_bwd(loss), "spmm_only": spmms}))
    fwd_bwd(whole)()
    res.update(alternated(args, {"adam": opt.step}))
    total = res["model_fwd_bwd_eager"][0]
    res["share_of_fwd_bwd"] = {k: round(res[k + "_fwd_bwd"][0] / total, 3)
                               for k in ("mlp", "layer1_v", "layer1_t", "layers23", "loss")}
    m.zero_grad(set_to_none=True)

    # ---- the step through the Trainer, eager and captured
    res.update(trainer_runs(args, c, m, batches))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
