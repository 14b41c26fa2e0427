#!/usr/bin/env python3
"""ms/step of the DRAGON training step at a baby-like synthetic shape (19,445 users, 7,050 items,
raw features 4096 / 384 wide, the representation 128 wide, B = 2048) on rsx.synth data, the user
graph from rsx.dualgnn.build_user_graph on the synthetic interactions, mm_adj from the device kNN.

Measured, each as `--repeats` windows of `--steps` iterations between two device events after
a warm-up on the timed shape (median, and minimum / maximum as the spread):
  * the step (zero_grad, forward, loss, backward, RsxAdam) replayed from the Trainer's captured
    graph and launched eagerly;
  * each stage of a step on the step's own tensors, forward and backward, and its share of the
    eager forward + backward: the two MLPs with the normalisation, the propagation x + A x + A^2 x
    of both modalities, and the tail (cat, item graph, user graph, loss and their backwards);
  * the same forward, loss and backward composed from torch ops as the reference writes them
    (tests/dragon_ref.py in float32 on the GPU, the operators torch sparse tensors), alternated
    window by window with the HIP path;
  * rsx_dragon_ugraph_fwd at d = 128 against the same lists as a CSR through rsx_spmm with the
    ADD epilogue, alternated window by window; the backward's SpMM on the transposed lists; the
    item graph's forward.
Prints one JSON line.  Needs a GPU: there is no CPU fallback for the measured path.

Usage:  python tools/dragon_step_time.py [--steps 20] [--repeats 5] [--warmup 5] [--scale 1.0]
"""
from __future__ import annotations

import json

import numpy as np
import torch

from _step_time import alternated, parser, require_gpu, synth_model, trainer_runs


def main():
    args = parser(steps=20, warmup=5).parse_args()
    require_gpu("dragon_step_time", args)
    import dragon_ref as R
    from rsx import _lib as L
    from rsx import dragon as M
    from rsx import ops
    from rsx.dense import _Gemm, _Normalize
    from rsx.dualgnn import propagate
    from rsx.optim import RsxAdam

    m, c, batches, n_edges = synth_model("DRAGON", "baby", args, dict(learning_rate=0.001, reg_weight=0.001,
                                                                       is_multimodal_model=True),
                                         (("image_feat_raw.npy", 4096, 5), ("text_feat_raw.npy", 384, 6)))
    m.train()
    np.random.seed(999)
    m.pre_epoch_processing()
    d, B, nu, ni, n = m.width, 2048, m.n_users, m.n_items, m.n_nodes
    dev = m.device
    lens = np.diff(m.user_graph.ptr)
    res = {"n_users": nu, "n_items": ni, "train_edges": n_edges, "d": d, "F": [4096, 384], "batch": B, "k": m.k,
           "knn_k": m.knn_k, "n_mm_layers": m.n_layers, "mm_adj_nnz": int(m.mm_adj.A.nnz),
           "user_lists": {"source": m.user_graph_source, "shorter_than_k": int((lens < m.k).sum()), "empty": int((lens == 0).sum())},
           "transposed_lists": {"n_long": int(m.PT.n_long), "max_in_degree": int(np.diff(m.PT.rowptr_host).max())},
           "steps_per_window": args.steps, "windows": args.repeats, "warmup": args.warmup, "format": "[median, min, max] ms"}
    trip = batches[0]
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

    mods = m._mods()

    def mlp2(g, f):
        hid = _Gemm.apply(f, None, g.MLP.weight, g.MLP.bias, False, True)
        return _Gemm.apply(hid, None, g.MLP_1.weight, g.MLP_1.bias, False, False)

    with torch.no_grad():
        xn = {k: _Normalize.apply(torch.cat([g.preference, mlp2(g, f)])) for k, g, f in mods}
        xh = {k: propagate(m.A, x) for k, x in xn.items()}

    def mlp():
        out = 0
        for k, g, f in mods:
            temp = mlp2(g, f)
            out = out + _Normalize.apply(torch.cat([g.preference, temp], dim=0)).sum()
        return out

    def prop():
        return sum(M._Prop.apply(leaf(xn[k]), m.A).sum() for k, _, _ in mods)

    def tail():
        cfg = (nu, m.reg_weight, m._table, m.mm_adj, m.n_layers, m.epoch_idx, m.epoch_W, m.PT, m._ws, None)
        return M._Tail.apply(cfg, trip, leaf(xh["v"]), leaf(xh["t"]), m.weight_u, m.v_gcn.preference,
                             m.t_gcn.preference)

    def whole():
        return m.calculate_loss(trip)

    opt = RsxAdam([p for name, p in m.named_parameters() if name not in R.UNUSED], lr=1e-3)
    fwd_bwd(whole)()  # gradients for the update to read

    # the reference's ops in float32 torch on the same tensors
    P = {name: p for name, p in m.named_parameters()}

    def sparse_of(csr, rows_n, cols_n):
        rows = torch.repeat_interleave(torch.arange(rows_n, device=dev), csr.rowptr[1:] - csr.rowptr[:-1])
        return torch.sparse_coo_tensor(torch.stack([rows, csr.col.long()]), csr.val, (rows_n, cols_n)).coalesce()

    A = sparse_of(m.A, n, n)
    mm = sparse_of(m.mm_adj.A, ni, ni)
    feats = {"v": m.v_feat, "t": m.t_feat}
    idx64 = m.epoch_idx.long()

    def torch_whole():
        result, _, _ = R.forward(P, feats, A, mm, m.n_layers, idx64, m.epoch_W, nu)
        return R.loss(P, feats, result, trip, nu, m.reg_weight)[0]

    with torch.no_grad():
        res["hip_vs_torch_loss_rel_diff"] = float(abs(whole() - torch_whole()) / abs(torch_whole()))
    res.update(alternated(args, {"model_fwd_bwd_eager": fwd_bwd(whole), "model_fwd_bwd_torch_ops": fwd_bwd(torch_whole)}))
    res.update(alternated(args, {"mlp_fwd_bwd": fwd_bwd(mlp), "prop_fwd_bwd": fwd_bwd(prop), "tail_fwd_bwd": fwd_bwd(tail)}))
    fwd_bwd(whole)()
    res.update(alternated(args, {"adam": opt.step}))
    total = res["model_fwd_bwd_eager"][0]
    res["share_of_fwd_bwd"] = {k: round(res[k + "_fwd_bwd"][0] / total, 3) for k in ("mlp", "prop", "tail")}
    m.zero_grad(set_to_none=True)

    # ---- the user graph's forward at 128: the list kernel against the same lists as a CSR on the SpMM
    user_rep = m.last_user_rep
    idx, W = m.epoch_idx.cpu().numpy(), m.epoch_W.cpu().numpy()
    Pcsr = ops.DeviceCSR(np.arange(nu + 1, dtype=np.int64) * m.k, idx.reshape(-1), W.reshape(-1), nu, dev, m.chunk)
    out_a, out_b = torch.empty_like(user_rep), torch.empty_like(user_rep)
    g = torch.randn(n, d, device=dev)
    item_rep = torch.randn(ni, d, device=dev)
    item_out = torch.empty_like(item_rep)
    res.update(alternated(args, {
        "ugraph_fwd_kernel": lambda: M.ugraph_fwd(user_rep, m.epoch_idx, m.epoch_W, out=out_a),
        "ugraph_fwd_spmm_add": lambda: Pcsr.spmm_epi(user_rep, ops.epi(L.RSX_EPI_ADD, y=out_b, s_in=user_rep), d),
        "ugraph_bwd_spmm_add": lambda: M.ugraph_bwd(m.PT, g, nu),
        "item_graph_fwd": lambda: M.graph_residual(m.mm_adj.A, item_rep, m.n_layers, out=item_out),
        "cat_fwd": lambda: M.cat_fwd(xh["v"], xh["t"], m.weight_u, nu)}, steps=5 * args.steps))
    res["ugraph_kernel_vs_spmm_max_abs_diff"] = float((out_a - out_b).abs().max())

    # ---- the step through the Trainer, eager and captured
    res.update(trainer_runs(args, c, m, batches))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
