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


def torch_ssl(T1, T2, idx, tau):
    """lgmrec.py:159-166 on whole tables: the B x N matrix is formed."""
    n1, n2, na = F.normalize(T1[idx]), F.normalize(T2[idx]), F.normalize(T2)
    pos = torch.exp((n1 * n2).sum(1) / tau)
    ttl = torch.exp(n1 @ na.t() / tau).sum(1)
    return -torch.log(pos / ttl).sum()


def build(args, root):
    from scipy.sparse import coo_matrix

    from rsx import synth
    from rsx.config import Config
    from rsx.lgmrec import LGMRec
    from rsx.utils import init_seed

    df = synth.shaped("baby", seed=0, scale=args.scale)
    df = df[df.x_label == 0]
    nu, ni = int(df.userID.max()) + 1, int(df.itemID.max()) + 1
    os.makedirs(os.path.join(root, "baby"))
    np.save(os.path.join(root, "baby", "image_feat_raw.npy"), synth.features(ni, 4096, seed=5))
    np.save(os.path.join(root, "baby", "text_feat_raw.npy"), synth.features(ni, 384, seed=6))
    c = Config("LGMRec", "baby", dict(data_path=root + "/", train_batch_size=2048, learning_rate=0.001, seed=999,
                                      is_multimodal_model=True))
    for k in c["hyper_parameters"]:
        if isinstance(c[k], list):
            c[k] = c[k][0]
    ds = types.SimpleNamespace(get_user_num=lambda: nu, get_item_num=lambda: ni)
    loader = types.SimpleNamespace(dataset=ds, inter_matrix=lambda form="coo": coo_matrix(
        (np.ones(len(df)), (df.userID.values, df.itemID.values)), shape=(nu, ni)))
    init_seed(999)
    m = LGMRec(c, loader)
    rng = np.random.default_rng(1)
    sel = rng.permutation(len(df))[: 4 * 2048].reshape(4, 2048)
    batches = [torch.from_numpy(np.stack([df.userID.values[s], df.itemID.values[s],
                                          rng.integers(0, ni, 2048)]).astype(np.int64)).cuda() for s in sel]
    return m, c, batches, len(df)


def alternated(args, runs: dict) -> dict:
    """ms per iteration of each run in `runs`, their windows alternated: name -> [median, min, max]."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for run in runs.values():
        for _ in range(args.warmup):
            run()
    torch.cuda.synchronize()
    out = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, run in runs.items():
            e0.record()
            for _ in range(args.steps):
                run()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) / args.steps)
    return {k: [round(sorted(v)[len(v) // 2], 4), round(min(v), 4), round(max(v), 4)] for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50, help="iterations per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per variant (median, min, max reported)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graph (a rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lgmrec_step_time: needs a GPU (step times are device measurements)")
    if args.repeats < 5:
        raise SystemExit("lgmrec_step_time: at least 5 windows")
    from rsx import lgmrec as LG
    from rsx.trainer import Trainer

    with tempfile.TemporaryDirectory() as root:
        m, c, batches, n_edges = build(args, root)
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
    for graph in (False, True):  # the capture last: a failed capture leaves the stream unusable
        c["rsx_graph_step"] = graph
        t = Trainer(c, m)
        k = [0]

        def step(t=t, k=k):
            t.train_step(batches[k[0] % len(batches)], k[0])
            k[0] += 1

        try:
            res.update(alternated(args, {f"step_{'graph' if graph else 'eager'}": step}))
        except RuntimeError as e:
            if not graph:
                raise
            res["step_graph"] = "not measured: " + str(e).splitlines()[0][:160]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
