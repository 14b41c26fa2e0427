"""DRAGON restated in dense torch (float64 by default), from the formulas of the reference's
src/models/dragon.py, on the pieces of tests/dualgnn_ref.py: per modality DualGNN's GCN (`gcn`);
the concatenation of the two 64-wide tables with the per-user weights on the user rows (`cat`);
the frozen item graph's residual item_rep + mm_adj^L item_rep (`item_prop`); DualGNN's user graph
(`ugraph`); the base-2 BPR loss with the preference and `weight_u` regularisers and no `weight_i`
term (`loss`).

`cat_backward` is derived by hand; tests/test_dragon_cpu.py checks it against autograd through
`cat`.  `dtype=torch.float32` tensors give the float32 composition of the same ops: what a GPU
test of a kernel scales its bounds by.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from dualgnn_ref import (GOLD, K_USER, MODS, Adam, adam_tolerance, cast, gcn, hparams, lists_of, load,  # noqa: F401
                         rows, strides, sym_operator, topk_sample_ref, ugraph, ugraph_backward)

# nothing reads them (dragon.py:53-54, 64-68, 96-98, 140)
UNUSED = ("weight_i", "MLP_v.weight", "MLP_t.weight", "image_embedding.weight", "image_trs.weight", "image_trs.bias",
          "text_embedding.weight", "text_trs.weight", "text_trs.bias", "MLP_user.weight", "MLP_user.bias")
_FEAT = {"v": "image", "t": "text"}


def names(mods=MODS):
    """named_parameters() of the reference's model: its own Parameters, then the modules in
    creation order (dragon.py:53-156)."""
    out = ["weight_u", "weight_i", "MLP_v.weight", "MLP_t.weight"]
    for m in mods:
        out += [f"{_FEAT[m]}_embedding.weight", f"{_FEAT[m]}_trs.weight", f"{_FEAT[m]}_trs.bias"]
    out += ["MLP_user.weight", "MLP_user.bias"]
    for m in mods:
        out += [f"{m}_gcn.preference", f"{m}_gcn.MLP.weight", f"{m}_gcn.MLP.bias", f"{m}_gcn.MLP_1.weight",
                f"{m}_gcn.MLP_1.bias"]
    return tuple(out)


def trained(mods=MODS):
    return tuple(n for n in names(mods) if n not in UNUSED)


def cat(xv, xt, weight_u, n_users: int):
    """(user_rep, item_rep) of dragon.py:231-245.  Both tables: [w0 v | w1 t] on the user rows and
    [v | t] on the item rows, 128 wide; one table: its row blocks, `weight_u` not applied."""
    if xv is None or xt is None:
        x = xv if xt is None else xt
        return x[:n_users], x[n_users:]
    w = weight_u.reshape(n_users, 2)
    user_rep = torch.cat((w[:, :1] * xv[:n_users], w[:, 1:] * xt[:n_users]), dim=1)
    return user_rep, torch.cat((xv[n_users:], xt[n_users:]), dim=1)


def cat_backward(g_user, g_item, xv, xt, weight_u, n_users: int):
    """(g_v, g_t, g_weight_u [nu, 2]) of `cat` (both modalities) by hand."""
    w = weight_u.reshape(n_users, 2)
    h = xv.shape[1]
    g_v = torch.cat((w[:, :1] * g_user[:, :h], g_item[:, :h]))
    g_t = torch.cat((w[:, 1:] * g_user[:, h:], g_item[:, h:]))
    g_w = torch.stack(((g_user[:, :h] * xv[:n_users]).sum(1), (g_user[:, h:] * xt[:n_users]).sum(1)), dim=1)
    return g_v, g_t, g_w


def item_prop(item_rep, mm_adj, layers: int):
    """item_rep + mm_adj^layers item_rep (dragon.py:248-253); layers = 0 doubles the rows."""
    h = item_rep
    for _ in range(layers):
        h = mm_adj @ h
    return item_rep + h


def mm_adj_dense(z, n_items: int, dtype=torch.float64) -> torch.Tensor:
    """The fixture's mm_adj (COO, float32 values) as a dense [ni, ni] matrix."""
    A = torch.zeros(n_items, n_items, dtype=torch.float64)
    A[torch.from_numpy(z["mm_adj_row"].astype(np.int64)), torch.from_numpy(z["mm_adj_col"].astype(np.int64))] = \
        torch.from_numpy(z["mm_adj_val"]).double()
    return A.to(dtype)


def forward(P, feats, A, mm_adj, layers: int, idx, W, n_users: int, keep=None):
    """(result [n, 128 | 64], user_rep, {modality: x_hat}); feats: {"v": X_v, "t": X_t}, either
    alone is legal."""
    xs = {}
    for m in MODS:
        if m in feats:
            km = None if keep is None else keep.setdefault(m, {})
            xs[m] = gcn(P, m, feats[m], A, km)
    user_rep, item_rep = cat(xs.get("v"), xs.get("t"), P["weight_u"], n_users)
    result = torch.cat((ugraph(user_rep, idx, W), item_prop(item_rep, mm_adj, layers)), dim=0)
    return result, user_rep, xs


def loss(P, feats, result, trip, n_users: int, reg_weight: float):
    """(total, bpr, reg) of dragon.py:262-277 on int64 triplets [3, B] (item ids, not offset)."""
    u, p, n = trip[0], trip[1] + n_users, trip[2] + n_users
    pos, neg = (result[u] * result[p]).sum(1), (result[u] * result[n]).sum(1)
    bpr = F.softplus(-(pos - neg)).mean() / math.log(2.0)
    reg = sum((P[f"{m}_gcn.preference"][u] ** 2).mean() for m in MODS if m in feats) * reg_weight
    reg = reg + reg_weight * (P["weight_u"] ** 2).mean()
    return bpr + reg, bpr, reg


def step(P, feats, A, mm_adj, layers, idx, W, trip, n_users: int, reg_weight: float, keep=None):
    """One forward / backward: (result, user_rep, x_hats, (total, bpr, reg), grads by name; None
    for a parameter nothing reads)."""
    for v in P.values():
        v.grad = None
    result, user_rep, xs = forward(P, feats, A, mm_adj, layers, idx, W, n_users, keep)
    terms = loss(P, feats, result, trip, n_users, reg_weight)
    terms[0].backward()
    return (result.detach(), user_rep.detach(), {m: x.detach() for m, x in xs.items()}, terms,
            {k: (None if v.grad is None else v.grad.clone()) for k, v in P.items()})
