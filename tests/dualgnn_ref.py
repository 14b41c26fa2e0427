"""DualGNN restated in dense torch (float64 by default), from the formulas of the reference's
src/models/dualgnn.py: per modality x = normalize([preference; MLP_1(leaky(MLP(feat)))]),
x_hat = (A x + x) + A A x on the symmetric operator D^-1/2 A D^-1/2; the in-place alias of the
modality sum (the image table holds v + t when the user mix reads it); the user graph's weighted
sum over the epoch's lists; the base-2 BPR loss and its regularisers; `topk_sample_ref`, the
sampler as the reference's literal loop.

`mix_backward` and `ugraph_backward` are derived by hand; tests/test_dualgnn_cpu.py checks them
against autograd through `mix` and `ugraph`.  `dtype=torch.float32` gives the float32 composition
of the same ops: what a GPU test of a kernel scales its bounds by.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from grcn_ref import Adam, adam_tolerance, cast  # noqa: F401 - the same optimiser and bounds
from mmgcn_ref import GOLD, hparams, load, rows, strides  # noqa: F401 - the fixtures' conventions

MODS = ("v", "t")
K_USER = 40
UNUSED = ("MLP_v.weight", "MLP_t.weight", "MLP_user.weight", "MLP_user.bias")  # nothing reads them


def names(mods=MODS):
    """named_parameters() of the reference's model: its own Parameters, then the modules in
    creation order (dualgnn.py:49-129)."""
    out = ["weight_u", "weight_i", "MLP_v.weight", "MLP_t.weight", "MLP_user.weight", "MLP_user.bias"]
    for m in mods:
        out += [f"{m}_gcn.preference", f"{m}_gcn.MLP.weight", f"{m}_gcn.MLP.bias", f"{m}_gcn.MLP_1.weight",
                f"{m}_gcn.MLP_1.bias"]
    return tuple(out)


def trained(mods=MODS):
    return tuple(n for n in names(mods) if n not in UNUSED)


def sym_operator(train_u, train_i, n_users: int, n_items: int, dtype=torch.float64) -> torch.Tensor:
    """Dense D^-1/2 A D^-1/2 [n, n]: the training interactions in both directions, a duplicate
    counted with its multiplicity, deg the plain edge count (dualgnn.py:334-342); a node without
    edges: a zero row."""
    n = n_users + n_items
    u = torch.as_tensor(np.asarray(train_u), dtype=torch.int64)
    i = torch.as_tensor(np.asarray(train_i), dtype=torch.int64) + n_users
    A = torch.zeros(n, n, dtype=torch.float64)
    one = torch.ones(u.numel(), dtype=torch.float64)
    A.index_put_((u, i), one, accumulate=True)
    A.index_put_((i, u), one, accumulate=True)
    dis = A.sum(1).clamp_min(1.0).pow(-0.5)
    return (dis[:, None] * A * dis[None, :]).to(dtype)


def lists_of(ptr, nbr, cnt):
    """{u: [[neighbours], [counts]]} of the flat arrays: the reference's dict, Python lists of int
    and float."""
    return {u: [[int(x) for x in nbr[ptr[u]:ptr[u + 1]]], [float(x) for x in cnt[ptr[u]:ptr[u + 1]]]]
            for u in range(len(ptr) - 1)}


def topk_sample_ref(d: dict, k: int = K_USER):
    """dualgnn.py:207-250 as written (softmax mode), on the global numpy generator: (idx [nu, k]
    int64, W [nu, k] float32)."""
    index, W = [], torch.zeros(len(d), k)
    for i in range(len(d)):
        if len(d[i][0]) < k:
            if len(d[i][0]) == 0:
                index.append([0] * k)
                continue
            sample, weight = d[i][0][:k], d[i][1][:k]
            while len(sample) < k:
                r = np.random.randint(0, len(sample))
                sample.append(sample[r])
                weight.append(weight[r])
            index.append(sample)
            W[i] = F.softmax(torch.tensor(weight), dim=0)
            continue
        index.append(d[i][0][:k])
        W[i] = F.softmax(torch.tensor(d[i][1][:k]), dim=0)
    return np.asarray(index, dtype=np.int64), W.numpy()


def gcn(P, m, feat, A, keep=None):
    """One modality's x_hat [n, 64] (dualgnn.py:304-315).  keep: `pre` (the MLP's pre-activation), `x`."""
    p = f"{m}_gcn."
    pre = feat @ P[p + "MLP.weight"].t() + P[p + "MLP.bias"]
    temp = F.leaky_relu(pre) @ P[p + "MLP_1.weight"].t() + P[p + "MLP_1.bias"]
    x = F.normalize(torch.cat((P[p + "preference"], temp), dim=0))
    if keep is not None:
        keep.update(pre=pre, x=x)
    h = A @ x
    h1 = A @ h
    return h + x + h1


def mix(xv, xt, weight_u, n_users: int, alias: bool = True):
    """(user_rep, item_rep) of dualgnn.py:146-170.  alias: `representation += t_rep` has added
    the text table into the image table before the user mix reads it (what the reference
    executes); alias=False is w0 v + w1 t, what the paper says."""
    if xv is None or xt is None:
        x = xv if xt is None else xt
        return x[:n_users], x[n_users:]
    s = xv + xt
    w = weight_u.reshape(n_users, 2)
    first = s if alias else xv
    user_rep = w[:, :1] * first[:n_users] + w[:, 1:] * xt[:n_users]
    return user_rep, s[n_users:]


def mix_backward(g_user, g_item, xv, xt, weight_u, n_users: int):
    """(g_v, g_t, g_weight_u [nu, 2]) of `mix` (both modalities, the alias) by hand."""
    w = weight_u.reshape(n_users, 2)
    w0, w1 = w[:, :1], w[:, 1:]
    g_v = torch.cat((w0 * g_user, g_item))
    g_t = torch.cat(((w0 + w1) * g_user, g_item))
    s = (xv + xt)[:n_users]
    g_w = torch.stack(((g_user * s).sum(1), (g_user * xt[:n_users]).sum(1)), dim=1)
    return g_v, g_t, g_w


def _index(idx):
    return idx.to(torch.int64) if torch.is_tensor(idx) else torch.as_tensor(np.asarray(idx), dtype=torch.int64)


def ugraph(user_rep, idx, W):
    """user_rep + sum_j W[u, j] user_rep[idx[u, j]] (dualgnn.py:172-173, 259-266)."""
    idx = _index(idx)
    return user_rep + (W.to(user_rep.dtype).unsqueeze(2) * user_rep[idx]).sum(1)


def ugraph_backward(g_out, idx, W):
    """g_user_rep = g_out + P^T g_out by hand: row s gathers W[u, j] g_out[u] over idx[u, j] = s."""
    idx = _index(idx)
    nu, k = idx.shape
    contrib = (W.to(g_out.dtype).unsqueeze(2) * g_out.unsqueeze(1)).reshape(nu * k, -1)
    return g_out + torch.zeros_like(g_out).index_add_(0, idx.reshape(-1), contrib)


def forward(P, feats, A, idx, W, n_users: int, keep=None, alias: bool = True):
    """(result [n, 64], user_rep, {modality: x_hat}); feats: {"v": X_v, "t": X_t}, either alone is legal."""
    xs = {}
    for m in MODS:
        if m in feats:
            km = None if keep is None else keep.setdefault(m, {})
            xs[m] = gcn(P, m, feats[m], A, km)
    user_rep, item_rep = mix(xs.get("v"), xs.get("t"), P["weight_u"], n_users, alias)
    result = torch.cat((ugraph(user_rep, idx, W), item_rep), dim=0)
    return result, user_rep, xs


def loss(P, feats, result, trip, n_users: int, reg_weight: float):
    """(total, bpr, reg) of dualgnn.py:182-197 on int64 triplets [3, B] (item ids, not offset)."""
    u, p, n = trip[0], trip[1] + n_users, trip[2] + n_users
    pos, neg = (result[u] * result[p]).sum(1), (result[u] * result[n]).sum(1)
    bpr = F.softplus(-(pos - neg)).mean() / math.log(2.0)
    reg = sum((P[f"{m}_gcn.preference"][u] ** 2).mean() for m in MODS if m in feats) * reg_weight
    reg = reg + reg_weight * (P["weight_u"] ** 2).mean() + reg_weight * (P["weight_i"] ** 2).mean()
    return bpr + reg, bpr, reg


def step(P, feats, A, idx, W, trip, n_users: int, reg_weight: float, keep=None, alias: bool = True):
    """One forward / backward: (result, user_rep, x_hats, (total, bpr, reg), grads by name; None
    for a parameter nothing reads)."""
    for v in P.values():
        v.grad = None
    result, user_rep, xs = forward(P, feats, A, idx, W, n_users, keep, alias)
    terms = loss(P, feats, result, trip, n_users, reg_weight)
    terms[0].backward()
    return (result.detach(), user_rep.detach(), {m: x.detach() for m, x in xs.items()}, terms,
            {k: (None if v.grad is None else v.grad.clone()) for k, v in P.items()})
