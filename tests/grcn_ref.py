"""GRCN restated in dense torch with autograd (float64 by default), from the formulas of the
reference's src/models/grcn.py: the content GCNs with their literal routing loop, the edge
attention with PyG's softmax (the 1e-16 in the denominator differentiated exactly), the
confidence / max / ReLU edge weight, the two id propagation layers, the loss and Adam.

`dtype=torch.float32` gives the float32 composition of the same ops: what a GPU test of a
kernel scales its bounds by (its error against the float64 run on the same inputs).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

SLOPE = 0.01  # F.leaky_relu's default


def edge_index(train_u, train_i, n_users: int) -> torch.Tensor:
    """[2, E] int64: row 0 the users, row 1 n_users + item (grcn.py:191-193, 217-221)."""
    u = torch.as_tensor(train_u, dtype=torch.int64)
    return torch.stack([u, torch.as_tensor(train_i, dtype=torch.int64).to(u.device) + int(n_users)])


def both_ways(ei: torch.Tensor) -> torch.Tensor:
    """The 2 E edges: the E user -> item edges, then the E item -> user edges."""
    return torch.cat([ei, ei[[1, 0]]], dim=1)


def edge_softmax(s: torch.Tensor, index: torch.Tensor, n: int) -> torch.Tensor:
    """PyG's softmax: exp(s - max) / (sum exp(s - max) + 1e-16) over the edges of one target."""
    mx = torch.full((n,), -float("inf"), dtype=s.dtype, device=s.device).scatter_reduce(
        0, index, s.detach(), reduce="amax", include_self=True)
    out = (s - mx[index]).exp()
    den = torch.zeros(n, dtype=s.dtype, device=s.device).index_add_(0, index, out) + 1e-16
    return out / den[index]


def gat(x: torch.Tensor, ei: torch.Tensor):
    """(h, alpha): h_t = sum over the edges (j -> t) of alpha x_j, alpha the softmax over t's
    in-edges of <x_t, x_j> (grcn.py:46-76; source row 0, target row 1)."""
    xj, xi = x[ei[0]], x[ei[1]]
    a = edge_softmax((xi * xj).sum(-1), ei[1], x.shape[0])
    return torch.zeros_like(x).index_add_(0, ei[1], xj * a[:, None]), a


def cgcn(feat, pref, W, b, ei, n_users: int, n_routing: int, keep=None):
    """(rep [n, d_c], alpha [2 E]) of one content GCN (grcn.py:139-166).  keep: a dict that
    receives `routing_user_rows`, the user rows of every routing aggregate."""
    f = F.normalize(F.leaky_relu(feat @ W.t() + b, SLOPE))
    p = F.normalize(pref)
    rows = []
    for _ in range(n_routing):  # the directed edges: the aggregate lands on item rows only
        h, _ = gat(torch.cat([p, f], dim=0), ei)
        rows.append(h[:n_users].detach())
        p = F.normalize(p + h[:n_users])
    if keep is not None:
        keep["routing_user_rows"] = rows
    x = torch.cat([p, f], dim=0)
    h, a = gat(x, both_ways(ei))
    return x + h, a


def refined_weight(alphas, conf, ei):
    """relu(max_m alpha_m * C[source, m]) [2 E] and the winning modality (grcn.py:272-281)."""
    c = torch.cat([conf[ei[0]], conf[ei[1]]], dim=0)
    w, arg = torch.max(torch.stack(alphas, dim=1) * c, dim=1)
    return torch.relu(w), arg


def egcn(emb, ei2, w):
    """x + h1 + h2 (grcn.py:93-109): two propagations through the same edge weights."""
    x = F.normalize(emb)
    h1 = torch.zeros_like(x).index_add_(0, ei2[1], x[ei2[0]] * w[:, None])
    h2 = torch.zeros_like(x).index_add_(0, ei2[1], h1[ei2[0]] * w[:, None])
    return x + h1 + h2


MODS = ("v", "t")


def cast(params: dict, dtype, device=None) -> dict:
    return {k: v.detach().to(dtype=dtype, device=device).clone().requires_grad_(True) for k, v in params.items()}


def forward(P: dict, feats: dict, ei, n_users: int, n_layers: int, keep=None) -> dict:
    """P: parameters by the reference's names; feats: {"v": X_v, "t": X_t} (t optional).
    Returns id_rep, reps, alphas (reference [2 E] order), weight, arg, representation."""
    reps, alphas = [], []
    for m in MODS:
        if m in feats:
            r, a = cgcn(feats[m], P[f"{m}_gcn.preference"], P[f"{m}_gcn.MLP.weight"], P[f"{m}_gcn.MLP.bias"], ei,
                        n_users, n_layers, keep if m == "v" else None)
            reps.append(r)
            alphas.append(a)
    w, arg = refined_weight(alphas, P["model_specific_conf"], ei)
    id_rep = egcn(P["id_gcn.id_embedding"], both_ways(ei), w)
    return dict(id_rep=id_rep, reps=reps, alphas=alphas, weight=w, arg=arg,
                representation=torch.cat([id_rep, *reps], dim=1))


def loss(P: dict, feats: dict, rep: torch.Tensor, trip: torch.Tensor, n_users: int, reg_weight: float):
    """(total, bpr, reg) of grcn.py:300-333 on int64 triplets [3, B] (item ids, not offset)."""
    u, p, n = trip[0], trip[1] + n_users, trip[2] + n_users
    ut = u.repeat_interleave(2)
    it = torch.stack([p, n]).t().reshape(-1)
    score = (rep[ut] * rep[it]).sum(1).view(-1, 2)
    bpr = F.softplus(-(score[:, 0] - score[:, 1])).mean()
    E = P["id_gcn.id_embedding"]
    reg = (E[ut] ** 2 + E[it] ** 2).mean()
    if "v" in feats:
        reg = reg + (P["v_gcn.preference"] ** 2).mean()
    for m in MODS:
        if m in feats:
            reg = reg + (P[f"{m}_gcn.preference"][ut] ** 2).mean()
    reg = reg_weight * reg
    return bpr + reg, bpr, reg


def step(P: dict, feats: dict, ei, trip, n_users: int, n_layers: int, reg_weight: float):
    """One forward / backward: (forward dict, (total, bpr, reg), grads by name)."""
    for v in P.values():
        v.grad = None
    fw = forward(P, feats, ei, n_users, n_layers)
    terms = loss(P, feats, fw["representation"], trip, n_users, reg_weight)
    terms[0].backward()
    return fw, terms, {k: v.grad.clone() for k, v in P.items()}


class Adam:
    """torch.optim.Adam's update (no weight decay, no amsgrad) in the parameters' dtype."""

    def __init__(self, P: dict, lr: float, betas=(0.9, 0.999), eps: float = 1e-8):
        self.P, self.lr, self.b1, self.b2, self.eps, self.t = P, lr, betas[0], betas[1], eps, 0
        self.m = {k: torch.zeros_like(v) for k, v in P.items()}
        self.v = {k: torch.zeros_like(v) for k, v in P.items()}

    def step(self, grads: dict):
        self.t += 1
        with torch.no_grad():
            for k, p in self.P.items():
                g = grads[k]
                self.m[k].mul_(self.b1).add_(g, alpha=1 - self.b1)
                self.v[k].mul_(self.b2).addcmul_(g, g, value=1 - self.b2)
                den = (self.v[k].sqrt() / (1 - self.b2 ** self.t) ** 0.5).add_(self.eps)
                p.addcdiv_(self.m[k], den, value=-self.lr / (1 - self.b1 ** self.t))


def adam_tolerance(grad_diffs, grads_ref, lr: float, eps: float = 1e-8):
    """What Adam's first two updates can turn a gradient difference into, per element (numpy):
    3 lr sum_s |dg_s| / (|g_s| + eps) over the steps taken so far.  The first update is
    lr g / (|g| + eps), whose change under g -> g + dg is lr eps |dg| / ((|g| + eps)(|g + dg| + eps))
    <= lr |dg| / (|g| + eps).  The second is lr m / (sqrt(v) + eps) with m = 0.474 g0 + 0.526 g1
    and v = 0.4997 g0^2 + 0.5003 g1^2 (bias-corrected): |m| <= sqrt(v) and sqrt(v) >= 0.707 |g_s|,
    so its derivative in either gradient is below 1.75 lr / (|g_s| + eps); with the first
    update's term that is below 3 lr |dg_s| / (|g_s| + eps) a step.  Where |g| is far above eps
    the term vanishes (the update is lr sign(g)); where |g| is near eps a float32 rounding of g
    moves the update by a fraction of lr, whichever implementation rounded."""
    import numpy as np

    tol = 0.0
    for dg, g in zip(grad_diffs, grads_ref):
        tol = tol + 3.0 * lr * np.abs(dg) / (np.abs(g) + eps)
    return tol
