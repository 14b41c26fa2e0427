"""MMGCN restated in dense torch (float64 by default), from the formulas of the reference's
src/models/mmgcn.py: the concatenating branch (`self.concate = 'False'` is a non-empty string),
three layers whatever `n_layers` says, the id embedding, the preferences and `result` plain
tensors (constants: no gradient, never updated), the mean operator D^-1 A on the n_users +
n_items nodes, the loss and Adam.

One layer is `layer` (the literal `cat`) with the hand-derived backward `layer_backward`; the
model's own gradients come from autograd through the same `layer`, so the two check each other
(tests/test_mmgcn_cpu.py).  `dtype=torch.float32` gives the float32 composition of the same
ops: what a GPU test of a kernel scales its bounds by.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

from grcn_ref import Adam, adam_tolerance, cast  # noqa: F401 - the same optimiser and bounds

SLOPE = 0.01  # F.leaky_relu's default
MODS = ("v", "t")
LATENT = 256  # the image branch's MLP width (mmgcn.py:47)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONSTS = ("id_embedding", "v_gcn.preference", "t_gcn.preference", "result")


def names(mods=MODS):
    """The trained parameters in the reference's creation order (mmgcn.py:125-162)."""
    out = []
    for m in mods:
        if m == "v":
            out += ["v_gcn.MLP.weight", "v_gcn.MLP.bias"]
        for k in (1, 2, 3):
            out += [f"{m}_gcn.conv_embed_{k}.weight", f"{m}_gcn.linear_layer{k}.weight", f"{m}_gcn.linear_layer{k}.bias",
                    f"{m}_gcn.g_layer{k}.weight", f"{m}_gcn.g_layer{k}.bias"]
    return tuple(out)


def load(name):
    return np.load(os.path.join(GOLD, name))


def hparams(z):
    return dict(s.split("=", 1) for s in z["hparams"])


def strides(z):
    return {k: int(v) for k, v in (s.split("=", 1) for s in z["row_strides"])}


def rows(a, k):
    """What the fixtures keep of an array: tables of 64 rows or more at row stride k."""
    return a[::k] if a.ndim == 2 and a.shape[0] >= 64 else a


def mean_operator(train_u, train_i, n_users: int, n_items: int, dtype=torch.float64) -> torch.Tensor:
    """Dense D^-1 A [n, n]: the training interactions in both directions (mmgcn.py:39-42), a
    duplicate interaction counted with its multiplicity, PyG's mean over the in-edges (a node
    without edges: a zero row)."""
    n = n_users + n_items
    u = torch.as_tensor(np.asarray(train_u), dtype=torch.int64)
    i = torch.as_tensor(np.asarray(train_i), dtype=torch.int64) + n_users
    A = torch.zeros(n, n, dtype=torch.float64)
    one = torch.ones(u.numel(), dtype=torch.float64)
    A.index_put_((u, i), one, accumulate=True)
    A.index_put_((i, u), one, accumulate=True)
    deg = A.sum(1, keepdim=True)
    return (A / deg.clamp_min(1.0)).to(dtype)


def operator_coo(A: torch.Tensor):
    """(idx [2, nnz] int64, val) of a dense operator, row-major."""
    idx = A.nonzero().t().contiguous()
    return idx.numpy(), A[idx[0], idx[1]].numpy()


def leaky(x):
    return F.leaky_relu(x, SLOPE)


def slope(pre):
    return torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, SLOPE))


def layer(a, x, E, Wc, Wl, bl, Wg, bg, keep=None):
    """One GCN layer (mmgcn.py:170-174) on a = A_hat x: h = leaky(a Wc), x_hat = leaky(x Wl^T + bl) + E,
    out = leaky(cat(h, x_hat) Wg^T + bg).  keep: receives the three pre-activations and h, u, x_hat."""
    ph = a @ Wc
    h = leaky(ph)
    pu = x @ Wl.t() + bl
    u = leaky(pu)
    xh = u + E
    po = torch.cat((h, xh), dim=1) @ Wg.t() + bg
    if keep is not None:
        keep.update(ph=ph, pu=pu, po=po, h=h, u=u, xh=xh)
    return leaky(po)


def layer_backward(g_out, a, x, E, Wc, Wl, bl, Wg, bg):
    """The gradients of `layer` by hand: g_a, g_x (the direct part, through Wl), g_E, the three
    pre-activation gradients (go, gh, gu) and dWc, dWl, dbl, dWg, dbg."""
    k = {}
    layer(a, x, E, Wc, Wl, bl, Wg, bg, k)
    w = Wc.shape[1]
    go = g_out * slope(k["po"])
    gcat = go @ Wg
    gh = gcat[:, :w] * slope(k["ph"])
    gxh = gcat[:, w:]
    gu = gxh * slope(k["pu"])
    return dict(g_a=gh @ Wc.t(), g_x=gu @ Wl, g_E=gxh, go=go, gh=gh, gu=gu, dWc=a.t() @ gh, dWl=gu.t() @ x,
                dbl=gu.sum(0), dWg=go.t() @ torch.cat((k["h"], k["xh"]), dim=1), dbg=go.sum(0))


def layer_inputs(d, w, n, seed, dtype=torch.float64):
    """Seeded inputs of one layer of input width w, output width d, on n rows (the CPU and the
    GPU tests build theirs here, so the flagged-row rate checked on the CPU is the GPU tests')."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(dtype)  # noqa: E731
    return dict(a=r(n, w) * 0.5, x=r(n, w) * 0.5, E=r(n, d) * 0.3, Wc=r(w, w) / w ** 0.5, Wl=r(d, w) / w ** 0.5,
                bl=r(d) * 0.1, Wg=r(d, w + d) / (w + d) ** 0.5, bg=r(d) * 0.1)


def near_zero_rows(pres, rel=1e-5):
    """Rows where any of the pre-activation tensors `pres` is within rel of that tensor's scale of
    zero: where a float32 rounding can move an element across leaky_relu's kink."""
    flag = torch.zeros(pres[0].shape[0], dtype=torch.bool)
    for p in pres:
        flag |= (p.abs() <= rel * p.abs().max()).any(dim=1)
    return flag


def gcn(P, C, m, feat, A, keep=None):
    """One modality's GCN (mmgcn.py:164-188): x [n, d].  keep: `x0`, and per layer k = 1..3
    `x{k}` and the pre-activations `ph{k}`, `pu{k}`, `po{k}`."""
    pre = f"{m}_gcn."
    temp = feat @ P[pre + "MLP.weight"].t() + P[pre + "MLP.bias"] if m == "v" else feat
    x = F.normalize(torch.cat((C[pre + "preference"], temp), dim=0))
    if keep is not None:
        keep["x0"] = x
    for k in (1, 2, 3):
        kk = {}
        x = layer(A @ x, x, C["id_embedding"], P[f"{pre}conv_embed_{k}.weight"], P[f"{pre}linear_layer{k}.weight"],
                  P[f"{pre}linear_layer{k}.bias"], P[f"{pre}g_layer{k}.weight"], P[f"{pre}g_layer{k}.bias"], kk)
        if keep is not None:
            keep[f"x{k}"] = x
            for s in ("ph", "pu", "po"):
                keep[f"{s}{k}"] = kk[s]
    return x


def forward(P, C, feats, A, keep=None):
    """(representation, {modality: x}) (mmgcn.py:64-77); feats: {"v": X_v, "t": X_t}, either alone is legal."""
    xs = {}
    for m in MODS:
        if m in feats:
            km = None if keep is None else keep.setdefault(m, {})
            xs[m] = gcn(P, C, m, feats[m], A, km)
    rep = sum(xs.values()) / len(xs)
    return rep, xs


def loss(C, feats, rep, trip, n_users: int, reg_weight: float):
    """(total, bpr, reg) of mmgcn.py:79-97 on int64 triplets [3, B] (item ids, not offset).  reg has no
    gradient (its tensors are constants) but is part of the value."""
    u, p, n = trip[0], trip[1] + n_users, trip[2] + n_users
    ut = u.repeat_interleave(2)
    it = torch.stack([p, n]).t().reshape(-1)
    score = (rep[ut] * rep[it]).sum(1).view(-1, 2)
    bpr = F.softplus(-(score[:, 0] - score[:, 1])).mean()
    E = C["id_embedding"]
    reg = (E[ut] ** 2 + E[it] ** 2).mean()
    if "v" in feats:
        reg = reg + (C["v_gcn.preference"] ** 2).mean()
    reg = reg_weight * reg
    return bpr + reg, bpr, reg


def step(P, C, feats, A, trip, n_users: int, reg_weight: float, keep=None):
    """One forward / backward: (representation, (total, bpr, reg), grads by name)."""
    for v in P.values():
        v.grad = None
    rep, _ = forward(P, C, feats, A, keep)
    terms = loss(C, feats, rep, trip, n_users, reg_weight)
    terms[0].backward()
    return rep.detach(), terms, {k: v.grad.clone() for k, v in P.items()}


def consts(C, dtype, device=None):
    return {k: v.detach().to(dtype=dtype, device=device) for k, v in C.items()}
