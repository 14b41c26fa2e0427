"""The contract of each kernel of csrc/grcn.hip stated in torch on slot-order arrays (float64 by
default): explicit formulas, forward AND backward, no autograd anywhere in this file.  The graph is
rsx.grcn.target_csr's: `Graph(rowptr, col, rev)` holds the target row `t` and the source `s` of
every slot.  `step` chains them (with F.normalize's and the MLP's hand-written backwards) into one
training step: tests/test_grcn_model_cpu.py checks it against autograd of tests/grcn_ref.py.

Every function takes the dtype of its inputs, so the same code in float32 is the torch composition
a GPU test scales its bound by."""
from __future__ import annotations

import numpy as np
import torch

SLOPE = 0.01
EPS = 1e-12  # F.normalize's


class Graph:
    def __init__(self, rowptr, col, rev):
        self.rowptr = torch.as_tensor(np.asarray(rowptr), dtype=torch.int64)
        self.n = self.rowptr.numel() - 1
        self.s = torch.as_tensor(np.asarray(col), dtype=torch.int64)  # source of a slot
        self.rev = torch.as_tensor(np.asarray(rev), dtype=torch.int64)
        self.t = torch.repeat_interleave(torch.arange(self.n), self.rowptr[1:] - self.rowptr[:-1])  # target
        self.nnz = self.s.numel()


def _rowsum(g: Graph, v: torch.Tensor) -> torch.Tensor:
    """Per target row, the sum of the per-slot values v ([nnz] or [nnz, d])."""
    return torch.zeros((g.n,) + tuple(v.shape[1:]), dtype=v.dtype).index_add_(0, g.t, v)


def attn_fwd(g: Graph, x):
    """(alpha [nnz], rep [n, d]): the softmax over a row's in-edges of <x_t, x_s>, max subtracted."""
    s = (x[g.t] * x[g.s]).sum(-1)
    mx = torch.full((g.n,), -float("inf"), dtype=x.dtype).scatter_reduce(0, g.t, s, reduce="amax", include_self=True)
    ex = (s - mx[g.t]).exp()
    alpha = ex / _rowsum(g, ex)[g.t]
    return alpha, x + _rowsum(g, alpha[:, None] * x[g.s])


def attn_bwd(g: Graph, g_rep, dalpha_ext, x, alpha):
    """dx [n, d] from g = d rep and the alphas' external gradient."""
    da = (g_rep[g.t] * x[g.s]).sum(-1) + dalpha_ext
    ds = alpha * (da - _rowsum(g, alpha * da)[g.t])
    dx = g_rep + _rowsum(g, ds[:, None] * x[g.s])  # row-local
    # the gather: row s collects, from every edge e it is the source of, ds_e x_t + alpha_e g_t
    e = g.rev  # slot j of row s = t(j) is the reverse of edge e = rev[j], whose target is s(j)
    return dx + _rowsum(g, ds[e][:, None] * x[g.s] + alpha[e][:, None] * g_rep[g.s])


def products(g: Graph, alphas, conf):
    """(the winning product [nnz], the winner [nnz], all products [nnz, M]); a tie goes to modality 0."""
    p = torch.stack(alphas, dim=1) * conf[g.s]
    win = torch.zeros(g.nnz, dtype=torch.int64) if len(alphas) == 1 else (p[:, 1] > p[:, 0]).long()
    return p.gather(1, win[:, None])[:, 0], win, p


def refine_fwd(g: Graph, alphas, conf):
    """(val, valT): w_e = relu(max_m alpha_m[e] conf[s, m]); valT[rev[e]] = w_e."""
    w = products(g, alphas, conf)[0].clamp_min(0)
    valT = torch.empty_like(w)
    valT[g.rev] = w
    return w, valT


def min_relative_gap(g: Graph, alphas, conf) -> float:
    """On edges with w > 0: the smallest |p_0 - p_1| relative to the larger magnitude (inf with one modality)."""
    if len(alphas) == 1:
        return float("inf")
    pm, _, p = products(g, alphas, conf)
    live = pm > 0
    gap = (p[:, 0] - p[:, 1]).abs() / p.abs().max(dim=1).values
    return float(gap[live].min())


def spmm(g: Graph, val, x):
    return _rowsum(g, val[:, None] * x[g.s])


def edge_dots(g: Graph, G, h1, D, x):
    return (G[g.t] * h1[g.s]).sum(-1) + (D[g.t] * x[g.s]).sum(-1)


def refine_bwd(g: Graph, alphas, conf, dw):
    """(dalphas, dconf)."""
    pm, win, _ = products(g, alphas, conf)
    live = pm > 0
    M = len(alphas)
    das = [torch.where(live & (win == m), dw * conf[g.s, m], torch.zeros_like(dw)) for m in range(M)]
    a_win = torch.stack(alphas, dim=1).gather(1, win[:, None])[:, 0]
    dconf = torch.zeros_like(conf).index_put_((g.s, win), torch.where(live, dw * a_win, torch.zeros_like(dw)),
                                              accumulate=True)
    return das, dconf


def id_gcn_fwd(g: Graph, val, xn):
    h1 = spmm(g, val, xn)
    return h1, xn + h1 + spmm(g, val, h1)


def id_gcn_bwd(g: Graph, val, valT, G, h1, xn):
    """(d xn, dw) from G = d id_rep."""
    D = G + spmm(g, valT, G)
    return G + spmm(g, valT, D), edge_dots(g, G, h1, D, xn)


def _softplus(x):
    return x.clamp_min(0) + torch.log1p(torch.exp(-x.abs()))


def loss_fwd(id_rep, reps, E, prefs, trip, nu: int, reg_weight: float):
    """({total, bpr, reg} [3], result [n, dx + M dc])."""
    rep = torch.cat([id_rep, *reps], dim=1)
    u, p, n = trip[0], trip[1] + nu, trip[2] + nu
    B = trip.shape[1]
    x = (rep[u] * rep[p]).sum(1) - (rep[u] * rep[n]).sum(1)
    bpr = _softplus(-x).sum() / B
    reg = (2 * E[u].pow(2).sum() + E[p].pow(2).sum() + E[n].pow(2).sum()) / (2 * B * E.shape[1])
    reg = reg + prefs[0].pow(2).mean()
    for pm in prefs:
        reg = reg + pm[u].pow(2).sum() / (B * pm.shape[1])
    reg = reg_weight * reg
    return torch.stack([bpr + reg, bpr, reg]), rep


def loss_bwd(id_rep, reps, E, prefs, trip, nu: int, reg_weight: float, go=1.0):
    """(g_id, [g_rep_m], gE, [gpref_m]): dense, zero off the batch, repeated rows summed."""
    rep = torch.cat([id_rep, *reps], dim=1)
    u, p, n = trip[0], trip[1] + nu, trip[2] + nu
    B = trip.shape[1]
    x = (rep[u] * rep[p]).sum(1) - (rep[u] * rep[n]).sum(1)
    ck = (-go / B * torch.sigmoid(-x))[:, None]
    G = torch.zeros_like(rep)
    G.index_add_(0, u, ck * (rep[p] - rep[n]))
    G.index_add_(0, p, ck * rep[u])
    G.index_add_(0, n, -ck * rep[u])
    k = go * reg_weight
    gE = torch.zeros_like(E)
    gE.index_add_(0, u, E[u] * (k * 4 / (2 * B * E.shape[1])))
    gE.index_add_(0, p, E[p] * (k * 2 / (2 * B * E.shape[1])))
    gE.index_add_(0, n, E[n] * (k * 2 / (2 * B * E.shape[1])))
    gps = []
    for j, pm in enumerate(prefs):
        gp = torch.zeros_like(pm).index_add_(0, u, pm[u] * (k * 2 / (B * pm.shape[1])))
        if j == 0:
            gp = gp + pm * (k * 2 / pm.numel())
        gps.append(gp)
    dx = id_rep.shape[1]
    widths = [r.shape[1] for r in reps]
    return G[:, :dx].clone(), list(G[:, dx:].split(widths, dim=1)), gE, gps


# ------------------------------------------------------- the dense ops around the kernels
def normalize_fwd(x):
    den = x.norm(dim=1, keepdim=True).clamp_min(EPS)
    return x / den, den


def normalize_bwd(g, y, den):
    dot = torch.where(den > EPS, (g * y).sum(1, keepdim=True), torch.zeros_like(den))
    return (g - y * dot) / den


def mlp_fwd(X, W, b):
    pre = X @ W.t() + b
    return torch.where(pre > 0, pre, SLOPE * pre)


def mlp_bwd(g, out, X):
    """(dW, db) of leaky(X W^T + b) from its output's sign."""
    gp = torch.where(out > 0, g, SLOPE * g)
    return gp.t() @ X, gp.sum(0)


MODS = ("v", "t")


def step(P: dict, feats: dict, g: Graph, trip, nu: int, reg_weight: float):
    """One forward / backward by the formulas above, the preferences normalised once.
    Returns (dict of forward pieces in slot order, terms [3], grads by name)."""
    mods = [m for m in MODS if m in feats]
    fw = {"x": [], "alpha": [], "rep": [], "mlp": [], "nf": [], "np": []}
    for m in mods:
        out = mlp_fwd(feats[m], P[f"{m}_gcn.MLP.weight"], P[f"{m}_gcn.MLP.bias"])
        f, fden = normalize_fwd(out)
        p, pden = normalize_fwd(P[f"{m}_gcn.preference"])
        x = torch.cat([p, f], dim=0)
        a, rep = attn_fwd(g, x)
        for k, v in (("x", x), ("alpha", a), ("rep", rep), ("mlp", out), ("nf", (f, fden)), ("np", (p, pden))):
            fw[k].append(v)
    conf, E = P["model_specific_conf"], P["id_gcn.id_embedding"]
    val, valT = refine_fwd(g, fw["alpha"], conf)
    xn, eden = normalize_fwd(E)
    h1, id_rep = id_gcn_fwd(g, val, xn)
    prefs = [P[f"{m}_gcn.preference"] for m in mods]
    terms, rep = loss_fwd(id_rep, fw["rep"], E, prefs, trip, nu, reg_weight)
    fw.update(weight=val, id_rep=id_rep, representation=rep)
    # backward
    G, g_reps, gE, gprefs = loss_bwd(id_rep, fw["rep"], E, prefs, trip, nu, reg_weight)
    dxn, dw = id_gcn_bwd(g, val, valT, G, h1, xn)
    das, dconf = refine_bwd(g, fw["alpha"], conf, dw)
    grads = {"model_specific_conf": dconf, "id_gcn.id_embedding": gE + normalize_bwd(dxn, xn, eden)}
    for j, m in enumerate(mods):
        dx = attn_bwd(g, g_reps[j], das[j], fw["x"][j], fw["alpha"][j])
        (f, fden), (p, pden) = fw["nf"][j], fw["np"][j]
        grads[f"{m}_gcn.preference"] = gprefs[j] + normalize_bwd(dx[:nu], p, pden)
        dW, db = mlp_bwd(normalize_bwd(dx[nu:], f, fden), fw["mlp"][j], feats[m])
        grads[f"{m}_gcn.MLP.weight"], grads[f"{m}_gcn.MLP.bias"] = dW, db
    return fw, terms, grads
