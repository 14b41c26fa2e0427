"""float64 numpy restatement of MGCN's two per-row blocks (reference src/models/mgcn.py:
the behaviour-guided purifier :152-154, the behaviour-aware fuser :187-201), forward and
every gradient, of the whole training loss (:146-253) on dense graphs at the fixture's
scale, and the fixture plumbing the MGCN tests share.

`purify` / `fuse` are the kernels' contracts (rsx_mgcn_purify / rsx_mgcn_fuse,
include/rsx.h); `model_loss_grad` chains them to the 19 parameters: projections, the
mean-of-layers UI propagation, the item views, BPR + InfoNCE and their backward.
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("user_embedding.weight", "item_id_embedding.weight", "image_embedding.weight", "text_embedding.weight",
         "image_trs.weight", "image_trs.bias", "text_trs.weight", "text_trs.bias",
         "query_common.0.weight", "query_common.0.bias", "query_common.2.weight",
         "gate_v.0.weight", "gate_v.0.bias", "gate_t.0.weight", "gate_t.0.bias",
         "gate_image_prefer.0.weight", "gate_image_prefer.0.bias",
         "gate_text_prefer.0.weight", "gate_text_prefer.0.bias")
QUERY = ("query_common.0.weight", "query_common.0.bias", "query_common.2.weight")
TAU = 0.2  # mgcn.py:250


def _f(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


# ---------------------------------------------------------------------------
# purifier
# ---------------------------------------------------------------------------
def purify(item, feat, W, b, gout=None):
    """out[m] = item * sigmoid(feat[m] W[m]^T + b[m]), m = 0, 1.  With gout (two arrays or
    None each): also g_item, g_feat[m], dz[m], dW[m], db[m]."""
    item = _f(item)
    feat, W, b = [_f(x) for x in feat], [_f(x) for x in W], [_f(x) for x in b]
    s = [_sig(feat[m] @ W[m].T + b[m]) for m in range(2)]
    r = {"out": [item * s[m] for m in range(2)]}
    if gout is None:
        return r
    go = [np.zeros_like(item) if g is None else _f(g) for g in gout]
    r["g_item"] = go[0] * s[0] + go[1] * s[1]
    r["dz"] = [go[m] * item * s[m] * (1 - s[m]) for m in range(2)]
    r["g_feat"] = [r["dz"][m] @ W[m] for m in range(2)]
    r["dW"] = [r["dz"][m].T @ feat[m] for m in range(2)]
    r["db"] = [r["dz"][m].sum(0) for m in range(2)]
    return r


# ---------------------------------------------------------------------------
# fuser
# ---------------------------------------------------------------------------
def fuse(C, I, T, W1, b1, w2, Wip, bip, Wtp, btp, rows=None, g_all=None, g_side=None, g_cin=None):
    """The fuser on table rows `rows` (None: every row).  Returns all / side / content rows
    and, given g_all (with optional g_side, g_cin), the table gradients gC / gI / gT
    (summed over repeated rows), the weight gradients and the dz rows."""
    Ct, It, Tt = _f(C), _f(I), _f(T)
    W1, b1, w2, Wip, bip, Wtp, btp = (_f(x) for x in (W1, b1, w2, Wip, bip, Wtp, btp))
    w2 = w2.reshape(-1)
    idx = np.arange(Ct.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    C, I, T = Ct[idx], It[idx], Tt[idx]
    hI, hT = np.tanh(I @ W1.T + b1), np.tanh(T @ W1.T + b1)
    aI, aT = hI @ w2, hT @ w2
    wI = _sig(aI - aT)[:, None]  # the two-way softmax
    wT = 1.0 - wI
    cm = wI * I + wT * T
    pI, pT = _sig(C @ Wip.T + bip), _sig(C @ Wtp.T + btp)
    side = (pI * (I - cm) + pT * (T - cm) + cm) / 3.0
    r = {"all": C + side, "side": side, "content": C, "wI": wI[:, 0]}
    if g_all is None:
        return r
    gA = _f(g_all)
    gs = (gA + (0 if g_side is None else _f(g_side))) / 3.0
    gc = gs * (1 - pI - pT)
    daI = (wI * wT)[:, 0] * (gc * (I - T)).sum(1)
    dzI = gs * (I - cm) * pI * (1 - pI)
    dzT = gs * (T - cm) * pT * (1 - pT)
    dz1I = daI[:, None] * w2 * (1 - hI * hI)
    dz1T = -daI[:, None] * w2 * (1 - hT * hT)
    gI = gs * pI + wI * gc + dz1I @ W1
    gT = gs * pT + wT * gc + dz1T @ W1
    gC = gA + (0 if g_cin is None else _f(g_cin)) + dzI @ Wip + dzT @ Wtp
    tabs = []
    for g, t in ((gC, Ct), (gI, It), (gT, Tt)):
        z = np.zeros_like(t)
        np.add.at(z, idx, g)
        tabs.append(z)
    r.update(gC=tabs[0], gI=tabs[1], gT=tabs[2], dz=[dz1I, dz1T, dzI, dzT],
             dW1=dz1I.T @ I + dz1T.T @ T, db1=dz1I.sum(0) + dz1T.sum(0),
             dw2=(daI[:, None] * (hI - hT)).sum(0).reshape(1, -1),
             dWip=dzI.T @ C, dbip=dzI.sum(0), dWtp=dzT.T @ C, dbtp=dzT.sum(0))
    return r


# ---------------------------------------------------------------------------
# the whole model on dense graphs
# ---------------------------------------------------------------------------
def dense(idx, val, shape):
    A = np.zeros(shape)
    np.add.at(A, (idx[0].astype(np.int64), idx[1].astype(np.int64)), val.astype(np.float64))
    return A


def _nce(v1, v2, tau):
    """(mean -log(exp(<a_b, c_b> / tau) / sum_j exp(<a_b, c_j> / tau)), d v1, d v2) of the
    L2-normalised rows (F.normalize: norms clamped at 1e-12)."""
    n1 = np.maximum(np.linalg.norm(v1, axis=1, keepdims=True), 1e-12)
    n2 = np.maximum(np.linalg.norm(v2, axis=1, keepdims=True), 1e-12)
    a, c = v1 / n1, v2 / n2
    S = a @ c.T / tau
    m = S.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(S - m).sum(1))
    B = v1.shape[0]
    loss = (lse - np.diag(S)).mean()
    P = np.exp(S - lse[:, None])
    dS = (P - np.eye(B)) / B / tau
    da, dc = dS @ c, dS.T @ a
    d1 = (da - a * (da * a).sum(1, keepdims=True)) / n1
    d2 = (dc - c * (dc * c).sum(1, keepdims=True)) / n2
    return loss, d1, d2


def forward(p, graphs, n_ui_layers, n_layers):
    """(all, side, content, cache) tables of the eval-mode forward; graphs: dict of dense
    norm_adj [N, N], R [nu, ni], image / text [ni, ni]."""
    p = {k: _f(v) for k, v in p.items()}
    U, H = p["user_embedding.weight"], p["item_id_embedding.weight"]
    Fi = p["image_embedding.weight"] @ p["image_trs.weight"].T + p["image_trs.bias"]
    Ft = p["text_embedding.weight"] @ p["text_trs.weight"].T + p["text_trs.bias"]
    pur = purify(H, [Fi, Ft], [p["gate_v.0.weight"], p["gate_t.0.weight"]], [p["gate_v.0.bias"], p["gate_t.0.bias"]])
    A = graphs["norm_adj"]
    ego = np.concatenate([U, H])
    acc, cur = ego.copy(), ego
    for _ in range(n_ui_layers):
        cur = A @ cur
        acc = acc + cur
    content = acc / (n_ui_layers + 1)
    views = []
    for x, G in ((pur["out"][0], graphs["image"]), (pur["out"][1], graphs["text"])):
        for _ in range(n_layers):
            x = G @ x
        views.append(np.concatenate([graphs["R"] @ x, x]))
    f = fuse(content, views[0], views[1], p["query_common.0.weight"], p["query_common.0.bias"],
             p["query_common.2.weight"], p["gate_image_prefer.0.weight"], p["gate_image_prefer.0.bias"],
             p["gate_text_prefer.0.weight"], p["gate_text_prefer.0.bias"])
    return f["all"], f["side"], content, dict(p=p, Fi=Fi, Ft=Ft, views=views)


def model_loss_grad(p, graphs, n_ui_layers, n_layers, trip, reg_weight, batch_size, cl_loss):
    """(loss, dict name -> gradient) of mgcn.py:233-253 for the triplets trip [3, B]."""
    all_, side, content, c = forward(p, graphs, n_ui_layers, n_layers)
    p = c["p"]
    nu = p["user_embedding.weight"].shape[0]
    u, pos, neg = (np.asarray(t, dtype=np.int64) for t in trip)
    B = len(u)
    eu, ep, en = all_[u], all_[nu + pos], all_[nu + neg]
    x = (eu * ep).sum(1) - (eu * en).sum(1)
    mf = np.mean(np.logaddexp(0, -x))
    reg = 0.5 * ((eu ** 2).sum() + (ep ** 2).sum() + (en ** 2).sum()) / batch_size
    li, dsi, dci = _nce(side[nu + pos], content[nu + pos], TAU)
    lu, dsu, dcu = _nce(side[u], content[u], TAU)
    loss = mf + reg_weight * reg + cl_loss * (li + lu)
    # backward
    g_all, g_side, g_cont = np.zeros_like(all_), np.zeros_like(all_), np.zeros_like(all_)
    dx = -_sig(-x)[:, None] / B
    k = reg_weight / batch_size
    np.add.at(g_all, u, dx * (ep - en) + k * eu)
    np.add.at(g_all, nu + pos, dx * eu + k * ep)
    np.add.at(g_all, nu + neg, -dx * eu + k * en)
    np.add.at(g_side, nu + pos, cl_loss * dsi)
    np.add.at(g_side, u, cl_loss * dsu)
    np.add.at(g_cont, nu + pos, cl_loss * dci)
    np.add.at(g_cont, u, cl_loss * dcu)
    f = fuse(content, c["views"][0], c["views"][1], p["query_common.0.weight"], p["query_common.0.bias"],
             p["query_common.2.weight"], p["gate_image_prefer.0.weight"], p["gate_image_prefer.0.bias"],
             p["gate_text_prefer.0.weight"], p["gate_text_prefer.0.bias"], g_all=g_all, g_side=g_side, g_cin=g_cont)
    g = {"query_common.0.weight": f["dW1"], "query_common.0.bias": f["db1"], "query_common.2.weight": f["dw2"],
         "gate_image_prefer.0.weight": f["dWip"], "gate_image_prefer.0.bias": f["dbip"],
         "gate_text_prefer.0.weight": f["dWtp"], "gate_text_prefer.0.bias": f["dbtp"]}
    # content = mean_k A^k ego (A symmetric)
    A = graphs["norm_adj"]
    acc, cur = f["gC"].copy(), f["gC"]
    for _ in range(n_ui_layers):
        cur = A.T @ cur
        acc = acc + cur
    g_ego = acc / (n_ui_layers + 1)
    gout = []
    for gv, G in ((f["gI"], graphs["image"]), (f["gT"], graphs["text"])):
        gx = gv[nu:] + graphs["R"].T @ gv[:nu]
        for _ in range(n_layers):
            gx = G.T @ gx
        gout.append(gx)
    H = p["item_id_embedding.weight"]
    pur = purify(H, [c["Fi"], c["Ft"]], [p["gate_v.0.weight"], p["gate_t.0.weight"]],
                 [p["gate_v.0.bias"], p["gate_t.0.bias"]], gout=gout)
    g["user_embedding.weight"] = g_ego[:nu]
    g["item_id_embedding.weight"] = g_ego[nu:] + pur["g_item"]
    for m, (gate, mod) in enumerate((("gate_v", "image"), ("gate_t", "text"))):
        g[gate + ".0.weight"], g[gate + ".0.bias"] = pur["dW"][m], pur["db"][m]
        gf = pur["g_feat"][m]
        g[mod + "_trs.weight"] = gf.T @ p[mod + "_embedding.weight"]
        g[mod + "_trs.bias"] = gf.sum(0)
        g[mod + "_embedding.weight"] = gf @ p[mod + "_trs.weight"]
    return loss, g


# ---------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------
_CACHE = {}


def load_fixture():
    """mgcn_step0_small.npz + mgcn_small.npz as one dict, with what the capture left out put
    back: v_feat / t_feat (smore_small.npz's), init.{image,text}_embedding.weight (= them),
    and the XOR-stored parameters decoded."""
    if "z" not in _CACHE:
        z = dict(np.load(os.path.join(GOLD, "mgcn_step0_small.npz")))
        z.update(np.load(os.path.join(GOLD, "mgcn_small.npz")))
        s = np.load(os.path.join(GOLD, "smore_small.npz"))
        z["v_feat"], z["t_feat"] = s["v_feat"], s["t_feat"]
        z["init.image_embedding.weight"], z["init.text_embedding.weight"] = z["v_feat"], z["t_feat"]
        for k in [k for k in z if "_param_xor." in k]:
            pre, name = k.split("_param_xor.")
            z[f"{pre}_param.{name}"] = (z[k] ^ z["init." + name].view(np.int32)).view(np.float32)
        _CACHE["z"] = z
    return _CACHE["z"]


def init_params(z):
    return {n: z["init." + n] for n in NAMES}


def dense_graphs(z):
    nu, ni = int(z["n_users"]), int(z["n_items"])
    return {"norm_adj": dense(z["norm_adj_idx"], z["norm_adj_val"], (nu + ni, nu + ni)),
            "R": dense(z["R_idx"], z["R_val"], (nu, ni)),
            "image": dense(z["image_original_adj_idx"], z["image_original_adj_val"], (ni, ni)),
            "text": dense(z["text_original_adj_idx"], z["text_original_adj_val"], (ni, ni))}


def step0(z):
    """(loss, grads) of the restatement on the fixture's first batch (computed once)."""
    if "step0" not in _CACHE:
        _CACHE["step0"] = model_loss_grad(init_params(z), dense_graphs(z), 2, 1, z["step0_triplets"].astype(np.int64),
                                          1e-4, 512, 0.01)
    return _CACHE["step0"]
