"""float64 numpy restatement of BM3's bootstrap loss and all its gradients (reference
src/models/bm3.py:86-149, src/common/loss.py:38-51), explicit dropout keep masks included,
and the fixture plumbing the BM3 tests share.

`loss_grad` is the kernel's contract (rsx_bm3_loss_fwd / _bwd, include/rsx.h): the loss on
given tables E, H, T, V.  `model_loss_grad` chains it to the parameters: the mean-of-layers
propagation, the two feature projections and their backward.
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 1e-8  # torch.nn.functional.cosine_similarity's eps
NAMES = ("user_embedding.weight", "item_id_embedding.weight", "predictor.weight", "predictor.bias",
         "image_embedding.weight", "image_trs.weight", "image_trs.bias",
         "text_embedding.weight", "text_trs.weight", "text_trs.bias")
STREAMS = ("user", "item", "text", "image")


def pack_keep(keep):
    """bool [n, d] -> uint32 [n, d / 32]: bit (c & 31) of word c // 32 = column c kept."""
    n, d = keep.shape
    bits = keep.reshape(n, d // 32, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)
    return bits.sum(-1).astype(np.uint32)


def unpack_keep(words, d):
    n = words.shape[0]
    bits = (words.astype(np.uint64)[:, :, None] >> np.arange(32, dtype=np.uint64)) & 1
    return bits.reshape(n, d).astype(bool)


def _cos(q, t):
    """(cos [B], dcos/dq [B, d]) of torch's cosine_similarity: each norm clamped at EPS, the
    clamp outside autograd (the gradient of |q| still flows)."""
    qn = np.linalg.norm(q, axis=1, keepdims=True)
    n = np.maximum(qn, EPS)
    th = t / np.maximum(np.linalg.norm(t, axis=1, keepdims=True), EPS)
    c = (q * th).sum(1, keepdims=True) / n
    unit = np.divide(q, qn, out=np.zeros_like(q), where=qn > 0)
    return c[:, 0], th / n - c / n * unit


def loss_grad(E, H, T, V, P, pb, users, items, n_users, reg_weight, cl_weight, p_drop, keep=None, go=1.0):
    """keep: dict stream name -> bool [table rows, d] (missing / None: everything kept).
    Returns dict(out [8] = total, ui, iu, t, v, tv, vt, reg; gE, gT, gV, gP, gpb)."""
    f = lambda a: None if a is None else np.asarray(a, dtype=np.float64)  # noqa: E731
    E, H, T, V, P, pb = (f(a) for a in (E, H, T, V, P, pb))
    keep = keep or {}
    nu, B = int(n_users), len(users)
    ni = E.shape[0] - nu
    XI = E[nu:] + H
    tabs = {"user": E[:nu], "item": XI, "text": T, "image": V}
    idx = {"user": users, "item": items, "text": items, "image": items}
    x, q, tg = {}, {}, {}
    for s in STREAMS:
        if tabs[s] is None:
            continue
        x[s] = tabs[s][idx[s]]
        q[s] = x[s] @ P.T + pb
        k = keep.get(s)
        tg[s] = x[s] * (1.0 if k is None else k[idx[s]]) / (1.0 - p_drop)
    pairs = (("user", "item", 1.0), ("item", "user", 1.0), ("text", "item", cl_weight), ("image", "item", cl_weight),
             ("text", "text", cl_weight), ("image", "image", cl_weight))
    terms = np.zeros(7)
    gq = {s: np.zeros_like(q[s]) for s in q}
    for k, (o, t, w) in enumerate(pairs):
        if o not in q:
            continue
        c, dc = _cos(q[o], tg[t])
        terms[k] = 1.0 - c.mean()
        gq[o] += -go * w / B * dc
    nU, nI = np.sqrt((E[:nu] ** 2).sum()), np.sqrt((XI ** 2).sum())
    terms[6] = (nU + nI) / ni
    total = terms[0] + terms[1] + reg_weight * terms[6] + cl_weight * terms[2:6].sum()
    gE = np.zeros_like(E)
    gE[:nu] = go * reg_weight / ni * (E[:nu] / nU if nU > 0 else 0.0)
    gE[nu:] = go * reg_weight / ni * (XI / nI if nI > 0 else 0.0)
    res = dict(out=np.concatenate([[total], terms]), gE_reg=gE.copy(), gT=None, gV=None)
    gP, gpb = np.zeros_like(P), np.zeros_like(pb)
    for s in q:
        gP += gq[s].T @ x[s]
        gpb += gq[s].sum(0)
        gx = gq[s] @ P
        if s == "user":
            np.add.at(gE, users, gx)
        elif s == "item":
            np.add.at(gE, nu + np.asarray(items), gx)
        else:
            g = np.zeros_like(tabs[s])
            np.add.at(g, items, gx)
            res["gT" if s == "text" else "gV"] = g
    res.update(gE=gE, gP=gP, gpb=gpb, x=x, q=q, tg=tg, gq=gq)
    return res


def dense_adj(idx, val, n):
    A = np.zeros((n, n))
    A[idx[0], idx[1]] = val
    return A


def model_loss_grad(params, adj, n_layers, users, items, reg_weight, cl_weight, p_drop, keep=None):
    """params: dict NAMES -> array (feature entries may be missing); adj dense [n, n] symmetric.
    Returns (out [8], dict name -> gradient)."""
    p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    U, I = p[NAMES[0]], p[NAMES[1]]
    nu = U.shape[0]
    ego = np.concatenate([U, I])
    layers, h = [ego], ego
    for _ in range(n_layers):
        h = adj @ h
        layers.append(h)
    E = sum(layers) / (n_layers + 1)
    proj = {}
    for s, pre in (("text", "text"), ("image", "image")):
        if pre + "_trs.weight" in p:
            proj[s] = p[pre + "_embedding.weight"] @ p[pre + "_trs.weight"].T + p[pre + "_trs.bias"]
    r = loss_grad(E, I, proj.get("text"), proj.get("image"), p["predictor.weight"], p["predictor.bias"], users, items,
                  nu, reg_weight, cl_weight, p_drop, keep)
    g, acc = r["gE"], r["gE"]
    for _ in range(n_layers):  # the backward of the mean of powers of a symmetric operator
        g = adj @ g
        acc = acc + g
    gego = acc / (n_layers + 1)
    grads = {NAMES[0]: gego[:nu], NAMES[1]: gego[nu:] + r["gE"][nu:], "predictor.weight": r["gP"],
             "predictor.bias": r["gpb"]}
    for s, pre, key in (("text", "text", "gT"), ("image", "image", "gV")):
        if s in proj:
            grads[pre + "_embedding.weight"] = r[key] @ p[pre + "_trs.weight"]
            grads[pre + "_trs.weight"] = r[key].T @ p[pre + "_embedding.weight"]
            grads[pre + "_trs.bias"] = r[key].sum(0)
    return r["out"], grads


# ------------------------------------------------------------------ fixtures
_CACHE = {}


def load_fixture(which):
    """'step0' (bm3_step0_small.npz) or 'small' (bm3_small.npz, the XOR-stored final
    parameters restored under `epoch1_param.*`), loaded once."""
    if which not in _CACHE:
        z = dict(np.load(os.path.join(GOLD, {"step0": "bm3_step0_small.npz", "small": "bm3_small.npz"}[which])))
        z["init.image_embedding.weight"], z["init.text_embedding.weight"] = z["v_feat"], z["t_feat"]
        for k in [k for k in z if "_param_xor." in k]:
            ep, name = k.split("_param_xor.")
            z[f"{ep}_param.{name}"] = (z[k] ^ z["init." + name].view(np.int32)).view(np.float32)
        _CACHE[which] = z
    return _CACHE[which]


def init_params(z):
    return {n: z["init." + n] for n in NAMES}


def epoch_pairs(z, epoch, batch=512):
    p = z[f"epoch{epoch}_pairs"].astype(np.int64)
    return [p[:, s: s + batch] for s in range(0, p.shape[1], batch)]
