"""float64 numpy restatement of FREEDOM (reference src/models/freedom.py): the three-term
loss and its gradients on given tables (the contract of rsx_freedom_loss_fwd / _bwd,
include/rsx.h), the whole model on dense graphs at the fixture's scale (forward :166-180,
loss :182-212, all 8 parameter gradients, repeated rows summed), the item graph's values
(:86-100, :74), and the fixture plumbing the FREEDOM tests share.
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("user_embedding.weight", "item_id_embedding.weight", "image_embedding.weight", "image_trs.weight",
         "image_trs.bias", "text_embedding.weight", "text_trs.weight", "text_trs.bias")
BIASES = ("image_trs.bias", "text_trs.bias")
HPARAMS = dict(seed=999, dropout=0.8, reg_weight=0.001)
N_UI_LAYERS, N_MM_LAYERS, KNN_K, IMAGE_WEIGHT = 2, 1, 10, 0.1


def _f(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _sig(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))  # no overflow at |x| = 40 and beyond


# ---------------------------------------------------------------------------
# the loss on given tables
# ---------------------------------------------------------------------------
def loss_grad(E, H, T, V, trip, n_users, reg, go=1.0):
    """(out [4] = total, id, text, image; gE, gT, gV) for triplets trip [3, B]: gE / gT / gV
    whole tables, zero off the batch rows, repeated rows summed.  H, T or V may be None."""
    E, H, T, V = _f(E), _f(H), _f(T), _f(V)
    nu = int(n_users)
    u, p, n = (np.asarray(t, dtype=np.int64) for t in trip)
    B = len(u)
    eu = E[u]
    items = E[nu:] if H is None else E[nu:] + H
    out = np.zeros(4)
    gE = np.zeros_like(E)
    grads = [None, None]
    gu = np.zeros_like(eu)
    for k, tab in enumerate((items, T, V)):
        if tab is None:
            continue
        tp, tn = tab[p], tab[n]
        x = (eu * tp).sum(1) - (eu * tn).sum(1)
        out[1 + k] = np.mean(np.logaddexp(0.0, -x))
        w = 1.0 if k == 0 else reg
        dx = (-go * w * _sig(-x) / B)[:, None]
        gu += dx * (tp - tn)
        g = np.zeros_like(tab)
        np.add.at(g, p, dx * eu)
        np.add.at(g, n, -dx * eu)
        if k == 0:
            gE[nu:] += g
        else:
            grads[k - 1] = g
    np.add.at(gE, u, gu)
    out[0] = out[1] + reg * (out[2] + out[3])
    return out, gE, grads[0], grads[1]


# ---------------------------------------------------------------------------
# the whole model on dense graphs
# ---------------------------------------------------------------------------
def dense(idx, val, shape):
    A = np.zeros(shape)
    np.add.at(A, (np.asarray(idx[0], dtype=np.int64), np.asarray(idx[1], dtype=np.int64)),
              np.asarray(val, dtype=np.float64))
    return A


def _tables(p, A, M, n_ui_layers, n_mm_layers):
    U, I = p["user_embedding.weight"], p["item_id_embedding.weight"]
    ego = np.concatenate([U, I])
    acc, cur = ego.copy(), ego
    for _ in range(n_ui_layers):
        cur = A @ cur
        acc = acc + cur
    E = acc / (n_ui_layers + 1)
    H = I
    for _ in range(n_mm_layers):
        H = M @ H
    return E, H


def forward(p, A, M, n_ui_layers=N_UI_LAYERS, n_mm_layers=N_MM_LAYERS):
    """(user table, item table) of freedom.py:166-180 on the dense UI graph A and item graph M."""
    p = {k: _f(v) for k, v in p.items()}
    nu = p["user_embedding.weight"].shape[0]
    E, H = _tables(p, A, M, n_ui_layers, n_mm_layers)
    return E[:nu], E[nu:] + H


def model_loss_grad(p, A, M, trip, reg, n_ui_layers=N_UI_LAYERS, n_mm_layers=N_MM_LAYERS):
    """(loss, its four words, dict name -> gradient) of freedom.py:191-212; a modality whose
    `<name>_embedding.weight` is absent from p is absent from the model."""
    p = {k: _f(v) for k, v in p.items()}
    nu = p["user_embedding.weight"].shape[0]
    E, H = _tables(p, A, M, n_ui_layers, n_mm_layers)
    proj = {}
    for m in ("text", "image"):
        if m + "_embedding.weight" in p:
            proj[m] = p[m + "_embedding.weight"] @ p[m + "_trs.weight"].T + p[m + "_trs.bias"]
    out, gE, gT, gV = loss_grad(E, H, proj.get("text"), proj.get("image"), trip, nu, reg)
    g = {}
    acc, cur = gE.copy(), gE
    for _ in range(n_ui_layers):
        cur = A.T @ cur
        acc = acc + cur
    g_ego = acc / (n_ui_layers + 1)
    gh = gE[nu:]
    for _ in range(n_mm_layers):
        gh = M.T @ gh
    g["user_embedding.weight"] = g_ego[:nu]
    g["item_id_embedding.weight"] = g_ego[nu:] + gh
    for m, gt in (("text", gT), ("image", gV)):
        if m in proj:
            g[m + "_trs.weight"] = gt.T @ p[m + "_embedding.weight"]
            g[m + "_trs.bias"] = gt.sum(0)
            g[m + "_embedding.weight"] = gt @ p[m + "_trs.weight"]
    return out[0], out, g


# ---------------------------------------------------------------------------
# the item graph
# ---------------------------------------------------------------------------
def topk_ids(feat, k):
    """Top-k cosine neighbours per row (float64 similarities; ties by lower index)."""
    x = _f(feat)
    xn = x / np.linalg.norm(x, axis=1, keepdims=True)
    return np.argsort(-(xn @ xn.T), axis=1, kind="stable")[:, :k]


def item_graph(idx_v, idx_t, n, w):
    """dict (row, col) -> value of w * A_image + (1 - w) * A_text from the two [n, k]
    neighbour id arrays (either may be None), the arithmetic in float32 as freedom.py:93-100
    and :74 do it: r_inv = (1e-7 + row count)^-0.5, value r_inv[row] * r_inv[col]."""
    f32 = np.float32
    mats = []
    for idx in (idx_v, idx_t):
        if idx is None:
            mats.append(None)
            continue
        k = idx.shape[1]
        rows = np.repeat(np.arange(n), k)
        cols = np.asarray(idx, dtype=np.int64).reshape(-1)
        r_inv = np.power(f32(1e-7) + np.bincount(rows, minlength=n).astype(f32), f32(-0.5)).astype(f32)
        mats.append(dict(zip(zip(rows.tolist(), cols.tolist()), (r_inv[rows] * r_inv[cols]).astype(f32))))
    if mats[0] is None or mats[1] is None:
        return mats[0] if mats[1] is None else mats[1]
    out = {}
    for m, s in ((mats[0], f32(w)), (mats[1], f32(1.0 - w))):
        for rc, v in m.items():
            out[rc] = f32(out.get(rc, f32(0.0)) + s * v)
    return out


# ---------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------
_CACHE = {}


def load_fixture():
    """freedom_step0_small.npz + freedom_small.npz as one dict, with what the capture left out
    put back: v_feat / t_feat (smore_small.npz's), init.{image,text}_embedding.weight (= them),
    the XOR-stored parameters decoded and the kept edge masks unpacked (`e{k}_keep_ids`:
    ascending edge ids)."""
    if "z" not in _CACHE:
        z = dict(np.load(os.path.join(GOLD, "freedom_step0_small.npz")))
        z.update(np.load(os.path.join(GOLD, "freedom_small.npz")))
        s = np.load(os.path.join(GOLD, "smore_small.npz"))
        z["v_feat"], z["t_feat"] = s["v_feat"], s["t_feat"]
        z["init.image_embedding.weight"], z["init.text_embedding.weight"] = z["v_feat"], z["t_feat"]
        for k in [k for k in z if "_param_xor." in k]:
            pre, name = k.split("_param_xor.")
            z[f"{pre}_param.{name}"] = (z[k] ^ z["init." + name].view(np.int32)).view(np.float32)
        n_edges = z["edge_idx"].shape[1]
        for e in (0, 1):
            z[f"e{e}_keep_ids"] = np.flatnonzero(np.unpackbits(z[f"e{e}_keep"])[:n_edges]).astype(np.int64)
        _CACHE["z"] = z
    return _CACHE["z"]


def init_params(z):
    return {n: z["init." + n] for n in NAMES}


def masked_coo(z, epoch):
    """(rows, cols, vals) of the epoch's masked_adj in coalesced order: the kept edges both
    ways, sorted by (row, col), with the fixture's values."""
    nu = int(z["n_users"])
    e = z["edge_idx"].astype(np.int64)[:, z[f"e{epoch}_keep_ids"]]
    rows = np.concatenate([e[0], e[1] + nu])
    cols = np.concatenate([e[1] + nu, e[0]])
    order = np.lexsort((cols, rows))
    return rows[order], cols[order], z[f"e{epoch}_masked_val"]


def dense_graphs(z, epoch=0):
    """(norm_adj, masked_adj of `epoch`, mm_adj) dense float64."""
    key = ("graphs", epoch)
    if key not in _CACHE:
        nu, ni = int(z["n_users"]), int(z["n_items"])
        n = nu + ni
        r, c, v = masked_coo(z, epoch)
        _CACHE[key] = (dense(z["norm_adj_idx"], z["norm_adj_val"], (n, n)), dense((r, c), v, (n, n)),
                       dense(z["mm_adj_idx"], z["mm_adj_val"], (ni, ni)))
    return _CACHE[key]


def step0(z):
    """(loss, words, grads) of the restatement on the fixture's first batch (computed once)."""
    if "step0" not in _CACHE:
        _, masked, mm = dense_graphs(z, 0)
        _CACHE["step0"] = model_loss_grad(init_params(z), masked, mm, z["step0_triplets"].astype(np.int64),
                                          HPARAMS["reg_weight"])
    return _CACHE["step0"]
