"""float64 numpy restatement of SELFCFED_LGN, written from its mathematics (reference
src/models/selfcfed_lgn.py:41-78, src/common/encoders.py:80-134, src/common/loss.py:54-62), the
explicit draws included, and the fixture plumbing the SELFCFED_LGN tests share.

`loss_grad` is the kernels' contract (rsx_selfcf_loss_fwd / _bwd, include/rsx.h): the loss on a
given propagated table E.  `model_loss_grad` chains it to the parameters through the mean of
powers of a NON-symmetric operator (the dropped graph): the backward runs on its transpose.
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 1e-8  # torch.nn.functional.cosine_similarity's eps
U_EMB, I_EMB = "online_encoder.embedding_dict.user_emb", "online_encoder.embedding_dict.item_emb"
NAMES = (I_EMB, U_EMB, "predictor.weight", "predictor.bias")  # the reference's named_parameters() order


def pack_bits(keep):
    """bool [n] -> uint32 [ceil(n / 32)]: bit (e & 31) of word e // 32 = entry e kept."""
    keep = np.asarray(keep, dtype=bool).ravel()
    pad = np.zeros((keep.size + 31) // 32 * 32, dtype=np.uint64)
    pad[: keep.size] = keep
    return (pad.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def unpack_bits(words, n):
    bits = (np.asarray(words).astype(np.uint64)[:, None] >> np.arange(32, dtype=np.uint64)) & 1
    return bits.reshape(-1)[:n].astype(bool)


def pack_keep(keep):
    """bool [..., d] -> uint32 [..., d / 32]: bit (c & 31) of word c // 32 = column c kept."""
    *lead, d = keep.shape
    bits = keep.reshape(*lead, d // 32, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)
    return bits.sum(-1).astype(np.uint32)


def unpack_keep(words, d):
    bits = (np.asarray(words).astype(np.uint64)[..., None] >> np.arange(32, dtype=np.uint64)) & 1
    return bits.reshape(*words.shape[:-1], d).astype(bool)


def _cos(q, t):
    """(cos [B], dcos/dq [B, d]) of torch's cosine_similarity: each norm clamped at EPS, the
    clamp outside autograd (the gradient of |q| still flows)."""
    qn = np.linalg.norm(q, axis=1, keepdims=True)
    n = np.maximum(qn, EPS)
    th = t / np.maximum(np.linalg.norm(t, axis=1, keepdims=True), EPS)
    c = (q * th).sum(1, keepdims=True) / n
    unit = np.divide(q, qn, out=np.zeros_like(q), where=qn > 0)
    return c[:, 0], th / n - c / n * unit


def loss_grad(E, P, pb, users, items, n_users, reg_weight, p_drop, keep=None, go=1.0, scale=None):
    """keep: bool [2, B, d] keyed on the batch position (user stream, item stream), None: all kept.
    scale: the kept values' factor (None: 1 / (1 - p_drop)).
    Returns dict(out [4] = total, ui, iu, reg; gE, gP, gpb, x, q, tg)."""
    E, P, pb = (np.asarray(a, dtype=np.float64) for a in (E, P, pb))
    users, items = np.asarray(users), np.asarray(items)
    nu, B = int(n_users), len(users)
    scale = 1.0 / (1.0 - p_drop) if scale is None else float(scale)
    xu, xi = E[users], E[nu + items]
    qu, qi = xu @ P.T + pb, xi @ P.T + pb
    tu = xu * (scale if keep is None else keep[0] * scale)
    ti = xi * (scale if keep is None else keep[1] * scale)
    cui, dui = _cos(qu, ti)
    ciu, diu = _cos(qi, tu)
    ui, iu = -cui.mean() / 2, -ciu.mean() / 2
    reg = 0.5 * ((xu ** 2).sum() + (xi ** 2).sum())
    gqu, gqi = -go / (2 * B) * dui, -go / (2 * B) * diu
    gP = gqu.T @ xu + gqi.T @ xi
    gpb = gqu.sum(0) + gqi.sum(0)
    gE = np.zeros_like(E)
    np.add.at(gE, users, gqu @ P + go * reg_weight * xu)
    np.add.at(gE, nu + items, gqi @ P + go * reg_weight * xi)
    return dict(out=np.array([ui + iu + reg_weight * reg, ui, iu, reg]), gE=gE, gP=gP, gpb=gpb,
                x=np.concatenate([xu, xi]), q=np.concatenate([qu, qi]), tg=np.concatenate([tu, ti]))


def dense_adj(idx, val, n):
    A = np.zeros((n, n))
    A[idx[0], idx[1]] = val
    return A


def dropped(val0, edge_keep, scale):
    """The step's values: f32 val0 * f32 scale on the kept entries (the reference's product is an
    f32 one), 0 elsewhere."""
    v = np.asarray(val0, dtype=np.float32) * np.float32(scale)
    return np.where(edge_keep, v, np.float32(0)).astype(np.float32)


def propagate(A, ego, n_layers):
    layers, h = [ego], ego
    for _ in range(n_layers):
        h = A @ h
        layers.append(h)
    return sum(layers) / (n_layers + 1)


def model_loss_grad(params, A, n_layers, users, items, reg_weight, p_drop, keep=None, scale=None):
    """params: dict NAMES -> array; A dense [n, n] float64, the step's (dropped) operator.
    Returns (out [4], dict name -> gradient)."""
    p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    U, I = p[U_EMB], p[I_EMB]
    nu = U.shape[0]
    E = propagate(A, np.concatenate([U, I]), n_layers)
    r = loss_grad(E, p["predictor.weight"], p["predictor.bias"], users, items, nu, reg_weight, p_drop, keep,
                  scale=scale)
    gego = propagate(A.T, r["gE"], n_layers)
    return r["out"], {U_EMB: gego[:nu], I_EMB: gego[nu:], "predictor.weight": r["gP"], "predictor.bias": r["gpb"]}


def eval_scores(params, A, n_layers, users):
    """q_u . i + u . q_i over every item, for the given users (selfcfed_lgn.py:71-78)."""
    p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    nu = p[U_EMB].shape[0]
    E = propagate(A, np.concatenate([p[U_EMB], p[I_EMB]]), n_layers)
    q = E @ p["predictor.weight"].T + p["predictor.bias"]
    return q[:nu][users] @ E[nu:].T + E[:nu][users] @ q[nu:].T


def train(params, adj_idx, adj_val, n_layers, steps, reg_weight, p_drop, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam (no weight decay) over `steps`, an iterable of (pairs [2, B], edge keep
    bool [nnz] in adj_idx's order | None, scale), in float64.  Returns (params, losses)."""
    p = {k: np.asarray(v, dtype=np.float64).copy() for k, v in params.items()}
    n = p[U_EMB].shape[0] + p[I_EMB].shape[0]
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v2 = {k: np.zeros_like(v) for k, v in p.items()}
    losses = []
    for t, (pairs, keep, scale) in enumerate(steps, 1):
        val = adj_val if keep is None else dropped(adj_val, keep, scale)
        out, g = model_loss_grad(p, dense_adj(adj_idx, val.astype(np.float64), n), n_layers, pairs[0], pairs[1],
                                 reg_weight, p_drop)
        losses.append(out[0])
        for k in p:
            m[k] = betas[0] * m[k] + (1 - betas[0]) * g[k]
            v2[k] = betas[1] * v2[k] + (1 - betas[1]) * g[k] ** 2
            p[k] -= lr / (1 - betas[0] ** t) * m[k] / (np.sqrt(v2[k]) / np.sqrt(1 - betas[1] ** t) + eps)
    return p, np.array(losses)


# ------------------------------------------------------------------ fixtures
_CACHE = {}
FILES = {"step0": "selfcfed_lgn_step0_small.npz", "small": "selfcfed_lgn_small.npz"}


def load_fixture(which):
    """'step0' or 'small', loaded once."""
    if which not in _CACHE:
        _CACHE[which] = dict(np.load(os.path.join(GOLD, FILES[which])))
    return _CACHE[which]


def init_params(z):
    return {n: z["init." + n] for n in NAMES}


def epoch_pairs(z, epoch, batch=512):
    p = z[f"epoch{epoch}_pairs"].astype(np.int64)
    return [p[:, s: s + batch] for s in range(0, p.shape[1], batch)]


def csr_order(adj_idx, n):
    """The permutation from the fixture's nonzero order to CSR slots (sorted by row, then column)."""
    return np.lexsort((adj_idx[1], adj_idx[0]))
