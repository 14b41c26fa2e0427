"""float64 torch restatement of LGMRec (AAAI'24; reference src/models/lgmrec.py), dense and with
autograd, written from the formulas of include/rsx.h: the table-wide InfoNCE (rsx_lgm_ssl_*), the
hyperedge assignments (rsx_lgm_assign_*), the hypergraph layer (rsx_lgm_hgnn_*), the loss on the
five tables (rsx_lgm_loss_*), the whole forward and loss under explicit draws, Adam, and the
fixture plumbing the LGMRec tests share.  `dtype=torch.float32` gives the float32 torch
composition whose own error the GPU tests scale their bounds by.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("item_image_trs", "v_hyper", "item_text_trs", "t_hyper", "user_embedding.weight",
         "item_id_embedding.weight")  # the trainable parameters, named_parameters' order
HPARAMS = dict(seed=999, hyper_num=4, n_hyper_layer=1, keep_rate=0.5, alpha=0.3, n_ui_layers=2, n_mm_layers=2,
               cl_weight=0.01, reg_weight=1e-3, learning_rate=1e-3, train_batch_size=512, cf_model="lightgcn")
TAU = 0.2


def tt(a, dtype=torch.float64, grad=False):
    t = torch.as_tensor(np.asarray(a), dtype=dtype).clone()
    return t.requires_grad_(True) if grad else t


def unpack_keep(words: np.ndarray, H: int) -> np.ndarray:
    """uint32 [n, ceil(H / 32)] -> bool [n, H]: bit (h & 31) of word h // 32."""
    w = np.asarray(words).astype(np.uint32)
    h = np.arange(H)
    return ((w[:, h // 32] >> (h % 32).astype(np.uint32)) & 1).astype(bool)


def pack_keep(keep: np.ndarray) -> np.ndarray:
    n, H = keep.shape
    out = np.zeros((n, (H + 31) // 32), np.uint32)
    for h in range(H):
        out[:, h // 32] |= keep[:, h].astype(np.uint32) << np.uint32(h % 32)
    return out


# ---------------------------------------------------------------------------
# a. InfoNCE against a whole table
# ---------------------------------------------------------------------------
def ssl_term(T1, T2, idx, tau=TAU):
    n1, m = F.normalize(T1[idx]), F.normalize(T2)
    pos = (n1 * m[idx]).sum(1) / tau
    ttl = torch.exp(n1 @ m.t() / tau).sum(1)
    return (torch.log(ttl) - pos).sum()


def ssl_grad(T1, T2, idx, tau=TAU, dtype=torch.float64):
    """(loss, gT1, gT2); T2 None: one table, (loss, g, None)."""
    a = tt(T1, dtype, True)
    b = a if T2 is None else tt(T2, dtype, True)
    loss = ssl_term(a, b, torch.as_tensor(np.asarray(idx), dtype=torch.int64), tau)
    loss.backward()
    return float(loss), a.grad.numpy(), None if T2 is None else b.grad.numpy()


# ---------------------------------------------------------------------------
# b. assignments
# ---------------------------------------------------------------------------
def assign(x, noise, keep, keep_rate, tau=TAU):
    """(y, out) for logits x [n, H], Gumbel noise [n, H], keep bool [n, H] or None."""
    y = torch.softmax((x + noise) / tau, dim=1)
    return y, y if keep is None else y * keep.to(y.dtype) / keep_rate


def assign_grad(x, noise, keep, keep_rate, dy, tau=TAU, dtype=torch.float64):
    xx = tt(x, dtype, True)
    k = None if keep is None else torch.as_tensor(np.asarray(keep))
    y, out = assign(xx, tt(noise, dtype), k, keep_rate, tau)
    (out * tt(dy, dtype)).sum().backward()
    return y.detach().numpy(), out.detach().numpy(), xx.grad.numpy()


def gumbel_of_bits(bits):
    """The hashed draw's map from 32 bits to Gumbel noise, in float32 as the kernel forms it:
    u = (k + 1/2) 2^-23 with k the top 23 bits (k + 1/2 is exact in float32), g = -log(-log u)."""
    k = (np.asarray(bits, dtype=np.uint64) >> np.uint64(9)).astype(np.float32)
    u = (k + np.float32(0.5)) * np.float32(2.0 ** -23)
    return u, -np.log(-np.log(u.astype(np.float64)))


# ---------------------------------------------------------------------------
# c. hypergraph layer
# ---------------------------------------------------------------------------
def hgnn(Pi, Pu, X, n_layers):
    """[u_ret; i_ret] of lgmrec.py:202-214."""
    i_ret = X
    for _ in range(n_layers):
        lat = Pi.t() @ i_ret
        i_ret = Pi @ lat
        u_ret = Pu @ lat
    return torch.cat([u_ret, i_ret], 0)


def hgnn_grad(Pi, Pu, X, n_layers, g, dtype=torch.float64):
    a, b, c = tt(Pi, dtype, True), tt(Pu, dtype, True), tt(X, dtype, True)
    out = hgnn(a, b, c, n_layers)
    (out * tt(g, dtype)).sum().backward()
    return out.detach().numpy(), a.grad.numpy(), b.grad.numpy(), c.grad.numpy()


# ---------------------------------------------------------------------------
# d. the loss on the five tables
# ---------------------------------------------------------------------------
def combine(C, Mv, Mt, Gv, Gt, alpha):
    return C + F.normalize(Mv) + F.normalize(Mt) + alpha * F.normalize(Gv + Gt)


def loss_terms(all_, trip, n_users, reg):
    u, p, n = (torch.as_tensor(np.asarray(t), dtype=torch.int64) for t in trip)
    eu, ep, en = all_[u], all_[n_users + p], all_[n_users + n]
    bpr = -F.logsigmoid((eu * ep).sum(1) - (eu * en).sum(1)).mean()
    rg = reg * (torch.norm(eu, p=2) + torch.norm(ep, p=2) + torch.norm(en, p=2)) / eu.shape[0]
    return bpr + rg, bpr, rg


def loss_grad(tables, trip, n_users, alpha, reg, dtype=torch.float64):
    """(out [3] = total, bpr, reg; the five gradient tables)."""
    ts = [tt(t, dtype, True) for t in tables]
    out = loss_terms(combine(*ts, alpha), trip, int(n_users), reg)
    out[0].backward()
    return np.array([float(x) for x in out]), [t.grad.numpy() for t in ts]


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def dense_graphs(train_u, train_i, nu, ni, dtype=torch.float64):
    """(norm_adj [n, n] with float32 values as the reference stores them, R [nu, ni], num_inters)."""
    n = nu + ni
    deg = (np.bincount(train_u, minlength=n) + np.bincount(train_i + nu, minlength=n)).astype(np.float64) + 1e-7
    dinv = np.power(deg, -0.5)
    A = torch.zeros(n, n, dtype=dtype)
    v = torch.as_tensor((dinv[train_u] * dinv[train_i + nu]).astype(np.float32)).to(dtype)
    A[train_u, train_i + nu] = v
    A[train_i + nu, train_u] = v
    R = torch.zeros(nu, ni, dtype=dtype)
    R[train_u, train_i] = 1.0
    return A, R, torch.as_tensor((1.0 / deg).astype(np.float32)).to(dtype)


def tables(p, feats, graphs, hp, draws, training):
    """(CGE, MGE_v, MGE_t, GHE_v, GHE_t); p: dict name -> tensor, feats = (v, t), draws: the
    four noise tensors (iv, uv, it, ut) then the four keep masks (bool, or None)."""
    A, R, ninv = graphs
    U, I = p["user_embedding.weight"], p["item_id_embedding.weight"]
    nu = U.shape[0]
    ego = torch.cat([U, I], 0)
    if hp["cf_model"] == "mf":
        cge = ego
    else:
        layers, cur = [ego], ego
        for _ in range(hp["n_ui_layers"]):
            cur = A @ cur
            layers.append(cur)
        cge = torch.stack(layers, 1).mean(1)
    kr = hp["keep_rate"] if training else 1.0
    mge, ghe = [], []
    for m, (X, trs, hyper) in enumerate(((feats[0], p["item_image_trs"], p["v_hyper"]),
                                         (feats[1], p["item_text_trs"], p["t_hyper"]))):
        li = X @ hyper
        lu = R @ li
        keep = [draws[4 + 2 * m + s] if training and len(draws) > 4 else None for s in range(2)]
        Pi = assign(li, draws[2 * m], keep[0], kr)[1]
        Pu = assign(lu, draws[2 * m + 1], keep[1], kr)[1]
        ghe.append(hgnn(Pi, Pu, cge[nu:], hp["n_hyper_layer"]))
        fi = X @ trs
        x = torch.cat([(R @ fi) * ninv[:nu, None], fi], 0)
        for _ in range(hp["n_mm_layers"]):
            x = A @ x
        mge.append(x)
    return cge, mge[0], mge[1], ghe[0], ghe[1]


def model_loss(p, feats, graphs, hp, draws, trip, training=True):
    """(loss, {bpr, reg, ssl_u, ssl_i}) of lgmrec.py:175-194."""
    ts = tables(p, feats, graphs, hp, draws, training)
    nu = p["user_embedding.weight"].shape[0]
    total, bpr, rg = loss_terms(combine(*ts, hp["alpha"]), trip, nu, hp["reg_weight"])
    u, pos = (torch.as_tensor(np.asarray(t), dtype=torch.int64) for t in trip[:2])
    Gv, Gt = ts[3], ts[4]
    su, si = ssl_term(Gv[:nu], Gt[:nu], u), ssl_term(Gv[nu:], Gt[nu:], pos)
    return total + hp["cl_weight"] * (su + si), dict(bpr=bpr, reg=rg, ssl_u=su, ssl_i=si)


def adam_step(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    return p - lr / (1 - b1 ** t) * m / ((v / (1 - b2 ** t)).sqrt() + eps), m, v


def load(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


def fixture_draws(z, prefix, dtype=torch.float64, H=4):
    """The eight draws stored under `prefix` (noise0..3, keep0..3 packed) as restatement inputs."""
    noise = [tt(z[f"{prefix}noise{k}"], dtype) for k in range(4)]
    keeps = [torch.as_tensor(unpack_keep(z[f"{prefix}keep{k}"], H)) for k in range(4)] if f"{prefix}keep0" in z else []
    return noise + keeps
