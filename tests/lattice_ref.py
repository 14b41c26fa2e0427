"""float64 torch restatement of LATTICE (ACM MM'21; reference src/models/lattice.py), dense and
with autograd: the loss on given tables (the contract of rsx_lattice_loss_fwd / _bwd,
include/rsx.h), the learned item graph as a dense operator (the contract of rsx_lattice_graph /
_prop / _graph_bwd), the whole model with its once-per-epoch graph build and the detached
graph of every other batch, Adam, and the fixture plumbing the LATTICE tests share.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# named_parameters' order: the module's own parameter first, then its children as created
NAMES = ("modal_weight", "user_embedding.weight", "item_id_embedding.weight", "image_embedding.weight",
         "text_embedding.weight", "image_trs.weight", "image_trs.bias", "text_trs.weight", "text_trs.bias")
GRAPH_ONLY = NAMES[:1] + NAMES[3:]  # parameters that only the graph-build batch reaches
HPARAMS = dict(seed=999, reg_weight=1e-3, learning_rate=1e-3, knn_k=10, lambda_coeff=0.9, n_layers=1, n_ui_layers=2,
               train_batch_size=512)
MODS = ("image", "text")


def t64(a, grad=False):
    if a is None:
        return None
    t = torch.as_tensor(np.asarray(a), dtype=torch.float64).clone()
    return t.requires_grad_(True) if grad else t


# ---------------------------------------------------------------------------
# the loss on given tables
# ---------------------------------------------------------------------------
def loss_terms(users, items, trip, reg, batch_size):
    """(total, mf, emb) of lattice.py:199-227 on the two tables."""
    u, p, n = (torch.as_tensor(np.asarray(t), dtype=torch.int64) for t in trip)
    eu, ep, en = users[u], items[p], items[n]
    mf = -F.logsigmoid((eu * ep).sum(1) - (eu * en).sum(1)).mean()
    emb = reg * (0.5 * (eu ** 2).sum() + 0.5 * (ep ** 2).sum() + 0.5 * (en ** 2).sum()) / batch_size
    return mf + emb, mf, emb


def loss_grad(E, H, trip, n_users, reg, batch_size, dtype=torch.float64):
    """(out [3] = total, mf, emb; gE; gH): whole tables, zero off the batch rows, repeated rows
    summed; the item rows are E[nu + i] + normalize(H)[i]."""
    E = torch.as_tensor(np.asarray(E), dtype=dtype).clone().requires_grad_(True)
    H = torch.as_tensor(np.asarray(H), dtype=dtype).clone().requires_grad_(True)
    nu = int(n_users)
    out = loss_terms(E[:nu], E[nu:] + F.normalize(H, p=2, dim=1), trip, reg, batch_size)
    out[0].backward()
    return np.array([float(x) for x in out]), E.grad.numpy(), H.grad.numpy()


# ---------------------------------------------------------------------------
# the item graph as a dense operator
# ---------------------------------------------------------------------------
def cos_sim(Fm):
    xn = Fm / torch.norm(Fm, p=2, dim=-1, keepdim=True)
    return xn @ xn.t()


def topk_ids(Fm, k):
    """The top-k columns of a row's cosine similarities (self included), [n, k] int64."""
    return torch.topk(cos_sim(Fm.detach()), k, dim=-1)[1]


def kept(Fm, idx):
    """build_knn_neighbourhood on given columns: the similarities at idx, zero elsewhere."""
    sim = cos_sim(Fm)
    return torch.zeros_like(sim).scatter(-1, idx, sim.gather(-1, idx))


def normalized(adj):
    """compute_normalized_laplacian: D^-1/2 adj D^-1/2, D the row sums, inf -> 0."""
    dis = adj.sum(-1).pow(-0.5)
    dis = torch.where(torch.isinf(dis), torch.zeros_like(dis), dis)
    return dis[:, None] * adj * dis[None, :]


def original_graph(feat, k):
    """(idx [n, k], val [n, k], dense [n, n]) of the fixed graph of a raw feature table."""
    feat = t64(feat)
    idx = topk_ids(feat, k)
    O = normalized(kept(feat, idx))
    return idx, O.gather(-1, idx), O


def dense_lists(idx, val, n):
    idx = torch.as_tensor(np.asarray(idx), dtype=torch.int64)
    return torch.zeros(n, n, dtype=torch.float64).scatter(-1, idx, t64(val))


def item_adj(Fs, idxs, Os, modal_weight, lam):
    """The dense item_adj of lattice.py:137-157 from the projected features Fs (list over the
    modalities present), their kept columns idxs, the dense original graphs Os and the raw
    modal_weight (used with two modalities only).  Differentiable in Fs and modal_weight."""
    A = [kept(f, i) for f, i in zip(Fs, idxs)]
    if len(Fs) == 2:
        w = torch.softmax(modal_weight, dim=0)
        learned, orig = w[0] * A[0] + w[1] * A[1], w[0] * Os[0] + w[1] * Os[1]
    else:
        learned, orig = A[0], Os[0]
    return (1 - lam) * normalized(learned) + lam * orig


def propagate(M, x, n_layers):
    for _ in range(n_layers):
        x = M @ x
    return x


# ---------------------------------------------------------------------------
# the whole model
# ---------------------------------------------------------------------------
class Model:
    """LATTICE at the fixture's scale.  params: dict name -> array (a modality whose
    `<name>_embedding.weight` is absent is absent from the model); A: the dense UI graph
    (row-normalised with self loops, lattice.py:100-122); origs: dict modality -> dense original graph."""

    def __init__(self, params, A, origs, hp=None, cf_model="lightgcn", lr=None):
        self.hp = dict(HPARAMS, **(hp or {}))
        self.p = {k: t64(v, grad=True) for k, v in params.items()}
        self.A, self.cf_model = t64(A), cf_model
        self.mods = [m for m in MODS if m + "_embedding.weight" in self.p]
        self.O = [t64(origs[m]) for m in self.mods]
        self.nu = self.p["user_embedding.weight"].shape[0]
        self.build = True
        self.M = None
        self.idx = None  # the kept columns of the last build, per modality
        self.opt = torch.optim.Adam(list(self.p.values()), lr=lr if lr is not None else self.hp["learning_rate"])

    def projected(self):
        return [self.p[m + "_embedding.weight"] @ self.p[m + "_trs.weight"].t() + self.p[m + "_trs.bias"]
                for m in self.mods]

    def graph(self, idxs=None):
        Fs = self.projected()
        self.idx = idxs if idxs is not None else [topk_ids(f, self.hp["knn_k"]) for f in Fs]
        return item_adj(Fs, self.idx, self.O, self.p.get("modal_weight"), self.hp["lambda_coeff"])

    def forward(self, build):
        self.M = self.graph() if build else self.M.detach()
        U, I = self.p["user_embedding.weight"], self.p["item_id_embedding.weight"]
        h = propagate(self.M, I, self.hp["n_layers"])
        if self.cf_model == "mf":
            return U, I + F.normalize(h, p=2, dim=1)
        ego = torch.cat([U, I])
        acc, cur = ego, ego
        for _ in range(self.hp["n_ui_layers"]):
            cur = self.A @ cur
            acc = acc + cur
        E = acc / (self.hp["n_ui_layers"] + 1)
        return E[: self.nu], E[self.nu:] + F.normalize(h, p=2, dim=1)

    def new_epoch(self):
        self.build = True

    def loss_backward(self, trip):
        """(loss, dict name -> gradient or None) of one batch; gradients are left for step()."""
        self.opt.zero_grad(set_to_none=True)
        u, i = self.forward(self.build)
        self.build = False
        loss = loss_terms(u, i, trip, self.hp["reg_weight"], self.hp["train_batch_size"])[0]
        loss.backward()
        return float(loss), {k: (None if v.grad is None else v.grad.numpy().copy()) for k, v in self.p.items()}

    def step(self):
        self.opt.step()

    def eval_tables(self):
        with torch.no_grad():
            u, i = self.forward(True)
        return u.numpy(), i.numpy()


# ---------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------
_CACHE = {}


def load_fixture():
    """lattice_step0_small.npz + lattice_small.npz as one dict, with what the capture left out
    put back: init.{image,text}_embedding.weight (= v_feat / t_feat) and the XOR-stored
    parameters decoded."""
    if "z" not in _CACHE:
        z = dict(np.load(os.path.join(GOLD, "lattice_step0_small.npz")))
        z.update(np.load(os.path.join(GOLD, "lattice_small.npz")))
        z["init.image_embedding.weight"], z["init.text_embedding.weight"] = z["v_feat"], z["t_feat"]
        for k in [k for k in z if "_param_xor." in k]:
            pre, name = k.split("_param_xor.")
            z[f"{pre}_param.{name}"] = (z[k] ^ z["init." + name].view(np.int32)).view(np.float32)
        _CACHE["z"] = z
    return _CACHE["z"]


def init_params(z, mods=MODS):
    """The initial parameters of a model with the modalities `mods`."""
    return {n: z["init." + n] for n in NAMES if not n.startswith(MODS) or n.startswith(tuple(mods))}


def ui_dense(z):
    if "ui" not in _CACHE:
        n = int(z["n_users"]) + int(z["n_items"])
        A = np.zeros((n, n))
        i = z["norm_adj_idx"].astype(np.int64)
        np.add.at(A, (i[0], i[1]), z["norm_adj_val"].astype(np.float64))
        _CACHE["ui"] = A
    return _CACHE["ui"]


def orig_dense(z):
    ni = int(z["n_items"])
    return {m: dense_lists(z[f"orig_{m}_idx"], z[f"orig_{m}_val"], ni) for m in MODS}


def batches(z, epoch):
    trip = z[f"epoch{epoch}_triplets"].astype(np.int64)
    B = HPARAMS["train_batch_size"]
    return [trip[:, s: s + B] for s in range(0, trip.shape[1], B)]


def two_epochs(z):
    """The restatement trained on the fixture's batches (computed once): per-step losses, the
    gradients of the first two steps, the kept columns of each build, the final parameters."""
    if "run" not in _CACHE:
        m = Model(init_params(z), ui_dense(z), orig_dense(z))
        out = dict(losses=[], grads=[], idx=[], epoch_params=[])
        for ep in (0, 1):
            m.new_epoch()
            for b, trip in enumerate(batches(z, ep)):
                loss, g = m.loss_backward(trip)
                if b == 0:
                    out["idx"].append([i.numpy() for i in m.idx])
                if ep == 0 and b < 2:
                    out["grads"].append(g)
                out["losses"].append(loss)
                m.step()
            out["epoch_params"].append({k: v.detach().numpy().copy() for k, v in m.p.items()})
        out["model"] = m
        _CACHE["run"] = out
    return _CACHE["run"]
