"""DualGNN on the rsx HIP path — drop-in for the reference's models/dualgnn.py (TMM'21): per
modality a two-hop GCN on the symmetrically normalised user-item graph, a per-user mix of the
modalities, and one aggregation over the user co-occurrence graph (top-k lists, softmax weights,
resampled every epoch).

Same class name, constructor `(config, dataloader)`, YAML keys, module and parameter names,
creation order and initial draws (reference src/models/dualgnn.py:22-129, 269-302), forward, loss
and scoring (:141-205), as the reference really computes them:

* `dim_latent = 64` is hard-coded (:47): the representation is 64 wide; k = 40, one "layer",
  softmax user weights, `construction = 'weighted_sum'`; `aggr_mode` 'add' only;
* per modality x = normalize([preference; MLP_1(leaky(MLP(feat)))]), h = A x, h1 = A h,
  x_hat = (h + x) + h1 (:304-315), A = D^-1/2 A D^-1/2 over both directions of the training edges
  (:334-342); `preference` is a trainable Parameter; the dropped-edge lists are never read;
* `representation = self.v_rep; representation += self.t_rep` (:148-154) adds into v_rep itself:
  user_rep[u] = w0 (v + t) + w1 t, item rows v + t.  One modality: that modality's rows,
  `weight_u` not applied (still regularised);
* `result_embed` is the representation of the last TRAINING forward (`result` here; one
  optimiser step stale at evaluation; before any training the random float64 draw of :129);
* `MLP_v`, `MLP_t`, `MLP_user` exist, are drawn, named and saved, and nothing reads them: they
  never get a gradient and the optimiser skips them; `weight_i` gets its regulariser's alone.

The user graph is host work (rsx.dualgnn.load_user_graph / build_user_graph / topk_sample); the
step's kernels are csrc/dualgnn.hip (rsx_dualgnn_mix_*, rsx_dualgnn_ugraph_fwd,
rsx_dualgnn_loss_*), the MLP and F.normalize are rsx.dense's wide product and normalise, A x
and the user graph's backward (the transposed lists as a CSR) run on rsx_spmm.

One GPU; anything the kernels are not built for raises RSX_ERR_UNSUPPORTED at construction.
"""
from __future__ import annotations

import ctypes as C
import io
import os
import pickle

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import ops
from .dense import _Gemm, _Normalize
from .recommender import GeneralRecommender

DIM_LATENT = 64  # dualgnn.py:47
HIDDEN = 4 * DIM_LATENT  # the MLP's width (:294)
K_USER = 40  # dualgnn.py:34
KEEP = 200  # the generator's cut (preprocessing/dualgnn-gen-u-u-matrix.py)
CACHE_NAME = "rsx_user_graph_200.npz"


def unsupported(what: str) -> RuntimeError:
    return RuntimeError(f"RSX_ERR_UNSUPPORTED: {what} (DualGNN runs on the HIP path only)")


# ---------------------------------------------------------------------------
# the user graph (host; numpy, scipy, the CPU generators)
# ---------------------------------------------------------------------------
class UserGraph:
    """The users' co-occurrence lists as flat arrays: user u's neighbours nbr[ptr[u]:ptr[u + 1]]
    (int32) with their co-occurrence counts cnt (float32), in the file's order."""

    def __init__(self, ptr, nbr, cnt):
        self.ptr = np.ascontiguousarray(ptr, dtype=np.int64)
        self.nbr = np.ascontiguousarray(nbr, dtype=np.int32)
        self.cnt = np.ascontiguousarray(cnt, dtype=np.float32)
        if self.ptr.ndim != 1 or self.ptr.size < 1 or self.ptr[0] != 0 or np.any(np.diff(self.ptr) < 0) \
                or self.ptr[-1] != self.nbr.size or self.nbr.size != self.cnt.size:
            raise ValueError("UserGraph: ptr / nbr / cnt do not describe lists")
        self.n_users = self.ptr.size - 1

    def lists(self, u: int):
        a, b = self.ptr[u], self.ptr[u + 1]
        return self.nbr[a:b], self.cnt[a:b]


_NUMPY_GLOBALS = {(mod, name) for mod in ("numpy.core.multiarray", "numpy._core.multiarray") for name in ("_reconstruct",)}
_NUMPY_GLOBALS |= {("numpy", "ndarray"), ("numpy", "dtype")}


class _NumpyOnlyUnpickler(pickle.Unpickler):
    """Admits the globals a pickled numpy object array needs and nothing else."""

    def find_class(self, module, name):
        if (module, name) in _NUMPY_GLOBALS:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"global {module}.{name} is not admitted")


def load_user_graph(path: str, n_users: int):
    """The reference's `user_graph_dict.npy` (np.save of {u: [[neighbours], [counts]]}, a pickled
    object array) as a UserGraph, read without allow_pickle: the .npy header through
    numpy.lib.format, the payload through an Unpickler that admits only numpy's reconstruction
    globals.  None when the file is absent, refused, or not a dict of `n_users` well-formed lists
    (the stance of blocks.load_reference_knn: such a file is rebuilt, not trusted)."""
    if not os.path.isfile(path):
        return None
    try:
        with open(path, "rb") as f:
            major, _ = np.lib.format.read_magic(f)
            hdr = np.lib.format.read_array_header_1_0(f) if major == 1 else np.lib.format.read_array_header_2_0(f)
            shape, _, dtype = hdr
            if not dtype.hasobject or shape != ():
                return None
            obj = _NumpyOnlyUnpickler(io.BytesIO(f.read())).load()
        d = obj.item() if isinstance(obj, np.ndarray) else obj
        if not isinstance(d, dict) or len(d) != n_users:
            return None
        ptr = np.zeros(n_users + 1, dtype=np.int64)
        nbr, cnt = [], []
        for u in range(n_users):
            pair = d[u]
            if len(pair) != 2 or len(pair[0]) != len(pair[1]):
                return None
            a = np.asarray(pair[0], dtype=np.int64).reshape(-1)
            c = np.asarray(pair[1], dtype=np.float32).reshape(-1)
            if a.size and (a.min() < 0 or a.max() >= n_users):
                return None
            ptr[u + 1] = ptr[u] + a.size
            nbr.append(a)
            cnt.append(c)
        return UserGraph(ptr, np.concatenate(nbr) if nbr else np.zeros(0), np.concatenate(cnt) if cnt else np.zeros(0))
    except Exception:  # noqa: BLE001 - a file the safe reader refuses is rebuilt, not trusted
        return None


def build_user_graph(train_u, train_i, n_users: int, keep: int = KEEP) -> UserGraph:
    """The generator's graph from the training interactions: co-occurrence counts B B^T (B the
    binary user x item matrix), the diagonal removed, a row's `keep` largest, ordered by count
    descending.  Ties are ordered by user id ascending: our rule.  The reference's order among
    equal counts is whatever torch.topk gave on the dense row, which is not specified."""
    import scipy.sparse as sp

    u = np.asarray(train_u, dtype=np.int64).ravel()
    i = np.asarray(train_i, dtype=np.int64).ravel()
    n_items = int(i.max()) + 1 if i.size else 1
    Bm = sp.csr_matrix((np.ones(u.size, dtype=np.float32), (u, i)), shape=(n_users, n_items))
    Bm.data[:] = 1.0  # (duplicates were summed: binary)
    Cm = (Bm @ Bm.T).tocsr()
    Cm.setdiag(0)
    Cm.eliminate_zeros()
    Cm.sort_indices()
    ptr = np.zeros(n_users + 1, dtype=np.int64)
    nbr, cnt = [], []
    for r in range(n_users):
        a, b = Cm.indptr[r], Cm.indptr[r + 1]
        cols, vals = Cm.indices[a:b], Cm.data[a:b]
        order = np.lexsort((cols, -vals))[:keep]  # count descending, then id ascending
        nbr.append(cols[order])
        cnt.append(vals[order])
        ptr[r + 1] = ptr[r] + order.size
    return UserGraph(ptr, np.concatenate(nbr) if nbr else np.zeros(0), np.concatenate(cnt) if cnt else np.zeros(0))


def cached_user_graph(root: str, train_u, train_i, n_users: int) -> UserGraph:
    """build_user_graph, cached next to the dataset as rsx_user_graph_200.npz with a signature of
    the interactions; one writer a job, tmp + os.replace (as blocks.cached_knn)."""
    u = np.asarray(train_u, dtype=np.int64).ravel()
    i = np.asarray(train_i, dtype=np.int64).ravel()
    sig = np.array([n_users, u.size, int(u.sum()), int(i.sum()), int((u * 31 + i).sum() % (1 << 61))], dtype=np.int64)
    path = os.path.join(root, CACHE_NAME)
    if os.path.exists(path):
        try:
            z = np.load(path)
            if np.array_equal(z["sig"], sig):
                return UserGraph(z["ptr"], z["nbr"], z["cnt"])
        except (OSError, ValueError, KeyError, EOFError):  # another rank still writing it: rebuild
            pass
    g = build_user_graph(u, i, n_users)
    if ops._world()[1] == 0:
        try:
            os.makedirs(root, exist_ok=True)
            tmp = f"{path}.{os.getpid()}.tmp.npz"
            np.savez(tmp, ptr=g.ptr, nbr=g.nbr, cnt=g.cnt, sig=sig)
            os.replace(tmp, path)
        except OSError:
            pass
    return g


def topk_sample(g: UserGraph, k: int = K_USER):
    """The reference's topk_sample (dualgnn.py:207-250): (idx int32 [nu, k], W float32 [nu, k]).
    A user's first k neighbours and the softmax of their counts; a list shorter than k is padded
    by np.random.randint re-draws from itself (the global numpy generator, consumed exactly as
    the reference consumes it; a duplicate keeps its own softmax share); an empty list gives the
    index row [0] * k and a zero weight row.  Only the short rows run in Python; the softmax is
    torch.softmax on float32, one row a call's row, as the reference evaluates it."""
    nu = g.n_users
    length = np.diff(g.ptr)
    idx = np.zeros((nu, k), dtype=np.int32)
    cnt = np.zeros((nu, k), dtype=np.float32)
    full = np.flatnonzero(length >= k)
    if full.size:
        pos = g.ptr[full][:, None] + np.arange(k)[None, :]
        idx[full] = g.nbr[pos]
        cnt[full] = g.cnt[pos]
    for u in np.flatnonzero((length < k) & (length > 0)):  # ascending: the reference's draw order
        nb, ct = g.lists(u)
        sel = list(range(nb.size))
        while len(sel) < k:
            sel.append(sel[np.random.randint(0, len(sel))])
        idx[u] = nb[sel]
        cnt[u] = ct[sel]
    W = torch.softmax(torch.from_numpy(cnt), dim=1).numpy()
    W[length == 0] = 0.0
    return idx, np.ascontiguousarray(W, dtype=np.float32)


def transposed_lists(idx: np.ndarray, W: np.ndarray):
    """(rowptr int64 [nu + 1], col int32, val float32) of P^T, P[u, idx[u, j]] += W[u, j]: row s
    lists every (u, j) with idx[u, j] = s, by u then j.  All nu k entries are kept, the
    zero-weight ones included, so the arrays' sizes do not change between epochs."""
    nu, k = idx.shape
    src = idx.reshape(-1).astype(np.int64)
    if src.size and (src.min() < 0 or src.max() >= nu):
        raise ValueError("transposed_lists: an index outside the user table")
    order = np.argsort(src, kind="stable")
    rowptr = np.zeros(nu + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=nu), out=rowptr[1:])
    return rowptr, (order // k).astype(np.int32), W.reshape(-1)[order].astype(np.float32)


def sym_operator(train_u, train_i, n_users: int, n_items: int):
    """(rows, cols, vals) of A_hat = D^-1/2 A D^-1/2 on the n_users + n_items nodes (dualgnn.py:
    58-60, 334-342): every training interaction in both directions, a repeated one counted with
    its multiplicity, deg the plain edge count (no epsilon); a node without edges has no entry."""
    n = n_users + n_items
    u = np.asarray(train_u, dtype=np.int64)
    i = np.asarray(train_i, dtype=np.int64) + n_users
    key, mult = np.unique(np.concatenate([u * n + i, i * n + u]), return_counts=True)
    rows, cols = key // n, key % n
    deg = np.bincount(rows, weights=mult.astype(np.float64), minlength=n)
    return rows, cols, (mult / np.sqrt(deg[rows] * deg[cols])).astype(np.float32)


# ---------------------------------------------------------------------------
# modules and initial draws
# ---------------------------------------------------------------------------
class GCN(nn.Module):
    """One modality's parameters, created and drawn in the reference's order (dualgnn.py:290-296):
    np.random.randn for the preference's shape, its xavier_normal_, MLP, MLP_1."""

    def __init__(self, num_user: int, dim_feat: int):
        super().__init__()
        self.preference = nn.Parameter(nn.init.xavier_normal_(
            torch.tensor(np.random.randn(num_user, DIM_LATENT), dtype=torch.float32), gain=1))
        self.MLP = nn.Linear(dim_feat, HIDDEN)
        self.MLP_1 = nn.Linear(HIDDEN, DIM_LATENT)


def dualgnn_init(host: nn.Module, n_users: int, n_items: int, dim_x: int, v_dim, t_dim):
    """Registers the reference's parameters and modules on `host` in its order and with its draws
    on the CPU generators (dualgnn.py:49-129); returns the float64 draw of result_embed."""
    host.MLP_v = nn.Linear(DIM_LATENT, DIM_LATENT, bias=False)
    host.MLP_t = nn.Linear(DIM_LATENT, DIM_LATENT, bias=False)
    host.weight_u = nn.Parameter(nn.init.xavier_normal_(
        torch.tensor(np.random.randn(n_users, 2, 1), dtype=torch.float32)))
    host.weight_u.data = F.softmax(host.weight_u.data, dim=1)
    host.weight_i = nn.Parameter(nn.init.xavier_normal_(
        torch.tensor(np.random.randn(n_items, 2, 1), dtype=torch.float32)))
    host.weight_i.data = F.softmax(host.weight_i.data, dim=1)
    # the dropped-edge machinery (:71-111) is never read; its one draw is consumed
    np.random.choice(n_items, int(n_items * 0.1), replace=False)
    host.MLP_user = nn.Linear(DIM_LATENT * 3, DIM_LATENT)
    if v_dim is not None:
        host.v_gcn = GCN(n_users, v_dim)
    if t_dim is not None:
        host.t_gcn = GCN(n_users, t_dim)
    return nn.init.xavier_normal_(torch.tensor(np.random.randn(n_users + n_items, dim_x)))


# ---------------------------------------------------------------------------
# kernel wrappers
# ---------------------------------------------------------------------------
def mix_fwd(xv, xt, weight_u, n_users: int, result: torch.Tensor):
    """user_rep [nu, 64]; the item rows of `result` are written in place."""
    ops._gpu(xv, xt, weight_u, result)
    n, d = result.shape
    user_rep = torch.empty(n_users, d, dtype=torch.float32, device=result.device)
    L.check(L.lib().rsx_dualgnn_mix_fwd(ops._p(xv), ops._p(xt), ops._p(weight_u), n_users, n - n_users, d,
                                        ops._p(user_rep), ops._p(result), ops._stream()), "rsx_dualgnn_mix_fwd")
    return user_rep


def mix_bwd(g_user_rep, g_result, xv, xt, weight_u, go, reg_weight: float, n_users: int):
    """(g_v | None, g_t | None, g_weight_u [nu, 2, 1])."""
    ops._gpu(g_user_rep, g_result, xv, xt, weight_u, go)
    n, d = g_result.shape
    g_v = None if xv is None else torch.empty_like(g_result)
    g_t = None if xt is None else torch.empty_like(g_result)
    g_w = torch.empty_like(weight_u)
    L.check(L.lib().rsx_dualgnn_mix_bwd(ops._p(g_user_rep), ops._p(g_result), ops._p(xv), ops._p(xt), ops._p(weight_u),
                                        ops._p(go), float(reg_weight), n_users, n - n_users, d, ops._p(g_v), ops._p(g_t),
                                        ops._p(g_w), ops._stream()), "rsx_dualgnn_mix_bwd")
    return g_v, g_t, g_w


def ugraph_fwd(user_rep, idx, W, out=None):
    """out[u] = user_rep[u] + sum_j W[u, j] user_rep[idx[u, j]]; `out`: the first nu rows of it are written."""
    ops._gpu(user_rep, idx, W, out)
    nu, d = user_rep.shape
    if idx.dtype != torch.int32 or W.dtype != torch.float32 or idx.shape != W.shape or idx.dim() != 2 or idx.shape[0] != nu:
        raise RuntimeError("dualgnn ugraph: idx int32 [nu, k] and W float32 [nu, k] expected")
    if out is None:
        out = torch.empty_like(user_rep)
    elif out.shape[0] < nu or out.shape[1] != d or out.data_ptr() == user_rep.data_ptr():
        raise RuntimeError("dualgnn ugraph: out must hold nu rows and must not be user_rep")
    L.check(L.lib().rsx_dualgnn_ugraph_fwd(ops._p(user_rep), ops._p(idx), ops._p(W), nu, idx.shape[1], d, ops._p(out),
                                           ops._stream()), "rsx_dualgnn_ugraph_fwd")
    return out


def ugraph_bwd(PT, g_result, n_users: int):
    """g_user_rep = g_out + P^T g_out, g_out the first nu rows of g_result: rsx_spmm on the
    transposed lists with the ADD epilogue."""
    d = g_result.shape[1]
    g = torch.empty(n_users, d, dtype=torch.float32, device=g_result.device)
    PT.spmm_epi(g_result, ops.epi(L.RSX_EPI_ADD, y=g, s_in=g_result), d)
    return g


def loss_args(result, pref_v, pref_t, weight_u, weight_i, triplets, n_users: int, reg_weight: float):
    ops._gpu(result, pref_v, pref_t, weight_u, weight_i, triplets)
    if triplets.dtype != torch.int64 or triplets.dim() != 2 or triplets.shape[0] != 3:
        raise RuntimeError("dualgnn loss: triplets must be an int64 [3, batch] tensor")
    if pref_v is None and pref_t is None:
        raise RuntimeError("dualgnn loss: at least one preference table")
    a = L.DualgnnLossArgs()
    a.result, a.pref_v, a.pref_t = result.data_ptr(), ops._pi(pref_v) or None, ops._pi(pref_t) or None
    a.weight_u, a.weight_i, a.triplets = weight_u.data_ptr(), weight_i.data_ptr(), triplets.data_ptr()
    a.n_users, a.n_items, a.batch = int(n_users), result.shape[0] - int(n_users), triplets.shape[1]
    a.d, a.reg_weight = result.shape[1], float(reg_weight)
    return a


def loss_fwd(a, ws):
    out = torch.empty(3, dtype=torch.float32, device=ws.device)
    L.check(L.lib().rsx_dualgnn_loss_fwd(C.byref(a), ops._p(out), ops._p(ws), ws.numel(), ops._stream()),
            "rsx_dualgnn_loss_fwd")
    return out


def loss_bwd(a, go, ws, pref_v, pref_t, weight_i):
    """(g_result [n, 64], g_pref_v | None, g_pref_t | None, g_weight_i)."""
    n, d = a.n_users + a.n_items, a.d
    g = torch.empty(n, d, dtype=torch.float32, device=ws.device)
    gpv = None if pref_v is None else torch.empty_like(pref_v)
    gpt = None if pref_t is None else torch.empty_like(pref_t)
    gwi = torch.empty_like(weight_i)
    L.check(L.lib().rsx_dualgnn_loss_bwd(C.byref(a), ops._p(go), ops._p(g), ops._p(gpv), ops._p(gpt), ops._p(gwi),
                                         ops._p(ws), ws.numel(), ops._stream()), "rsx_dualgnn_loss_bwd")
    return g, gpv, gpt, gwi


def loss_workspace(batch: int, d: int, device) -> torch.Tensor:
    return ops.loss_workspace(L.lib().rsx_dualgnn_loss_ws_bytes, batch, d, device, unsupported)


def propagate(A, x):
    """(h + x) + A h, h = A x: the first product stored, the second summed in its epilogue."""
    d = x.shape[1]
    h = A.spmm(x)
    out = torch.empty_like(x)
    A.spmm_epi(h, ops.epi(L.RSX_EPI_FINAL, beta=1.0, f=out, s_in=x, r_add=h), d)
    return out


class _Prop(torch.autograd.Function):
    """x_hat = x + A x + A^2 x (dualgnn.py:311-314); A is symmetric, so the backward is the same
    operator on the gradient.  Nothing is saved."""

    @staticmethod
    def forward(ctx, x, A):
        ctx.A = A
        return propagate(A, x.contiguous())

    @staticmethod
    def backward(ctx, g):
        return propagate(ctx.A, g.contiguous()), None


class _Tail(torch.autograd.Function):
    """The step from the modality tables to the loss word: mix, user graph, loss, and `result`.
    cfg = (n_users, reg_weight, result, idx, W, PT, ws, keep | None).  One differentiable output;
    every tensor is kept with save_for_backward."""

    @staticmethod
    def forward(ctx, cfg, triplets, xv, xt, weight_u, weight_i, pref_v, pref_t):
        n_users, reg_weight, result, idx, W, PT, ws, keep = cfg
        xv, xt, pref_v, pref_t = (None if t is None else t.contiguous() for t in (xv, xt, pref_v, pref_t))
        weight_u, weight_i, triplets = weight_u.contiguous(), weight_i.contiguous(), triplets.contiguous()
        user_rep = mix_fwd(xv, xt, weight_u, n_users, result)
        ugraph_fwd(user_rep, idx, W, out=result)
        ctx.args = loss_args(result, pref_v, pref_t, weight_u, weight_i, triplets, n_users, reg_weight)
        ctx.cfg = (n_users, reg_weight, PT, ws)
        ctx.save_for_backward(triplets, xv, xt, weight_u, weight_i, pref_v, pref_t, result)
        out = loss_fwd(ctx.args, ws)
        if keep is not None:
            keep["terms"], keep["user_rep"] = out, user_rep
        return out[0]

    @staticmethod
    def backward(ctx, go):
        _, xv, xt, weight_u, weight_i, pref_v, pref_t, _ = ctx.saved_tensors
        n_users, reg_weight, PT, ws = ctx.cfg
        go = go.to(torch.float32).contiguous()
        g_result, gpv, gpt, gwi = loss_bwd(ctx.args, go, ws, pref_v, pref_t, weight_i)
        g_user_rep = ugraph_bwd(PT, g_result, n_users)
        g_v, g_t, gwu = mix_bwd(g_user_rep, g_result, xv, xt, weight_u, go, reg_weight, n_users)
        return None, None, g_v, g_t, gwu, gwi, gpv, gpt


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
class DualGNN(GeneralRecommender):
    # calculate_loss has no host syncs and no data-dependent host branches: the Trainer may
    # capture a batch in a HIP graph.  pre_epoch_processing rebuilds the transposed lists' CSR
    # (its SpMM schedule follows the epoch's in-degrees and has no fixed size), so the captures
    # are dropped at every epoch start, as FREEDOM's are
    supports_graph_step = True
    graph_step_persistent = False

    @staticmethod
    def check_config(config):
        d = config["embedding_size"]
        if d != DIM_LATENT:
            raise unsupported(f"embedding_size {d}: the reference's dim_latent is hard-coded to {DIM_LATENT}")
        aggr = config["aggr_mode"]
        if aggr != "add":
            raise unsupported(f"aggr_mode {aggr!r}: 'add' only")
        ops.require_single_gpu(config, unsupported)

    def check_features(self) -> None:
        self.require_features(unsupported, need=1)

    def __init__(self, config, dataset):
        self.check_config(config)
        try:
            super().__init__(config, dataset)
        except AssertionError as e:  # recommender.py: "Features all NONE"
            raise unsupported("no feature file at all") from e
        ops.require_device(self.device)
        self.check_features()
        self.num_user, self.num_item = self.n_users, self.n_items
        self.dim_latent = d = DIM_LATENT
        self.k, self.num_layer = K_USER, 1
        self.aggr_mode, self.user_aggr_mode, self.construction = config["aggr_mode"], "softmax", "weighted_sum"
        self.n_layers = config["n_layers"]  # read and, as in the reference, never used
        self.reg_weight = float(config["reg_weight"])
        self.drop_rate = 0.1
        nu, ni, dev = self.n_users, self.n_items, self.device
        self.n_nodes = n = nu + ni
        self.chunk = int(config["rsx_chunk"] or 32)
        # the user graph: the reference's file when the dataset directory holds one, else built
        im = dataset.inter_matrix(form="coo")
        root = os.path.abspath((config["data_path"] or "") + config["dataset"])
        name = config["user_graph_dict_file"] or "user_graph_dict.npy"
        self.user_graph = load_user_graph(os.path.join(root, name), nu)
        self.user_graph_source = "file"
        if self.user_graph is None:
            self.user_graph = cached_user_graph(root, im.row, im.col, nu)
            self.user_graph_source = "built"
        self.A = ops.DeviceCSR(*_csr(*sym_operator(im.row, im.col, nu, ni), n), n, dev, self.chunk)
        # every draw on the CPU generators in the reference's order, `result_embed` included
        v_dim = None if self.v_feat is None else int(self.v_feat.shape[1])
        t_dim = None if self.t_feat is None else int(self.t_feat.shape[1])
        result = dualgnn_init(self, nu, ni, d, v_dim, t_dim)
        self.to(dev)
        self.result = result.to(torch.float32).to(dev).contiguous()  # persistent: the step's kernels write it
        self.epoch_idx = self.epoch_W = self.PT = None
        B = max(int(config["train_batch_size"] or 1), 1)
        self._ws = loss_workspace(B, d, dev)
        self.last_terms = None  # {total, bpr, reg} of the last calculate_loss (device)
        self.last_user_rep = None

    @property
    def result_embed(self) -> torch.Tensor:
        return self.result

    def _mods(self):
        return [(m, getattr(self, f"{m}_gcn"), f) for m, f in (("v", self.v_feat), ("t", self.t_feat)) if f is not None]

    # ------------------------------------------------------------- user graph
    def pre_epoch_processing(self):
        """topk_sample(40) on the host (the reference's draws), its lists and their transpose on
        the device."""
        idx, W = topk_sample(self.user_graph, self.k)
        dev = self.device
        self.epoch_idx = torch.from_numpy(idx).to(dev)
        self.epoch_W = torch.from_numpy(W).to(dev)
        self.PT = ops.DeviceCSR(*transposed_lists(idx, W), self.n_users, dev, self.chunk)

    # --------------------------------------------------------------- forward
    def _modal(self, g: GCN, feat: torch.Tensor):
        """x_hat [n, 64] of one modality (dualgnn.py:304-315), with autograd."""
        # leaky(X W^T + b) on a constant X of any width that is a multiple of 4
        hid = _Gemm.apply(feat, None, g.MLP.weight, g.MLP.bias, False, True)
        temp = _Gemm.apply(hid, None, g.MLP_1.weight, g.MLP_1.bias, False, False)
        x = _Normalize.apply(torch.cat([g.preference, temp], dim=0))
        return _Prop.apply(x, self.A)

    def _step(self, trip, keep):
        if self.PT is None:
            raise RuntimeError("DualGNN: pre_epoch_processing() has not sampled the user graph yet")
        xs = {m: self._modal(g, f) for m, g, f in self._mods()}
        prefs = {m: g.preference for m, g, _ in self._mods()}
        cfg = (self.n_users, self.reg_weight, self.result, self.epoch_idx, self.epoch_W, self.PT, self._ws, keep)
        loss = _Tail.apply(cfg, trip, xs.get("v"), xs.get("t"), self.weight_u, self.weight_i, prefs.get("v"),
                           prefs.get("t"))
        return loss, xs

    def forward(self, interaction=None):
        """The representation [out_users; item_rep] (dualgnn.py:141-174), without autograd; as the
        reference's forward it becomes `result`."""
        with torch.no_grad():
            if self.PT is None:
                raise RuntimeError("DualGNN: pre_epoch_processing() has not sampled the user graph yet")
            xs = {m: self._modal(g, f) for m, g, f in self._mods()}
            user_rep = mix_fwd(xs.get("v"), xs.get("t"), self.weight_u.contiguous(), self.n_users, self.result)
            ugraph_fwd(user_rep, self.epoch_idx, self.epoch_W, out=self.result)
            self.last_user_rep = user_rep
        return self.result

    def calculate_loss(self, interaction):
        """interaction: int64 [3, B] on the device."""
        B = interaction.shape[1]
        self._ws = ops.grow_workspace(L.lib().rsx_dualgnn_loss_ws_bytes, self._ws, B, self.dim_latent)
        keep = {}
        loss, _ = self._step(interaction[:3].contiguous(), keep)
        self.last_terms, self.last_user_rep = keep["terms"], keep["user_rep"]
        return loss

    # ------------------------------------------------------------ evaluation
    def full_sort_predict(self, interaction):
        nu = self.n_users
        return ops.score_dense(self.result[:nu], interaction[0].contiguous(), self.result[nu:])

    def full_sort_topk(self, interaction, k, eval_data):
        nu = self.n_users
        return ops.fullsort_topk(self.result[:nu], interaction[0].contiguous(), self.result[nu:], eval_data.mask_rowptr,
                                 eval_data.mask_col, k)


def _csr(rows, cols, vals, n: int):
    from . import graph

    return graph.to_csr(rows, cols, vals, n, n)
