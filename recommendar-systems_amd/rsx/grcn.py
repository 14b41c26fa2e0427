"""GRCN on the rsx HIP path — drop-in for the reference's models/grcn.py (MM'20): per modality a
content GCN whose edge-softmax attention scores every interaction, a refined edge weight
relu(max_m alpha_m conf[source, m]) learned every step, and an id GCN of two propagations
through those weights.

Same class name, constructor `(config, dataloader)`, YAML keys, module and parameter names,
`named_parameters()` order, creation order and initial draws (reference src/models/grcn.py:80-134,
169-214), forward, loss and scoring (:224-341), as the reference really computes them:

* the routing loop (:149-156) runs on the directed user -> item edges, so its aggregate is exactly
  zero on the user rows it reads: it only re-normalises the preferences.  The preferences are
  normalised once here; `n_layers` is read and accepts any value >= 0;
* `full_sort_predict` scores `result`, the representation of the last TRAINING forward (one
  optimiser step stale; before any training the random [n, dim_x] table of :214);
* text alone does not run in the reference (:257 assigns a misspelt name): refused here too.

The graph is a CSR by target row with the reversed edge's slot (`target_csr`, plain numpy).  Its
structure is symmetric, so A_w and A_w^T share rowptr and col; their value arrays are persistent
buffers that rsx_grcn_refine_fwd rewrites every step, and both id-GCN products and their
transposes run on rsx_spmm.

Kernels (csrc/grcn.hip): rsx_grcn_attn_fwd / _bwd, rsx_grcn_refine_fwd / _bwd, rsx_grcn_edge_dots,
rsx_grcn_loss_*; leaky_relu(X W^T + b) on the shared dense blocks' wide product (rsx.dense._Gemm,
a constant X: the masked rows from rsx_dense_leaky_bwd), F.normalize on its `_Normalize`.

The step's autograd: ONE Function (`_Step`) from the normalised inputs to the loss word, one
differentiable output, every tensor kept with save_for_backward (nothing with a grad_fn on ctx: a
ctx -> output -> grad_fn -> ctx cycle would let an eager batch's graph survive into the next
batch's HIP-graph capture); no torch F.normalize / leaky_relu / relu and no copy_ into `result`
inside calculate_loss: the loss kernel writes `result`.

One GPU; anything the kernels are not built for raises RSX_ERR_UNSUPPORTED at construction.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .dense import _Gemm, _Normalize
from .recommender import GeneralRecommender

SUPPORTED_D = (64, 128)
MAX_WIDTH = 256  # the loss kernels' row: a wave of float4 lanes; also the full sort's widest d
FULLSORT_D = (128, 256)


def unsupported(what: str) -> RuntimeError:
    return RuntimeError(f"RSX_ERR_UNSUPPORTED: {what} (GRCN runs on the HIP path only)")


# ---------------------------------------------------------------------------
# host structure (numpy; no GPU needed)
# ---------------------------------------------------------------------------
def target_csr(train_u, train_i, n_users: int, n_items: int):
    """(rowptr int64 [n + 1], col int32 [2 E], rev int32 [2 E], edge_slot int64 [2 E]) of the
    2 E directed edges (the E user -> item edges, then the E item -> user edges: the reference's
    order) as a CSR by TARGET row, col = source.  Inside a row the entries are ordered by source,
    then by occurrence; a repeated interaction stays as separate entries.  rev[e]: the slot of the
    reversed edge, the k-th copy paired with the k-th copy (rev[rev[e]] = e, col[rev[e]] = row(e)).
    edge_slot[k]: the slot of the reference's k-th edge."""
    n = int(n_users) + int(n_items)
    u = np.asarray(train_u, dtype=np.int64).ravel()
    i = np.asarray(train_i, dtype=np.int64).ravel() + int(n_users)
    E = u.size
    if 2 * E >= 2 ** 31:
        raise unsupported(f"{2 * E} directed edges: the slots are int32")
    if E and (u.min() < 0 or u.max() >= n_users or i.min() < n_users or i.max() >= n):
        raise ValueError("target_csr: an interaction outside the user / item tables")
    src, tgt = np.concatenate([u, i]), np.concatenate([i, u])
    order = np.argsort(tgt * n + src, kind="stable")  # by target, then source, then occurrence
    edge_slot = np.empty(2 * E, dtype=np.int64)
    edge_slot[order] = np.arange(2 * E, dtype=np.int64)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(tgt, minlength=n), out=rowptr[1:])
    col = src[order].astype(np.int32)
    # edge k and edge (k + E) mod 2 E are each other's reverse; occurrence order is k's on both sides
    rev = np.empty(2 * E, dtype=np.int32)
    rev[edge_slot] = edge_slot[(np.arange(2 * E) + E) % max(2 * E, 1)]
    return rowptr, col, rev, edge_slot


# ---------------------------------------------------------------------------
# modules and initial draws
# ---------------------------------------------------------------------------
class EGCN(nn.Module):
    """The id GCN's state (grcn.py:80-91)."""

    def __init__(self, n_nodes: int, dim_E: int):
        super().__init__()
        self.id_embedding = nn.Parameter(nn.init.xavier_normal_(torch.rand((n_nodes, dim_E))))


class CGCN(nn.Module):
    """One content GCN's state, created and drawn in the reference's order (grcn.py:112-136)."""

    def __init__(self, num_user: int, dim_feat: int, dim_C: int):
        super().__init__()
        self.preference = nn.Parameter(nn.init.xavier_normal_(torch.rand((num_user, dim_C))))
        self.MLP = nn.Linear(dim_feat, dim_C)
        nn.init.xavier_normal_(self.MLP.weight)


def grcn_init(n_users: int, n_items: int, dim_x: int, dim_C: int, v_dim, t_dim):
    """(id_gcn, v_gcn | None, t_gcn | None, model_specific_conf, result) on the CPU, every draw in
    the reference's order (grcn.py:196-214)."""
    n = n_users + n_items
    id_gcn = EGCN(n, dim_x)
    v = CGCN(n_users, v_dim, dim_C) if v_dim is not None else None
    t = CGCN(n_users, t_dim, dim_C) if t_dim is not None else None
    conf = nn.Parameter(nn.init.xavier_normal_(torch.rand((n, (v is not None) + (t is not None)))))
    result = nn.init.xavier_normal_(torch.rand((n, dim_x)))
    return id_gcn, v, t, conf, result


# ---------------------------------------------------------------------------
# the graph on the device and the kernel wrappers
# ---------------------------------------------------------------------------
class EdgeGraph:
    """target_csr on the device: rowptr / col / rev / edge_slot, the two SpMM graphs A_w and A_w^T
    over the persistent value buffers `val` / `valT`, and the persistent alpha buffers."""

    def __init__(self, rowptr, col, rev, edge_slot, device, n_mod: int = 2, chunk: int = 32):
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
        self.n, self.nnz = rowptr.size - 1, int(rowptr[-1])
        col, rev = np.asarray(col), np.asarray(rev)
        if col.size != self.nnz or rev.size != self.nnz:
            raise RuntimeError("EdgeGraph: col / rev do not hold rowptr[-1] entries")
        if self.nnz and (col.min() < 0 or col.max() >= self.n or rev.min() < 0 or rev.max() >= self.nnz):
            raise RuntimeError("EdgeGraph: a col or rev entry outside its range")
        if np.any(np.diff(rowptr) < 0) or rowptr[0] != 0:
            raise RuntimeError("EdgeGraph: rowptr is not a prefix sum")
        self.col = torch.from_numpy(np.ascontiguousarray(col, dtype=np.int32)).to(torch.device(device))
        self.device = dev = self.col.device  # (with its index, as DeviceCSR compares it)
        self.rev = torch.from_numpy(np.ascontiguousarray(rev, dtype=np.int32)).to(dev)
        self.edge_slot = torch.from_numpy(np.ascontiguousarray(edge_slot, dtype=np.int64)).to(dev)
        self.val = torch.zeros(self.nnz, dtype=torch.float32, device=dev)
        self.valT = torch.zeros(self.nnz, dtype=torch.float32, device=dev)
        self.A = ops.DeviceCSR(rowptr, self.col, self.val, self.n, dev, chunk)
        self.AT = ops.DeviceCSR(rowptr, self.col, self.valT, self.n, dev, chunk)
        self.rowptr = self.A.rowptr
        self.alpha = [torch.zeros(self.nnz, dtype=torch.float32, device=dev) for _ in range(n_mod)]

    def args(self, rev: bool = True):
        a = (ops._p(self.rowptr), ops._p(self.col)) + ((ops._p(self.rev),) if rev else ())
        return a + (self.n, self.nnz)


def _table(g: EdgeGraph, name: str, t: torch.Tensor, d: int | None = None) -> int:
    ops._gpu(t)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != g.n or (d is not None and t.shape[1] != d):
        raise RuntimeError(f"grcn: {name} {tuple(t.shape)} {t.dtype} is not a float32 [{g.n}, {d or 'd'}] table")
    return t.shape[1]


def _edges(g: EdgeGraph, name: str, t: torch.Tensor | None):
    if t is None:
        return
    ops._gpu(t)
    if t.dtype != torch.float32 or t.numel() != g.nnz:
        raise RuntimeError(f"grcn: {name} does not hold one float32 per slot ({g.nnz})")


def attn_fwd(g: EdgeGraph, x: torch.Tensor, alpha: torch.Tensor | None = None):
    """(alpha [nnz] in slot order, rep [n, d]) of rsx_grcn_attn_fwd; `alpha`: the buffer to write."""
    d = _table(g, "x", x)
    alpha = torch.empty(g.nnz, dtype=torch.float32, device=x.device) if alpha is None else alpha
    _edges(g, "alpha", alpha)
    rep = torch.empty_like(x)
    L.check(L.lib().rsx_grcn_attn_fwd(ops._p(x), *g.args(rev=False), d, ops._p(alpha), ops._p(rep), ops._stream()),
            "rsx_grcn_attn_fwd")
    return alpha, rep


def attn_bwd(g: EdgeGraph, g_rep, dalpha_ext, x, alpha):
    """dx [n, d] of rsx_grcn_attn_bwd."""
    d = _table(g, "x", x)
    _table(g, "g_rep", g_rep, d)
    _edges(g, "alpha", alpha)
    _edges(g, "dalpha_ext", dalpha_ext)
    ds = torch.empty(g.nnz, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    L.check(L.lib().rsx_grcn_attn_bwd(ops._p(g_rep), ops._p(dalpha_ext), ops._p(x), ops._p(alpha), *g.args(), d,
                                      ops._p(ds), ops._p(dx), ops._stream()), "rsx_grcn_attn_bwd")
    return dx


def _conf(g: EdgeGraph, alphas, conf):
    M = len(alphas)
    ops._gpu(conf)
    if conf.dtype != torch.float32 or tuple(conf.shape) != (g.n, M):
        raise RuntimeError(f"grcn: conf {tuple(conf.shape)} for {M} modalities over {g.n} nodes")
    for a in alphas:
        _edges(g, "alpha", a)
    return M, ops._p(alphas[0]), ops._p(alphas[1] if M > 1 else None)


def refine_fwd(g: EdgeGraph, alphas, conf):
    """g.val[e] = w_e, g.valT[rev[e]] = w_e (rsx_grcn_refine_fwd); returns g.val."""
    M, a0, a1 = _conf(g, alphas, conf)
    L.check(L.lib().rsx_grcn_refine_fwd(M, a0, a1, ops._p(conf), ops._p(g.col), ops._p(g.rev), g.n, g.nnz,
                                        ops._p(g.val), ops._p(g.valT), ops._stream()), "rsx_grcn_refine_fwd")
    return g.val


def edge_dots(g: EdgeGraph, G, h1, D, x):
    d = _table(g, "G", G)
    for name, t in (("h1", h1), ("D", D), ("x", x)):
        _table(g, name, t, d)
    dw = torch.empty(g.nnz, dtype=torch.float32, device=G.device)
    L.check(L.lib().rsx_grcn_edge_dots(ops._p(G), ops._p(h1), ops._p(D), ops._p(x), ops._p(g.col), ops._p(g.rev), g.n,
                                       g.nnz, d, ops._p(dw), ops._stream()), "rsx_grcn_edge_dots")
    return dw


def refine_bwd(g: EdgeGraph, alphas, conf, dw):
    """(dalphas, dconf) of rsx_grcn_refine_bwd."""
    M, a0, a1 = _conf(g, alphas, conf)
    _edges(g, "dw", dw)
    das = [torch.empty(g.nnz, dtype=torch.float32, device=dw.device) for _ in range(M)]
    dconf = torch.empty_like(conf)
    L.check(L.lib().rsx_grcn_refine_bwd(M, a0, a1, ops._p(conf), ops._p(dw), ops._p(g.rowptr), ops._p(g.rev), g.n,
                                        g.nnz, ops._p(das[0]), ops._p(das[1] if M > 1 else None), ops._p(dconf),
                                        ops._stream()), "rsx_grcn_refine_bwd")
    return das, dconf


def loss_ws_bytes(batch: int, width: int) -> int:
    return int(L.lib().rsx_grcn_loss_ws_bytes(int(batch), int(width)))


def loss_workspace(batch: int, width: int, device) -> torch.Tensor:
    return ops.loss_workspace(L.lib().rsx_grcn_loss_ws_bytes, batch, width, device, unsupported)


def loss_args(id_rep, rep_v, rep_t, E, pv, pt, triplets, n_users: int, reg_weight: float) -> "L.GrcnLossArgs":
    ops._gpu(id_rep, rep_v, rep_t, E, pv, pt, triplets)
    if triplets.dtype != torch.int64 or triplets.dim() != 2 or triplets.shape[0] != 3:
        raise RuntimeError("grcn loss: triplets must be an int64 [3, batch] tensor")
    n, dx = id_rep.shape
    dc = rep_v.shape[1]
    if (rep_t is None) != (pt is None):
        raise RuntimeError("grcn loss: the text table and the text preferences come together")
    for name, t, shape in (("rep_v", rep_v, (n, dc)), ("rep_t", rep_t, (n, dc)), ("E", E, (n, dx)),
                           ("pref_v", pv, (n_users, dc)), ("pref_t", pt, (n_users, dc))):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32):
            raise RuntimeError(f"grcn loss: {name} {tuple(t.shape)}, expected float32 {shape}")
    if id_rep.dtype != torch.float32 or not 0 < n_users < n:
        raise RuntimeError("grcn loss: a float32 id table over users and items")
    a = L.GrcnLossArgs()
    a.id_rep, a.rep_v, a.rep_t = id_rep.data_ptr(), rep_v.data_ptr(), ops._pi(rep_t) or None
    a.E, a.pref_v, a.pref_t, a.triplets = E.data_ptr(), pv.data_ptr(), ops._pi(pt) or None, triplets.data_ptr()
    a.n_users, a.n_items, a.batch = int(n_users), n - int(n_users), triplets.shape[1]
    a.dx, a.dc, a.reg_weight = dx, dc, float(reg_weight)
    return a


def loss_fwd(a, out, result, ws):
    ld = 0
    if result is not None:
        ops._gpu(result)
        if result.dtype != torch.float32 or result.dim() != 2 or result.shape[0] != a.n_users + a.n_items:
            raise RuntimeError("grcn loss: result is not a float32 [n, ld] table")
        ld = result.shape[1]
    L.check(L.lib().rsx_grcn_loss_fwd(C.byref(a), ops._p(out), ops._p(result), ld, ops._p(ws), ws.numel(),
                                      ops._stream()), "rsx_grcn_loss_fwd")


def loss_bwd(a, go, like_id, like_v, like_t, like_pv, ws):
    """(g_id, g_v, g_t | None, gE, gpv, gpt | None) of rsx_grcn_loss_bwd."""
    g_id, gE, g_v, gpv = (torch.empty_like(t) for t in (like_id, like_id, like_v, like_pv))
    g_t = torch.empty_like(like_t) if like_t is not None else None
    gpt = torch.empty_like(like_pv) if like_t is not None else None
    L.check(L.lib().rsx_grcn_loss_bwd(C.byref(a), ops._p(go), ops._p(g_id), ops._p(g_v), ops._p(g_t), ops._p(gE),
                                      ops._p(gpv), ops._p(gpt), ops._p(ws), ws.numel(), ops._stream()),
            "rsx_grcn_loss_bwd")
    return g_id, g_v, g_t, gE, gpv, gpt


def step_forward(g: EdgeGraph, xs, conf, xn):
    """The forward between the normalised inputs and the representation tables: (reps, h1, id_rep);
    the alphas and the edge weights land in g's persistent buffers."""
    reps = [attn_fwd(g, x, g.alpha[k])[1] for k, x in enumerate(xs)]
    refine_fwd(g, g.alpha[:len(xs)], conf)
    d = _table(g, "normalize(E)", xn)
    h1 = g.A.spmm(xn)
    id_rep = torch.empty_like(xn)
    g.A.spmm_epi(h1, ops.epi(L.RSX_EPI_ADD, y=id_rep, s_in=xn, r_add=h1), d)  # x + h1 + A_w h1
    return reps, h1, id_rep


class _Step(torch.autograd.Function):
    """(x_v, x_t | None, conf, normalize(E), E, pref_v, pref_t | None, triplets) -> the loss word.
    cfg = (EdgeGraph, n_users, reg_weight, result | None, ws, keep | None)."""

    @staticmethod
    def forward(ctx, cfg, triplets, x_v, x_t, conf, xn, E, pv, pt):
        g, n_users, reg_weight, result, ws, keep = cfg
        x_v, conf, xn, E, pv, triplets = (t.contiguous() for t in (x_v, conf, xn, E, pv, triplets))
        x_t = None if x_t is None else x_t.contiguous()
        pt = None if pt is None else pt.contiguous()
        xs = [x_v] if x_t is None else [x_v, x_t]
        reps, h1, id_rep = step_forward(g, xs, conf, xn)
        rep_t = reps[1] if len(reps) > 1 else None
        a = loss_args(id_rep, reps[0], rep_t, E, pv, pt, triplets, n_users, reg_weight)
        out = torch.empty(3, dtype=torch.float32, device=E.device)
        loss_fwd(a, out, result, ws)
        ctx.cfg = (g, n_users, reg_weight, ws)  # (no tensor with a grad_fn: persistent buffers only)
        ctx.save_for_backward(triplets, x_v, x_t, conf, xn, E, pv, pt, reps[0], rep_t, h1, id_rep)
        if keep is not None:
            keep["terms"] = out
        return out[0]

    @staticmethod
    def backward(ctx, go):
        g, n_users, reg_weight, ws = ctx.cfg
        triplets, x_v, x_t, conf, xn, E, pv, pt, rep_v, rep_t, h1, id_rep = ctx.saved_tensors
        a = loss_args(id_rep, rep_v, rep_t, E, pv, pt, triplets, n_users, reg_weight)
        G, g_v, g_t, gE, gpv, gpt = loss_bwd(a, go.to(torch.float32).contiguous(), id_rep, rep_v, rep_t, pv, ws)
        # id GCN: D = d h1 = G + A_w^T G, d x = G + A_w^T D, d w_e = <G_t, h1_s> + <D_t, x_s>
        d = xn.shape[1]
        D, dxn = torch.empty_like(G), torch.empty_like(G)
        g.AT.spmm_epi(G, ops.epi(L.RSX_EPI_ADD, y=D, s_in=G), d)
        g.AT.spmm_epi(D, ops.epi(L.RSX_EPI_ADD, y=dxn, s_in=G), d)
        dw = edge_dots(g, G, h1, D, xn)
        M = 1 if x_t is None else 2
        das, dconf = refine_bwd(g, g.alpha[:M], conf, dw)
        dx_v = attn_bwd(g, g_v, das[0], x_v, g.alpha[0])
        dx_t = attn_bwd(g, g_t, das[1], x_t, g.alpha[1]) if M == 2 else None
        return None, None, dx_v, dx_t, dconf, dxn, gE, gpv, gpt


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
class GRCN(GeneralRecommender):
    # calculate_loss has no host syncs and no data-dependent host branches: the Trainer may
    # capture a batch in a HIP graph; no per-epoch buffer rebuilds
    supports_graph_step = True
    graph_step_persistent = True

    @staticmethod
    def check_config(config):
        ops.require_single_gpu(config, unsupported)
        for key in ("embedding_size", "latent_embedding"):
            if config[key] not in SUPPORTED_D:
                raise unsupported(f"{key} {config[key]}: one value of {SUPPORTED_D}")
        n_layers = config["n_layers"]
        if n_layers is None or int(n_layers) < 0:
            raise unsupported(f"n_layers {n_layers}: a routing count >= 0")

    def check_features(self) -> None:
        self.require_features(unsupported, need=1)
        if self.v_feat is None:
            raise unsupported("text features alone: the reference's forward does not run without the image table "
                              "(grcn.py:257 assigns a misspelt name, content_rep stays None)")

    def __init__(self, config, dataset):
        self.check_config(config)
        try:
            super().__init__(config, dataset)
        except AssertionError as e:  # recommender.py: "Features all NONE"
            raise unsupported("no feature file at all") from e
        ops.require_device(self.device)
        self.check_features()
        self.num_user, self.num_item = self.n_users, self.n_items
        self.dim_x, self.dim_C = dx, dc = config["embedding_size"], config["latent_embedding"]
        self.n_layers = int(config["n_layers"])  # routing only re-normalises the preferences: read, not run
        self.aggr_mode, self.weight_mode, self.fusion_mode = "add", "confid", "concat"
        self.reg_weight = float(config["reg_weight"])
        nu, ni, dev = self.n_users, self.n_items, self.device
        self.n_nodes = n = nu + ni
        self.num_modal = M = 1 + (self.t_feat is not None)
        self.width = W = dx + M * dc
        if W > MAX_WIDTH:
            raise unsupported(f"embedding_size {dx} + {M} x latent_embedding {dc} = {W} > {MAX_WIDTH}")
        im = dataset.inter_matrix(form="coo")
        rowptr, col, rev, edge_slot = target_csr(im.row, im.col, nu, ni)
        self.graph = EdgeGraph(rowptr, col, rev, edge_slot, dev, M, int(config["rsx_chunk"] or 32))
        # every draw on the CPU generator in the reference's order, `result` included
        t_dim = None if self.t_feat is None else int(self.t_feat.shape[1])
        self.id_gcn, self.v_gcn, t_gcn, conf, result = grcn_init(nu, ni, dx, dc, int(self.v_feat.shape[1]), t_dim)
        if t_gcn is not None:
            self.t_gcn = t_gcn
        self.model_specific_conf = conf
        self.to(dev)
        # `result` lives in a zero-padded buffer of a width the full sort takes; the loss kernel
        # writes its first `width` columns, the zero columns add exact zeros to the scores
        ld = next(d for d in FULLSORT_D if d >= W)
        self._result = torch.zeros(n, ld, dtype=torch.float32, device=dev)
        self._result[:, :dx] = result.to(dev)
        self._result_w = dx
        B = max(int(config["train_batch_size"] or 1), 1)
        self._ws = loss_workspace(B, W, dev)
        self.last_terms = None  # {total, bpr, reg} of the last calculate_loss (device)

    # ------------------------------------------------------------ persistent state
    @property
    def result(self) -> torch.Tensor:
        """The scored representation, unpadded: [n, dim_x] before any training, then [n, width]."""
        return self._result[:, :self._result_w]

    @property
    def alpha_v(self):
        return self.graph.alpha[0]

    @property
    def alpha_t(self):
        return self.graph.alpha[1] if self.num_modal == 2 else None

    @property
    def edge_weight(self):
        return self.graph.val

    @property
    def edge_slot(self):
        return self.graph.edge_slot

    # --------------------------------------------------------------- forward
    def _inputs(self):
        """(x_v, x_t | None, normalize(E)) with autograd: x = [normalize(pref); normalize(leaky(MLP(feat)))]."""
        xs = []
        for g, feat in ((self.v_gcn, self.v_feat), (getattr(self, "t_gcn", None), self.t_feat)):
            if g is None:
                xs.append(None)
                continue
            f = _Normalize.apply(_Gemm.apply(feat, None, g.MLP.weight, g.MLP.bias, False, True))
            xs.append(torch.cat([_Normalize.apply(g.preference), f], dim=0))
        return xs[0], xs[1], _Normalize.apply(self.id_gcn.id_embedding)

    def _prefs(self):
        return self.v_gcn.preference, (self.t_gcn.preference if self.num_modal == 2 else None)

    def forward(self):
        """The representation [id_rep | rep_v | rep_t] (grcn.py:224-298), without autograd.  Unlike
        the reference's forward it leaves `result` alone: only a training step writes it."""
        with torch.no_grad():
            x_v, x_t, xn = self._inputs()
            reps, _, id_rep = step_forward(self.graph, [x for x in (x_v, x_t) if x is not None],
                                           self.model_specific_conf.contiguous(), xn)
            return torch.cat([id_rep, *reps], dim=1)

    def calculate_loss(self, interaction):
        """interaction: int64 [3, B] on the device."""
        B = interaction.shape[1]
        self._ws = ops.grow_workspace(L.lib().rsx_grcn_loss_ws_bytes, self._ws, B, self.width)
        trip = interaction[:3].contiguous()
        x_v, x_t, xn = self._inputs()
        pv, pt = self._prefs()
        keep = {}
        loss = _Step.apply((self.graph, self.n_users, self.reg_weight, self._result, self._ws, keep), trip, x_v, x_t,
                           self.model_specific_conf, xn, self.id_gcn.id_embedding, pv, pt)
        self._result_w = self.width
        self.last_terms = keep["terms"]
        return loss

    # ------------------------------------------------------------ evaluation
    def full_sort_predict(self, interaction):
        nu = self.n_users
        return ops.score_dense(self._result[:nu], interaction[0].contiguous(), self._result[nu:])

    def full_sort_topk(self, interaction, k, eval_data):
        nu = self.n_users
        return ops.fullsort_topk(self._result[:nu], interaction[0].contiguous(), self._result[nu:],
                                 eval_data.mask_rowptr, eval_data.mask_col, k)
