"""DRAGON on the rsx HIP path — drop-in for the reference's models/dragon.py: DualGNN's two
modality GCNs, their representations concatenated, a frozen item-item kNN graph on the item rows
and the user co-occurrence graph on the user rows.

Same class name, constructor `(config, dataloader)`, YAML keys, module and parameter names,
creation order and initial draws (reference src/models/dragon.py:53-156, 344-373), forward, loss
and scoring (:191-285), as the reference really computes them:

* per modality (:375-383), as DualGNN: x = normalize([preference; MLP_1(leaky_relu(MLP(feat)))]),
  x_hat = (A x + x) + A A x on the symmetric D^-1/2 A D^-1/2 over both directions of
  `self.edge_index` (:86-89, 402-409); the dropped-edge lists (:100-138) are built, consume one
  `np.random.choice` draw and are never read; `dim_latent = 64` is hard-coded (:51, :145);
  `features` is `self.v_feat` / `self.t_feat` (:146, :151), not the `image_embedding` /
  `text_embedding` tables;
* both modalities (:231-245): `representation = cat(v_rep, t_rep)` is [n, 128];
  user_rep[u] = [w_u0 v_rep[u] | w_u1 t_rep[u]] with `weight_u` [nu, 2, 1]; item_rep =
  representation[nu:].  One modality: the representation is 64 wide, user_rep its user rows,
  `weight_u` not applied (still regularised);
* the item graph (:248-253): h = mm_adj^L item_rep with L = n_mm_layers, item_rep + h (L = 0: the
  item rows doubled).  mm_adj is FREEDOM's construction (:158-179, `freedom_item_graph`): binary
  top-knn_k cosine graphs of the raw features, (1e-7 + rowcount)^-0.5 on both sides, mixed by
  mm_image_weight; its pattern is not symmetric, the backward runs on the transpose.  The
  reference's cache `mm_adj_{knn_k}.pt` (:61, :70-83) is read when the dataset directory holds it;
* the user graph (:251-252, :327-341): user_rep + sum_j W[u, j] user_rep[idx[u, j]], k = 40,
  softmax weights, resampled every epoch by `topk_sample` (:287-324);
* the loss (:262-277): -mean log2 sigmoid(pos - neg) + reg_weight (mean(pref_v[user]^2) +
  mean(pref_t[user]^2)) + reg_weight mean(weight_u^2); there is no `weight_i` term;
* `result_embed` (:254) is the table of the last TRAINING forward (`result` here: [n, 128] or
  [n, 64]; one optimiser step stale at evaluation; before any training the random float64
  [n, embedding_size] draw of :155-156);
* `MLP_v`, `MLP_t`, `MLP_user` (here Linear(128, 64), :140), `image_embedding`, `image_trs`,
  `text_embedding`, `text_trs` and `weight_i` exist, are drawn, named and saved, and nothing
  reads them: they never get a gradient (None, not zeros) and the optimiser skips them.

The user graph is host work, rsx.dualgnn's (load_user_graph / cached_user_graph / topk_sample /
transposed_lists); the step's kernels are csrc/dragon.hip (rsx_dragon_cat_*, rsx_dragon_ugraph_fwd,
rsx_dragon_loss_*), the MLP and F.normalize are rsx.dense's wide product and normalise; A x, the
item graph and the user graph's backward (the transposed lists as a CSR) run on rsx_spmm.

One GPU; anything the kernels are not built for raises RSX_ERR_UNSUPPORTED at construction.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import ops
from .blocks import _DevGraph, load_reference_knn
from .dense import _Gemm, _Normalize
from .dualgnn import (DIM_LATENT, GCN, K_USER, _csr, _Prop, cached_user_graph, load_user_graph, sym_operator,
                      topk_sample, transposed_lists, ugraph_bwd)
from .freedom import freedom_item_graph
from .recommender import GeneralRecommender

D_CAT = 2 * DIM_LATENT  # the concatenation's width


def unsupported(what: str) -> RuntimeError:
    return RuntimeError(f"RSX_ERR_UNSUPPORTED: {what} (DRAGON runs on the HIP path only)")


# ---------------------------------------------------------------------------
# modules and initial draws
# ---------------------------------------------------------------------------
def dragon_init(host: nn.Module, n_users: int, n_items: int, dim_x: int, feat_embed_dim: int, v_feat, t_feat):
    """Registers the reference's parameters and modules on `host` in its order and with its draws
    on the CPU generators (dragon.py:53-156); returns the float64 draw of result_embed."""
    host.MLP_v = nn.Linear(DIM_LATENT, DIM_LATENT, bias=False)
    host.MLP_t = nn.Linear(DIM_LATENT, DIM_LATENT, bias=False)
    if v_feat is not None:
        host.image_embedding = nn.Embedding.from_pretrained(v_feat, freeze=False)
        host.image_trs = nn.Linear(v_feat.shape[1], feat_embed_dim)
    if t_feat is not None:
        host.text_embedding = nn.Embedding.from_pretrained(t_feat, freeze=False)
        host.text_trs = nn.Linear(t_feat.shape[1], feat_embed_dim)
    host.weight_u = nn.Parameter(nn.init.xavier_normal_(
        torch.tensor(np.random.randn(n_users, 2, 1), dtype=torch.float32)))
    host.weight_u.data = F.softmax(host.weight_u.data, dim=1)
    host.weight_i = nn.Parameter(nn.init.xavier_normal_(
        torch.tensor(np.random.randn(n_items, 2, 1), dtype=torch.float32)))
    host.weight_i.data = F.softmax(host.weight_i.data, dim=1)
    # the dropped-edge machinery (:100-138) is never read; its one draw is consumed
    np.random.choice(n_items, int(n_items * 0.1), replace=False)
    host.MLP_user = nn.Linear(DIM_LATENT * 2, DIM_LATENT)
    if v_feat is not None:
        host.v_gcn = GCN(n_users, int(v_feat.shape[1]))
    if t_feat is not None:
        host.t_gcn = GCN(n_users, int(t_feat.shape[1]))
    return nn.init.xavier_normal_(torch.tensor(np.random.randn(n_users + n_items, dim_x)))


# ---------------------------------------------------------------------------
# kernel wrappers
# ---------------------------------------------------------------------------
def cat_fwd(xv, xt, weight_u, n_users: int):
    """(user_rep [nu, 128], item_rep [ni, 128]) of the two modality tables [n, 64]."""
    ops._gpu(xv, xt, weight_u)
    n, d = xv.shape
    if xt.shape != xv.shape or d != DIM_LATENT or weight_u.numel() != 2 * n_users:
        raise RuntimeError("dragon cat: two [n, 64] tables and weight_u [nu, 2, 1] expected")
    user_rep = torch.empty(n_users, D_CAT, dtype=torch.float32, device=xv.device)
    item_rep = torch.empty(n - n_users, D_CAT, dtype=torch.float32, device=xv.device)
    L.check(L.lib().rsx_dragon_cat_fwd(ops._p(xv), ops._p(xt), ops._p(weight_u), n_users, n - n_users, ops._p(user_rep),
                                       ops._p(item_rep), ops._stream()), "rsx_dragon_cat_fwd")
    return user_rep, item_rep


def cat_bwd(g_user_rep, g_item_rep, xv, xt, weight_u, n_users: int):
    """(g_v [n, 64], g_t [n, 64], g_weight_u [nu, 2, 1]: the two row dots, without the regulariser)."""
    ops._gpu(g_user_rep, g_item_rep, xv, xt, weight_u)
    n = xv.shape[0]
    if g_user_rep.shape != (n_users, D_CAT) or g_item_rep.shape != (n - n_users, D_CAT) or xt.shape != xv.shape:
        raise RuntimeError("dragon cat: g_user_rep [nu, 128] and g_item_rep [ni, 128] expected")
    g_v, g_t = torch.empty_like(xv), torch.empty_like(xt)
    g_w = torch.empty_like(weight_u)
    L.check(L.lib().rsx_dragon_cat_bwd(ops._p(g_user_rep), ops._p(g_item_rep), ops._p(xv), ops._p(xt), ops._p(weight_u),
                                       n_users, n - n_users, ops._p(g_v), ops._p(g_t), ops._p(g_w), ops._stream()),
            "rsx_dragon_cat_bwd")
    return g_v, g_t, g_w


def ugraph_fwd(user_rep, idx, W, out=None):
    """out[u] = user_rep[u] + sum_j W[u, j] user_rep[idx[u, j]], 64 or 128 wide; `out`: the first
    nu rows of it are written."""
    ops._gpu(user_rep, idx, W, out)
    nu, d = user_rep.shape
    if idx.dtype != torch.int32 or W.dtype != torch.float32 or idx.shape != W.shape or idx.dim() != 2 or idx.shape[0] != nu:
        raise RuntimeError("dragon ugraph: idx int32 [nu, k] and W float32 [nu, k] expected")
    if out is None:
        out = torch.empty_like(user_rep)
    elif out.shape[0] < nu or out.shape[1] != d or out.data_ptr() == user_rep.data_ptr():
        raise RuntimeError("dragon ugraph: out must hold nu rows and must not be user_rep")
    L.check(L.lib().rsx_dragon_ugraph_fwd(ops._p(user_rep), ops._p(idx), ops._p(W), nu, idx.shape[1], d, ops._p(out),
                                          ops._stream()), "rsx_dragon_ugraph_fwd")
    return out


def graph_residual(A, x, layers: int, out=None):
    """out = x + A^layers x (dragon.py:248-253; its backward with A the transposed operator): the
    inner products stored, the last one summed with x in the SpMM's ADD epilogue, written
    straight into `out`.  layers = 0: x + x."""
    d = x.shape[1]
    if out is None:
        out = torch.empty_like(x)
    if layers == 0:
        return torch.add(x, x, out=out)
    h = x
    for _ in range(layers - 1):
        h = A.spmm(h)
    A.spmm_epi(h, ops.epi(L.RSX_EPI_ADD, y=out, s_in=x), d)
    return out


def loss_args(result, pref_v, pref_t, weight_u, triplets, n_users: int, reg_weight: float):
    ops._gpu(result, pref_v, pref_t, weight_u, triplets)
    if triplets.dtype != torch.int64 or triplets.dim() != 2 or triplets.shape[0] != 3:
        raise RuntimeError("dragon loss: triplets must be an int64 [3, batch] tensor")
    if pref_v is None and pref_t is None:
        raise RuntimeError("dragon loss: at least one preference table")
    a = L.DragonLossArgs()
    a.result, a.pref_v, a.pref_t = result.data_ptr(), ops._pi(pref_v) or None, ops._pi(pref_t) or None
    a.weight_u, a.triplets = weight_u.data_ptr(), triplets.data_ptr()
    a.n_users, a.n_items, a.batch = int(n_users), result.shape[0] - int(n_users), triplets.shape[1]
    a.d, a.reg_weight = result.shape[1], float(reg_weight)
    return a


def loss_fwd(a, ws):
    """out [3] = total, bpr, reg."""
    out = torch.empty(3, dtype=torch.float32, device=ws.device)
    L.check(L.lib().rsx_dragon_loss_fwd(C.byref(a), ops._p(out), ops._p(ws), ws.numel(), ops._stream()),
            "rsx_dragon_loss_fwd")
    return out


def loss_bwd(a, go, ws, pref_v, pref_t, weight_u):
    """(g_result [n, d], g_pref_v | None, g_pref_t | None, g_weight_u: the regulariser's)."""
    n, d = a.n_users + a.n_items, a.d
    g = torch.empty(n, d, dtype=torch.float32, device=ws.device)
    gpv = None if pref_v is None else torch.empty_like(pref_v)
    gpt = None if pref_t is None else torch.empty_like(pref_t)
    gwu = torch.empty_like(weight_u)
    L.check(L.lib().rsx_dragon_loss_bwd(C.byref(a), ops._p(go), ops._p(g), ops._p(gpv), ops._p(gpt), ops._p(gwu),
                                        ops._p(ws), ws.numel(), ops._stream()), "rsx_dragon_loss_bwd")
    return g, gpv, gpt, gwu


def loss_workspace(batch: int, d: int, device) -> torch.Tensor:
    return ops.loss_workspace(L.lib().rsx_dragon_loss_ws_bytes, batch, d, device, unsupported)


def representation(xv, xt, weight_u, n_users: int, mm_adj, layers: int, idx, W, result):
    """The forward past the modality tables, written into `result` [n, 128] (both tables) or
    [n, 64] (one); returns (user_rep, item_rep)."""
    if xv is not None and xt is not None:
        user_rep, item_rep = cat_fwd(xv, xt, weight_u, n_users)
    else:
        x = xv if xv is not None else xt
        user_rep, item_rep = x[:n_users], x[n_users:]
    graph_residual(mm_adj.A, item_rep, layers, out=result[n_users:])
    ugraph_fwd(user_rep, idx, W, out=result)
    return user_rep, item_rep


class _Tail(torch.autograd.Function):
    """The step from the modality tables to the loss word: cat, item graph, user graph, loss, and
    `result`.  cfg = (n_users, reg_weight, result, mm_adj, layers, idx, W, PT, ws, keep | None).
    One differentiable output; every tensor is kept with save_for_backward."""

    @staticmethod
    def forward(ctx, cfg, triplets, xv, xt, weight_u, pref_v, pref_t):
        n_users, reg_weight, result, mm_adj, layers, idx, W, PT, ws, keep = cfg
        xv, xt, pref_v, pref_t = (None if t is None else t.contiguous() for t in (xv, xt, pref_v, pref_t))
        weight_u, triplets = weight_u.contiguous(), triplets.contiguous()
        user_rep, _ = representation(xv, xt, weight_u, n_users, mm_adj, layers, idx, W, result)
        ctx.args = loss_args(result, pref_v, pref_t, weight_u, triplets, n_users, reg_weight)
        ctx.cfg = (n_users, mm_adj, layers, PT, ws)
        ctx.save_for_backward(triplets, xv, xt, weight_u, pref_v, pref_t, result)
        out = loss_fwd(ctx.args, ws)
        if keep is not None:
            keep["terms"], keep["user_rep"] = out, user_rep
        return out[0]

    @staticmethod
    def backward(ctx, go):
        _, xv, xt, weight_u, pref_v, pref_t, _ = ctx.saved_tensors
        n_users, mm_adj, layers, PT, ws = ctx.cfg
        go = go.to(torch.float32).contiguous()
        g_result, gpv, gpt, gwu = loss_bwd(ctx.args, go, ws, pref_v, pref_t, weight_u)
        if xv is not None and xt is not None:
            g_user_rep = ugraph_bwd(PT, g_result, n_users)
            g_item_rep = graph_residual(mm_adj.AT, g_result[n_users:], layers)
            g_v, g_t, g_dots = cat_bwd(g_user_rep, g_item_rep, xv, xt, weight_u, n_users)
            return None, None, g_v, g_t, gwu + g_dots, gpv, gpt
        # one modality: the two row blocks of the table's gradient, written in place
        g = torch.empty_like(g_result)
        PT.spmm_epi(g_result, ops.epi(L.RSX_EPI_ADD, y=g, s_in=g_result), g.shape[1])
        graph_residual(mm_adj.AT, g_result[n_users:], layers, out=g[n_users:])
        return None, None, (g if xv is not None else None), (g if xt is not None else None), gwu, gpv, gpt


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
class DRAGON(GeneralRecommender):
    # calculate_loss has no host syncs and no data-dependent host branches: the Trainer may
    # capture a batch in a HIP graph.  pre_epoch_processing rebuilds the transposed lists' CSR
    # (its SpMM schedule follows the epoch's in-degrees and has no fixed size), so the captures
    # are dropped at every epoch start, as DualGNN's are
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
        if int(config["knn_k"]) > 32:
            raise unsupported(f"knn_k {config['knn_k']} > 32")
        if int(config["n_mm_layers"]) < 0:
            raise unsupported(f"n_mm_layers {config['n_mm_layers']} < 0")
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
        self.dim_latent = DIM_LATENT
        self.feat_embed_dim = int(config["feat_embed_dim"])
        self.n_layers = int(config["n_mm_layers"])  # the item graph's layers (dragon.py:29)
        self.knn_k = int(config["knn_k"])
        self.mm_image_weight = float(config["mm_image_weight"])
        self.k, self.num_layer = K_USER, 1
        self.aggr_mode, self.user_aggr_mode, self.construction = config["aggr_mode"], "softmax", "cat"
        self.reg_weight = float(config["reg_weight"])
        self.drop_rate = 0.1
        nu, ni, dev = self.n_users, self.n_items, self.device
        self.n_nodes = n = nu + ni
        self.chunk = int(config["rsx_chunk"] or 32)
        kchunk = int(config["rsx_knn_chunk"] or 64)
        if self.knn_k > ni:
            raise unsupported(f"knn_k {self.knn_k} > {ni} items")
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
        # the frozen item graph: the reference's own cache when the dataset directory holds one
        # (read by the loader that executes nothing from the file), else built here
        self.knn_mode = config["rsx_knn"] or config["rsx_sampler"] or "device"
        if self.knn_mode not in ("device", "host"):
            raise ValueError(f"rsx_knn must be 'device' or 'host', got {self.knn_mode!r}")
        mm = load_reference_knn(os.path.join(root, "mm_adj_{}.pt".format(self.knn_k)), ni)
        self.mm_adj_source = "file"
        if mm is None:
            mm = freedom_item_graph(self.v_feat, self.t_feat, self.knn_k, self.mm_image_weight, self.knn_mode)
            self.mm_adj_source = "built"
        self.mm_adj = _DevGraph(*mm, ni, ni, dev, kchunk)
        # every draw on the CPU generators in the reference's order, `result_embed` included
        cpu = lambda f: None if f is None else f.cpu()  # noqa: E731
        result = dragon_init(self, nu, ni, int(config["embedding_size"]), self.feat_embed_dim, cpu(self.v_feat),
                             cpu(self.t_feat))
        self.to(dev)
        both = self.v_feat is not None and self.t_feat is not None
        self.width = D_CAT if both else DIM_LATENT  # of the representation once a forward has run
        self.result = result.to(torch.float32).to(dev).contiguous()  # replaced by the first forward's table
        self._table = torch.empty(n, self.width, dtype=torch.float32, device=dev)  # persistent: the step's kernels write it
        self.epoch_idx = self.epoch_W = self.PT = None
        B = max(int(config["train_batch_size"] or 1), 1)
        self._ws = loss_workspace(B, self.width, dev)
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
        """x_hat [n, 64] of one modality (dragon.py:375-383), with autograd."""
        hid = _Gemm.apply(feat, None, g.MLP.weight, g.MLP.bias, False, True)
        temp = _Gemm.apply(hid, None, g.MLP_1.weight, g.MLP_1.bias, False, False)
        x = _Normalize.apply(torch.cat([g.preference, temp], dim=0))
        return _Prop.apply(x, self.A)

    def _sampled(self):
        if self.PT is None:
            raise RuntimeError("DRAGON: pre_epoch_processing() has not sampled the user graph yet")

    def _step(self, trip, keep):
        self._sampled()
        xs = {m: self._modal(g, f) for m, g, f in self._mods()}
        prefs = {m: g.preference for m, g, _ in self._mods()}
        cfg = (self.n_users, self.reg_weight, self._table, self.mm_adj, self.n_layers, self.epoch_idx, self.epoch_W,
               self.PT, self._ws, keep)
        loss = _Tail.apply(cfg, trip, xs.get("v"), xs.get("t"), self.weight_u, prefs.get("v"), prefs.get("t"))
        self.result = self._table
        return loss, xs

    def forward(self, interaction=None):
        """The representation [user_rep + its user graph's sum; item_rep + mm_adj^L item_rep]
        (dragon.py:191-254), without autograd; as the reference's forward it becomes `result`."""
        with torch.no_grad():
            self._sampled()
            xs = {m: self._modal(g, f).contiguous() for m, g, f in self._mods()}
            user_rep, _ = representation(xs.get("v"), xs.get("t"), self.weight_u.contiguous(), self.n_users, self.mm_adj,
                                         self.n_layers, self.epoch_idx, self.epoch_W, self._table)
            self.last_user_rep = user_rep
            self.result = self._table
        return self.result

    def calculate_loss(self, interaction):
        """interaction: int64 [3, B] on the device."""
        B = interaction.shape[1]
        self._ws = ops.grow_workspace(L.lib().rsx_dragon_loss_ws_bytes, self._ws, B, self.width)
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
