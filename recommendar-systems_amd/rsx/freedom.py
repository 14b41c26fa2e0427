"""FREEDOM on the rsx HIP path — drop-in for the reference's models/freedom.py (ACM MM'23):
a frozen item-item graph beside a per-epoch, degree-sensitively pruned user-item graph.

Same class name, constructor `(config, dataloader)`, YAML keys, module names and creation
order (reference src/models/freedom.py:22-77, so `init_seed` gives the reference's initial
weights), forward, loss and scoring (:166-222):

* the evaluation graph: LightGCN's float64 normalisation (rsx_adj_build, ADJ_LIGHTGCN);
* the epoch graph (:130-156): LayerGCN's edge dropout with `torch.multinomial` every epoch,
  on the device (`rsx.layergcn.DeviceEdgeDropout`) or, with rsx_edge_dropout: host, drawn
  by the reference's own CPU call and built by `graph.layergcn_masked_adj`;
* the frozen item graph mm_adj (:64-100): binary top-k graphs per modality, degree
  normalised, mixed by mm_image_weight (`freedom_item_graph`: construction-time host work;
  the neighbour ids from rsx_knn_graph or a CPU top-k);
* the UI backbone on the batch rows (`rsx.blocks.ui_backbone`), the item graph's propagation
  (`_DevGraph`), the whole-table feature projections (`rsx.dense._Project`);
* the three-term BPR loss, forward and backward: rsx_freedom_loss_fwd / _bwd
  (csrc/freedom.hip), deterministic;
* evaluation: the fused full-sort on the cached eval-mode tables.

One GPU, embedding_size = feat_embed_dim in (64, 128); anything else raises
RSX_ERR_UNSUPPORTED at construction (no torch fallback).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import graph, ops
from .blocks import (_DevGraph, _ego, _join_tables, _PropMean, _RowsOff, knn_graph_device,
                     load_reference_knn, ui_backbone)
from .dense import _Project
from .layergcn import DeviceEdgeDropout
from .recommender import EvalTables, GeneralRecommender

SUPPORTED_D = (64, 128)


def unsupported(what: str) -> RuntimeError:
    return RuntimeError(f"RSX_ERR_UNSUPPORTED: {what} (FREEDOM runs on the HIP path only)")


# ---------------------------------------------------------------------------
# the fused loss
# ---------------------------------------------------------------------------
def workspace(batch: int, d: int, device) -> torch.Tensor:
    return ops.loss_workspace(L.lib().rsx_freedom_ws_bytes, batch, d, device, unsupported)


def freedom_args(E, H, T, V, triplets, n_users: int, reg: float) -> "L.FreedomArgs":
    ops._gpu(E, H, T, V, triplets)
    if triplets.dtype != torch.int64 or triplets.dim() != 2 or triplets.shape[0] != 3:
        raise RuntimeError("freedom: triplets must be an int64 [3, batch] tensor")
    a = L.FreedomArgs()
    for k, t in (("E", E), ("H", H), ("T", T), ("V", V), ("triplets", triplets)):
        setattr(a, k, None if t is None else t.data_ptr())
    a.n_users, a.n_items, a.batch = int(n_users), E.shape[0] - int(n_users), triplets.shape[1]
    a.d, a.reg = E.shape[1], float(reg)
    return a


def loss_fwd(args: "L.FreedomArgs", ws: torch.Tensor) -> torch.Tensor:
    """out [4] = total, id, text, image (rsx_freedom_loss_fwd)."""
    out = torch.empty(4, dtype=torch.float32, device=ws.device)
    L.check(L.lib().rsx_freedom_loss_fwd(C.byref(args), ops._p(out), ops._p(ws), ws.numel(), ops._stream()),
            "rsx_freedom_loss_fwd")
    return out


def loss_bwd(args: "L.FreedomArgs", go: torch.Tensor, E, T, V, ws: torch.Tensor):
    """(gE, gT, gV) of rsx_freedom_loss_bwd: whole tables, zero off the batch rows."""
    gE = torch.empty_like(E)
    gT = None if T is None else torch.empty_like(T)
    gV = None if V is None else torch.empty_like(V)
    L.check(L.lib().rsx_freedom_loss_bwd(C.byref(args), ops._p(go), ops._p(gE), ops._p(gT), ops._p(gV), ops._p(ws),
                                         ws.numel(), ops._stream()), "rsx_freedom_loss_bwd")
    return gE, gT, gV


class _FreedomLoss(torch.autograd.Function):
    """The three-term loss on given tables; `cfg` = (n_users, reg, ws, terms_out).  The two
    projection biases enter only to receive their gradient: it is analytically zero (the
    bias is in T[pos] - T[neg] with both signs), and an exact zero tensor (not None, and not
    the rounding noise a column sum of gT would give) keeps Adam's state advancing as the
    reference's without moving the biases."""

    @staticmethod
    def forward(ctx, cfg, triplets, E, H, T, V, bias_t, bias_v):
        n_users, reg, ws, keep = cfg
        E, H = E.contiguous(), (None if H is None else H.contiguous())
        T = None if T is None else T.contiguous()
        V = None if V is None else V.contiguous()
        triplets = triplets.contiguous()
        ctx.args = freedom_args(E, H, T, V, triplets, n_users, reg)
        ctx.n_users, ctx.ws = n_users, ws
        ctx.held = (triplets, E, H, T, V, bias_t, bias_v)  # what the struct points at
        out = loss_fwd(ctx.args, ws)
        if keep is not None:
            keep["terms"] = out
        return out[0]

    @staticmethod
    def backward(ctx, go):
        _, E, H, T, V, bias_t, bias_v = ctx.held
        go = go.to(torch.float32).contiguous()
        gE, gT, gV = loss_bwd(ctx.args, go, E, T, V, ctx.ws)
        zero = lambda b: None if b is None else torch.zeros_like(b)  # noqa: E731
        return None, None, gE, (None if H is None else gE[ctx.n_users:]), gT, gV, zero(bias_t), zero(bias_v)


# ---------------------------------------------------------------------------
# the frozen item graph
# ---------------------------------------------------------------------------
def _topk_host(feat: torch.Tensor, k: int) -> torch.Tensor:
    """Top-k cosine neighbours per row on the CPU, float32 (freedom.py:79-82)."""
    x = feat.detach().cpu().to(torch.float32)
    xn = x.div(torch.norm(x, p=2, dim=-1, keepdim=True))
    n = xn.shape[0]
    step = max(1, (1 << 26) // max(n, 1))
    out = []
    for s in range(0, n, step):
        out.append(torch.topk(torch.mm(xn[s:s + step], xn.t()), k, dim=-1)[1])
    return torch.cat(out)


def _binary_knn_adj(idx: torch.Tensor, n: int) -> torch.Tensor:
    """The degree-normalised binary top-k graph of one modality (freedom.py:86-100):
    value = r_inv[row] * r_inv[col], r_inv = (1e-7 + row count)^-0.5 in float32."""
    k = idx.shape[1]
    rows = torch.arange(n).unsqueeze(1).expand(-1, k).reshape(-1)
    cols = idx.reshape(-1).to(torch.int64)
    row_sum = 1e-7 + torch.bincount(rows, minlength=n)
    r_inv = torch.pow(row_sum, -0.5)
    vals = r_inv[rows] * r_inv[cols]
    return torch.sparse_coo_tensor(torch.stack([rows, cols]), vals, (n, n))


def freedom_item_graph(v_feat, t_feat, k: int, image_weight: float, mode: str = "host"):
    """mm_adj = image_weight * A_image + (1 - image_weight) * A_text over the union of the
    two edge sets, added as torch's coalesce adds them (one modality: its graph).  Returns
    host (rows, cols, vals) in coalesced order.  mode "device": the neighbour ids come from
    rsx_knn_graph (its similarity weights are not used), "host": from a CPU top-k."""
    if mode not in ("device", "host"):
        raise ValueError(f"freedom_item_graph: mode must be 'device' or 'host', got {mode!r}")
    adj = []
    for f in (v_feat, t_feat):
        if f is None:
            adj.append(None)
            continue
        n = f.shape[0]
        if mode == "device":
            idx = torch.from_numpy(knn_graph_device(f, k)[1].reshape(n, k))
        else:
            idx = _topk_host(f, k)
        adj.append(_binary_knn_adj(idx, n))
    if adj[0] is not None and adj[1] is not None:
        mm = image_weight * adj[0] + (1.0 - image_weight) * adj[1]
    else:
        mm = adj[0] if adj[0] is not None else adj[1]
    mm = mm.coalesce()
    i, v = mm.indices().numpy(), mm.values().numpy()
    return i[0].astype(np.int64), i[1].astype(np.int64), v.astype(np.float32)


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
class FREEDOM(EvalTables, GeneralRecommender):
    # a training batch has no host syncs: the Trainer may capture it in a HIP graph.  The
    # epoch graph's buffers change in pre_epoch_processing, so the captures are dropped at
    # every epoch start
    supports_graph_step = True
    graph_step_persistent = False

    @staticmethod
    def check_config(config):
        ops.require_single_gpu(config, unsupported)
        d = config["embedding_size"]
        if d not in SUPPORTED_D:
            raise unsupported(f"embedding_size {d} not in {SUPPORTED_D}")
        if config["feat_embed_dim"] != d:
            raise unsupported(f"feat_embed_dim {config['feat_embed_dim']} != embedding_size {d}")
        if int(config["knn_k"]) > 32:
            raise unsupported(f"knn_k {config['knn_k']} > 32")
        if int(config["n_ui_layers"]) < 1:
            raise unsupported(f"n_ui_layers {config['n_ui_layers']} < 1")
        dr = config["dropout"]
        if isinstance(dr, (int, float)) and dr >= 1.0:
            raise unsupported(f"dropout {dr} >= 1")

    def __init__(self, config, dataset):
        self.check_config(config)
        try:
            super().__init__(config, dataset)
        except AssertionError as e:  # recommender.py: "Features all NONE"
            raise unsupported("no feature file at all") from e
        ops.require_device(self.device)
        self.require_features(unsupported)
        self.embedding_dim = d = config["embedding_size"]
        self.feat_embed_dim = config["feat_embed_dim"]
        self.knn_k = int(config["knn_k"])
        self.lambda_coeff = config["lambda_coeff"]  # read and unused, as in the reference
        self.cf_model = config["cf_model"]
        self.weight_size = config["weight_size"]
        self.n_layers = int(config["n_mm_layers"])
        self.n_ui_layers = int(config["n_ui_layers"])
        self.reg_weight = float(config["reg_weight"])  # the weight of the feature terms
        self.mm_image_weight = float(config["mm_image_weight"])
        self.dropout = float(config["dropout"])
        self.degree_ratio = config["degree_ratio"]
        nu, ni = self.n_users, self.n_items
        self.n_nodes = nu + ni
        self.chunk = int(config["rsx_chunk"] or 32)
        kchunk = int(config["rsx_knn_chunk"] or 64)
        self.interaction_matrix = im = dataset.inter_matrix(form="coo").astype(np.float32)
        # the training edges in canonical (user, item) order, each once: the order the
        # reference's edge ids count in (scipy canonicalises its interaction matrix when the
        # float32 cast changes the dtype), which the per-epoch draw depends on
        key = np.unique(im.row.astype(np.int64) * ni + im.col.astype(np.int64))
        e_u, e_i = key // ni, key % ni
        # norm_adj (freedom.py:102-128: LightGCN's float64 normalisation)
        drp, dcol, dval = ops.adj_build(e_u, e_i, nu, ni, ops.ADJ_LIGHTGCN, self.device)
        self.norm_adj_csr = ops.DeviceCSR.from_device(drp, dcol, dval, nu + ni, self.chunk)
        self.train_adj = self.norm_adj_csr
        # edge info of the per-epoch pruning (freedom.py:147-164), CPU tensors as in the reference
        self.edge_indices = torch.from_numpy(np.vstack([e_u, e_i]))
        self.edge_values = torch.from_numpy(graph.layergcn_edge_values(e_u, e_i, nu, ni))
        mode = config["rsx_edge_dropout"] or config["rsx_sampler"] or "device"
        if mode not in ("device", "host"):
            raise ValueError(f"rsx_edge_dropout must be 'device' or 'host', got {mode!r}")
        self.edge_dropout_mode = mode
        self._dev_dropout = None
        # parameters in the reference's creation order (identical init under init_seed), drawn
        # on the CPU generator as the reference does
        self.user_embedding = nn.Embedding(nu, d)
        self.item_id_embedding = nn.Embedding(ni, d)
        nn.init.xavier_uniform_(self.user_embedding.weight)
        nn.init.xavier_uniform_(self.item_id_embedding.weight)
        _join_tables(self.user_embedding, self.item_id_embedding, self.device)
        if self.v_feat is not None:
            self.image_embedding = nn.Embedding.from_pretrained(self.v_feat.clone(), freeze=False)
            self.image_trs = nn.Linear(self.v_feat.shape[1], self.feat_embed_dim)
        if self.t_feat is not None:
            self.text_embedding = nn.Embedding.from_pretrained(self.t_feat.clone(), freeze=False)
            self.text_trs = nn.Linear(self.t_feat.shape[1], self.feat_embed_dim)
        # the frozen item graph: the reference's own cache when the dataset directory holds
        # one (read by the loader that executes nothing from the file), else built here
        self.knn_mode = config["rsx_knn"] or config["rsx_sampler"] or "device"
        if self.knn_mode not in ("device", "host"):
            raise ValueError(f"rsx_knn must be 'device' or 'host', got {self.knn_mode!r}")
        root = os.path.abspath((config["data_path"] or "") + (config["dataset"] or ""))
        cache = os.path.join(root, "mm_adj_freedomdsp_{}_{}.pt".format(self.knn_k, int(10 * self.mm_image_weight)))
        mm = load_reference_knn(cache, ni)
        if mm is None:
            mm = freedom_item_graph(self.v_feat, self.t_feat, self.knn_k, self.mm_image_weight, self.knn_mode)
        self.mm_adj = _DevGraph(*mm, ni, ni, self.device, kchunk)
        self._ws = workspace(max(int(config["train_batch_size"] or 1), 1), d, self.device)
        self._rows_off = _RowsOff(self.n_users, self.device)
        self._tags = None
        self.last_terms = None  # the loss's four words of the last calculate_loss (device)
        self.to(self.device)

    # ---------------------------------------------------------------- graphs
    def build_epoch_graph(self, keep_ids):
        """The epoch's training graph from the kept edge ids (freedom.py:138-145), float32
        renormalised over the kept edges; public so that tests and tools can fix the set."""
        keep = torch.as_tensor(keep_ids, dtype=torch.int64).cpu()
        kept = self.edge_indices[:, keep].numpy()
        rp, col, val = graph.layergcn_masked_adj(kept[0], kept[1], self.n_users, self.n_items)
        self.train_adj = ops.DeviceCSR(rp, col, val, self.n_nodes, self.device, self.chunk)
        return self.train_adj

    def pre_epoch_processing(self):
        if self.dropout <= 0.0:
            self.train_adj = self.norm_adj_csr
            return
        if self.edge_dropout_mode == "device":
            if self._dev_dropout is None:
                ei = self.edge_indices.numpy()
                self._dev_dropout = DeviceEdgeDropout(ei[0], ei[1], self.n_users, self.n_items,
                                                      self.edge_values.numpy(), self.device, self.chunk)
            self.train_adj = self._dev_dropout.epoch_graph(self.dropout, pruning_random=False)
            return
        # the reference's own draw on the CPU generator: the kept edges are the reference's
        keep_len = int(self.edge_values.size(0) * (1.0 - self.dropout))
        self.build_epoch_graph(torch.multinomial(self.edge_values, keep_len))

    # --------------------------------------------------------------- forward
    def _item_prop(self):
        # n_mm_layers = 0 leaves h the item-id table itself, which the reference still adds
        # to the item rows (freedom.py:167-169,180): H is never absent in the model
        h = self.item_id_embedding.weight
        for _ in range(self.n_layers):
            h = self.mm_adj(h)
        return h

    def forward(self, adj=None):
        """(user rows, item rows + the item graph's table) on `adj` (default: norm_adj)."""
        A = adj if adj is not None else self.norm_adj_csr
        E = _PropMean.apply(_ego(self.user_embedding.weight, self.item_id_embedding.weight), A, self.n_ui_layers)
        return E[: self.n_users], E[self.n_users:] + self._item_prop()

    def _projected(self):
        T = V = bt = bv = None
        if self.t_feat is not None:
            bt = self.text_trs.bias
            T = _Project.apply(self.text_embedding.weight, self.text_trs.weight, bt.detach())
        if self.v_feat is not None:
            bv = self.image_trs.bias
            V = _Project.apply(self.image_embedding.weight, self.image_trs.weight, bv.detach())
        return T, V, bt, bv

    def calculate_loss(self, interaction):
        B = interaction.shape[1]
        d = self.embedding_dim
        self._ws = ops.grow_workspace(L.lib().rsx_freedom_ws_bytes, self._ws, B, d)
        trip = interaction[:3].contiguous()
        rows = self._rows_off.rows(trip)
        ego = _ego(self.user_embedding.weight, self.item_id_embedding.weight)
        E = ui_backbone(self, ego, self.train_adj, self.n_ui_layers, rows)
        H = self._item_prop()
        T, V, bt, bv = self._projected()
        keep = {}
        loss = _FreedomLoss.apply((self.n_users, self.reg_weight, self._ws, keep), trip, E, H, T, V, bt, bv)
        self.last_terms = keep["terms"]
        return loss
