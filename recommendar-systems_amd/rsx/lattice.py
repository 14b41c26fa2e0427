"""LATTICE on the rsx HIP path — drop-in for the reference's models/lattice.py (ACM MM'21):
an item-item graph learned from the projected features, rebuilt once per epoch, beside a
LightGCN (or plain MF) backbone.

Same class name, constructor `(config, dataloader)`, YAML keys, module names and creation
order (reference src/models/lattice.py:48-94, so `init_seed` gives the reference's initial
weights), forward, loss and scoring (:132-237):

* the UI graph (:100-122): D^-1 (A + I), row-normalised with self loops, float32 as scipy
  computes it (`graph.lattice_norm_adj`); its backward runs on a second CSR of the same
  structure holding the transposed values (`rsx.blocks.ui_backbone` with a transpose
  operand);
* the original graphs (:63-87): rsx_knn_graph's lists on the raw feature tables, always
  built from the features (the reference's dense caches are neither read nor written);
* the learned graph (:137-157): rsx_knn_graph on the projected tables for the top-k columns,
  rsx_lattice_graph for the similarities, the modality mix, the degree normalisation and
  the edge values, rsx_lattice_prop for item_adj^n_layers h and its transpose,
  rsx_lattice_graph_bwd for the build batch's gradient to the projected features and
  modal_weight (csrc/lattice.hip).  The n x n matrices are never formed;
* the loss, forward and backward: rsx_lattice_loss_fwd / _bwd, deterministic;
* evaluation: the graph rebuilt from the current parameters once per eval() session, then the
  fused full-sort on the cached tables.

Only the first calculate_loss after pre_epoch_processing carries gradient into the graph
(:159 detaches it on every other batch): on the other batches image_trs, text_trs, the raw
feature tables and modal_weight have no gradient (None) and Adam skips them, as the
reference's does.

One GPU, embedding_size and feat_embed_dim in (64, 128), cf_model lightgcn or mf; anything
else raises RSX_ERR_UNSUPPORTED at construction (no torch fallback).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import graph, ops
from .blocks import _ego, _join_tables, _RowsOff, ui_backbone
from .dense import _Project
from .recommender import EvalTables, GeneralRecommender

SUPPORTED_D = (64, 128)
MAX_ITEM_LAYERS = 4


def unsupported(what: str) -> RuntimeError:
    return RuntimeError(f"RSX_ERR_UNSUPPORTED: {what} (LATTICE runs on the HIP path only)")


# ---------------------------------------------------------------------------
# the fused loss
# ---------------------------------------------------------------------------
def workspace(batch: int, d: int, device) -> torch.Tensor:
    return ops.loss_workspace(L.lib().rsx_lattice_ws_bytes, batch, d, device, unsupported)


def lattice_args(E, H, triplets, n_users: int, reg: float, batch_size: float) -> "L.LatticeArgs":
    ops._gpu(E, H, triplets)
    if triplets.dtype != torch.int64 or triplets.dim() != 2 or triplets.shape[0] != 3:
        raise RuntimeError("lattice: triplets must be an int64 [3, batch] tensor")
    if H.shape != (E.shape[0] - int(n_users), E.shape[1]) or E.dtype != torch.float32 or H.dtype != torch.float32:
        raise RuntimeError("lattice: E must be f32 [n_users + n_items, d] and H f32 [n_items, d]")
    a = L.LatticeArgs()
    a.E, a.H, a.triplets = E.data_ptr(), H.data_ptr(), triplets.data_ptr()
    a.n_users, a.n_items, a.batch = int(n_users), E.shape[0] - int(n_users), triplets.shape[1]
    a.d, a.reg, a.batch_size = E.shape[1], float(reg), float(batch_size)
    return a


def loss_fwd(args: "L.LatticeArgs", ws: torch.Tensor) -> torch.Tensor:
    """out [3] = total, mf, emb (rsx_lattice_loss_fwd)."""
    out = torch.empty(3, dtype=torch.float32, device=ws.device)
    L.check(L.lib().rsx_lattice_loss_fwd(C.byref(args), ops._p(out), ops._p(ws), ws.numel(), ops._stream()),
            "rsx_lattice_loss_fwd")
    return out


def loss_bwd(args: "L.LatticeArgs", go: torch.Tensor, E, H, ws: torch.Tensor):
    """(gE, gH) of rsx_lattice_loss_bwd: whole tables, zero off the batch rows."""
    gE, gH = torch.empty_like(E), torch.empty_like(H)
    L.check(L.lib().rsx_lattice_loss_bwd(C.byref(args), ops._p(go), ops._p(gE), ops._p(gH), ops._p(ws), ws.numel(),
                                         ops._stream()), "rsx_lattice_loss_bwd")
    return gE, gH


class _LatticeLoss(torch.autograd.Function):
    """The loss on given tables; `cfg` = (n_users, reg, batch_size, ws, terms_out)."""

    @staticmethod
    def forward(ctx, cfg, triplets, E, H):
        n_users, reg, batch_size, ws, keep = cfg
        E, H, triplets = E.contiguous(), H.contiguous(), triplets.contiguous()
        ctx.args = lattice_args(E, H, triplets, n_users, reg, batch_size)
        ctx.ws, ctx.held = ws, (triplets, E, H)  # what the struct points at
        out = loss_fwd(ctx.args, ws)
        if keep is not None:
            keep["terms"] = out
        return out[0]

    @staticmethod
    def backward(ctx, go):
        _, E, H = ctx.held
        gE, gH = loss_bwd(ctx.args, go.to(torch.float32).contiguous(), E, H, ctx.ws)
        return None, None, gE, gH


# ---------------------------------------------------------------------------
# the learned item graph
# ---------------------------------------------------------------------------
def knn_lists(feat: torch.Tensor, k: int):
    """(idx int64 [n, k], weights f32 [n, k]) of rsx_knn_graph on the device: the top-k cosine
    columns of every row (self included) and the sym-normalised values of that graph."""
    x = feat.detach().to(torch.float32).contiguous()
    ops._gpu(x)
    n, f = x.shape
    if k > 32 or k > n or f % 4:
        raise unsupported(f"knn_k {k} with {n} items, feature width {f}")
    return ops.knn_lists(x, k)[1:]


class ItemGraph:
    """item_adj of one build (rsx_lattice_graph): the edge table [n, 2 M k], the per-row
    scalars and the transpose index.  Fs: the projected feature tables (M of them, f32 [n, f]),
    idxs: their kept columns (int64 [n, k]), oidx / oval: the original graphs' lists,
    modal_weight: the raw weights (M = 2) or None.  Everything stays on the device; the
    transpose index is a stable sort of the columns."""

    def __init__(self, Fs, idxs, oidx, oval, modal_weight, lam: float):
        M = len(Fs)
        if M not in (1, 2) or not (len(idxs) == len(oidx) == len(oval) == M):
            raise RuntimeError("lattice: one or two modalities, with their lists")
        n, f = Fs[0].shape
        k = idxs[0].shape[1]
        dev = Fs[0].device
        self.Fs = [t.detach().to(torch.float32).contiguous() for t in Fs]
        self.idx = [t.to(torch.int64).contiguous() for t in idxs]
        self.oidx = [t.to(torch.int64).contiguous() for t in oidx]
        self.oval = [t.to(torch.float32).contiguous() for t in oval]
        self.mw = None if M == 1 else modal_weight.detach().to(torch.float32).contiguous()
        ops._gpu(*self.Fs, *self.idx, *self.oidx, *self.oval, self.mw)
        for t in self.Fs:
            if t.shape != (n, f):
                raise RuntimeError("lattice: the projected tables must share one shape")
        for t in (*self.idx, *self.oidx, *self.oval):
            if t.shape != (n, k):
                raise RuntimeError("lattice: every list is [n_items, knn_k]")
        if f not in SUPPORTED_D or k > 32 or k > n:
            raise unsupported(f"feat_embed_dim {f}, knn_k {k}, {n} items")
        self.n, self.k, self.M, self.f, self.K, self.lam = n, k, M, f, 2 * M * k, float(lam)
        new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)  # noqa: E731
        self.w, self.r, self.dis = new(2), new(n), new(n)
        self.invn = [new(n) for _ in range(M)]
        self.a = [new(n, k) for _ in range(M)]
        self.col, self.val = new(n, self.K, dt=torch.int32), new(n, self.K)
        self.tptr = self.tedge = None
        s = self.struct = L.LatticeGraph()
        s.n, s.k, s.n_mod, s.f, s.lam = n, k, M, f, self.lam
        for m in range(M):
            s.F[m], s.idx[m], s.oidx[m], s.oval[m] = (t[m].data_ptr() for t in (self.Fs, self.idx, self.oidx, self.oval))
            s.invn[m], s.a[m] = self.invn[m].data_ptr(), self.a[m].data_ptr()
        s.modal_weight = None if self.mw is None else self.mw.data_ptr()
        s.w, s.r, s.dis, s.col, s.val = (t.data_ptr() for t in (self.w, self.r, self.dis, self.col, self.val))
        L.check(L.lib().rsx_lattice_graph(C.byref(s), ops._stream()), "rsx_lattice_graph")
        # the transpose index: the edge ids by column, equal columns in edge order
        cols = self.col.reshape(-1).to(torch.int64)
        self.tedge = torch.sort(cols, stable=True)[1].to(torch.int32).contiguous()
        self.tptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        self.tptr[1:] = torch.cumsum(torch.bincount(cols, minlength=n), 0)
        s.tptr, s.tedge = self.tptr.data_ptr(), self.tedge.data_ptr()
        self._ws = None

    def prop(self, x: torch.Tensor, transpose: bool = False) -> torch.Tensor:
        """item_adj x, or item_adj^T x (rsx_lattice_prop)."""
        x = x.contiguous()
        ops._gpu(x)
        if x.dim() != 2 or x.shape[0] != self.n or x.dtype != torch.float32:
            raise RuntimeError(f"lattice: prop needs an f32 [{self.n}, d] table")
        y = torch.empty_like(x)
        L.check(L.lib().rsx_lattice_prop(C.byref(self.struct), ops._p(x), ops._p(y), x.shape[1], int(transpose),
                                         ops._stream()), "rsx_lattice_prop")
        return y

    def backward(self, Gs, Xs):
        """(gradients of the projected tables, gradient of modal_weight or None) from the
        gradient at the output (Gs[l]) and the input (Xs[l]) of every item layer
        (rsx_lattice_graph_bwd)."""
        nl = len(Gs)
        Gs, Xs = [t.contiguous() for t in Gs], [t.contiguous() for t in Xs]
        ops._gpu(*Gs, *Xs)
        d = Gs[0].shape[1]
        for t in (*Gs, *Xs):
            if t.shape != (self.n, d) or t.dtype != torch.float32:
                raise RuntimeError("lattice: the layer tables must be f32 [n_items, d]")
        lib = L.lib()
        if self._ws is None:
            self._ws = torch.empty(max(int(lib.rsx_lattice_graph_bwd_ws_bytes(self.n, self.k, self.M)), 256),
                                   dtype=torch.uint8, device=self.val.device)
        gF = [torch.empty_like(t) for t in self.Fs]
        gmw = torch.empty(2, dtype=torch.float32, device=self.val.device) if self.M == 2 else None
        arr = C.c_void_p * nl
        L.check(lib.rsx_lattice_graph_bwd(C.byref(self.struct), nl, arr(*[t.data_ptr() for t in Gs]),
                                          arr(*[t.data_ptr() for t in Xs]), d, ops._p(gF[0]),
                                          ops._p(gF[1]) if self.M == 2 else None, ops._p(gmw), ops._p(self._ws),
                                          self._ws.numel(), ops._stream()), "rsx_lattice_graph_bwd")
        return gF, gmw


class _ItemProp(torch.autograd.Function):
    """item_adj^n_layers h0 on an ItemGraph.  With `build` the projected tables and
    modal_weight the graph was built from are inputs, and receive the graph's gradient;
    otherwise the graph is a constant."""

    @staticmethod
    def forward(ctx, h0, g, n_layers, build, mw, *Fs):
        xs = [h0.contiguous()]
        for _ in range(n_layers):
            xs.append(g.prop(xs[-1]))
        ctx.g, ctx.xs, ctx.build, ctx.has_mw, ctx.nf = g, xs[:-1], build, mw is not None, len(Fs)
        return xs[-1] if n_layers else xs[-1].clone()

    @staticmethod
    def backward(ctx, gh):
        g, n_layers = ctx.g, len(ctx.xs)
        Gs, cur = [None] * n_layers, gh.contiguous()
        for l in reversed(range(n_layers)):
            Gs[l] = cur
            cur = g.prop(cur, transpose=True)
        gF, gmw = [None] * ctx.nf, None
        if ctx.build and n_layers:
            gF, gmw = g.backward(Gs, ctx.xs)
        return (cur, None, None, None, gmw if ctx.has_mw else None, *gF)


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
class LATTICE(EvalTables, GeneralRecommender):
    # a steady training batch has no host syncs: the Trainer may capture it in a HIP graph.
    # The item graph's buffers change at every build, so the captures are dropped at every
    # epoch start, and the build batch itself runs eagerly (graph_step_eager)
    supports_graph_step = True
    graph_step_persistent = False

    @staticmethod
    def check_config(config):
        ops.require_single_gpu(config, unsupported)
        if config["cf_model"] not in ("lightgcn", "mf"):
            raise unsupported(f"cf_model {config['cf_model']!r} (lightgcn and mf are built)")
        d = config["embedding_size"]
        if d not in SUPPORTED_D:
            raise unsupported(f"embedding_size {d} not in {SUPPORTED_D}")
        f = config["feat_embed_dim"]
        if f not in SUPPORTED_D or not ops.linear_bwd_supported(f, 4):
            raise unsupported(f"feat_embed_dim {f} not in {SUPPORTED_D}")
        if int(config["knn_k"]) > 32 or int(config["knn_k"]) < 1:
            raise unsupported(f"knn_k {config['knn_k']} outside 1..32")
        if not 0 <= int(config["n_layers"]) <= MAX_ITEM_LAYERS:
            raise unsupported(f"n_layers {config['n_layers']} outside 0..{MAX_ITEM_LAYERS}")

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
        self.weight_size = list(config["weight_size"])
        self.knn_k = int(config["knn_k"])
        self.lambda_coeff = float(config["lambda_coeff"])
        self.cf_model = config["cf_model"]
        self.n_layers = int(config["n_layers"])
        self.reg_weight = float(config["reg_weight"])
        self.build_item_graph = True
        nu, ni = self.n_users, self.n_items
        if self.knn_k > ni:
            raise unsupported(f"knn_k {self.knn_k} > n_items {ni}")
        self.n_nodes = nu + ni
        self.n_ui_layers = len(self.weight_size)
        self.chunk = int(config["rsx_chunk"] or 32)
        self.interaction_matrix = im = dataset.inter_matrix(form="coo").astype(np.float32)
        # norm_adj (lattice.py:100-122) and, on the same structure, its transpose's values
        rp, col, val, val_t = graph.lattice_norm_adj(im.row.astype(np.int64), im.col.astype(np.int64), nu, ni)
        self.norm_adj_csr = ops.DeviceCSR(rp, col, val, nu + ni, self.device, self.chunk)
        self.norm_adj_t_csr = ops.DeviceCSR(rp, col, val_t, nu + ni, self.device, self.chunk)
        # parameters in the reference's creation order (identical init under init_seed), drawn
        # on the CPU generator as the reference does
        self.user_embedding = nn.Embedding(nu, d)
        self.item_id_embedding = nn.Embedding(ni, d)
        nn.init.xavier_uniform_(self.user_embedding.weight)
        nn.init.xavier_uniform_(self.item_id_embedding.weight)
        _join_tables(self.user_embedding, self.item_id_embedding, self.device)
        # the original graphs: always from the features (no dense cache is read or written)
        self._orig = {}
        if self.v_feat is not None:
            self.image_embedding = nn.Embedding.from_pretrained(self.v_feat.clone(), freeze=False)
            self._orig["image"] = knn_lists(self.v_feat.to(self.device), self.knn_k)
        if self.t_feat is not None:
            self.text_embedding = nn.Embedding.from_pretrained(self.t_feat.clone(), freeze=False)
            self._orig["text"] = knn_lists(self.t_feat.to(self.device), self.knn_k)
        if self.v_feat is not None:
            self.image_trs = nn.Linear(self.v_feat.shape[1], self.feat_embed_dim)
        if self.t_feat is not None:
            self.text_trs = nn.Linear(self.t_feat.shape[1], self.feat_embed_dim)
        self.modal_weight = nn.Parameter(torch.Tensor([0.5, 0.5]))
        self.softmax = nn.Softmax(dim=0)
        self.mods = [m for m in ("image", "text") if m in self._orig]
        self.item_graph = None  # the ItemGraph of the last training build
        self._ws = workspace(max(int(config["train_batch_size"] or 1), 1), d, self.device)
        self._rows_off = _RowsOff(self.n_users, self.device)
        self._tags = None
        self.last_terms = None  # the loss's three words of the last calculate_loss (device)
        self.to(self.device)

    # ---------------------------------------------------------------- graphs
    def pre_epoch_processing(self):
        self.build_item_graph = True

    def graph_step_eager(self) -> bool:
        """The Trainer's graph step asks this before every batch: the build batch (host-side
        structure work, another autograd graph) runs eagerly."""
        return bool(self.build_item_graph)

    def _projected(self):
        return [_Project.apply(getattr(self, m + "_embedding").weight, getattr(self, m + "_trs").weight,
                               getattr(self, m + "_trs").bias) for m in self.mods]

    def build_graph(self, Fs=None, idxs=None) -> ItemGraph:
        """The ItemGraph of the current parameters (lattice.py:137-157); `idxs` fixes the kept
        columns (tests), else they are rsx_knn_graph's on the projected tables."""
        Fs = self._projected() if Fs is None else Fs
        with torch.no_grad():
            if idxs is None:
                idxs = [knn_lists(f, self.knn_k)[0] for f in Fs]
            return ItemGraph(Fs, idxs, [self._orig[m][0] for m in self.mods], [self._orig[m][1] for m in self.mods],
                             self.modal_weight if len(self.mods) == 2 else None, self.lambda_coeff)

    # --------------------------------------------------------------- forward
    def _backbone(self, rows=None):
        ego = _ego(self.user_embedding.weight, self.item_id_embedding.weight)
        if self.cf_model == "mf":
            return ego
        return ui_backbone(self, ego, self.norm_adj_csr, self.n_ui_layers, rows, AT=self.norm_adj_t_csr)

    def _item_table(self, build: bool):
        h0 = self.item_id_embedding.weight
        if build:
            Fs = self._projected()
            self.item_graph = g = self.build_graph(Fs)
            mw = self.modal_weight if len(self.mods) == 2 else None
            return _ItemProp.apply(h0, g, self.n_layers, True, mw, *Fs)
        return _ItemProp.apply(h0, self.item_graph, self.n_layers, False, None)

    def forward(self, adj=None, build_item_graph=False):
        """(user table, item table + normalize(item_adj^n_layers item_id table))."""
        if not build_item_graph and self.item_graph is None:
            raise RuntimeError("LATTICE.forward: no item graph yet (build_item_graph=True builds one)")
        E = self._backbone()
        H = self._item_table(build_item_graph)
        return E[: self.n_users], E[self.n_users:] + F.normalize(H, p=2, dim=1)

    def calculate_loss(self, interaction):
        B = interaction.shape[1]
        d = self.embedding_dim
        self._ws = ops.grow_workspace(L.lib().rsx_lattice_ws_bytes, self._ws, B, d)
        trip = interaction[:3].contiguous()
        rows = self._rows_off.rows(trip)
        E = self._backbone(rows)
        build, self.build_item_graph = self.build_item_graph or self.item_graph is None, False
        H = self._item_table(build)
        keep = {}
        loss = _LatticeLoss.apply((self.n_users, self.reg_weight, float(self.batch_size), self._ws, keep), trip, E, H)
        self.last_terms = keep["terms"]
        return loss

    # ------------------------------------------------------------ evaluation
    def _eval_tables(self):
        with torch.no_grad():
            g = self.build_graph()
            E = self._backbone()
            H = _ItemProp.apply(self.item_id_embedding.weight, g, self.n_layers, False, None)
            items = E[self.n_users:] + F.normalize(H, p=2, dim=1)
            return E[: self.n_users].contiguous(), items.contiguous()
