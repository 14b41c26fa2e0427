"""MMGCN on the rsx HIP path — drop-in for the reference's models/mmgcn.py (MM'19): per modality
a three-layer GCN on the mean-normalised user-item graph, each layer four chained Linears with
leaky_relu around a neighbourhood mean, the modalities averaged.

Same class name, constructor `(config, dataloader)`, YAML keys, module and parameter names,
creation order and initial draws (reference src/models/mmgcn.py:22-56, 108-162), forward, loss and
scoring (:64-105, :164-188), as the reference really computes them:

* the concatenating branch (`self.concate = 'False'` is a non-empty string): g_layer* are
  Linear(w + d, d) on cat(h, x_hat);
* three layers whatever `n_layers` says (it is read and never used);
* `id_embedding`, each `preference` and `result` are plain tensors, not parameters: never
  trained, never saved.  The text branch's x0 = normalize([preference_t; t_feat]) and A_hat x0 are
  therefore constants (computed once here); the image branch's user rows of x0 are; the
  regulariser has no gradient and is a forward-only word of the loss;
* `full_sort_predict` scores `result`, the representation of the last training forward (one
  optimiser step stale; before any training the random table of :56).

Kernels: layer 1 (width 256 / the text width) and the image MLP on the shared dense blocks
(rsx.dense, csrc/dense.hip): the wide product rsx_dense_gemm, its weight gradients on
rsx_linear_wgrad, bias gradients on rsx_dense_colsum, F.normalize on rsx_dense_normalize_*;
layers 2 and 3 on the fused rsx_mmgcn_layer_fwd / _bwd with rsx_smore_wgrad, the loss, its dense
gradient and `result` on rsx_mmgcn_loss_* (csrc/mmgcn.hip); A_hat x and A_hat^T g on the SpMM
(rsx.blocks._DevGraph).

One GPU; anything the kernels are not built for raises RSX_ERR_UNSUPPORTED at construction.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .blocks import _DevGraph
from .dense import _Gemm, _wgrad, colsum, gemm, normalize_bwd, normalize_fwd
from .recommender import GeneralRecommender

SUPPORTED_D = (64, 128)
LATENT = 256  # the image branch's MLP width (mmgcn.py:47)
SPMM_D = (64, 128, 256)


def unsupported(what: str) -> RuntimeError:
    return RuntimeError(f"RSX_ERR_UNSUPPORTED: {what} (MMGCN runs on the HIP path only)")


# ---------------------------------------------------------------------------
# modules and initial draws
# ---------------------------------------------------------------------------
class BaseModel(nn.Module):
    """The reference's message-passing layer as far as its state goes: `weight` [in, out], applied
    as x @ weight; torch_geometric's inits.uniform draws it before the caller's xavier_normal_."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels))
        bound = 1.0 / math.sqrt(in_channels)
        self.weight.data.uniform_(-bound, bound)


class GCN(nn.Module):
    """One modality's parameters and its constant `preference`, created and drawn in the
    reference's order (mmgcn.py:125-162) on the CPU generator."""

    def __init__(self, num_user: int, dim_feat: int, dim_id: int, dim_latent=None):
        super().__init__()
        w = dim_latent if dim_latent else dim_feat
        self.dim_in = w
        self.preference = nn.init.xavier_normal_(torch.rand((num_user, w), requires_grad=True)).detach()
        if dim_latent:
            self.MLP = nn.Linear(dim_feat, dim_latent)
        self.conv_embed_1 = BaseModel(w, w)
        nn.init.xavier_normal_(self.conv_embed_1.weight)
        self.linear_layer1 = nn.Linear(w, dim_id)
        nn.init.xavier_normal_(self.linear_layer1.weight)
        self.g_layer1 = nn.Linear(w + dim_id, dim_id)
        nn.init.xavier_normal_(self.g_layer1.weight)
        self.conv_embed_2 = BaseModel(dim_id, dim_id)
        nn.init.xavier_normal_(self.conv_embed_2.weight)
        self.linear_layer2 = nn.Linear(dim_id, dim_id)
        nn.init.xavier_normal_(self.linear_layer2.weight)
        self.g_layer2 = nn.Linear(dim_id + dim_id, dim_id)
        self.conv_embed_3 = BaseModel(dim_id, dim_id)
        nn.init.xavier_normal_(self.conv_embed_3.weight)
        self.linear_layer3 = nn.Linear(dim_id, dim_id)
        nn.init.xavier_normal_(self.linear_layer3.weight)
        self.g_layer3 = nn.Linear(dim_id + dim_id, dim_id)

    def layer(self, k: int):
        c, l, g = (getattr(self, f"{s}{k}") for s in ("conv_embed_", "linear_layer", "g_layer"))
        return c.weight, l.weight, l.bias, g.weight, g.bias


def mmgcn_init(n_users: int, n_items: int, d: int, v_dim, t_dim):
    """(v_gcn | None, t_gcn | None, id_embedding, result) on the CPU, every draw in the reference's
    order (mmgcn.py:45-56): the image GCN, the text GCN, then the two random tables."""
    v = GCN(n_users, v_dim, d, LATENT) if v_dim is not None else None
    t = GCN(n_users, t_dim, d) if t_dim is not None else None
    n = n_users + n_items
    id_embedding = nn.init.xavier_normal_(torch.rand((n, d), requires_grad=True)).detach()
    result = nn.init.xavier_normal_(torch.rand((n, d)))
    return v, t, id_embedding, result


def mean_operator(train_u, train_i, n_users: int, n_items: int):
    """(rows, cols, vals) of A_hat = D^-1 A on the n_users + n_items nodes: every training
    interaction in both directions (mmgcn.py:39-42), a repeated one counted with its
    multiplicity, the mean over a node's in-edges; a node without edges has no entry."""
    n = n_users + n_items
    u = np.asarray(train_u, dtype=np.int64)
    i = np.asarray(train_i, dtype=np.int64) + n_users
    key, mult = np.unique(np.concatenate([u * n + i, i * n + u]), return_counts=True)
    rows, cols = key // n, key % n
    deg = np.bincount(rows, weights=mult.astype(np.float64), minlength=n)
    return rows, cols, (mult / deg[rows]).astype(np.float32)


# ---------------------------------------------------------------------------
# kernel wrappers
# ---------------------------------------------------------------------------
# (Every Function below keeps its tensors with save_for_backward, as rsx.dense's do and for its
# reason: nothing with a grad_fn on ctx.)
def layer_fwd(a, x, E, Wc, Wl, bl, Wg, bg):
    ops._gpu(a, x, E, Wc, Wl, bl, Wg, bg)
    n, d = x.shape
    h, u, out = (torch.empty_like(x) for _ in range(3))
    L.check(L.lib().rsx_mmgcn_layer_fwd(*(ops._p(t) for t in (a, x, E, Wc, Wl, bl, Wg, bg)), n, d, ops._p(h),
                                        ops._p(u), ops._p(out), ops._stream()), "rsx_mmgcn_layer_fwd")
    return h, u, out


def layer_bwd(g_out, out, h, u, E, Wc, Wl, Wg):
    """(go, gh, gu, xh, g_a, g_x) of rsx_mmgcn_layer_bwd."""
    ops._gpu(g_out, out, h, u, E, Wc, Wl, Wg)
    n, d = out.shape
    res = tuple(torch.empty_like(out) for _ in range(6))
    L.check(L.lib().rsx_mmgcn_layer_bwd(*(ops._p(t) for t in (g_out, out, h, u, E, Wc, Wl, Wg)), n, d,
                                        *(ops._p(t) for t in res), ops._stream()), "rsx_mmgcn_layer_bwd")
    return res


class _Layer(torch.autograd.Function):
    """One layer of width d on the fused kernels: a = A_hat x (SpMM), the chain in one launch; the
    backward one launch, the weight gradients one rsx_smore_wgrad, g_x = gu Wl + A_hat^T g_a.
    `a` given: the aggregate is the caller's and receives its own gradient (the kernel tests)."""

    @staticmethod
    def forward(ctx, graph, a, x, E, Wc, Wl, bl, Wg, bg):
        x, E, Wc, Wl, bl, Wg, bg = (t.contiguous() for t in (x, E, Wc, Wl, bl, Wg, bg))
        ctx.graph, ctx.own_a = graph, a is None
        a = graph.A.spmm(x) if a is None else a.contiguous()
        h, u, out = layer_fwd(a, x, E, Wc, Wl, bl, Wg, bg)
        ctx.save_for_backward(a, x, E, Wc, Wl, Wg, h, u, out)
        return out

    @staticmethod
    def backward(ctx, g):
        a, x, E, Wc, Wl, Wg, h, u, out = ctx.saved_tensors
        d = x.shape[1]
        go, gh, gu, xh, g_a, g_x = layer_bwd(g.contiguous(), out, h, u, E, Wc, Wl, Wg)
        (dWgh, dbg), (dWgx, _), (dWl, dbl), (dWc, _) = _wgrad(
            [(go, h, True), (go, xh, False), (gu, x, True), (a, gh, False)], d, x.device)
        if ctx.own_a:
            ctx.graph.AT.spmm_epi(g_a, ops.epi(L.RSX_EPI_ADD, y=g_x, s_in=g_x), d)
            g_a = None
        return None, g_a, g_x, None, dWc, dWl, dbl, torch.cat([dWgh, dWgx], dim=1), dbg


class _Layer1(torch.autograd.Function):
    """Layer 1 (width w = 256 or the text width) on the wide product.  x0 [n, w]; `a`: its aggregate
    A_hat x0 when that is a constant of the caller (the text branch), else None: one SpMM here.
    The gradient of x0 (and of a given `a`) is formed only when asked for."""

    @staticmethod
    def forward(ctx, graph, a, x0, E, Wc, Wl, bl, Wg, bg):
        x0, E, Wc, Wl, bl, Wg, bg = (t.contiguous() for t in (x0, E, Wc, Wl, bl, Wg, bg))
        n, w = x0.shape
        d = E.shape[1]
        ctx.graph, ctx.own_a = graph, a is None
        a = graph.A.spmm(x0) if a is None else a.contiguous()
        h = gemm(a, Wc, w, True, act=True)
        u, xh = gemm(x0, Wl, d, False, bias=bl, act=True, r=E)
        out = gemm(h, Wg, d, False, x1=xh, bias=bg, act=True)
        ctx.save_for_backward(a, x0, Wc, Wl, Wg, h, u, xh, out)
        return out

    @staticmethod
    def backward(ctx, g):
        a, x0, Wc, Wl, Wg, h, u, xh, out = ctx.saved_tensors
        n, w = x0.shape
        d = out.shape[1]
        g = g.contiguous()
        go = torch.empty_like(g)
        # [g_h | g_xh] = go Wg, each block masked by its own activation's slope
        gh = gemm(g, Wg, w, True, mx=out, xm_out=go, my=h)
        gu = gemm(go, Wg, d, True, my=u, b_col0=w)
        dWg = torch.cat([ops.linear_wgrad(go, h), ops.linear_wgrad(go, xh)], dim=1)
        dbg = colsum(go)
        dWl, dbl = ops.linear_wgrad(gu, x0), colsum(gu)
        dWc = ops.linear_wgrad(a, gh)  # a^T gh: [in, out] as BaseModel keeps it
        need_a, need_x = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        g_a = g_x = None
        if need_x or need_a:
            g_a = gemm(gh, Wc, w, False)  # gh Wc^T
        if need_x:
            if ctx.own_a:
                g_x = gemm(gu, Wl, w, True, r=ctx.graph.AT.spmm(g_a), y=False)
            else:
                g_x = gemm(gu, Wl, w, True)
        return None, (g_a if need_a and not ctx.own_a else None), g_x, None, dWc, dWl, dbl, dWg, dbg


def loss_args(xv, xt, E, triplets, n_users: int, reg_weight: float, pref_term: float) -> "L.MmgcnLossArgs":
    ops._gpu(xv, xt, E, triplets)
    if triplets.dtype != torch.int64 or triplets.dim() != 2 or triplets.shape[0] != 3:
        raise RuntimeError("mmgcn loss: triplets must be an int64 [3, batch] tensor")
    if any(t is not None and (t.shape != E.shape or t.dtype != torch.float32) for t in (xv, xt)) or (xv is None and xt is None):
        raise RuntimeError("mmgcn loss: f32 modality tables of the id table's shape, at least one")
    a = L.MmgcnLossArgs()
    a.xv, a.xt, a.E, a.triplets = ops._pi(xv) or None, ops._pi(xt) or None, E.data_ptr(), triplets.data_ptr()
    a.n_users, a.n_items, a.batch = int(n_users), E.shape[0] - int(n_users), triplets.shape[1]
    a.d, a.reg_weight, a.pref_term = E.shape[1], float(reg_weight), float(pref_term)
    return a


class _Loss(torch.autograd.Function):
    """{total, bpr, reg} of the batch and the whole-table `result`; cfg = (n_users, reg_weight,
    pref_term, E, result | None, ws, keep | None).  The two modality tables get the same dense
    gradient (one table, handed to both)."""

    @staticmethod
    def forward(ctx, cfg, triplets, xv, xt):
        n_users, reg_weight, pref_term, E, result, ws, keep = cfg
        xv = None if xv is None else xv.contiguous()
        xt = None if xt is None else xt.contiguous()
        triplets = triplets.contiguous()
        ctx.args = loss_args(xv, xt, E, triplets, n_users, reg_weight, pref_term)
        ctx.ws = ws
        ctx.save_for_backward(triplets, xv, xt, E)  # (the argument struct holds their addresses)
        out = torch.empty(3, dtype=torch.float32, device=E.device)
        L.check(L.lib().rsx_mmgcn_loss_fwd(C.byref(ctx.args), ops._p(out), ops._p(result), ops._p(ws), ws.numel(),
                                           ops._stream()), "rsx_mmgcn_loss_fwd")
        if keep is not None:
            keep["terms"] = out
        return out[0]

    @staticmethod
    def backward(ctx, go):
        _, xv, xt, E = ctx.saved_tensors
        g = torch.empty_like(E)
        L.check(L.lib().rsx_mmgcn_loss_bwd(C.byref(ctx.args), ops._p(go.to(torch.float32).contiguous()), ops._p(g),
                                           ops._p(ctx.ws), ctx.ws.numel(), ops._stream()), "rsx_mmgcn_loss_bwd")
        return None, None, (g if xv is not None else None), (g if xt is not None else None)


def loss_workspace(batch: int, d: int, device) -> torch.Tensor:
    return ops.loss_workspace(L.lib().rsx_mmgcn_loss_ws_bytes, batch, d, device, unsupported)


def spmm_wide(A, x: torch.Tensor) -> torch.Tensor:
    """A x for an x whose width the SpMM is not built for: column blocks of 64, zero-padded
    (construction-time work: the text branch's constant aggregate)."""
    n, w = x.shape
    if w in SPMM_D:
        return A.spmm(x.contiguous())
    out = torch.empty(A.n_rows, w, dtype=torch.float32, device=x.device)
    for c0 in range(0, w, 64):
        c1 = min(c0 + 64, w)
        blk = torch.zeros(n, 64, dtype=torch.float32, device=x.device)
        blk[:, : c1 - c0] = x[:, c0:c1]
        out[:, c0:c1] = A.spmm(blk)[:, : c1 - c0]
    return out


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
class MMGCN(GeneralRecommender):
    # calculate_loss has no host syncs and no data-dependent host branches: the Trainer may
    # capture a batch in a HIP graph; no per-epoch buffer rebuilds
    supports_graph_step = True
    graph_step_persistent = True

    @staticmethod
    def check_config(config):
        d = config["embedding_size"]
        if d not in SUPPORTED_D:
            raise unsupported(f"embedding_size {d}: one value of {SUPPORTED_D}")
        ops.require_single_gpu(config, unsupported)

    def check_features(self) -> None:
        """At least one feature table, widths multiples of 4; the text width a multiple of 32 (it is
        layer 1's width: the wide product's columns and rsx_linear_wgrad's rows come in 32s)."""
        self.require_features(unsupported, need=1)
        if self.t_feat is not None and self.t_feat.shape[1] % 32:
            raise unsupported(f"text feature width {self.t_feat.shape[1]} is not a multiple of 32")

    def __init__(self, config, dataset):
        self.check_config(config)
        try:
            super().__init__(config, dataset)
        except AssertionError as e:  # recommender.py: "Features all NONE"
            raise unsupported("no feature file at all") from e
        ops.require_device(self.device)
        self.check_features()
        self.num_user, self.num_item = self.n_users, self.n_items
        self.dim_x = d = config["embedding_size"]
        self.n_layers = config["n_layers"]  # read and, as in the reference, never used: three layers
        self.aggr_mode, self.concate = "mean", "False"
        self.reg_weight = float(config["reg_weight"])
        nu, ni, dev = self.n_users, self.n_items, self.device
        self.n_nodes = n = nu + ni
        chunk = int(config["rsx_chunk"] or 32)
        im = dataset.inter_matrix(form="coo")
        self.graph = _DevGraph(*mean_operator(im.row, im.col, nu, ni), n, n, dev, chunk)
        # every draw on the CPU generator in the reference's order, constants and `result` included
        v_dim = None if self.v_feat is None else int(self.v_feat.shape[1])
        t_dim = None if self.t_feat is None else int(self.t_feat.shape[1])
        v_gcn, t_gcn, id_embedding, result = mmgcn_init(nu, ni, d, v_dim, t_dim)
        self.num_modal = 0
        if v_gcn is not None:
            self.v_gcn = v_gcn
            self.num_modal += 1
        if t_gcn is not None:
            self.t_gcn = t_gcn
            self.num_modal += 1
        self.to(dev)
        self.id_embedding = id_embedding.to(dev).contiguous()
        self.result = result.to(dev).contiguous()  # persistent: the step's own kernel writes it
        self._pref_term = 0.0
        self._x0 = {}  # per modality: the constant rows of x0 (and, for text, the constant aggregate)
        for m, g in (("v", v_gcn), ("t", t_gcn)):
            if g is None:
                continue
            g.preference = g.preference.to(dev).contiguous()
            if m == "v":
                self._pref_term = float(g.preference.double().pow(2).mean().item())
                self._x0[m] = (normalize_fwd(g.preference)[0],)
            else:
                x0, _ = normalize_fwd(torch.cat([g.preference, self.t_feat], dim=0).contiguous())
                self._x0[m] = (x0, spmm_wide(self.graph.A, x0))
        B = max(int(config["train_batch_size"] or 1), 1)
        self._ws = loss_workspace(B, d, dev)
        self.last_terms = None  # {total, bpr, reg} of the last calculate_loss (device)

    # --------------------------------------------------------------- forward
    def _modal(self, m: str):
        """x [n, d] of one modality's three layers, with autograd."""
        E, G = self.id_embedding, self.graph
        if m == "v":
            g = self.v_gcn
            temp = _Gemm.apply(self.v_feat, None, g.MLP.weight, g.MLP.bias, False, False)
            x = _ImageRows.apply(temp, self._x0[m][0])
            x = _Layer1.apply(G, None, x, E, *g.layer(1))
        else:
            g = self.t_gcn
            x0, a0 = self._x0[m]
            x = _Layer1.apply(G, a0, x0, E, *g.layer(1))
        for k in (2, 3):
            x = _Layer.apply(G, None, x, E, *g.layer(k))
        return x

    def forward(self, keep_result: bool = True):
        """The representation (x_v + x_t) / num_modal (mmgcn.py:64-77), without autograd; as the
        reference's forward it becomes `result`."""
        with torch.no_grad():
            xs = [self._modal(m) for m in ("v", "t") if m in self._x0]
            rep = xs[0] if len(xs) == 1 else (xs[0] + xs[1]) / self.num_modal
            if keep_result:
                self.result.copy_(rep)
        return rep

    def calculate_loss(self, interaction):
        """interaction: int64 [3, B] on the device."""
        B, d = interaction.shape[1], self.dim_x
        self._ws = ops.grow_workspace(L.lib().rsx_mmgcn_loss_ws_bytes, self._ws, B, d)
        trip = interaction[:3].contiguous()
        xv = self._modal("v") if "v" in self._x0 else None
        xt = self._modal("t") if "t" in self._x0 else None
        keep = {}
        loss = _Loss.apply((self.n_users, self.reg_weight, self._pref_term, self.id_embedding, self.result, self._ws,
                            keep), trip, xv, xt)
        self.last_terms = keep["terms"]
        return loss

    # ------------------------------------------------------------ evaluation
    def full_sort_predict(self, interaction):
        nu = self.n_users
        return ops.score_dense(self.result[:nu], interaction[0].contiguous(), self.result[nu:])

    def full_sort_topk(self, interaction, k, eval_data):
        nu = self.n_users
        return ops.fullsort_topk(self.result[:nu], interaction[0].contiguous(), self.result[nu:], eval_data.mask_rowptr,
                                 eval_data.mask_col, k)


class _ImageRows(torch.autograd.Function):
    """x0 = [the constant normalised preferences; F.normalize(temp)]: the image branch's input
    table; the gradient of temp from the item rows of the table's gradient."""

    @staticmethod
    def forward(ctx, temp, pref_rows):
        nu, ni = pref_rows.shape[0], temp.shape[0]
        x0 = torch.empty(nu + ni, temp.shape[1], dtype=torch.float32, device=temp.device)
        x0[:nu].copy_(pref_rows)
        _, den = normalize_fwd(temp.contiguous(), out=x0[nu:])
        ctx.n_users = nu
        ctx.save_for_backward(x0, den)
        return x0

    @staticmethod
    def backward(ctx, g):
        x0, den = ctx.saved_tensors
        return normalize_bwd(g.contiguous()[ctx.n_users:], x0[ctx.n_users:], den), None
