"""BM3 on the rsx HIP path — drop-in for the reference's models/bm3.py (WWW'23).

Same class name, constructor `(config, dataloader)`, YAML keys (embedding_size, n_layers,
reg_weight, cl_weight, dropout), parameter names, creation order and initial draws
(reference src/models/bm3.py:23-56), forward, loss and scoring (:86-156).  BM3 trains
without negatives (`use_neg_sampling: False`: the loader yields [2, B] pairs) against a
dropped-out, gradient-stopped copy of its own embeddings:

* the mean-of-layers propagation of [U; I] and its backward: `rsx.blocks._PropMean` (the
  dense variant: the regulariser's gradient touches every row), the two tables adjacent in
  one buffer so that the ego table is that buffer (`_ego`);
* the text / image projections over the whole feature tables: `rsx_linear_rows_fwd`
  forward, `rsx_linear_bwd` (dX, dW, db in one pass) backward;
* predictor, the four dropout streams, the six cosine terms and the Frobenius regulariser,
  forward and backward: `rsx_bm3_loss_fwd` / `rsx_bm3_loss_bwd` (csrc/bm3.hip);
* evaluation: the predictor on both whole tables (`rsx_linear_rows_fwd`), then the fused
  full-sort.

The dropout masks are a hash of (seed, stream, table row, column); the seed word lives on
the device and advances once per training forward, so a captured step replays with fresh
masks.  No torch fallback: an unsupported configuration raises RSX_ERR_UNSUPPORTED at
construction.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .blocks import _ego, _join_tables, _PropMean
from .dense import _Project
from .recommender import GeneralRecommender

SUPPORTED_D = (32, 64, 128)
STREAMS = ("user", "item", "text", "image")


def unsupported(what: str) -> RuntimeError:
    return RuntimeError(f"RSX_ERR_UNSUPPORTED: {what} (BM3 runs on the HIP path only)")


def bm3_init(n_users: int, n_items: int, d: int, image_dim: int | None, text_dim: int | None):
    """BM3's initial parameters by the reference's torch calls in its order on the CPU
    generator (bm3.py:39-56): two nn.Embedding (their normal_ draws, then xavier_uniform_),
    the predictor nn.Linear (kaiming / bias draws, then xavier_normal_ on the weight), then
    per modality, image first, an nn.Linear the same way (from_pretrained draws nothing).
    Returns dict name -> tensor (the raw feature tables are not in it)."""
    ue, ie = nn.Embedding(n_users, d), nn.Embedding(n_items, d)
    nn.init.xavier_uniform_(ue.weight)
    nn.init.xavier_uniform_(ie.weight)
    pred = nn.Linear(d, d)
    nn.init.xavier_normal_(pred.weight)
    out = {"user_embedding.weight": ue.weight.data, "item_id_embedding.weight": ie.weight.data,
           "predictor.weight": pred.weight.data, "predictor.bias": pred.bias.data}
    for name, dim in (("image", image_dim), ("text", text_dim)):
        if dim is not None:
            lin = nn.Linear(dim, d)
            nn.init.xavier_normal_(lin.weight)
            out[name + "_trs.weight"], out[name + "_trs.bias"] = lin.weight.data, lin.bias.data
    return out


def bm3_args(E, H, T, V, P, pb, users, items, n_users, reg_weight, cl_weight, p_drop, seed, masks, ws) -> "L.Bm3Args":
    """The rsx_bm3_args of one call; `masks`: dict stream -> uint32 [rows, d / 32] device
    tensor, or None."""
    ops._gpu(E, H, T, V, P, pb, users, items, seed, ws)
    if users.dtype != torch.int64 or items.dtype != torch.int64 or users.numel() != items.numel():
        raise RuntimeError("bm3: users / items must be int64 tensors of one length")
    a = L.Bm3Args()
    a.n_users, a.n_items, a.d = int(n_users), E.shape[0] - int(n_users), E.shape[1]
    for k, t in (("E", E), ("H", H), ("T", T), ("V", V), ("P", P), ("pb", pb), ("users", users), ("items", items),
                 ("seed", seed), ("ws", ws)):
        setattr(a, k, None if t is None else t.data_ptr())
    a.batch = users.numel()
    a.reg_weight, a.cl_weight, a.p_drop = float(reg_weight), float(cl_weight), float(p_drop)
    for s, name in enumerate(STREAMS):
        m = (masks or {}).get(name)
        if m is not None:
            rows = a.n_users if name == "user" else a.n_items
            if m.dtype not in (torch.int32, torch.uint32) or tuple(m.shape) != (rows, a.d // 32):
                raise RuntimeError(f"bm3: the {name} keep mask must be 32-bit words [{rows}, {a.d // 32}]")
            ops._gpu(m)
            a.mask[s] = m.data_ptr()
    a.ws_bytes = ws.numel()
    return a


def loss_fwd(args: "L.Bm3Args", device) -> torch.Tensor:
    """out [8] = total, ui, iu, t, v, tv, vt, reg (rsx_bm3_loss_fwd)."""
    out = torch.empty(8, dtype=torch.float32, device=device)
    L.check(L.lib().rsx_bm3_loss_fwd(C.byref(args), ops._p(out), ops._stream()), "rsx_bm3_loss_fwd")
    return out


def targets(args: "L.Bm3Args", device) -> torch.Tensor:
    """[S B, d] dropout targets of the batch, stacked by stream (rsx_bm3_targets)."""
    S = 2 + (args.T is not None) + (args.V is not None)
    out = torch.empty(S * args.batch, args.d, dtype=torch.float32, device=device)
    L.check(L.lib().rsx_bm3_targets(C.byref(args), ops._p(out), ops._stream()), "rsx_bm3_targets")
    return out


def loss_bwd(args: "L.Bm3Args", go: torch.Tensor, E, T, V, P):
    """(gE, gT, gV, gP, gpb) of rsx_bm3_loss_bwd after loss_fwd with the same args."""
    gE = torch.empty_like(E)
    gT = None if T is None else torch.empty_like(T)
    gV = None if V is None else torch.empty_like(V)
    gP = torch.empty_like(P)
    gpb = torch.empty(P.shape[0], dtype=torch.float32, device=P.device)
    L.check(L.lib().rsx_bm3_loss_bwd(C.byref(args), ops._p(go), ops._p(gE), ops._p(gT), ops._p(gV), ops._p(gP),
                                     ops._p(gpb), ops._stream()), "rsx_bm3_loss_bwd")
    return gE, gT, gV, gP, gpb


def workspace(batch: int, d: int, device) -> torch.Tensor:
    return ops.loss_workspace(L.lib().rsx_bm3_ws_bytes, batch, d, device, unsupported)


class _Bm3Loss(torch.autograd.Function):
    """The bootstrap loss on given tables; `cfg` = (n_users, reg_weight, cl_weight, p_drop,
    seed, masks, ws, terms_out).  The kernels keep the batch's online and predicted rows in
    `ws` between forward and backward."""

    @staticmethod
    def forward(ctx, cfg, users, items, E, H, P, pb, T, V):
        n_users, reg_weight, cl_weight, p_drop, seed, masks, ws, keep = cfg
        E, H, P, pb = (t.contiguous() for t in (E, H, P, pb))
        T = None if T is None else T.contiguous()
        V = None if V is None else V.contiguous()
        users, items = users.contiguous(), items.contiguous()
        ctx.args = bm3_args(E, H, T, V, P, pb, users, items, n_users, reg_weight, cl_weight, p_drop, seed, masks, ws)
        ctx.n_users = n_users
        ctx.held = (users, items, E, H, P, pb, T, V, seed, masks, ws)  # what the struct points at
        out = loss_fwd(ctx.args, E.device)
        if keep is not None:
            keep["terms"] = out
        return out[0]

    @staticmethod
    def backward(ctx, go):
        _, _, E, _, P, _, T, V, *_ = ctx.held
        go = go.to(torch.float32).contiguous()
        gE, gT, gV, gP, gpb = loss_bwd(ctx.args, go, E, T, V, P)
        return None, None, None, gE, gE[ctx.n_users:], gP, gpb, gT, gV


class BM3(GeneralRecommender):
    # calculate_loss has no host syncs and no data-dependent host branches: the Trainer may
    # capture a batch in a HIP graph (rsx.trainer._GraphStep); no per-epoch buffer rebuilds
    supports_graph_step = True
    graph_step_persistent = True

    @staticmethod
    def check_config(config):
        ops.require_single_gpu(config, unsupported)
        if config["embedding_size"] not in SUPPORTED_D:
            raise unsupported(f"embedding_size {config['embedding_size']} not in {SUPPORTED_D}")

    def __init__(self, config, dataset):
        self.check_config(config)
        super().__init__(config, dataset)
        ops.require_device(self.device)
        self.embedding_dim = self.feat_embed_dim = d = config["embedding_size"]
        self.n_layers = int(config["n_layers"])
        self.reg_weight = float(config["reg_weight"])
        self.cl_weight = float(config["cl_weight"])
        self.dropout = float(config["dropout"])
        if not 0.0 <= self.dropout < 1.0:
            raise unsupported(f"dropout {self.dropout} outside [0, 1)")
        self.require_features(unsupported, need=0, vision="vision")
        self.n_nodes = nu_ni = self.n_users + self.n_items
        nu, ni = self.n_users, self.n_items
        # parameters in the reference's creation order (identical init under init_seed), drawn
        # on the CPU generator as the reference does
        init = bm3_init(nu, ni, d, None if self.v_feat is None else int(self.v_feat.shape[1]),
                        None if self.t_feat is None else int(self.t_feat.shape[1]))
        dev = self.device
        # the two tables as adjacent row blocks of one device buffer: the propagation's ego
        # table [U; I] is that buffer itself (rsx.blocks._ego), no per-forward concatenation
        self.user_embedding = nn.Embedding(nu, d, _weight=init["user_embedding.weight"])
        self.item_id_embedding = nn.Embedding(ni, d, _weight=init["item_id_embedding.weight"])
        _join_tables(self.user_embedding, self.item_id_embedding, dev)
        self.predictor = nn.Linear(d, d)
        for name, f in (("image", self.v_feat), ("text", self.t_feat)):
            if f is not None:
                setattr(self, name + "_embedding", nn.Embedding.from_pretrained(f.clone(), freeze=False))
                setattr(self, name + "_trs", nn.Linear(int(f.shape[1]), d))
        self.to(dev)
        with torch.no_grad():
            for n, p in self.named_parameters():
                if n in init and not n.endswith("embedding.weight"):
                    p.copy_(init[n])
        # the normalised graph of bm3.py:58-84: lightgcn.py's Laplacian (float64 (deg + 1e-7)^-1/2)
        im = dataset.inter_matrix(form="coo")
        chunk = int(config["rsx_chunk"] or 32)
        rp, col, val = ops.adj_build(im.row.astype(np.int64), im.col.astype(np.int64), nu, ni, ops.ADJ_LIGHTGCN, dev)
        self.norm_adj_csr = ops.DeviceCSR.from_device(rp, col, val, nu_ni, chunk)
        # the dropout seed: derived from the config seed, not torch's RNG, so the parameter
        # initialisation stream matches the reference; advanced on the device
        self._drop_seed = torch.tensor([int(config["seed"] or 999) * 1000003 + 29], dtype=torch.int64, device=dev)
        self._ws = workspace(max(int(config["train_batch_size"] or 1), 1), d, dev)
        self.last_terms = None  # the loss's eight words of the last calculate_loss (device)

    # ------------------------------------------------------------------ forward
    def _tables(self):
        """(E [N, d] propagated mean, H, T | None, V | None), with autograd."""
        ego = _ego(self.user_embedding.weight, self.item_id_embedding.weight)
        E = _PropMean.apply(ego, self.norm_adj_csr, self.n_layers)
        T = V = None
        if self.t_feat is not None:
            T = _Project.apply(self.text_embedding.weight, self.text_trs.weight, self.text_trs.bias)
        if self.v_feat is not None:
            V = _Project.apply(self.image_embedding.weight, self.image_trs.weight, self.image_trs.bias)
        return E, self.item_id_embedding.weight, T, V

    def forward(self):
        """(user rows, item rows + item-id table) as reference bm3.py:86-97."""
        E, H, _, _ = self._tables()
        return E[: self.n_users], E[self.n_users:] + H

    def calculate_loss(self, interaction, keep_masks=None):
        """interaction: int64 [2, B] (user, item) on the device (rows past the second are
        ignored).  keep_masks: optional dict stream -> packed keep mask (rsx_bm3_args) in
        place of the hashed dropout."""
        users, items = interaction[0], interaction[1]
        self._ws = ops.grow_workspace(L.lib().rsx_bm3_ws_bytes, self._ws, users.numel(), self.embedding_dim)
        if self.dropout > 0.0 and keep_masks is None:
            self._drop_seed.add_(1)
        E, H, T, V = self._tables()
        keep = {}
        cfg = (self.n_users, self.reg_weight, self.cl_weight, self.dropout, self._drop_seed, keep_masks, self._ws, keep)
        loss = _Bm3Loss.apply(cfg, users, items, E, H, self.predictor.weight, self.predictor.bias, T, V)
        self.last_terms = keep["terms"]
        return loss

    # ------------------------------------------------------------------ evaluation
    def _predicted(self):
        """predictor(user rows), predictor(item rows) over the whole tables (bm3.py:153-154)."""
        with torch.no_grad():
            E = _PropMean.apply(_ego(self.user_embedding.weight, self.item_id_embedding.weight), self.norm_adj_csr,
                                self.n_layers)
            x = E.clone()
            x[self.n_users:] += self.item_id_embedding.weight
            q = ops.linear_rows_fwd(x, self.predictor.weight.contiguous(), self.predictor.bias.contiguous(), None)
        return q[: self.n_users], q[self.n_users:]

    def full_sort_predict(self, interaction):
        u, i = self._predicted()
        return ops.score_dense(u, interaction[0].contiguous(), i)

    def full_sort_topk(self, interaction, k: int, eval_data):
        u, i = self._predicted()
        return ops.fullsort_topk(u, interaction[0].contiguous(), i, eval_data.mask_rowptr, eval_data.mask_col, k)
