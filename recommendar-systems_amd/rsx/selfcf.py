"""SELFCFED_LGN on the rsx HIP path — drop-in for the reference's models/selfcfed_lgn.py (SelfCF with
embedding dropout) on common/encoders.py's LightGCN_Encoder.

Same class name, constructor `(config, dataloader)`, YAML keys (embedding_size, n_layers with None
-> 3, dropout, reg_weight, `use_neg_sampling: False`), parameter names in the reference's
`named_parameters()` order (online_encoder.embedding_dict.item_emb, .user_emb, predictor.weight,
predictor.bias) and initial draws on the CPU generator in its creation order (user table, item
table, the nn.Linear default init).  It needs no feature file.

* the graph: the LightGCN Laplacian (encoders.py:39-78) through `ops.adj_build`, its structure
  fixed; the encoder's `sparse_dropout` (:80-96) rewrites the VALUES of A and A^T on every training
  forward in one launch (`DropGraph.drop`, rsx_selfcf_edge_drop): a rate uniform in [0, 1), each
  of the 2 E directed entries kept independently (A is then not symmetric: the backward runs on
  A^T), survivors scaled by 1 / (1 - rate).  Zeroed entries are still walked by the SpMM;
* the propagation: `rsx.blocks.ui_backbone` on the batch's rows (1 <= n_layers <= 4: the tagged
  rows path, else the dense `_PropMean`), the two tables adjacent in one buffer;
* predictor, target dropout, the two halved cosine terms and the batch L2, forward and backward:
  rsx_selfcf_loss_fwd / _bwd (csrc/selfcf.hip).  The target dropout is keyed on the batch position
  (the reference drops the gathered rows): two occurrences of a row get independent masks;
* evaluation: q_u . i + u . q_i as ONE dot product of [q_u | u] with [i | q_i] at width 2 d
  (rsx_selfcf_eval_tables, built once per eval() session), then the fused full sort.

Every draw is a hash of a device seed word that advances once per training forward, so a captured
step replays with a fresh rate and fresh masks; a run is therefore not the reference's run sample
for sample.  `set_replay` feeds a recorded draw (tests) through persistent buffers instead.  No
torch fallback: an unsupported configuration raises RSX_ERR_UNSUPPORTED at construction.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .blocks import _ego, _join_params, _PropMean, ui_backbone
from .recommender import GeneralRecommender

SUPPORTED_D = (64, 128)
MAX_BATCH = 65536


def unsupported(what: str) -> RuntimeError:
    return RuntimeError(f"RSX_ERR_UNSUPPORTED: {what} (SELFCFED_LGN runs on the HIP path only)")


def selfcf_init(n_users: int, n_items: int, d: int):
    """The initial parameters by the reference's torch calls in its order on the CPU generator
    (encoders.py:30-37, selfcfed_lgn.py:37-38): xavier_uniform_ user table, item table, then the
    predictor nn.Linear's default init.  Returns dict name -> tensor."""
    u = nn.init.xavier_uniform_(torch.empty(n_users, d))
    i = nn.init.xavier_uniform_(torch.empty(n_items, d))
    pred = nn.Linear(d, d)
    return {"online_encoder.embedding_dict.user_emb": u, "online_encoder.embedding_dict.item_emb": i,
            "predictor.weight": pred.weight.data, "predictor.bias": pred.bias.data}


def reverse_slots(rowptr: torch.Tensor, col: torch.Tensor) -> torch.Tensor:
    """rev int32 [nnz] of a CSR whose structure is symmetric (rowptr int64 [n + 1], col [nnz]; any
    device): the slot of the reversed entry, rev[rev[e]] = e and col[rev[e]] = row(e), the k-th copy
    of a repeated entry paired with the k-th copy.  The slots sorted by (col, row), stably, list the
    transposed entries in CSR order: that order is the permutation.  Raises when the structure is
    not symmetric."""
    n, nnz = rowptr.numel() - 1, col.numel()
    if nnz >= 2 ** 31:
        raise unsupported(f"{nnz} directed entries: the slots are int32")
    row = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=col.device), rowptr[1:] - rowptr[:-1])
    c = col.to(torch.int64)
    key = row * n + c
    if nnz > 1 and not bool((key[1:] >= key[:-1]).all()):  # rows ascending by construction; columns inside a row
        raise RuntimeError("reverse_slots: the columns of a row are not sorted")
    rev = torch.sort(c * n + row, stable=True).indices
    if not (torch.equal(c[rev], row) and torch.equal(row[rev], c)):
        raise RuntimeError("reverse_slots: the structure is not symmetric")
    return rev.to(torch.int32)


class DropGraph:
    """The fixed structure with its three value buffers on the device: `val0` (undropped, A0: the
    evaluation's graph), `val` / `valT` (A and A^T of the current step, rewritten by `drop`), the
    reverse-slot permutation, and the draw's persistent words: `seed` (int64, advanced by the
    model), `info` = {rate, scale} as the last drop used them, and the replay buffers."""

    def __init__(self, rowptr: torch.Tensor, col: torch.Tensor, val0: torch.Tensor, seed: int, chunk: int = 32):
        dev = col.device
        self.n, self.nnz = rowptr.numel() - 1, col.numel()
        self.col, self.val0 = col.contiguous(), val0.contiguous()
        self.rev = reverse_slots(rowptr, col).contiguous()
        self.val, self.valT = torch.zeros_like(self.val0), torch.zeros_like(self.val0)
        rp = rowptr.cpu().numpy()
        self.A0 = ops.DeviceCSR(rp, self.col, self.val0, self.n, dev, chunk)
        self.A = ops.DeviceCSR(rp, self.col, self.val, self.n, dev, chunk)
        self.AT = ops.DeviceCSR(rp, self.col, self.valT, self.n, dev, chunk)
        self.rowptr = self.A0.rowptr
        self.seed = torch.tensor([int(seed)], dtype=torch.int64, device=dev)
        self.info = torch.zeros(2, dtype=torch.float32, device=dev)
        self.replay_mask = torch.zeros((self.nnz + 31) // 32, dtype=torch.int32, device=dev)
        self.replay_scale = torch.ones(1, dtype=torch.float32, device=dev)

    def drop(self, replay: bool = False) -> None:
        """One launch: val / valT of this step, hashed from `seed` or (replay) from the replay buffers."""
        mask, scale, seed = (self.replay_mask, self.replay_scale, None) if replay else (None, None, self.seed)
        edge_drop(self.val0, self.rev, seed, mask, scale, self.val, self.valT, self.info)


def edge_drop(val0, rev, seed, mask, scale, val, valT, info) -> None:
    """rsx_selfcf_edge_drop on caller-owned device buffers."""
    ops._gpu(val0, rev, seed, mask, scale, val, valT, info)
    nnz = val0.numel()
    if rev.dtype != torch.int32 or rev.numel() != nnz or val.numel() != nnz or valT.numel() != nnz:
        raise RuntimeError("selfcf edge drop: rev (int32), val and valT hold one entry per slot")
    if any(t.dtype != torch.float32 for t in (val0, val, valT, info)) or info.numel() < 2:
        raise RuntimeError("selfcf edge drop: float32 value buffers and a float32 info [2]")
    if mask is not None and (mask.dtype not in (torch.int32, torch.uint32) or mask.numel() < (nnz + 31) // 32):
        raise RuntimeError(f"selfcf edge drop: the keep mask must be {(nnz + 31) // 32} 32-bit words")
    if seed is not None and seed.dtype != torch.int64:
        raise RuntimeError("selfcf edge drop: the seed is an int64 device word")
    L.check(L.lib().rsx_selfcf_edge_drop(ops._p(val0), ops._p(rev), nnz, ops._p(seed), ops._p(mask), ops._p(scale),
                                         ops._p(val), ops._p(valT), ops._p(info), ops._stream()),
            "rsx_selfcf_edge_drop")


def selfcf_args(E, P, pb, users, items, n_users, reg_weight, p_drop, seed, masks, ws) -> "L.SelfcfArgs":
    """The rsx_selfcf_args of one call; `masks`: uint32 / int32 [2, B, d / 32] device tensor, or None."""
    ops._gpu(E, P, pb, users, items, seed, masks, ws)
    if users.dtype != torch.int64 or items.dtype != torch.int64 or users.numel() != items.numel():
        raise RuntimeError("selfcf: users / items must be int64 tensors of one length")
    a = L.SelfcfArgs()
    a.n_users, a.n_items, a.d, a.batch = int(n_users), E.shape[0] - int(n_users), E.shape[1], users.numel()
    if masks is not None and (masks.dtype not in (torch.int32, torch.uint32)
                              or tuple(masks.shape) != (2, a.batch, a.d // 32)):
        raise RuntimeError(f"selfcf: the keep masks must be 32-bit words [2, {a.batch}, {a.d // 32}]")
    for k, t in (("E", E), ("P", P), ("pb", pb), ("users", users), ("items", items), ("seed", seed), ("mask", masks),
                 ("ws", ws)):
        setattr(a, k, None if t is None else t.data_ptr())
    a.reg_weight, a.p_drop = float(reg_weight), float(p_drop)
    a.ws_bytes = 0 if ws is None else ws.numel()
    return a


def loss_fwd(args: "L.SelfcfArgs", device) -> torch.Tensor:
    """out [4] = total, ui, iu, reg (rsx_selfcf_loss_fwd)."""
    out = torch.empty(4, dtype=torch.float32, device=device)
    L.check(L.lib().rsx_selfcf_loss_fwd(C.byref(args), ops._p(out), ops._stream()), "rsx_selfcf_loss_fwd")
    return out


def targets(args: "L.SelfcfArgs", device) -> torch.Tensor:
    """[2 B, d] dropout targets of the batch, user stream then item stream (rsx_selfcf_targets)."""
    out = torch.empty(2 * args.batch, args.d, dtype=torch.float32, device=device)
    L.check(L.lib().rsx_selfcf_targets(C.byref(args), ops._p(out), ops._stream()), "rsx_selfcf_targets")
    return out


def loss_bwd(args: "L.SelfcfArgs", go: torch.Tensor, E, P):
    """(gE, gP, gpb) of rsx_selfcf_loss_bwd after loss_fwd with the same args."""
    gE, gP = torch.empty_like(E), torch.empty_like(P)
    gpb = torch.empty(P.shape[0], dtype=torch.float32, device=P.device)
    L.check(L.lib().rsx_selfcf_loss_bwd(C.byref(args), ops._p(go), ops._p(gE), ops._p(gP), ops._p(gpb), ops._stream()),
            "rsx_selfcf_loss_bwd")
    return gE, gP, gpb


def workspace(batch: int, d: int, device) -> torch.Tensor:
    return ops.loss_workspace(L.lib().rsx_selfcf_ws_bytes, batch, d, device, unsupported)


def eval_tables(E, P, pb, n_users: int):
    """(UC [n_users, 2 d] = [q_u | u], IC [n_items, 2 d] = [i | q_i]) of rsx_selfcf_eval_tables."""
    ops._gpu(E, P, pb)
    n, d = E.shape
    UC = torch.empty(n_users, 2 * d, dtype=torch.float32, device=E.device)
    IC = torch.empty(n - n_users, 2 * d, dtype=torch.float32, device=E.device)
    L.check(L.lib().rsx_selfcf_eval_tables(ops._p(E), ops._p(P), ops._p(pb), n_users, n - n_users, d, ops._p(UC),
                                           ops._p(IC), ops._stream()), "rsx_selfcf_eval_tables")
    return UC, IC


class _SelfcfLoss(torch.autograd.Function):
    """The bootstrap loss on the propagated table; cfg = (n_users, reg_weight, p_drop, seed, masks,
    ws, keep | None).  The kernels keep the row list, the keys and the predicted rows in `ws`
    between forward and backward.  Nothing with a grad_fn is kept on ctx: the tensors go through
    save_for_backward, the rest are persistent buffers."""

    @staticmethod
    def forward(ctx, cfg, users, items, E, P, pb):
        n_users, reg_weight, p_drop, seed, masks, ws, keep = cfg
        users, items, E, P, pb = (t.contiguous() for t in (users, items, E, P, pb))
        out = loss_fwd(selfcf_args(E, P, pb, users, items, n_users, reg_weight, p_drop, seed, masks, ws), E.device)
        ctx.cfg = (n_users, reg_weight, p_drop, seed, masks, ws)
        ctx.save_for_backward(users, items, E, P, pb)
        if keep is not None:
            keep["terms"] = out
        return out[0]

    @staticmethod
    def backward(ctx, go):
        users, items, E, P, pb = ctx.saved_tensors
        args = selfcf_args(E, P, pb, users, items, *ctx.cfg)
        gE, gP, gpb = loss_bwd(args, go.to(torch.float32).contiguous(), E, P)
        return None, None, None, gE, gP, gpb


class _PairRows(dict):
    """off[B] = [0] * B ++ [n_users] * B (int64, on the device), made once per batch length and
    kept (a captured step must not allocate); rows(pairs) = the batch's rows of [U; I]."""

    def __init__(self, n_users: int, device):
        super().__init__()
        self.n_users, self.device = int(n_users), device

    def __missing__(self, B: int) -> torch.Tensor:
        off = self[B] = torch.cat([torch.zeros(B, dtype=torch.int64, device=self.device),
                                   torch.full((B,), self.n_users, dtype=torch.int64, device=self.device)])
        return off

    def rows(self, pairs: torch.Tensor) -> torch.Tensor:
        return pairs.reshape(-1) + self[pairs.shape[1]]


class _Encoder(nn.Module):
    """The reference's LightGCN_Encoder as far as its state goes: `embedding_dict`."""

    def __init__(self, user_emb: nn.Parameter, item_emb: nn.Parameter):
        super().__init__()
        # the reference's named_parameters() lists item_emb before user_emb
        self.embedding_dict = nn.ParameterDict({"item_emb": item_emb, "user_emb": user_emb})


class SELFCFED_LGN(GeneralRecommender):
    # calculate_loss has no host syncs and no data-dependent host branches: the Trainer may
    # capture a batch in a HIP graph (rsx.trainer._GraphStep); no per-epoch buffer rebuilds
    supports_graph_step = True
    graph_step_persistent = True

    @staticmethod
    def check_config(config):
        ops.require_single_gpu(config, unsupported)
        if config["embedding_size"] not in SUPPORTED_D:
            raise unsupported(f"embedding_size {config['embedding_size']} not in {SUPPORTED_D}")
        p = float(config["dropout"])
        if not 0.0 <= p < 1.0:
            raise unsupported(f"dropout {p} outside [0, 1)")
        if config["n_layers"] is not None and int(config["n_layers"]) < 0:
            raise unsupported(f"n_layers {config['n_layers']} < 0")

    @staticmethod
    def check_edges(n_interactions: int) -> None:
        if 2 * int(n_interactions) >= 2 ** 31:
            raise unsupported(f"{2 * int(n_interactions)} directed entries: the slots are int32")

    def __init__(self, config, dataset):
        self.check_config(config)
        super().__init__(config, dataset)
        ops.require_device(self.device)
        self.user_count, self.item_count = nu, ni = self.n_users, self.n_items
        self.latent_size = d = config["embedding_size"]
        self.n_layers = 3 if config["n_layers"] is None else int(config["n_layers"])
        self.dropout = float(config["dropout"])
        self.reg_weight = float(config["reg_weight"])
        self.drop_ratio, self.drop_flag = 1.0, True  # as the reference hard-codes them (encoders.py:24-25)
        im = dataset.inter_matrix(form="coo")
        self.check_edges(im.nnz)
        dev = self.device
        # parameters drawn on the CPU generator in the reference's creation order; the two tables
        # adjacent row blocks of one device buffer: the ego table [U; I] is that buffer (_ego)
        init = selfcf_init(nu, ni, d)
        u, i = _join_params(init["online_encoder.embedding_dict.user_emb"],
                            init["online_encoder.embedding_dict.item_emb"], dev)
        self.online_encoder = _Encoder(u, i)
        self.predictor = nn.Linear(d, d)
        self.to(dev)
        with torch.no_grad():
            self.predictor.weight.copy_(init["predictor.weight"])
            self.predictor.bias.copy_(init["predictor.bias"])
        rp, col, val = ops.adj_build(im.row.astype(np.int64), im.col.astype(np.int64), nu, ni, ops.ADJ_LIGHTGCN, dev)
        # the seed of every draw: derived from the config seed, not torch's RNG, so the parameter
        # initialisation stream matches the reference; advanced on the device
        self.graph = DropGraph(rp, col, val, int(config["seed"] or 999) * 1000003 + 41, int(config["rsx_chunk"] or 32))
        self._ws = workspace(min(max(int(config["train_batch_size"] or 1), 1), MAX_BATCH), d, dev)
        self._rows = _PairRows(nu, dev)
        self._tags = None  # ui_backbone's batch-row tags, made on first use
        self._replay = False
        self._eval_cache = None
        self.last_terms = None  # the loss's four words of the last calculate_loss (device)

    # ------------------------------------------------------------------ draws
    @property
    def drop_seed(self) -> torch.Tensor:
        return self.graph.seed

    @property
    def drop_info(self) -> torch.Tensor:
        """{rate, scale} of the last edge drop (device)."""
        return self.graph.info

    def set_replay(self, keep_mask, scale) -> None:
        """Feeds a recorded edge draw: the packed keep mask [ceil(nnz / 32)] and the f32 scale are
        copied into persistent buffers that every later training forward's edge drop reads instead
        of hashing (a step captured in this mode replays whatever the buffers then hold).
        None, None: back to the hashed draws.  Call it outside a capture."""
        if keep_mask is None:
            self._replay = False
            return
        g = self.graph
        g.replay_mask.copy_(torch.as_tensor(keep_mask).view(torch.int32).reshape(-1))
        g.replay_scale.copy_(torch.as_tensor(scale, dtype=torch.float32).reshape(1))
        self._replay = True

    # ------------------------------------------------------------------ forward
    def _tables(self):
        e = self.online_encoder.embedding_dict
        return e["user_emb"], e["item_emb"]

    def _propagate(self, rows=None):
        """mean_{k <= K} A^k [U; I] with autograd, on this step's graph (training with drop_flag:
        the dropped A, backward on A^T) or the undropped one."""
        g = self.graph
        ego = _ego(*self._tables())
        if self.n_layers == 0:
            return ego
        if self.training and self.drop_flag:
            return ui_backbone(self, ego, g.A, self.n_layers, rows, AT=g.AT)
        return ui_backbone(self, ego, g.A0, self.n_layers, rows)

    def _draw(self, hashed_targets: bool) -> None:
        """This training forward's draws: the seed word advances once, then the edge drop."""
        if (self.drop_flag and not self._replay) or hashed_targets:
            self.graph.seed.add_(1)
        if self.drop_flag:
            self.graph.drop(self._replay)

    def forward(self, inputs):
        """(u_online, u_target, i_online, i_target) of the pairs `inputs` [2, B] as reference
        selfcfed_lgn.py:41-50, without autograd (calculate_loss is the differentiable path)."""
        users, items = inputs[0].contiguous(), inputs[1].contiguous()
        with torch.no_grad():
            if self.training:
                self._draw(self.dropout > 0.0)
            E = self._propagate().contiguous()
            self._ws = ops.grow_workspace(L.lib().rsx_selfcf_ws_bytes, self._ws, users.numel(), self.latent_size)
            a = selfcf_args(E, self.predictor.weight, self.predictor.bias, users, items, self.n_users, self.reg_weight,
                            self.dropout, self.graph.seed, None, self._ws)
            t = targets(a, E.device)
            B = users.numel()
            return E[users], t[:B], E[self.n_users + items], t[B:]

    def calculate_loss(self, interaction, keep_masks=None):
        """interaction: int64 [2, B] (user, item) on the device (rows past the second are ignored).
        keep_masks: optional packed keep masks [2, B, d / 32] of the target dropout in place of the
        hashed ones (the edge draw is replayed through set_replay)."""
        pairs = interaction[:2].contiguous()
        users, items = pairs[0], pairs[1]
        B = users.numel()
        if B > MAX_BATCH:
            raise unsupported(f"a batch of {B} pairs > {MAX_BATCH}")
        self._ws = ops.grow_workspace(L.lib().rsx_selfcf_ws_bytes, self._ws, B, self.latent_size)
        self._draw(self.dropout > 0.0 and keep_masks is None)
        E = self._propagate(self._rows.rows(pairs))
        keep = {}
        cfg = (self.n_users, self.reg_weight, self.dropout, self.graph.seed, keep_masks, self._ws, keep)
        loss = _SelfcfLoss.apply(cfg, users, items, E, self.predictor.weight, self.predictor.bias)
        self.last_terms = keep["terms"]
        return loss

    # ------------------------------------------------------------------ evaluation
    def train(self, mode: bool = True):
        self._eval_cache = None
        return super().train(mode)

    def get_embedding(self):
        """(predictor(u), u, predictor(i), i) over the whole tables on the undropped graph
        (selfcfed_lgn.py:52-55), as views of the two concatenated evaluation tables."""
        d, (UC, IC) = self.latent_size, self._eval_tables()
        return UC[:, :d], UC[:, d:], IC[:, d:], IC[:, :d]

    def _eval_tables(self):
        if self._eval_cache is None or self.training:
            with torch.no_grad():
                ego = _ego(*self._tables())
                E = ego if self.n_layers == 0 else _PropMean.apply(ego, self.graph.A0, self.n_layers)
                tabs = eval_tables(E.contiguous(), self.predictor.weight.contiguous(),
                                   self.predictor.bias.contiguous(), self.n_users)
            if self.training:
                return tabs
            self._eval_cache = tabs
        return self._eval_cache

    def full_sort_predict(self, interaction):
        UC, IC = self._eval_tables()
        return ops.score_dense(UC, interaction[0].contiguous(), IC)

    def full_sort_topk(self, interaction, k: int, eval_data):
        UC, IC = self._eval_tables()
        return ops.fullsort_topk(UC, interaction[0].contiguous(), IC, eval_data.mask_rowptr, eval_data.mask_col, k)
