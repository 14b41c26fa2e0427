"""LGMRec on the rsx HIP path — drop-in for the reference's models/lgmrec.py (AAAI'24): a
LightGCN (or plain MF) backbone, modality graph embeddings, and a hypergraph whose soft
hyperedge assignments are Gumbel-softmax draws on projected features.

Same class name, constructor `(config, dataloader)`, YAML keys, parameter names, shapes,
creation order and initial draws (reference src/models/lgmrec.py:19-61), forward, loss and
scoring (:115-200):

* CGE: `rsx.blocks._PropMean` on the joint [U; I] table (dense: the hypergraph reads every
  item row);
* MGE: `X_m @ item_m_trs` (`rsx_linear_rows_fwd` / `rsx_linear_rows_wgrad`; the feature
  tables are frozen, no dX is formed), `R @ .` scaled by num_inters (one SpMM on
  diag(num_inters) R), then norm_adj^n_mm_layers (SpMM);
* the hyperedge logits `X_m @ m_hyper` and `R @ .` at the padded width 32 ceil(H / 32) with
  zero columns, so that the same projection and SpMM kernels take them;
* Gumbel-softmax and dropout on the assignments: rsx_lgm_assign_fwd / _bwd, the draws a hash
  of (seed word on the device, stream, row, column);
* HGNNLayer: rsx_lgm_hgnn_reduce / _expand / _rowdots, forward and backward;
* the table-wide InfoNCE: rsx_lgm_ssl_fwd / _bwd; BPR and regulariser on the combined rows:
  rsx_lgm_loss_fwd / _bwd (csrc/lgmrec.hip).

The seed word advances once per forward, so a captured step replays with fresh draws;
`draws` (four Gumbel noise tensors iv, uv, it, ut, then four packed keep masks in that order)
replaces the hash.  Evaluation builds the tables once per eval() session with one draw (the
reference redraws per evaluation batch: the same distribution of every user's scores, the
draws shared across batches).

One GPU; anything the kernels are not built for raises RSX_ERR_UNSUPPORTED at construction.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import graph, ops
from .blocks import _DevGraph, _ego, _join_tables, _PropMean, _SpMM
from .recommender import EvalTables, GeneralRecommender

SUPPORTED_D = (64, 128)
TAU = 0.2
MAX_LAYERS = 4  # of either propagation


def unsupported(what: str) -> RuntimeError:
    return RuntimeError(f"RSX_ERR_UNSUPPORTED: {what} (LGMRec runs on the HIP path only)")


def padded(H: int) -> int:
    """The row stride the assignment matrices are kept at: 32 ceil(H / 32), zero columns past H."""
    return 32 * ((int(H) + 31) // 32)


def lgmrec_init(n_users: int, n_items: int, d: int, feat_d: int, hyper_num: int, image_dim, text_dim):
    """LGMRec's initial parameters by the reference's torch calls in its order on the CPU
    generator (lgmrec.py:46-61): two nn.Embedding (normal_ draws, then xavier_uniform_), then
    per modality, image first, item_*_trs [dim, feat_d] and *_hyper [dim, hyper_num]
    (xavier_uniform_ on zeros; from_pretrained draws nothing)."""
    ue, ie = nn.Embedding(n_users, d), nn.Embedding(n_items, d)
    nn.init.xavier_uniform_(ue.weight)
    nn.init.xavier_uniform_(ie.weight)
    out = {"user_embedding.weight": ue.weight.data, "item_id_embedding.weight": ie.weight.data}
    for name, short, dim in (("image", "v", image_dim), ("text", "t", text_dim)):
        if dim is not None:
            out[f"item_{name}_trs"] = nn.init.xavier_uniform_(torch.zeros(dim, feat_d))
            out[f"{short}_hyper"] = nn.init.xavier_uniform_(torch.zeros(dim, hyper_num))
    return out


def lgmrec_graphs(train_u: np.ndarray, train_i: np.ndarray, n_users: int, n_items: int):
    """(norm_adj CSR triple, R CSR triple, num_inters f32 [n_users + n_items]) as lgmrec.py:40-43,
    70-86: the LightGCN Laplacian with float64 (deg + 1e-7)^-1/2 factors, the binary
    [n_users, n_items] interaction matrix and float32(1 / (deg + 1e-7))."""
    n = n_users + n_items
    deg = (np.bincount(train_u, minlength=n) + np.bincount(train_i + n_users, minlength=n)).astype(np.float64)
    R = graph.to_csr(train_u, train_i, np.ones(train_u.size, np.float32), n_users, n_items)
    return graph.lightgcn_norm_adj(train_u, train_i, n_users, n_items), R, (1.0 / (deg + 1e-7)).astype(np.float32)


# ---------------------------------------------------------------------------
# kernel wrappers
# ---------------------------------------------------------------------------
def ssl_workspace(n: int, batch: int, d: int, device) -> torch.Tensor:
    nbytes = L.lib().rsx_lgm_ssl_ws_bytes(int(n), int(batch), int(d))
    if nbytes == 0:
        raise unsupported(f"InfoNCE over {n} rows, batch {batch}, width {d}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def ssl_args(T1, T2, idx, tau: float) -> "L.LgmSslArgs":
    ops._gpu(T1, T2, idx)
    if idx.dtype != torch.int64 or idx.dim() != 1 or T1.shape != T2.shape or T1.dtype != torch.float32:
        raise RuntimeError("lgm ssl: f32 tables of one shape and an int64 [batch] index")
    a = L.LgmSslArgs()
    a.T1, a.T2, a.idx = T1.data_ptr(), T2.data_ptr(), idx.data_ptr()
    a.n, a.batch, a.d, a.tau = T1.shape[0], idx.numel(), T1.shape[1], float(tau)
    return a


def ssl_fwd(args, ws) -> torch.Tensor:
    out = torch.empty(1, dtype=torch.float32, device=ws.device)
    L.check(L.lib().rsx_lgm_ssl_fwd(C.byref(args), ops._p(out), ops._p(ws), ws.numel(), ops._stream()),
            "rsx_lgm_ssl_fwd")
    return out


def ssl_bwd(args, go, gT1, gT2, ws):
    L.check(L.lib().rsx_lgm_ssl_bwd(C.byref(args), ops._p(go), ops._p(gT1), ops._p(gT2), ops._p(ws), ws.numel(),
                                    ops._stream()), "rsx_lgm_ssl_bwd")


class _Ssl(torch.autograd.Function):
    """sum_b (log sum_j exp(<n1_b, m_j> / tau) - <n1_b, m_idx_b> / tau); cfg = (tau, ws).  The
    backward reads what the forward left in ws: one ws a term."""

    @staticmethod
    def forward(ctx, cfg, idx, T1, T2):
        tau, ws = cfg
        T1, T2, idx = T1.contiguous(), T2.contiguous(), idx.contiguous()
        ctx.args, ctx.ws, ctx.held = ssl_args(T1, T2, idx, tau), ws, (idx, T1, T2)
        return ssl_fwd(ctx.args, ws)[0]

    @staticmethod
    def backward(ctx, go):
        _, T1, T2 = ctx.held
        same = T1.data_ptr() == T2.data_ptr()
        g1 = torch.empty_like(T1)
        g2 = g1 if same else torch.empty_like(T2)
        ssl_bwd(ctx.args, go.to(torch.float32).contiguous(), g1, g2, ctx.ws)
        return None, None, g1, None if same else g2


def assign_args(x, H, tau, keep_rate, noise, keep, seed, stream_id) -> "L.LgmAssignArgs":
    ops._gpu(x, noise, keep, seed)
    n, ld = x.shape
    if noise is not None and (tuple(noise.shape) != (n, H) or noise.dtype != torch.float32):
        raise RuntimeError(f"lgm assign: the noise must be f32 [{n}, {H}]")
    if keep is not None and (tuple(keep.shape) != (n, (H + 31) // 32) or keep.dtype not in (torch.int32, torch.uint32)):
        raise RuntimeError(f"lgm assign: the keep mask must be 32-bit words [{n}, {(H + 31) // 32}]")
    a = L.LgmAssignArgs()
    a.x, a.noise, a.keep, a.seed = x.data_ptr(), ops._pi(noise) or None, ops._pi(keep) or None, ops._pi(seed) or None
    a.n, a.H, a.ld, a.stream_id, a.tau, a.keep_rate = n, int(H), ld, int(stream_id), float(tau), float(keep_rate)
    return a


def assign_fwd(x, H, tau, keep_rate, noise=None, keep=None, seed=None, stream_id=0, noise_out=None, out=None, y=None):
    """(y, out) of rsx_lgm_assign_fwd on logits x [n, ld]; the columns past H of the given
    `y` / `out` (fresh zeros when None) are left as they are."""
    x = x.contiguous()
    args = assign_args(x, H, tau, keep_rate, noise, keep, seed, stream_id)
    y = torch.zeros_like(x) if y is None else y
    out = torch.zeros_like(x) if out is None else out
    L.check(L.lib().rsx_lgm_assign_fwd(C.byref(args), ops._p(y), ops._p(out), ops._p(noise_out), ops._stream()),
            "rsx_lgm_assign_fwd")
    return y, out


def assign_bwd(x, H, tau, keep_rate, y, dy, keep=None, seed=None, stream_id=0, dx=None):
    x, dy = x.contiguous(), dy.contiguous()
    args = assign_args(x, H, tau, keep_rate, None, keep, seed, stream_id)
    dx = torch.zeros_like(x) if dx is None else dx
    L.check(L.lib().rsx_lgm_assign_bwd(C.byref(args), ops._p(y), ops._p(dy), ops._p(dx), ops._stream()),
            "rsx_lgm_assign_bwd")
    return dx


class _Assign(torch.autograd.Function):
    """dropout(gumbel_softmax(x)) on padded logits; cfg = (H, tau, keep_rate, noise, keep, seed,
    stream_id).  The forward keeps its own copy of the seed word (8 bytes, on the device), so
    that the backward redraws the same keep bits whatever forwards ran in between."""

    @staticmethod
    def forward(ctx, cfg, x):
        H, tau, keep_rate, noise, keep, seed, stream_id = cfg
        x = x.contiguous()
        seed = None if seed is None else seed.clone()
        y, out = assign_fwd(x, H, tau, keep_rate, noise, keep, seed, stream_id)
        ctx.cfg, ctx.held = cfg, (x, y, seed)
        return out

    @staticmethod
    def backward(ctx, dy):
        H, tau, keep_rate, _, keep, _, stream_id = ctx.cfg
        x, y, seed = ctx.held
        return None, assign_bwd(x, H, tau, keep_rate, y, dy, keep, seed, stream_id)


def _hg_ws(n, n2, H, d, device):
    return torch.empty(max(int(L.lib().rsx_lgm_hgnn_ws_bytes(n, n2, H, d)), 256), dtype=torch.uint8, device=device)


def hgnn_reduce(P, X, H, P2=None, X2=None, ws=None) -> torch.Tensor:
    """lat [H, d] = P[:, :H]^T X (+ P2[:, :H]^T X2); ws: a workspace to use when it is large enough."""
    ops._gpu(P, X, P2, X2)
    n, ld = P.shape
    d = X.shape[1]
    n2 = 0 if P2 is None else P2.shape[0]
    if X.shape[0] != n or (P2 is not None and (P2.shape[1] != ld or X2.shape != (n2, d))):
        raise RuntimeError("lgm hgnn: P [n, ld] with X [n, d]")
    if L.lib().rsx_lgm_hgnn_ws_bytes(n, n2, H, d) == 0:
        raise unsupported(f"hypergraph product with H {H}, width {d}")
    if ws is None or ws.numel() < L.lib().rsx_lgm_hgnn_ws_bytes(n, n2, H, d):
        ws = _hg_ws(n, n2, H, d, X.device)
    lat = torch.empty(H, d, dtype=torch.float32, device=X.device)
    L.check(L.lib().rsx_lgm_hgnn_reduce(ops._p(P), ops._p(X), n, ops._p(P2), ops._p(X2), n2, ld, H, d, ops._p(lat),
                                        ops._p(ws), ws.numel(), ops._stream()), "rsx_lgm_hgnn_reduce")
    return lat


def hgnn_expand(P, H, lat, out=None) -> torch.Tensor:
    """[n, d] = P[:, :H] lat."""
    ops._gpu(P, lat, out)
    n, ld = P.shape
    d = lat.shape[1]
    out = torch.empty(n, d, dtype=torch.float32, device=P.device) if out is None else out
    L.check(L.lib().rsx_lgm_hgnn_expand(ops._p(P), ld, H, ops._p(lat), n, d, ops._p(out), ops._stream()),
            "rsx_lgm_hgnn_expand")
    return out


def hgnn_rowdots(X, lat, ld, out=None, accumulate=False) -> torch.Tensor:
    """[n, ld], columns [0, H) = X lat^T (added to `out` with accumulate); fresh zeros when out is None."""
    ops._gpu(X, lat, out)
    n, d = X.shape
    H = lat.shape[0]
    if out is None:
        out = torch.zeros(n, ld, dtype=torch.float32, device=X.device)
    L.check(L.lib().rsx_lgm_hgnn_rowdots(ops._p(X), ops._p(lat), H, n, d, ops._p(out), ld, int(accumulate),
                                         ops._stream()), "rsx_lgm_hgnn_rowdots")
    return out


class _Hgnn(torch.autograd.Function):
    """HGNNLayer (lgmrec.py:202-214) as one table [u_ret; i_ret]: n_layers times
    lat = Pi^T i_ret, i_ret = Pi lat; u_ret = Pu lat of the last layer."""

    @staticmethod
    def forward(ctx, Pi, Pu, X, H, n_layers, ws=None):
        Pi, Pu, X = Pi.contiguous(), Pu.contiguous(), X.contiguous()
        nu, ni, d = Pu.shape[0], Pi.shape[0], X.shape[1]
        out = torch.empty(nu + ni, d, dtype=torch.float32, device=X.device)
        xs, lats, cur = [], [], X
        for l in range(n_layers):
            xs.append(cur)
            lats.append(hgnn_reduce(Pi, cur, H, ws=ws))
            cur = hgnn_expand(Pi, H, lats[-1], out=out[nu:] if l == n_layers - 1 else None)
        hgnn_expand(Pu, H, lats[-1], out=out[:nu])
        ctx.H, ctx.ws, ctx.held = H, ws, (Pi, Pu, xs, lats)
        return out

    @staticmethod
    def backward(ctx, g):
        Pi, Pu, xs, lats = ctx.held
        H, nu, ld = ctx.H, Pu.shape[0], Pi.shape[1]
        g = g.contiguous()
        gu, gi = g[:nu], g[nu:]
        gPu = hgnn_rowdots(gu, lats[-1], ld)
        gPi = None
        for l in reversed(range(len(xs))):
            last = l == len(xs) - 1
            glat = hgnn_reduce(Pi, gi, H, Pu if last else None, gu if last else None, ws=ctx.ws)
            gPi = hgnn_rowdots(gi, lats[l], ld, out=gPi, accumulate=gPi is not None)
            gPi = hgnn_rowdots(xs[l], glat, ld, out=gPi, accumulate=True)
            gi = hgnn_expand(Pi, H, glat)
        return gPi, gPu, gi, None, None, None


def loss_workspace(batch: int, d: int, device) -> torch.Tensor:
    return ops.loss_workspace(L.lib().rsx_lgm_loss_ws_bytes, batch, d, device, unsupported)


def loss_args(tables, triplets, n_users: int, alpha: float, reg: float) -> "L.LgmLossArgs":
    ops._gpu(*tables, triplets)
    if triplets.dtype != torch.int64 or triplets.dim() != 2 or triplets.shape[0] != 3:
        raise RuntimeError("lgm loss: triplets must be an int64 [3, batch] tensor")
    if len(tables) != 5 or any(t.shape != tables[0].shape or t.dtype != torch.float32 for t in tables):
        raise RuntimeError("lgm loss: five f32 tables [n_users + n_items, d]")
    a = L.LgmLossArgs()
    a.C, a.Mv, a.Mt, a.Gv, a.Gt = (t.data_ptr() for t in tables)
    a.triplets = triplets.data_ptr()
    a.n_users, a.n_items, a.batch = int(n_users), tables[0].shape[0] - int(n_users), triplets.shape[1]
    a.d, a.alpha, a.reg = tables[0].shape[1], float(alpha), float(reg)
    return a


def loss_fwd(args, ws) -> torch.Tensor:
    """out [3] = total, bpr, reg (rsx_lgm_loss_fwd)."""
    out = torch.empty(3, dtype=torch.float32, device=ws.device)
    L.check(L.lib().rsx_lgm_loss_fwd(C.byref(args), ops._p(out), ops._p(ws), ws.numel(), ops._stream()),
            "rsx_lgm_loss_fwd")
    return out


def loss_bwd(args, go, tables, ws):
    gs = [torch.empty_like(t) for t in tables]
    L.check(L.lib().rsx_lgm_loss_bwd(C.byref(args), ops._p(go), *[ops._p(g) for g in gs], ops._p(ws), ws.numel(),
                                     ops._stream()), "rsx_lgm_loss_bwd")
    return gs


class _LgmLoss(torch.autograd.Function):
    """BPR + regulariser on the five tables; cfg = (n_users, alpha, reg, ws, terms_out)."""

    @staticmethod
    def forward(ctx, cfg, triplets, *tables):
        n_users, alpha, reg, ws, keep = cfg
        tables, triplets = [t.contiguous() for t in tables], triplets.contiguous()
        ctx.args, ctx.ws, ctx.held = loss_args(tables, triplets, n_users, alpha, reg), ws, (triplets, tables)
        out = loss_fwd(ctx.args, ws)
        if keep is not None:
            keep["terms"] = out
        return out[0]

    @staticmethod
    def backward(ctx, go):
        return (None, None, *loss_bwd(ctx.args, go.to(torch.float32).contiguous(), ctx.held[1], ctx.ws))


class _ProjectT(torch.autograd.Function):
    """x W over every row of a frozen feature table, W [in, out] (the reference's raw
    nn.Parameter layout), written at row stride `ld` >= out with zero columns past out:
    rsx_linear_rows_fwd, and rsx_linear_rows_wgrad for dW; no dx.  `buf`: a kept [ld, in] buffer
    for the transposed weight, zero in its rows past out (a fresh one when None)."""

    @staticmethod
    def forward(ctx, x, W, ld, buf=None):
        fin, o = W.shape
        Wt = torch.zeros(ld, fin, dtype=torch.float32, device=W.device) if buf is None else buf
        Wt[:o].copy_(W.t())
        ctx.save_for_backward(x)
        ctx.o = o
        return ops.linear_rows_fwd(x, Wt, None, None)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        dw, _ = ops.linear_rows_wgrad(g.contiguous(), x, None, bias=False)
        return None, dw[: ctx.o].t().contiguous(), None, None


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
class LGMRec(EvalTables, GeneralRecommender):
    # calculate_loss has no host syncs and no data-dependent host branches: the Trainer may
    # capture a batch in a HIP graph; no per-epoch buffer rebuilds
    supports_graph_step = True
    graph_step_persistent = True

    @staticmethod
    def check_config(config):
        ops.require_single_gpu(config, unsupported)
        if config["cf_model"] not in ("lightgcn", "mf"):
            raise unsupported(f"cf_model {config['cf_model']!r} (lightgcn and mf are built)")
        d = config["embedding_size"]
        if d not in SUPPORTED_D or config["feat_embed_dim"] != d:
            raise unsupported(f"embedding_size {d}, feat_embed_dim {config['feat_embed_dim']}: one value of {SUPPORTED_D}")
        H = config["hyper_num"]
        if not isinstance(H, int) or H % 4 or not 4 <= H <= 64:
            raise unsupported(f"hyper_num {H} is not a multiple of 4 in 4..64")
        if not 1 <= int(config["n_hyper_layer"]) <= MAX_LAYERS:
            raise unsupported(f"n_hyper_layer {config['n_hyper_layer']} outside 1..{MAX_LAYERS}")
        if not 0.0 < float(config["keep_rate"]) <= 1.0:
            raise unsupported(f"keep_rate {config['keep_rate']} outside (0, 1]")
        for key, lo in (("n_mm_layers", 0), ("n_ui_layers", 1)):
            if not lo <= int(config[key]) <= MAX_LAYERS:
                raise unsupported(f"{key} {config[key]} outside {lo}..{MAX_LAYERS}")

    def __init__(self, config, dataset):
        self.check_config(config)
        try:
            super().__init__(config, dataset)
        except AssertionError as e:  # recommender.py: "Features all NONE"
            raise unsupported("no feature file at all") from e
        ops.require_device(self.device)
        self.require_features(unsupported, need=2)
        self.embedding_dim = d = config["embedding_size"]
        self.feat_embed_dim = config["feat_embed_dim"]
        self.cf_model = config["cf_model"]
        self.n_mm_layer = int(config["n_mm_layers"])
        self.n_ui_layers = int(config["n_ui_layers"])
        self.n_hyper_layer = int(config["n_hyper_layer"])
        self.hyper_num = H = int(config["hyper_num"])
        self.keep_rate = float(config["keep_rate"])
        self.alpha = float(config["alpha"])
        self.cl_weight = float(config["cl_weight"])
        self.reg_weight = float(config["reg_weight"])
        self.tau = TAU
        self.ld = padded(H)
        nu, ni, dev = self.n_users, self.n_items, self.device
        self.n_nodes = nu + ni
        chunk = int(config["rsx_chunk"] or 32)
        # graphs: norm_adj, the binary R for the logits, diag(num_inters) R for the user features
        self.interaction_matrix = im = dataset.inter_matrix(form="coo").astype(np.float32)
        tu, ti = im.row.astype(np.int64), im.col.astype(np.int64)
        (rp, col, val), _, ninv = lgmrec_graphs(tu, ti, nu, ni)  # R: through _DevGraph, with its transpose
        self.norm_adj_csr = ops.DeviceCSR(rp, col, val, nu + ni, dev, chunk)
        self.num_inters = torch.from_numpy(ninv).to(dev)
        self.adj = _DevGraph(tu, ti, np.ones(tu.size, np.float32), nu, ni, dev, chunk)
        self.adj_mean = _DevGraph(tu, ti, ninv[tu], nu, ni, dev, chunk)
        # parameters in the reference's creation order, drawn on the CPU generator
        init = lgmrec_init(nu, ni, d, self.feat_embed_dim, H, int(self.v_feat.shape[1]), int(self.t_feat.shape[1]))
        self.user_embedding = nn.Embedding(nu, d, _weight=init["user_embedding.weight"])
        self.item_id_embedding = nn.Embedding(ni, d, _weight=init["item_id_embedding.weight"])
        _join_tables(self.user_embedding, self.item_id_embedding, dev)
        self.image_embedding = nn.Embedding.from_pretrained(self.v_feat.clone(), freeze=True)
        self.item_image_trs = nn.Parameter(init["item_image_trs"])
        self.v_hyper = nn.Parameter(init["v_hyper"])
        self.text_embedding = nn.Embedding.from_pretrained(self.t_feat.clone(), freeze=True)
        self.item_text_trs = nn.Parameter(init["item_text_trs"])
        self.t_hyper = nn.Parameter(init["t_hyper"])
        self.to(dev)
        # the draws' seed: derived from the config seed, not torch's RNG; advanced on the device
        self._seed = torch.tensor([int(config["seed"] or 999) * 1000003 + 57], dtype=torch.int64, device=dev)
        B = max(int(config["train_batch_size"] or 1), 1)
        self._ws = loss_workspace(B, d, dev)
        self._ssl_ws = [ssl_workspace(nu, B, d, dev), ssl_workspace(ni, B, d, dev)]
        self._hg_ws = _hg_ws(ni, nu, H, d, dev)  # the largest reduce: the last layer's two pairs
        # the transposed, zero-padded weights the projection kernels read: one kept buffer a weight
        self._wt = {n: torch.zeros(self.ld if n.endswith("_hyper") else self.feat_embed_dim, p.shape[0],
                                   dtype=torch.float32, device=dev)
                    for n, p in self.named_parameters() if n.endswith("_hyper") or n.endswith("_trs")}
        self.last_terms = None  # {total, bpr, reg} of the last calculate_loss (device)
        self.last_ssl = None  # the two ssl terms of the last calculate_loss (device)

    # --------------------------------------------------------------- forward
    def _tables(self, draws=None, training=None):
        """(CGE, MGE_v, MGE_t, GHE_v, GHE_t), each [n_users + n_items, d], with autograd."""
        training = self.training if training is None else training
        keep_rate = self.keep_rate if training else 1.0
        # the seed advances whenever a draw is hashed: all of them, or the keep bits alone when
        # `draws` holds only the noise
        if draws is None or (keep_rate < 1.0 and len(draws) <= 4):
            self._seed.add_(1)
        nu, H = self.n_users, self.hyper_num
        ego = _ego(self.user_embedding.weight, self.item_id_embedding.weight)
        cge = ego if self.cf_model == "mf" else _PropMean.apply(ego, self.norm_adj_csr, self.n_ui_layers)
        A = self.norm_adj_csr
        mge, ghe = [], []
        mods = ((self.image_embedding.weight, "item_image_trs", "v_hyper"),
                (self.text_embedding.weight, "item_text_trs", "t_hyper"))
        for m, (X, trs, hyper) in enumerate(mods):
            li = _ProjectT.apply(X, getattr(self, hyper), self.ld, self._wt[hyper])
            lu = self.adj(li)
            P = []
            for s, logits in ((2 * m, li), (2 * m + 1, lu)):
                noise = None if draws is None else draws[s]
                keep = draws[4 + s] if draws is not None and training and len(draws) > 4 else None
                P.append(_Assign.apply((H, self.tau, keep_rate, noise, keep, self._seed, s), logits))
            ghe.append(_Hgnn.apply(P[0], P[1], cge[nu:], H, self.n_hyper_layer, self._hg_ws))
            fi = _ProjectT.apply(X, getattr(self, trs), self.feat_embed_dim, self._wt[trs])
            x = torch.cat([self.adj_mean(fi), fi], dim=0)
            for _ in range(self.n_mm_layer):
                x = _SpMM.apply(x, A, A)
            mge.append(x)
        return cge, mge[0], mge[1], ghe[0], ghe[1]

    def forward(self, draws=None):
        """(user rows, item rows, [uv, iv, ut, it hyper embeddings]) as lgmrec.py:115-151."""
        nu = self.n_users
        C_, Mv, Mt, Gv, Gt = self._tables(draws)
        all_ = C_ + F.normalize(Mv) + F.normalize(Mt) + self.alpha * F.normalize(Gv + Gt)
        return all_[:nu], all_[nu:], [Gv[:nu], Gv[nu:], Gt[:nu], Gt[nu:]]

    def calculate_loss(self, interaction, draws=None):
        """interaction: int64 [3, B] on the device.  draws: the four Gumbel noise tensors
        (iv, uv, it, ut; f32 [rows, hyper_num]) and the four packed keep masks, in place of
        the hashed draws."""
        B, d, nu = interaction.shape[1], self.embedding_dim, self.n_users
        self._ws = ops.grow_workspace(L.lib().rsx_lgm_loss_ws_bytes, self._ws, B, d)
        for k, n in enumerate((nu, self.n_items)):
            if L.lib().rsx_lgm_ssl_ws_bytes(n, B, d) > self._ssl_ws[k].numel():
                self._ssl_ws[k] = ssl_workspace(n, B, d, self.device)
        trip = interaction[:3].contiguous()
        tables = self._tables(draws)
        Gv, Gt = tables[3], tables[4]
        keep = {}
        loss = _LgmLoss.apply((nu, self.alpha, self.reg_weight, self._ws, keep), trip, *tables)
        su = _Ssl.apply((self.tau, self._ssl_ws[0]), trip[0], Gv[:nu], Gt[:nu])
        si = _Ssl.apply((self.tau, self._ssl_ws[1]), trip[1], Gv[nu:], Gt[nu:])
        self.last_terms, self.last_ssl = keep["terms"], (su.detach(), si.detach())
        return loss + self.cl_weight * (su + si)

    # ------------------------------------------------------------ evaluation
    def _eval_tables(self, draws=None):
        with torch.no_grad():
            u, i, _ = self.forward(draws)
            return u.contiguous(), i.contiguous()
