"""The autograd blocks and host-side scaffolding the graph models share (SMORE, BM3, MGCN,
FREEDOM, LATTICE): the mean-of-layers propagation, dense (`_PropMean`) and on the tagged
batch rows (`_PropMeanRows`, `_RowTags`, `ui_backbone`), the joint [U; I] table (`_join_tables`,
`_ego`), the per-batch-size index caches (`_RowsOff`, `_BatchIndex`), a sparse operator with
its transpose (`_DevGraph`) and the kNN item graphs (`knn_graph`, `knn_graph_device`,
`load_reference_knn`, `cached_knn`).  The dense layer blocks are rsx.dense's.

Models import this module; it imports no model.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import graph, ops


class _SpMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, A, AT):
        ctx.AT = AT
        return A.spmm(x.contiguous())

    @staticmethod
    def backward(ctx, g):
        return ctx.AT.spmm(g.contiguous()), None, None


def _prop_mean(A, x, K):
    import ctypes as C

    x = x.contiguous()
    out = torch.empty_like(x)
    s, h0, h1 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    d = x.shape[1]
    rc = L.lib().rsx_lightgcn_forward(C.byref(A.struct), d, K, ops._p(x), ops._p(s), ops._p(h0), ops._p(h1),
                                      ops._p(out), ops._p(A.slab(d)), ops._stream())
    L.check(rc, "rsx_lightgcn_forward")
    return out


class _PropMean(torch.autograd.Function):
    """mean_{k=0..K} A^k x; the backward is the same mean on AT, the transposed operator
    (None: A is symmetric and is its own transpose)."""

    @staticmethod
    def forward(ctx, x, A, K, AT=None):
        ctx.AT, ctx.K = AT if AT is not None else A, K
        return _prop_mean(A, x, K)

    @staticmethod
    def backward(ctx, g):
        return _prop_mean(ctx.AT, g, ctx.K), None, None, None


class _Joined(torch.autograd.Function):
    """torch.cat([U, I]) without the copy when U and I are adjacent row blocks of one
    buffer (SMORE keeps its user and item-id tables so: rsx.smore.SMORE.__init__): the
    output aliases their storage (a new tensor, not an autograd view of either input);
    backward: the two row blocks of the gradient, as cat's."""

    @staticmethod
    def forward(ctx, u, i):
        ctx.nu = u.shape[0]
        out = torch.empty(0, dtype=u.dtype, device=u.device)
        out.set_(u.untyped_storage(), u.storage_offset(), (u.shape[0] + i.shape[0], u.shape[1]), (u.shape[1], 1))
        return out

    @staticmethod
    def backward(ctx, g):
        return g[: ctx.nu], g[ctx.nu:]


def _ego(u: torch.Tensor, i: torch.Tensor) -> torch.Tensor:
    """[U; I] (the reference's torch.cat([user_embeds, item_embeds]), smore.py:278)."""
    adjacent = (u.device == i.device and u.dtype == i.dtype and u.is_contiguous() and i.is_contiguous()
                and u.dim() == 2 and i.dim() == 2 and u.shape[1] == i.shape[1]
                and u.untyped_storage().data_ptr() == i.untyped_storage().data_ptr()
                and i.storage_offset() == u.storage_offset() + u.numel())
    return _Joined.apply(u, i) if adjacent else torch.cat([u, i], dim=0)


def _join_tables(user_embedding: nn.Embedding, item_embedding: nn.Embedding, device) -> None:
    """Moves the two tables (created and initialised by the caller, on the CPU generator as the
    reference does) into adjacent row blocks of one device buffer: the UI backbone's ego table
    [U; I] is then that buffer itself (_ego), no per-forward concatenation copy."""
    user_embedding.weight, item_embedding.weight = _join_params(user_embedding.weight, item_embedding.weight, device)


def _join_params(u: torch.Tensor, i: torch.Tensor, device):
    """_join_tables for two bare tables (a model that keeps nn.Parameters, not nn.Embeddings):
    the two new nn.Parameters, adjacent row blocks of one device buffer."""
    u, i = u.detach(), i.detach()
    nu = u.shape[0]
    joint = torch.empty(nu + i.shape[0], u.shape[1], dtype=torch.float32, device=device)
    joint[:nu].copy_(u)
    joint[nu:].copy_(i)
    return nn.Parameter(joint[:nu]), nn.Parameter(joint[nu:])


class _RowsOff(dict):
    """off[B] = [0] * B ++ [n_users] * 2 B (int64, on the device), made once per batch length
    and kept: a captured graph step must not allocate.  rows(trip) are the batch's rows of
    [U; I] for int64 triplets [3, B]: [users; nu + positives; nu + negatives]."""

    def __init__(self, n_users: int, device):
        super().__init__()
        self.n_users, self.device = int(n_users), device

    def __missing__(self, B: int) -> torch.Tensor:
        off = self[B] = torch.cat([torch.zeros(B, dtype=torch.int64, device=self.device),
                                   torch.full((2 * B,), self.n_users, dtype=torch.int64, device=self.device)])
        return off

    def rows(self, trip: torch.Tensor) -> torch.Tensor:
        return trip.reshape(-1) + self[trip.shape[1]]


class _BatchIndex(dict):
    """idx[B] = (ar, trip): arange(B) and the compact triplets (b, b, B + b) of the batch rows
    [users; B + positives; 2B + negatives] (int64, on the device), made once per batch size
    and kept, like _RowsOff."""

    def __init__(self, device):
        super().__init__()
        self.device = device

    def __missing__(self, B: int):
        ar = torch.arange(B, dtype=torch.int64, device=self.device)
        c = self[B] = (ar, torch.stack([ar, ar, ar + B]).contiguous())
        return c


class _RowTags:
    """Batch-row tags for the tagged propagation: row r is in the batch when
    row_tag[r] == *tag_dev; `mark` bumps the device tag and tags the batch's rows
    (one launch, rsx_tag_rows_next; no host sync: graph-capture safe).  tag_dev is
    {tag, ticket}: the products read word 0."""

    def __init__(self, n: int, device):
        self.row_tag = torch.zeros(n, dtype=torch.int32, device=device)
        self.tag_dev = torch.zeros(2, dtype=torch.int32, device=device)

    def mark(self, rows: torch.Tensor):
        rows = rows.to(torch.int64).contiguous()
        L.check(L.lib().rsx_tag_rows_next(ops._p(self.row_tag), ops._p(rows), rows.numel(), ops._p(self.tag_dev),
                                          ops._stream()), "rsx_tag_rows_next")


class _PropMeanRows(torch.autograd.Function):
    """mean_{k=0..K} A^k x, needed at the tagged rows only, for a symmetric A or, with AT, for
    an A whose transpose is the operator AT (the backward runs on AT) (K <= 4;
    the batch rows of the SMORE training loss): E^1..E^{K-1} stored (no running sum),
    the last layer and the mean on the tagged rows only, in the running sum's order
    (((E0 + E1) + E2) + E3) + A E3 (other rows of the output are left unwritten).  The
    backward is Horner on the incoming gradient G, which is zero off the tagged rows
    (`rows`: the forward's rows, re-tagged in the backward, so several forwards may run
    before their backwards, as in a sum of batch losses):
    H = G + A H from H = G, the first layer gathering only the tagged rows of G, every
    layer reading G on the tagged rows only, the last scaled by 1/(K+1) (the dense
    path's arithmetic: the same mean operator applied to G)."""

    @staticmethod
    def forward(ctx, x, A, K, tags, rows=None, AT=None):
        x = x.contiguous()
        n, d = x.shape
        out = torch.empty_like(x)
        hs = torch.empty(max(K - 1, 1), n, d, dtype=torch.float32, device=x.device)
        cur = x
        for k in range(1, K):
            A.spmm_epi(cur, ops.epi(L.RSX_EPI_STORE, y=hs[k - 1]), d)
            cur = hs[k - 1]
        stored = dict(zip(("s_in", "r_add", "aux", "e0"), [x] + [hs[i] for i in range(K - 1)]))
        e = ops.epi(L.RSX_EPI_FINAL, beta=1.0 / (K + 1), f=out, row_tag=tags.row_tag, tag_dev=tags.tag_dev, **stored)
        e.tag_flags = L.RSX_TAG_ROWS
        A.spmm_epi(cur, e, d)
        # ctx.A: the backward's operator
        ctx.A, ctx.K, ctx.tags, ctx.rows = AT if AT is not None else A, K, tags, rows
        return out

    @staticmethod
    def backward(ctx, g):
        A, K, tags = ctx.A, ctx.K, ctx.tags
        if ctx.rows is not None:
            # re-tag this forward's rows: a later forward (another calculate_loss before this
            # backward) may have moved the tag on, and G is zero off exactly these rows
            tags.mark(ctx.rows)
        g = g.contiguous()
        d = g.shape[1]
        bufs = torch.empty(2, *g.shape, dtype=torch.float32, device=g.device)
        h = g
        for k in range(1, K + 1):
            y = bufs[k & 1]
            e = ops.epi(L.RSX_EPI_ADD, beta=1.0 / (K + 1) if k == K else 1.0, y=y, s_in=g, row_tag=tags.row_tag,
                        tag_dev=tags.tag_dev)
            e.tag_flags = L.RSX_TAG_SPARSE_S | (L.RSX_TAG_SPARSE_X if k == 1 else 0)
            A.spmm_epi(h, e, d)
            h = y
        return h, None, None, None, None, None


def ui_backbone(model, ego, A, K, rows=None, bw_rows=None, AT=None):
    """mean_{k=0..K} A^k ego, a model's UI backbone.  With `rows` (the batch's rows of [U; I])
    and 1 <= K <= 4 it is exact on those rows only: the tagged propagation, the rows marked in
    model._tags (made on first use).  bw_rows: the rows the backward's incoming gradient is
    defined on, when they are not `rows`; AT: the transposed operator of an A that is not
    symmetric."""
    if rows is not None and 1 <= K <= 4:
        if model._tags is None:
            model._tags = _RowTags(ego.shape[0], model.device)
        model._tags.mark(rows)
        return _PropMeanRows.apply(ego, A, K, model._tags, bw_rows if bw_rows is not None else rows, AT)
    return _PropMean.apply(ego, A, K, AT)


def knn_graph(feat: np.ndarray, k: int):
    """build_sim + build_knn_normalized_graph(sparse, 'sym') (src/utils/utils.py:134-181) on the CPU,
    float32 as the reference: cosine similarities, top-k per row, deg = sum of kept values,
    w = d_r^-1/2 * s * d_c^-1/2.  Returns (rows, cols, vals)."""
    x = torch.from_numpy(feat)
    xn = x.div(torch.norm(x, p=2, dim=-1, keepdim=True))
    n = xn.shape[0]
    rows, cols, vals = [], [], []
    step = max(1, (1 << 26) // max(n, 1))
    for s in range(0, n, step):
        sim = torch.mm(xn[s:s + step], xn.t())
        v, i = torch.topk(sim, k, dim=-1)
        rows.append(torch.arange(s, s + sim.shape[0]).repeat_interleave(k))
        cols.append(i.reshape(-1))
        vals.append(v.reshape(-1))
    r, c, v = torch.cat(rows), torch.cat(cols), torch.cat(vals)
    deg = torch.zeros(n, dtype=v.dtype).index_add_(0, r, v)
    dis = deg.pow_(-0.5)
    dis.masked_fill_(dis == float("inf"), 0)
    w = dis[r] * v * dis[c]
    return r.numpy().astype(np.int64), c.numpy().astype(np.int64), w.numpy().astype(np.float32)


def knn_graph_device(feat: torch.Tensor, k: int):
    """build_sim + build_knn_normalized_graph(sparse, 'sym') on the device through the
    hand-written builder rsx_knn_graph (csrc/knn.hip: row normalisation, the cosine
    similarities on f32 MFMA with the per-row top-k kept in registers — the n x n
    matrix is never formed — and the sym-norm in the reference's order: deg = the
    row's kept values added in rank order, 1/sqrt(deg), (d_r * v) * d_c).  The
    similarities are f32 MFMA sums, so values can differ from the CPU build in the
    last bits and neighbours at exact near-ties can swap (tests/test_gpu_smore.py
    pins that).  Returns host (rows, cols, vals) like knn_graph."""
    x = feat.detach().to(torch.float32).contiguous()
    n = x.shape[0]
    if k > 32 or k > n:
        raise ValueError(f"rsx_knn_graph: k = {k} (supported: k <= 32 and k <= n = {n})")
    _, i, w = ops.knn_lists(x, k)
    r = np.repeat(np.arange(n, dtype=np.int64), k)
    return r, i.reshape(-1).cpu().numpy().astype(np.int64), w.reshape(-1).cpu().numpy().astype(np.float32)


def load_reference_knn(path: str, n: int):
    """The reference's own kNN cache (smore.py:46-47,56-62: `torch.save` of the
    sparse [n, n] graph as `{image,text}_adj_{k}_{sparse}.pt` in the dataset
    directory), read with the loader that executes nothing from the file
    (`weights_only=True`).  Returns (rows, cols, vals) in coalesced order, or None
    when the file is absent, refused by the safe loader or not an [n, n] graph."""
    if not os.path.exists(path):
        return None
    try:
        t = torch.load(path, map_location="cpu", weights_only=True)
    except Exception:  # noqa: BLE001 - a file the safe loader refuses is rebuilt, not trusted
        return None
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or tuple(t.shape) != (n, n):
        return None
    if t.layout == torch.sparse_coo:
        t = t.coalesce()
        idx, val = t.indices(), t.values()
    elif t.layout == torch.strided:  # is_sparse False: build_knn_normalized_graph's dense matrix
        idx = t.nonzero().t()
        val = t[idx[0], idx[1]]
    else:
        return None
    return (idx[0].numpy().astype(np.int64), idx[1].numpy().astype(np.int64),
            val.to(torch.float32).numpy().astype(np.float32))


def cached_knn(root, name, feat, k, sparse, knn_mode, device):
    """kNN item graph (reference smore.py:45-75): the reference's own
    {name}_adj_{k}_{sparse}.pt cache when the dataset directory holds one, else
    built on the device (knn_graph_device) or, with rsx_knn: host (the default when
    rsx_sampler is host), by the CPU restatement of the reference's build."""
    # a cache the reference wrote for this dataset is the graph its runs trained on: use it
    ref = load_reference_knn(os.path.join(root, f"{name}_adj_{k}_{sparse}.pt"), feat.shape[0])
    if ref is not None:
        return ref
    device_build = knn_mode == "device"
    path = os.path.join(root, f"rsx_{name}_knn_{k}{'_dev' if device_build else ''}.npz")
    f = feat.detach().cpu().numpy()
    sig = np.array([f.shape[0], f.shape[1], float(np.float64(f[:4].sum())), float(np.float64(f[-4:].sum()))])
    if os.path.exists(path):
        try:
            z = np.load(path)
            if np.array_equal(z["sig"], sig):
                return z["r"], z["c"], z["v"]
        except (OSError, ValueError, KeyError, EOFError):  # another rank still writing it: rebuild
            pass
    r, c, v = knn_graph_device(feat.detach().to(device), k) if device_build else knn_graph(f, k)
    if ops._world()[1] == 0:  # one writer per job (every rank builds the same graph)
        try:
            os.makedirs(root, exist_ok=True)
            tmp = f"{path}.{os.getpid()}.tmp.npz"
            np.savez(tmp, r=r, c=c, v=v, sig=sig)
            os.replace(tmp, path)
        except OSError:
            pass
    return r, c, v


class _DevGraph:
    """A sparse operator with its transpose on the device (forward / backward SpMM)."""

    def __init__(self, rows, cols, vals, n_rows, n_cols, device, chunk):
        self.A = ops.DeviceCSR(*graph.to_csr(rows, cols, vals, n_rows, n_cols), n_cols, device, chunk)
        self.AT = ops.DeviceCSR(*graph.to_csr(cols, rows, vals, n_cols, n_rows), n_rows, device, chunk)

    def __call__(self, x):
        return _SpMM.apply(x, self.A, self.AT)
