"""The dense layer blocks the models share (MMGCN, GRCN, DualGNN; BM3, MGCN, FREEDOM, LATTICE;
SMORE, MGCN's fused blocks), with autograd: the wide f32-MFMA product with its epilogues (`gemm`,
`_Gemm`), F.normalize over rows (`normalize_fwd`, `normalize_bwd`, `_Normalize`), the ordered
column sum (`colsum`) and the leaky mask (`leaky_bwd`) on csrc/dense.hip; the whole-table
projection (`_Project`) on rsx_linear_rows_fwd / rsx_linear_bwd; the batched weight gradient
(`_wgrad`) on rsx_smore_wgrad.

Models import this module; it imports no model.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from . import ops


# Every Function below keeps its tensors with save_for_backward, its own outputs included: an
# output held on ctx directly is a cycle ctx -> output -> grad_fn -> ctx that nothing frees, so
# an eager batch's autograd graph (its AccumulateGrad nodes bound to the eager stream) would
# survive into the next batch's HIP-graph capture, whose backward then syncs with a stream
# outside the capture (rsx.trainer.Trainer.train_step).
def _col_block(t: torch.Tensor, col0: int) -> int:
    return t.data_ptr() + 4 * int(col0)


def gemm(x0, B, n_out: int, b_kn: bool, *, k0=None, x1=None, mx=None, xm_out=None, bias=None, act=False, my=None,
         r=None, y=True, b_col0: int = 0):
    """rsx_dense_gemm on contiguous f32 tensors: V = act((x0[:, :k0] .* slope(mx) | x1) op(B) + bias)
    .* slope(my).  B: the weight (b_kn: [K, n_out], else [n_out, K]); b_col0 selects the column
    block [b_col0, b_col0 + width) of a wider weight.  Returns y (V), or y2 = V + r when r is
    given, or both (y, y2) when r is given and y is True."""
    ops._gpu(x0, x1, mx, xm_out, B, bias, my, r)
    n = x0.shape[0]
    a = L.DenseGemmArgs()
    a.n, a.n_out, a.b_kn, a.act = n, int(n_out), int(b_kn), int(act)
    a.k0 = int(x0.shape[1] if k0 is None else k0)
    a.x0, a.ld0 = x0.data_ptr(), x0.shape[1]
    a.k1 = 0
    if x1 is not None:
        a.x1, a.ld1, a.k1 = x1.data_ptr(), x1.shape[1], x1.shape[1]
    K = a.k0 + a.k1
    if mx is not None:
        a.mx, a.ldmx = mx.data_ptr(), mx.shape[1]
    rows_b, cols_b = (K, n_out) if b_kn else (n_out, K)
    if B.shape[0] != rows_b or B.shape[1] < b_col0 + cols_b:
        raise RuntimeError(f"dense gemm: weight {tuple(B.shape)} does not hold a [{rows_b}, {cols_b}] block at column {b_col0}")
    a.B, a.ldb = _col_block(B, b_col0), B.shape[1]
    for name, t, shape in (("xm_out", xm_out, (n, a.k0)), ("my", my, (n, n_out)), ("r", r, (n, n_out))):
        if t is not None:
            if tuple(t.shape) != shape:
                raise RuntimeError(f"dense gemm: {name} {tuple(t.shape)}, expected {shape}")
            setattr(a, name, t.data_ptr())
    if mx is not None and (mx.shape[0] != n or mx.shape[1] < a.k0):
        raise RuntimeError("dense gemm: mx does not cover x0")
    if bias is not None:
        if bias.numel() != n_out:
            raise RuntimeError("dense gemm: bias length")
        a.bias = bias.data_ptr()
    out = []
    if y or r is None:
        yt = torch.empty(n, n_out, dtype=torch.float32, device=x0.device)
        a.y = yt.data_ptr()
        out.append(yt)
    if r is not None:
        y2 = torch.empty(n, n_out, dtype=torch.float32, device=x0.device)
        a.y2 = y2.data_ptr()
        out.append(y2)
    L.check(L.lib().rsx_dense_gemm(C.byref(a), ops._stream()), "rsx_dense_gemm")
    return out[0] if len(out) == 1 else tuple(out)


def colsum(g: torch.Tensor) -> torch.Tensor:
    """The column sums of g [n, N] in a fixed order (rsx_dense_colsum)."""
    ops._gpu(g)
    n, N = g.shape
    lib = L.lib()
    out = torch.empty(N, dtype=torch.float32, device=g.device)
    ws = torch.empty(max(int(lib.rsx_dense_colsum_ws_bytes(n, N)), 4), dtype=torch.uint8, device=g.device)
    L.check(lib.rsx_dense_colsum(ops._p(g), n, N, ops._p(out), ops._p(ws), ws.numel(), ops._stream()),
            "rsx_dense_colsum")
    return out


def leaky_bwd(g: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """g .* slope(y) for a saved leaky_relu output y (rsx_dense_leaky_bwd)."""
    ops._gpu(g, y)
    if g.shape != y.shape:
        raise RuntimeError(f"dense leaky_bwd: g {tuple(g.shape)} and y {tuple(y.shape)} differ")
    out = torch.empty_like(g)
    L.check(L.lib().rsx_dense_leaky_bwd(ops._p(g), ops._p(y), g.numel(), ops._p(out), ops._stream()),
            "rsx_dense_leaky_bwd")
    return out


def normalize_fwd(x: torch.Tensor, out: torch.Tensor | None = None):
    """(F.normalize(x) over rows, the divisors max(|x|, 1e-12)); `out` may be x."""
    ops._gpu(x, out)
    n, w = x.shape
    y = torch.empty_like(x) if out is None else out
    den = torch.empty(n, dtype=torch.float32, device=x.device)
    L.check(L.lib().rsx_dense_normalize_fwd(ops._p(x), n, w, ops._p(y), ops._p(den), ops._stream()),
            "rsx_dense_normalize_fwd")
    return y, den


def normalize_bwd(gy, y, den):
    ops._gpu(gy, y, den)
    n, w = y.shape
    gx = torch.empty_like(y)
    L.check(L.lib().rsx_dense_normalize_bwd(ops._p(gy), ops._p(y), ops._p(den), n, w, ops._p(gx), ops._stream()),
            "rsx_dense_normalize_bwd")
    return gx


class _Normalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y, den = normalize_fwd(x.contiguous())
        ctx.save_for_backward(y, den)
        return y

    @staticmethod
    def backward(ctx, g):
        return normalize_bwd(g.contiguous(), *ctx.saved_tensors)


class _Gemm(torch.autograd.Function):
    """Y = act(X op(B) + bias) with X the column segments x0 | x1 (x1 may be None): the wide product,
    its data gradients through the same kernel, its weight gradient through rsx_linear_wgrad.
    The rows g .* slope(y) the weight and bias gradients of an `act` product need come out of
    the first data-gradient launch; with no data gradient wanted (a constant X of any width
    that is a multiple of 4: a content MLP on a feature table) leaky_bwd forms them."""

    @staticmethod
    def forward(ctx, x0, x1, B, bias, b_kn, act):
        x0, B = x0.contiguous(), B.contiguous()
        x1 = None if x1 is None else x1.contiguous()
        n_out = B.shape[1] if b_kn else B.shape[0]
        y = gemm(x0, B, n_out, b_kn, x1=x1, bias=bias, act=act)
        ctx.b_kn, ctx.act, ctx.has_bias = b_kn, act, bias is not None
        ctx.save_for_backward(x0, x1, B, y)
        return y

    @staticmethod
    def backward(ctx, g):
        x0, x1, B, y = ctx.saved_tensors
        g = g.contiguous()
        k0 = x0.shape[1]
        need = ctx.needs_input_grad
        gx0 = gx1 = None
        want0 = need[0]
        want1 = x1 is not None and need[1]
        go = None
        if ctx.act:
            go = torch.empty_like(g) if want0 or want1 else leaky_bwd(g, y)
        mx = y if ctx.act else None
        # d X = (g .* slope(y)) op(B)^T: B seen in its other layout, a column block a segment
        if ctx.b_kn:  # B [K, N]: d X0 = G B[:k0]^T
            if want0:
                gx0 = gemm(g, B[:k0], k0, False, mx=mx, xm_out=go)
            if want1:
                gx1 = gemm(g, B[k0:], x1.shape[1], False, mx=mx, xm_out=go if gx0 is None else None)
        else:  # B [N, K]: d X0 = G B[:, :k0]
            if want0:
                gx0 = gemm(g, B, k0, True, mx=mx, xm_out=go)
            if want1:
                gx1 = gemm(g, B, x1.shape[1], True, mx=mx, xm_out=go if gx0 is None else None, b_col0=k0)
        gz = go if ctx.act else g
        gB = gb = None
        if need[2]:
            parts = [ops.linear_wgrad(x, gz) if ctx.b_kn else ops.linear_wgrad(gz, x) for x in (x0, x1) if x is not None]
            gB = parts[0] if len(parts) == 1 else torch.cat(parts, dim=0 if ctx.b_kn else 1)
        if ctx.has_bias and need[3]:
            gb = colsum(gz)
        return gx0, gx1, gB, gb, None, None


class _Project(torch.autograd.Function):
    """x W^T + b over every row of a feature table: rsx_linear_rows_fwd, and rsx_linear_bwd
    (dX, dW, db in one pass over the rows) for the dense gradient BM3 sends back."""

    @staticmethod
    def forward(ctx, x, W, b):
        x, W, b = x.contiguous(), W.contiguous(), b.contiguous()
        ctx.save_for_backward(x, W)
        return ops.linear_rows_fwd(x, W, b, None)

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        dw, dx, db = ops.linear_bwd(g.contiguous(), x, W, bias=True)
        return dx, dw, db


def _wgrad(pairs, d, device):
    """[(dz, x, has_bias)] -> [(dW, db | None)] through rsx_smore_wgrad (<= 8 pairs)."""
    lib = L.lib()
    n = pairs[0][0].shape[0]
    dws = [torch.empty(d, d, dtype=torch.float32, device=device) for _ in pairs]
    dbs = [torch.empty(d, dtype=torch.float32, device=device) if hb else None for _, _, hb in pairs]
    ws = torch.empty(max(int(lib.rsx_smore_wgrad_ws_bytes(n, d, len(pairs))), 4), dtype=torch.uint8,
                     device=device)
    L.check(lib.rsx_smore_wgrad(len(pairs), ops._arr([p[0] for p in pairs]), ops._arr([p[1] for p in pairs]),
                                ops._arr(dws), ops._arr(dbs), n, d, ops._p(ws), ws.numel(), ops._stream()),
            "rsx_smore_wgrad")
    return list(zip(dws, dbs))
