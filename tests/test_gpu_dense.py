"""The dense layer blocks on the GPU: the kernels of csrc/dense.hip (rsx.dense's wrappers) against
torch float64 on the CPU.

Bound: helpers.check_vs_f32 — 1e-4 of the tensor's scale, or 4x the error the float32 torch
composition of the same ops (on the CPU) makes against the same float64 values, whichever is
larger.  leaky_relu's slope is discontinuous at zero, so a test flags the rows where the float64
run has any pre-activation within 1e-5 of that tensor's scale of zero (about 7x the rounding of a
<= 512-term float32 dot product), zeroes the upstream gradient on those rows for kernel and
restatement alike, and asserts that at most 5 % of the rows are flagged (helpers.unflagged).

Every sum is in a fixed order (no float atomics): two runs are bit-equal."""
import numpy as np
import pytest
import torch

import mmgcn_ref as R
from helpers import check_vs_f32, dev, unflagged

pytestmark = pytest.mark.gpu
c = lambda t: t.detach().cpu().numpy()  # noqa: E731
f32 = lambda a: a.astype(np.float32)  # noqa: E731


# ------------------------------------------------------------ the wide product
# (K or (K0, K1), N, B given [K, N], n, leaky): each extreme of K, N, n, both layouts, the two-segment input
GEMM_CASES = [(32, 32, False, 5, False), (32, 256, True, 65, True), (96, 96, False, 1001, True), (96, 32, True, 5, False),
              (256, 256, True, 65, True), (256, 96, False, 1001, False), (384, 256, False, 65, True),
              (384, 32, True, 1001, True), (384, 96, True, 5, True), ((96, 64), 96, False, 65, True),
              ((96, 64), 256, True, 1001, False), (32, 96, False, 1001, True)]


@pytest.mark.parametrize("K,N,b_kn,n,act", GEMM_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_wide_product_and_its_gradients_vs_float64(cuda, K, N, b_kn, n, act):
    from rsx import dense as M

    ks = K if isinstance(K, tuple) else (K,)
    Kt = sum(ks)
    rng = np.random.default_rng(1000 + Kt + N + n)
    xs = [f32(rng.standard_normal((n, k)) * 0.5) for k in ks]
    B = f32(rng.standard_normal((Kt, N) if b_kn else (N, Kt)) / np.sqrt(Kt))
    b = f32(rng.standard_normal(N) * 0.1)

    def compose(dtype, go=None):
        t = lambda a: torch.from_numpy(a).to(dtype).requires_grad_(True)  # noqa: E731
        X, Bt, bt = [t(a) for a in xs], t(B), t(b)
        pre = torch.cat(X, dim=1) @ (Bt if b_kn else Bt.t()) + bt
        y = R.leaky(pre) if act else pre
        if go is not None:
            (y * go.to(dtype)).sum().backward()
        return pre.detach(), y.detach(), [a.grad for a in X], Bt.grad, bt.grad

    pre64 = compose(torch.float64)[0]
    keep = unflagged([pre64], n) if act else torch.ones(n, 1, dtype=torch.float64)
    go = torch.from_numpy(f32(rng.standard_normal((n, N)))).double() * keep
    _, y64, gx64, gB64, gb64 = compose(torch.float64, go)
    _, y32, gx32, gB32, gb32 = compose(torch.float32, go)
    X = [dev(a, cuda, True) for a in xs]
    Bd, bd = dev(B, cuda, True), dev(b, cuda, True)
    y = M._Gemm.apply(X[0], X[1] if len(X) > 1 else None, Bd, bd, b_kn, act)
    check_vs_f32("y", c(y), y64, y32)
    y.backward(dev(go.float().numpy(), cuda))
    for j, t in enumerate(X):
        check_vs_f32(f"dX{j}", c(t.grad), gx64[j], gx32[j])
    check_vs_f32("dB", c(Bd.grad), gB64, gB32)
    check_vs_f32("db", c(bd.grad), gb64, gb32)


# (K, N, n): a K below one 32-slab, a slab plus a partial one, a K that is a multiple of 4 and not
# of 32, half a column tile, n below, one past and far past the 64-row tile
CONST_INPUT_CASES = [(4, 32, 65), (36, 64, 5), (36, 64, 65), (36, 32, 1001), (100, 256, 1001)]


@pytest.mark.parametrize("K,N,n", CONST_INPUT_CASES, ids=lambda v: str(v))
def test_wide_product_on_a_constant_input_vs_float64(cuda, K, N, n):
    """leaky(X W^T + b) on an X that needs no gradient (a content MLP on a feature table of any
    width that is a multiple of 4): no data-gradient launch, the masked rows from leaky_bwd."""
    from rsx import dense as M

    rng = np.random.default_rng(1000 + K + N + n)
    x = f32(rng.standard_normal((n, K)) * 0.5)
    B = f32(rng.standard_normal((N, K)) / np.sqrt(K))
    b = f32(rng.standard_normal(N) * 0.1)

    def compose(dtype, go=None):
        t = lambda a: torch.from_numpy(a).to(dtype).requires_grad_(True)  # noqa: E731
        Bt, bt = t(B), t(b)
        pre = torch.from_numpy(x).to(dtype) @ Bt.t() + bt
        y = R.leaky(pre)
        if go is not None:
            (y * go.to(dtype)).sum().backward()
        return pre.detach(), y.detach(), Bt.grad, bt.grad

    pre64 = compose(torch.float64)[0]
    keep = unflagged([pre64], n)
    go = torch.from_numpy(f32(rng.standard_normal((n, N)))).double() * keep
    _, y64, gB64, gb64 = compose(torch.float64, go)
    _, y32, gB32, gb32 = compose(torch.float32, go)
    X, Bd, bd = dev(x, cuda), dev(B, cuda, True), dev(b, cuda, True)
    y = M._Gemm.apply(X, None, Bd, bd, False, True)
    check_vs_f32("y", c(y), y64, y32)
    y.backward(dev(go.float().numpy(), cuda))
    assert X.grad is None
    check_vs_f32("dB", c(Bd.grad), gB64, gB32)
    check_vs_f32("db", c(bd.grad), gb64, gb32)


def test_wide_product_epilogues(cuda):
    """The residual output (y and y + r from one launch), the output mask, the masked input rows."""
    from rsx import dense as M

    rng = np.random.default_rng(5)
    n, K, N = 65, 96, 64
    x, W, b, r, m = (f32(rng.standard_normal(s)) for s in ((n, K), (N, K), (N,), (n, N), (n, N)))
    saved = f32(rng.standard_normal((n, K)))
    X, Wd, bd, Rd, Md, Sd = (dev(a, cuda) for a in (x, W, b, r, m, saved))
    want = R.leaky(torch.from_numpy(x).double() @ torch.from_numpy(W).double().t() + torch.from_numpy(b).double())
    u, xh = M.gemm(X, Wd, N, False, bias=bd, act=True, r=Rd)
    check_vs_f32("u", c(u), want, want.float())
    assert torch.equal(xh, u + Rd)
    masked = M.gemm(X, Wd, N, False, bias=bd, act=True, my=Md)
    assert torch.equal(masked, torch.where(Md > 0, u, u * np.float32(0.01)))
    xm = torch.empty_like(X)
    y = M.gemm(X, Wd, N, False, mx=Sd, xm_out=xm)
    assert torch.equal(xm, torch.where(Sd > 0, X, X * np.float32(0.01)))
    assert torch.equal(y, M.gemm(xm, Wd, N, False))
    for bad in (dict(n_out=40), dict(k=6)):
        with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):
            if "k" in bad:
                M.gemm(dev(x[:, :6].copy(), cuda), dev(W[:, :6].copy(), cuda), N, False)
            else:
                M.gemm(X, dev(W[:40].copy(), cuda), 40, False)


# ------------------------------------------------------------- the leaky mask
# (4 elements: one float4; the second: one grid-stride pass past the 4096-block cap)
@pytest.mark.parametrize("n_elems", [4, 4 * (4096 * 256 + 3)])
def test_leaky_bwd_is_exact(cuda, n_elems):
    from rsx import dense as M

    rng = np.random.default_rng(n_elems % 1000)
    g = dev(f32(rng.standard_normal(n_elems)).reshape(-1, 4), cuda)
    y = dev(f32(rng.standard_normal(n_elems)).reshape(-1, 4), cuda)
    y[0, 1] = 0.0  # y = 0 takes the slope, as leaky_relu's backward does
    got = M.leaky_bwd(g, y)
    assert torch.equal(got, torch.where(y > 0, g, g * np.float32(0.01)))


# ------------------------------------------------------------------ normalise
@pytest.mark.parametrize("n,w", [(5, 256), (67, 256), (130, 32), (9, 384)])
def test_normalize_forward_and_gradient(cuda, n, w):
    from rsx import dense as M

    rng = np.random.default_rng(n + w)
    x = rng.standard_normal((n, w)).astype(np.float32)
    x[n // 2] = 0.0  # an all-zero row: zeros out, g / 1e-12 back (the clamp passes nothing through the norm)
    g = rng.standard_normal((n, w)).astype(np.float32) * 1e-6
    res = {}
    for dtype in (torch.float64, torch.float32):
        t = torch.from_numpy(x).to(dtype).requires_grad_(True)
        y = torch.nn.functional.normalize(t)
        y.backward(torch.from_numpy(g).to(dtype))
        res[dtype] = (y.detach(), t.grad)
    X = dev(x, cuda, True)
    y = M._Normalize.apply(X)
    assert not c(y)[n // 2].any()
    y.backward(dev(g, cuda))
    check_vs_f32("y", c(y), *(res[k][0] for k in res))
    rest = np.arange(n) != n // 2  # (the zero row's gradient is 1e12 times the others': checked apart)
    check_vs_f32("g_x", c(X.grad)[rest], *(res[k][1][rest] for k in res))
    check_vs_f32("g_x, zero row", c(X.grad)[~rest], *(res[k][1][~rest] for k in res))
    # in place, as the image branch writes its item rows
    buf = dev(x, cuda)
    y2, _ = M.normalize_fwd(buf, out=buf)
    assert torch.equal(y2, y.detach())


def test_colsum_is_ordered(cuda):
    from rsx import dense as M

    g = torch.from_numpy(np.random.default_rng(2).standard_normal((1001, 320)).astype(np.float32))
    got = M.colsum(g.to(cuda))
    check_vs_f32("colsum", c(got), g.double().sum(0), g.sum(0))
    assert torch.equal(got, M.colsum(g.to(cuda)))
