"""LGMRec on the GPU: the table-wide InfoNCE, the hyperedge assignments, the hypergraph products
and the loss (csrc/lgmrec.hip, rsx.lgmrec) against the float64 restatement (tests/lgmrec_ref.py),
and the model (rsx.lgmrec.LGMRec) against the reference's own run
(tests/golden/lgmrec_step0_small.npz, lgmrec_small.npz).

Bounds (tests/test_gpu_lattice.py's rules).
* A loss word: 1e-5 relative to the restatement, or 4x the error the same formulas in float32
  torch on the CPU make against it on the same inputs, whichever is larger.
* A gradient: 1e-4 of the tensor's scale, or 4x that float32 error, whichever is larger.
* Assignment forward: 1e-6 absolute.  Hypergraph forward: 1e-5 of sum |terms| per element.
* Model: see the tests.
"""
import numpy as np
import pytest
import torch

import lgmrec_ref as R
from helpers import (assert_same_run, check_vs_f32, coo_sorted, csr_to_sorted, dev, loaders, make_model,
                     topk_equal_modulo_ties, write_dataset)

pytestmark = pytest.mark.gpu
TAU = float(np.float32(0.2))  # the float32 tau the kernels are handed


def _check_word(name, got, ref, tor):
    bound = max(1e-5 * abs(ref), 4 * abs(tor - ref))
    print(f"  {name}: {got:.8f} vs {ref:.8f}, torch f32 err {abs(tor - ref):.3e}, bound {bound:.3e}")
    assert np.isfinite(got) and abs(got - ref) <= bound, name


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


# ------------------------------------------------------------------ 1. the InfoNCE
def _run_ssl(T1, T2, idx, cuda):
    from rsx import lgmrec as LG

    a = dev(T1, cuda, True)
    b = a if T2 is None else dev(T2, cuda, True)
    ws = LG.ssl_workspace(T1.shape[0], idx.size, T1.shape[1], cuda)
    loss = LG._Ssl.apply((TAU, ws), dev(idx, cuda), a, b)
    loss.backward()
    return loss.item(), a.grad.cpu().numpy(), None if T2 is None else b.grad.cpu().numpy()


def _ssl_case(T1, T2, idx, cuda, tag):
    print(tag)
    ref = R.ssl_grad(T1, T2, idx, TAU)
    tor = R.ssl_grad(T1, T2, idx, TAU, dtype=torch.float32)
    got = _run_ssl(T1, T2, idx, cuda)
    _check_word("loss", got[0], ref[0], tor[0])
    check_vs_f32("gT1", got[1], ref[1], tor[1])
    if T2 is not None:
        check_vs_f32("gT2", got[2], ref[2], tor[2])
        off = np.setdiff1d(np.arange(T1.shape[0]), idx)  # rows of T1 the loss cannot reach
        assert not got[1][off].any()
    again = _run_ssl(T1, T2, idx, cuda)  # deterministic: a second call is bit-equal
    assert got[0] == again[0] and _bits(got[1], again[1]) and (T2 is None or _bits(got[2], again[2]))
    return got, ref, tor


# N = 4,099 crosses the kernel's table split (chunks of at least 1,024 rows); N is never a multiple of 16
@pytest.mark.parametrize("same", [False, True])
@pytest.mark.parametrize("B,N", [(1, 5), (67, 17), (300, 1000), (512, 4099)])
@pytest.mark.parametrize("d", [64, 128])
def test_ssl_kernel_vs_restatement(cuda, d, B, N, same):
    rng = np.random.default_rng(17 + d + B + N)
    T1 = (rng.standard_normal((N, d)) * 0.4).astype(np.float32)
    T2 = None if same else (rng.standard_normal((N, d)) * 0.4).astype(np.float32)
    idx = rng.integers(0, N, B).astype(np.int64)
    if B > 1:
        idx[1] = idx[0]  # a repeat
    _ssl_case(T1, T2, idx, cuda, f"d={d} B={B} N={N} same={same}")


@pytest.mark.parametrize("same", [False, True])
@pytest.mark.parametrize("N", [5, 17])
def test_ssl_kernel_long_repeats(cuda, N, same):
    """B = 512 over 5 or 17 rows: a row repeats more than a wave's 64 lanes."""
    rng = np.random.default_rng(N)
    T1 = (rng.standard_normal((N, 64)) * 0.4).astype(np.float32)
    T2 = None if same else (rng.standard_normal((N, 64)) * 0.4).astype(np.float32)
    idx = rng.integers(0, N - 1, 512).astype(np.int64)  # the last row stays off the batch
    idx[:80] = 2
    assert np.bincount(idx).max() > 64
    _ssl_case(T1, T2, idx, cuda, f"repeats N={N} same={same}")


def test_ssl_kernel_rank4_tables(cuda):
    """Tables of rank 4 (P @ lat with H = 4, as the model produces them)."""
    rng = np.random.default_rng(4)
    N, d, B = 333, 64, 67
    lat = rng.standard_normal((4, d)).astype(np.float32)
    T1 = (rng.random((N, 4)).astype(np.float32) @ lat).astype(np.float32)
    T2 = (rng.random((N, 4)).astype(np.float32) @ lat).astype(np.float32)
    _ssl_case(T1, T2, rng.integers(0, N, B).astype(np.int64), cuda, "rank 4")


@pytest.mark.parametrize("same", [False, True])
def test_ssl_kernel_equal_rows_and_zero_row(cuda, same):
    """Two identical rows and an all-zero row: finite, and equal to the restatement, which
    follows torch's clamp (the zero row's gradient is its unnormalised one over 1e-12)."""
    rng = np.random.default_rng(9)
    N, d = 37, 64
    T1 = (rng.standard_normal((N, d)) * 0.4).astype(np.float32)
    T1[5] = T1[3]
    T1[7] = 0.0
    T2 = None
    if not same:
        T2 = (rng.standard_normal((N, d)) * 0.4).astype(np.float32)
        T2[5], T2[7] = T2[3], 0.0
    idx = np.concatenate([rng.integers(0, N, 20), [3, 5, 7]]).astype(np.int64)
    got, ref, tor = _ssl_case(T1, T2, idx, cuda, f"equal rows, zero row, same={same}")
    rest = np.arange(N) != 7  # the other rows at their own scale
    check_vs_f32("gT1 off the zero row", got[1][rest], ref[1][rest], tor[1][rest])
    if not same:
        check_vs_f32("gT2 off the zero row", got[2][rest], ref[2][rest], tor[2][rest])


def test_ssl_kernel_limits(cuda):
    from rsx import _lib as L
    from rsx import lgmrec as LG

    lib = L.lib()
    assert lib.rsx_lgm_ssl_ws_bytes(100, 8, 32) == 0 and lib.rsx_lgm_ssl_ws_bytes(100, 65537, 64) == 0
    assert lib.rsx_lgm_ssl_ws_bytes(1 << 31, 8, 64) == 0 and lib.rsx_lgm_ssl_ws_bytes(100, 8, 64) > 0
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):
        LG.ssl_workspace(100, 8, 32, cuda)
    # an index outside the table contributes nothing
    rng = np.random.default_rng(2)
    T = (rng.standard_normal((9, 64)) * 0.4).astype(np.float32)
    idx = np.array([1, 2, 3], dtype=np.int64)
    bad = np.array([1, 2, 3, 9, -1], dtype=np.int64)
    a, b = _run_ssl(T, None, idx, cuda), _run_ssl(T, None, bad, cuda)
    assert a[0] == b[0] and _bits(a[1], b[1])


# ------------------------------------------------------------------ 2. the assignments
def _gumbel(rng, shape):
    return (-np.log(rng.exponential(size=shape))).astype(np.float32)


@pytest.mark.parametrize("keep_rate", [1.0, 0.5])
@pytest.mark.parametrize("H", [4, 12, 64])
@pytest.mark.parametrize("n", [1, 7, 300])
def test_assign_kernel_vs_restatement(cuda, n, H, keep_rate):
    from rsx import lgmrec as LG

    rng = np.random.default_rng(n * 100 + H)
    ld = LG.padded(H) + (32 if H == 12 else 0)  # a padded stride (ld > H for every H but 64)
    x = np.full((n, ld), 7.0, dtype=np.float32)  # the pad columns: never read
    x[:, :H] = rng.standard_normal((n, H)) * 0.5
    noise = _gumbel(rng, (n, H))
    keep = rng.random((n, H)) < keep_rate
    dy = rng.standard_normal((n, H)).astype(np.float32)
    ref = R.assign_grad(x[:, :H], noise, keep, keep_rate, dy, TAU)
    tor = R.assign_grad(x[:, :H], noise, keep, keep_rate, dy, TAU, dtype=torch.float32)
    xd, nd, kd = dev(x, cuda), dev(noise, cuda), dev(R.pack_keep(keep).view(np.int32), cuda)
    y0 = torch.full((n, ld), -3.0, device=cuda)
    o0 = torch.full((n, ld), -4.0, device=cuda)
    y, out = LG.assign_fwd(xd, H, TAU, keep_rate, nd, kd, y=y0, out=o0)
    err_y = np.abs(y[:, :H].cpu().numpy() - ref[0]).max()
    err_o = np.abs(out[:, :H].cpu().numpy() - ref[1]).max()
    print(f"n={n} H={H} keep_rate={keep_rate}: forward err y {err_y:.3e} out {err_o:.3e}")
    assert err_y <= 1e-6 and err_o <= 1e-6
    assert (y[:, H:] == -3.0).all() and (out[:, H:] == -4.0).all()  # the pad columns: untouched
    dyp = np.full((n, ld), np.nan, dtype=np.float32)  # the pad columns: never read
    dyp[:, :H] = dy
    dx0 = torch.full((n, ld), -5.0, device=cuda)
    dx = LG.assign_bwd(xd, H, TAU, keep_rate, y, dev(dyp, cuda), kd, dx=dx0)
    check_vs_f32("dx", dx[:, :H].cpu().numpy(), ref[2], tor[2])
    assert (dx[:, H:] == -5.0).all()


@pytest.mark.parametrize("keep_rate", [0.5, 0.2])
def test_assign_kernel_hashed_draws(cuda, keep_rate):
    """65,536 hashed samples: the Gumbel noise's mean within 6 standard errors of Euler's
    constant, the keep share within 6 binomial standard errors of keep_rate; the draws follow
    the seed."""
    from rsx import lgmrec as LG

    n, H = 16384, 4
    M = n * H
    x = torch.zeros(n, LG.padded(H), device=cuda)

    def draw(seed, stream=0):
        s = torch.tensor([seed], dtype=torch.int64, device=cuda)
        g = torch.empty(n, H, device=cuda)
        y, out = LG.assign_fwd(x, H, TAU, keep_rate, seed=s, stream_id=stream, noise_out=g)
        return g.cpu().numpy().astype(np.float64), (out[:, :H] != 0).cpu().numpy(), y[:, :H].cpu().numpy()

    g, kept, y = draw(1234)
    assert np.all(np.isfinite(g)) and g.min() >= -2.82 and g.max() <= 16.64  # u in [2^-24, 1 - 2^-24]
    se = np.sqrt((np.pi ** 2 / 6) / M)
    print(f"gumbel mean {g.mean():.5f} (0.57722 +- {6 * se:.5f}), keep share {kept.mean():.5f}")
    assert abs(g.mean() - 0.5772156649) <= 6 * se
    # y > 0 in float32 here (tau 0.2 over a noise range of ~16 gives e^-80 at the smallest), so a zero is a drop
    assert abs(kept.mean() - keep_rate) <= 6 * np.sqrt(keep_rate * (1 - keep_rate) / M)
    g2, kept2, _ = draw(1234)
    assert _bits(g.astype(np.float32), g2.astype(np.float32)) and np.array_equal(kept, kept2)
    g3, kept3, _ = draw(1235)
    assert not np.array_equal(g, g3) and not np.array_equal(kept, kept3)
    g4, _, _ = draw(1234, stream=1)
    assert not np.array_equal(g, g4)
    # the hashed forward is the explicit one on the noise it reports
    ref = R.assign_grad(np.zeros((n, H), np.float32), g.astype(np.float32), kept, keep_rate, np.ones((n, H)), TAU)
    assert np.abs(y - ref[0]).max() <= 1e-6


def test_assign_kernel_limits(cuda):
    from rsx import lgmrec as LG

    x = torch.zeros(4, 96, device=cuda)
    s = torch.zeros(1, dtype=torch.int64, device=cuda)
    for H in (2, 6, 68):
        with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):
            LG.assign_fwd(x, H, TAU, 1.0, seed=s)


# ------------------------------------------------------------------ 3. the hypergraph products
# n = 300 already splits the reduce (parts of 128 rows); 5,000 gives 40 parts
@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("H", [4, 12, 64])
@pytest.mark.parametrize("n", [1, 7, 300, 5000])
def test_hgnn_kernels_vs_restatement(cuda, n, H, d, layers):
    from rsx import lgmrec as LG

    rng = np.random.default_rng(n + H + d + layers)
    nu, ld = n // 2 + 3, LG.padded(H)
    Pi = np.zeros((n, ld), dtype=np.float32)
    Pu = np.zeros((nu, ld), dtype=np.float32)
    # softmax-like rows scaled so that two layers keep the magnitudes near one
    Pi[:, :H] = rng.dirichlet(np.ones(H), n) / np.sqrt(max(n / H, 1.0))
    Pu[:, :H] = rng.dirichlet(np.ones(H), nu)
    X = rng.standard_normal((n, d)).astype(np.float32)
    g = rng.standard_normal((nu + n, d)).astype(np.float32)
    ref = R.hgnn_grad(Pi[:, :H], Pu[:, :H], X, layers, g)
    tor = R.hgnn_grad(Pi[:, :H], Pu[:, :H], X, layers, g, dtype=torch.float32)

    def run():
        a, b, c = dev(Pi, cuda, True), dev(Pu, cuda, True), dev(X, cuda, True)
        out = LG._Hgnn.apply(a, b, c, H, layers)
        out.backward(dev(g, cuda))
        return [t.cpu().numpy() for t in (out.detach(), a.grad, b.grad, c.grad)]

    got = run()
    # forward: 1e-5 of sum |terms| per element, the terms of the last products
    P64, X64 = np.abs(Pi[:, :H]).astype(np.float64), np.abs(X).astype(np.float64)
    cur = X64
    for _ in range(layers):
        lat = P64.T @ cur
        cur = P64 @ lat
    mag = np.concatenate([np.abs(Pu[:, :H]).astype(np.float64) @ lat, cur])
    ratio = float((np.abs(got[0] - ref[0]) / (1e-5 * mag + 1e-30)).max())
    print(f"n={n} H={H} d={d} layers={layers}: forward err / bound {ratio:.3f}")
    assert np.all(np.isfinite(got[0])) and ratio <= 1.0
    check_vs_f32("gPi", got[1][:, :H], ref[1], tor[1])
    check_vs_f32("gPu", got[2][:, :H], ref[2], tor[2])
    check_vs_f32("gX", got[3], ref[3], tor[3])
    assert not got[1][:, H:].any() and not got[2][:, H:].any()
    for a, b in zip(got, run()):  # deterministic
        assert _bits(a, b)


def test_hgnn_primitives(cuda):
    """The three products on their own, with a second pair in the reduce and an accumulating
    row-dot; unsupported widths are refused."""
    from rsx import lgmrec as LG

    rng = np.random.default_rng(3)
    n, n2, H, d, ld = 301, 77, 12, 64, 32
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    P, P2, X, X2, lat = f(n, ld), f(n2, ld), f(n, d), f(n2, d), f(H, d)
    Pd, P2d, Xd, X2d, latd = (dev(t, cuda) for t in (P, P2, X, X2, lat))
    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    want = f64(P[:, :H]).T @ f64(X) + f64(P2[:, :H]).T @ f64(X2)
    mag = np.abs(f64(P[:, :H])).T @ np.abs(f64(X)) + np.abs(f64(P2[:, :H])).T @ np.abs(f64(X2))
    got = LG.hgnn_reduce(Pd, Xd, H, P2d, X2d).cpu().numpy()
    assert (np.abs(got - want) <= 1e-5 * mag).all()
    got = LG.hgnn_expand(Pd, H, latd).cpu().numpy()
    assert (np.abs(got - f64(P[:, :H]) @ f64(lat)) <= 1e-5 * (np.abs(f64(P[:, :H])) @ np.abs(f64(lat)))).all()
    base = f(n, ld)
    got = LG.hgnn_rowdots(Xd, latd, ld, out=dev(base, cuda), accumulate=True).cpu().numpy()
    want = f64(base[:, :H]) + f64(X) @ f64(lat).T
    mag = np.abs(f64(base[:, :H])) + np.abs(f64(X)) @ np.abs(f64(lat)).T
    assert (np.abs(got[:, :H] - want) <= 1e-5 * mag).all() and np.array_equal(got[:, H:], base[:, H:])
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):
        LG.hgnn_reduce(dev(f(8, 96), cuda), dev(f(8, 64), cuda), 68)
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):
        LG.hgnn_expand(Pd, H, dev(f(H, 32), cuda))


# ------------------------------------------------------------------ 4. the loss
def _loss_inputs(d, B, nu, ni, seed):
    rng = np.random.default_rng(seed)
    tabs = [(rng.standard_normal((nu + ni, d)) * 0.3).astype(np.float32) for _ in range(5)]
    trip = np.stack([rng.integers(0, nu, B), rng.integers(0, ni, B), rng.integers(0, ni, B)]).astype(np.int64)
    if B > 1:  # an item that is a positive in one triplet and a negative in another
        trip[2, 1] = trip[1, 0]
        trip[1, B - 1] = trip[2, 0]
    return tabs, trip


def _run_loss(tabs, trip, nu, alpha, reg, cuda):
    from rsx import lgmrec as LG

    ws = LG.loss_workspace(trip.shape[1], tabs[0].shape[1], cuda)
    ts = [dev(t, cuda, True) for t in tabs]
    keep = {}
    loss = LG._LgmLoss.apply((nu, alpha, reg, ws, keep), dev(trip, cuda), *ts)
    loss.backward()
    out = keep["terms"].detach().cpu().numpy()
    assert out[0] == loss.item() or (np.isnan(out[0]) and np.isnan(loss.item()))
    return out, [t.grad.cpu().numpy() for t in ts]


NAMES5 = ("gC", "gMv", "gMt", "gGv", "gGt")


@pytest.mark.parametrize("nu,ni", [(5, 7), (400, 200)])
@pytest.mark.parametrize("B", [1, 67, 300, 512])
@pytest.mark.parametrize("d", [64, 128])
def test_loss_kernel_vs_restatement(cuda, d, B, nu, ni):
    tabs, trip = _loss_inputs(d, B, nu, ni, 500 + d + B + nu)
    if B == 512 and nu == 5:  # every row repeats more than a wave's 64 lanes
        assert np.bincount(trip[0], minlength=nu).min() > 64
    for alpha, reg in ((0.0, 0.0), (0.3, 0.05)):
        print(f"d={d} B={B} tables=({nu},{ni}) alpha={alpha} reg={reg}")
        ref = R.loss_grad(tabs, trip, nu, alpha, reg)
        tor = R.loss_grad(tabs, trip, nu, alpha, reg, dtype=torch.float32)
        got = _run_loss(tabs, trip, nu, alpha, reg, cuda)
        for k, name in enumerate(("total", "bpr", "reg")):
            _check_word(name, float(got[0][k]), ref[0][k], tor[0][k])
        rows = np.concatenate([trip[0], nu + trip[1], nu + trip[2]])
        off = np.setdiff1d(np.arange(nu + ni), rows)
        for name, g, r, t in zip(NAMES5, got[1], ref[1], tor[1]):
            check_vs_f32(name, g, r, t)
            assert not g[off].any()
        again = _run_loss(tabs, trip, nu, alpha, reg, cuda)  # deterministic
        assert _bits(got[0], again[0]) and all(_bits(a, b) for a, b in zip(got[1], again[1]))


@pytest.mark.parametrize("d", [64, 128])
def test_loss_kernel_saturated_scores(cuda, d):
    """Scores of +-40: softplus and its derivative neither overflow nor lose the answer."""
    nu, ni, B = 8, 2, 8
    e = np.full(d, 1.0 / np.sqrt(d), dtype=np.float32)
    C = np.concatenate([np.tile(20.0 * e, (nu, 1)), np.stack([2.0 * e, -2.0 * e])]).astype(np.float32)
    rng = np.random.default_rng(d)
    tabs = [C] + [(rng.standard_normal((nu + ni, d)) * 1e-3).astype(np.float32) for _ in range(4)]
    for t in tabs[1:]:
        t[:nu] = 0.0  # the user rows: C alone (normalize(0) = 0)
    tabs[1][nu:], tabs[2][nu:] = 0.0, 0.0
    b = np.arange(B)
    trip = np.stack([b, b % 2, 1 - b % 2]).astype(np.int64)  # even b: x = +80, odd b: x = -80 (alpha 0)
    ref = R.loss_grad(tabs, trip, nu, 0.0, 0.01)
    got = _run_loss(tabs, trip, nu, 0.0, 0.01, cuda)
    assert abs(ref[0][1] - 40.0) <= 1e-6  # x = +-(20 * 2 * 2): half the triplets cost 80
    np.testing.assert_allclose(got[0], ref[0], rtol=1e-5)
    for g, r in zip(got[1], ref[1]):
        assert np.all(np.isfinite(g))
        np.testing.assert_allclose(g, r, rtol=1e-5, atol=1e-6 * np.abs(ref[1][0]).max())


def test_loss_kernel_zero_batch_matrix(cuda):
    """All-zero tables: the Frobenius norms are 0, their gradient is zero and finite (torch's norm)."""
    nu, ni, B, d = 5, 7, 16, 64
    tabs = [np.zeros((nu + ni, d), dtype=np.float32) for _ in range(5)]
    _, trip = _loss_inputs(d, B, nu, ni, 1)
    ref = R.loss_grad(tabs, trip, nu, 0.3, 0.05)
    got = _run_loss(tabs, trip, nu, 0.3, 0.05, cuda)
    np.testing.assert_allclose(got[0], ref[0], rtol=1e-6)
    assert got[0][2] == 0.0
    for g, r in zip(got[1], ref[1]):
        assert np.all(np.isfinite(g)) and not g.any() and not r.any()


def test_loss_kernel_bad_index_and_batch_cap(cuda):
    from rsx import lgmrec as LG

    tabs, trip = _loss_inputs(64, 8, 5, 7, 1)
    trip[1, 3] = 7  # an item outside its table
    out, gs = _run_loss(tabs, trip, 5, 0.3, 0.1, cuda)
    assert np.isnan(out[0]) and all(np.all(np.isfinite(g)) for g in gs)
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):
        LG.loss_workspace(65537, 64, cuda)


# ------------------------------------------------------------------ 5. the model against the fixtures
HP = R.HPARAMS


def _setup(tmp_path, extra=None, feats="both"):
    z0, z = R.load("lgmrec_step0_small.npz"), R.load("lgmrec_small.npz")
    # narrow: a text table whose width is no multiple of 4
    text = {"both": z["t_feat"], "text": z["t_feat"], "narrow": z["t_feat"][:, :6]}.get(feats)
    write_dataset(tmp_path, z["v_feat"] if feats != "text" else None, text)
    cfg = dict(is_multimodal_model=True)
    cfg.update({k: v for k, v in HP.items() if k not in ("train_batch_size",)})
    cfg.update(extra or {})
    c, train, valid, _ = loaders("LGMRec", tmp_path, cfg)
    return z0, z, c, train, valid


def _model(c, train):
    return make_model("LGMRec", c, train)


def _draws(z, prefix, cuda):
    """The recorded draws as the model takes them: four noise tensors, then the packed keep masks."""
    out = [dev(z[f"{prefix}noise{k}"], cuda) for k in range(4)]
    if f"{prefix}keep0" in z:
        out += [dev(z[f"{prefix}keep{k}"].view(np.int32), cuda) for k in range(4)]
    return out


def _param(z0, z, key, n):
    return (z[key + n] ^ z0["init." + n].view(np.int32)).view(np.float32)


def test_lgmrec_init_graphs_forward(cuda, tmp_path):
    z0, z, c, train, _ = _setup(tmp_path)
    m = _model(c, train)
    named = dict(m.named_parameters())
    assert tuple(n for n, p in named.items() if p.requires_grad) == R.NAMES
    assert not named["image_embedding.weight"].requires_grad and not named["text_embedding.weight"].requires_grad
    for n in R.NAMES:
        assert np.array_equal(named[n].detach().cpu().numpy().view(np.int32), z0["init." + n].view(np.int32)), n
    ref = coo_sorted(z0["norm_adj_idx"].astype(np.int64), z0["norm_adj_val"])
    A = m.norm_adj_csr
    mine = csr_to_sorted(A.rowptr.cpu().numpy(), A.col.cpu().numpy()[: A.nnz], A.val.cpu().numpy()[: A.nnz])
    for a, b in zip(ref, mine):
        assert np.array_equal(a, b)
    assert np.array_equal(m.num_inters.cpu().numpy().view(np.int32), z0["num_inters"].reshape(-1).view(np.int32))
    R_ = m.adj.A
    r, col, val = csr_to_sorted(R_.rowptr.cpu().numpy(), R_.col.cpu().numpy()[: R_.nnz], R_.val.cpu().numpy()[: R_.nnz])
    order = np.lexsort((z["train_i"], z["train_u"]))
    assert np.array_equal(r, z["train_u"][order]) and np.array_equal(col, z["train_i"][order]) and (val == 1).all()
    m.eval()
    nu = m.n_users
    with torch.no_grad():
        u, i, hyper = m.forward(_draws(z0, "fwd_", cuda))
        np.testing.assert_allclose(u.cpu().numpy(), z0["fwd_user"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(i.cpu().numpy(), z0["fwd_item"], rtol=1e-5, atol=1e-6)
        for name, t in zip(("uv", "iv", "ut", "it"), hyper):
            want = z0["fwd_hyper_" + name]
            np.testing.assert_allclose(t.cpu().numpy()[::8], want, rtol=1e-5, atol=1e-6 * np.abs(want).max())
        u2, i2 = m._eval_tables(_draws(z0, "fwd_", cuda))
        assert torch.equal(u2, u.contiguous()) and torch.equal(i2, i.contiguous()) and u.shape[0] == nu


def test_lgmrec_first_two_steps(cuda, tmp_path):
    from rsx.optim import RsxAdam

    z0, z, c, train, _ = _setup(tmp_path)
    m = _model(c, train)
    m.train()
    opt = RsxAdam([p for p in m.parameters() if p.requires_grad], lr=c["learning_rate"])
    for s in (0, 1):
        pre = f"step{s}_"
        opt.zero_grad(set_to_none=True)
        loss = m.calculate_loss(dev(z0[pre + "triplets"].astype(np.int64), cuda), draws=_draws(z0, pre, cuda))
        loss.backward()
        want = z0[pre + "terms"]  # bpr, ssl_u, ssl_i, the norms' sum over B
        got = [m.last_terms[1].item(), m.last_ssl[0].item(), m.last_ssl[1].item(), m.last_terms[2].item()]
        want = [want[0], want[1], want[2], HP["reg_weight"] * want[3]]
        print(f"step {s}: loss {loss.item():.8f} vs {float(z0[pre + 'loss']):.8f}; terms {got} vs {want}")
        for g, w in zip(got + [loss.item()], want + [float(z0[pre + "loss"])]):
            assert abs(g - w) <= 1e-5 * abs(w)
        none = {n for n, p in m.named_parameters() if p.grad is None}
        assert none == set(z0[pre + "no_grad"].tolist()) == {"image_embedding.weight", "text_embedding.weight"}
        for n, p in m.named_parameters():
            if p.grad is None:
                continue
            w = z0[pre + "grad." + n]
            g = p.grad.detach().cpu().numpy()
            scale = max(float(np.abs(w).max()), 1e-30)
            print(f"  step {s} grad {n}: err {np.abs(g - w).max():.3e}, scale {scale:.3e}")
            np.testing.assert_allclose(g, w, rtol=1e-3, atol=1e-5 * scale, err_msg=f"step {s} {n}")
        opt.step()
        for n in R.NAMES:
            got_p, want_p = dict(m.named_parameters())[n].detach().cpu().numpy(), _param(z0, z0, pre + "param_xor.", n)
            assert np.abs(got_p - want_p).max() <= 1e-5 * float(np.abs(want_p).max()), (s, n)


def test_lgmrec_epoch_and_scores_vs_reference(cuda, tmp_path):
    """One epoch through the Trainer with every draw replayed (eager steps: a captured step
    would replay the first batch's draw tensors), then the reference's first two evaluation
    batches under their draws."""
    from rsx.trainer import Trainer

    z0, z, c, train, valid = _setup(tmp_path, dict(rsx_graph_step=False))
    m = _model(c, train)
    t = Trainer(c, m)
    assert not t.fused and type(t.optimizer).__name__ == "RsxAdam"
    m.train()
    t._gate = False
    trip, nb = z["epoch0_triplets"].astype(np.int64), int(z["epoch0_nbatch"])
    step = {"k": 0}
    inner = m.calculate_loss
    m.calculate_loss = lambda inter: inner(inter, draws=_draws(z, f"epoch0_b{step['k']}_", cuda))
    total = 0.0
    for k in range(nb):
        step["k"] = k
        total += float(t.train_step(dev(trip[:, 512 * k: 512 * (k + 1)], cuda), k)[1])
    del m.calculate_loss
    torch.cuda.synchronize()
    print(f"epoch loss {total:.6f} vs reference {float(z['epoch0_loss']):.6f}")
    assert abs(total - float(z["epoch0_loss"])) <= 1e-5 * abs(float(z["epoch0_loss"]))
    named = dict(m.named_parameters())
    for n in R.NAMES:
        w = _param(z0, z, "epoch0_param_xor.", n)
        scale = float(np.abs(w).max())
        err = float(np.abs(named[n].detach().cpu().numpy() - w).max())
        print(f"  {n}: err / scale {err / scale:.2e} (bound 5e-5)")
        assert err <= 5e-5 * scale, n
    m.eval()
    for b in range(2):
        users = dev(z[f"eval_b{b}_users"].astype(np.int64), cuda)
        want = z[f"eval_b{b}_scores"]
        m._eval_cache = m._eval_tables(_draws(z, f"eval_b{b}_", cuda))
        scores = m.full_sort_predict([users, None]).cpu().numpy()
        scale = float(np.abs(want).max())
        print(f"  eval batch {b}: score err / scale {np.abs(scores - want).max() / scale:.2e} (bound 1e-4)")
        assert np.abs(scores - want).max() <= 1e-4 * scale
        masked = scores.copy()
        mask = z[f"eval_b{b}_mask"].astype(np.int64)
        masked[mask[0], mask[1]] = -1e10
        idx = np.argsort(-masked, axis=1, kind="stable")[:, :50]
        assert topk_equal_modulo_ties(idx, z[f"eval_b{b}_topk_idx"].astype(np.int64), masked) == 0
        if b == 0:  # the fused full-sort on the same tables, with the loader's own mask
            assert np.array_equal(valid.eval_u.cpu().numpy()[: users.numel()], users.cpu().numpy())
            vals, top = m.full_sort_topk([valid.eval_u, None], 50, valid)
            top = top.cpu().numpy()[: users.numel()]
            assert topk_equal_modulo_ties(top, z[f"eval_b{b}_topk_idx"].astype(np.int64), masked) == 0
            np.testing.assert_allclose(vals.cpu().numpy()[: users.numel()], np.take_along_axis(masked, top, 1),
                                       rtol=1e-5, atol=1e-6 * scale)
    m.train()
    assert m._eval_cache is None


@pytest.mark.parametrize("what", ["cf_model", "dims", "width", "one_modality", "narrow", "hyper_num", "layers",
                                  "keep_rate", "mm_layers"])
def test_lgmrec_unsupported_configurations_raise(cuda, tmp_path, what):
    extra = {"cf_model": dict(cf_model="ngcf"), "dims": dict(embedding_size=64, feat_embed_dim=128),
             "width": dict(embedding_size=32, feat_embed_dim=32), "hyper_num": dict(hyper_num=6),
             "layers": dict(n_hyper_layer=5), "keep_rate": dict(keep_rate=0.0), "mm_layers": dict(n_mm_layers=5)}
    feats = {"one_modality": "image", "narrow": "narrow"}.get(what, "both")
    _, _, c, train, _ = _setup(tmp_path, extra.get(what), feats)
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):
        _model(c, train)


def test_lgmrec_mf_backbone_and_wide_hypergraph(cuda, tmp_path):
    """cf_model mf, 12 hyperedges, two hypergraph layers, keep_rate 1: one step against the restatement."""
    over = dict(cf_model="mf", hyper_num=12, n_hyper_layer=2, keep_rate=1.0)
    z0, z, c, train, _ = _setup(tmp_path, over)
    m = _model(c, train)
    m.train()
    hp = dict(HP, **over)
    nu, ni = m.n_users, m.n_items
    rng = np.random.default_rng(5)
    noise = [_gumbel(rng, (n, 12)) for n in (ni, nu, ni, nu)]
    trip = z0["step0_triplets"].astype(np.int64)
    loss = m.calculate_loss(dev(trip, cuda), draws=[dev(g, cuda) for g in noise])
    loss.backward()

    def ref(dtype):
        graphs = R.dense_graphs(z["train_u"].astype(np.int64), z["train_i"].astype(np.int64), nu, ni, dtype)
        p = {n: R.tt(t.detach().cpu().numpy(), dtype, True) for n, t in m.named_parameters() if n in R.NAMES}
        feats = (R.tt(z["v_feat"], dtype), R.tt(z["t_feat"], dtype))
        out, _ = R.model_loss(p, feats, graphs, hp, [R.tt(g, dtype) for g in noise], trip)
        out.backward()
        return float(out), {n: t.grad.numpy() for n, t in p.items()}

    r64, r32 = ref(torch.float64), ref(torch.float32)
    _check_word("loss", loss.item(), r64[0], r32[0])
    for n, p in m.named_parameters():
        if n in R.NAMES:
            check_vs_f32(n, p.grad.cpu().numpy(), r64[1][n], r32[1][n])


# ------------------------------------------------------------------ 6. capture
def _steps(tmp_path, tag, z, cuda, graph, draws):
    from rsx.trainer import Trainer

    _, _, c, train, _ = _setup(tmp_path / tag, dict(rsx_graph_step=graph))
    m = _model(c, train)
    t = Trainer(c, m)
    m.train()
    t._gate = False
    if draws:  # the same draw tensors every batch: their addresses are what a capture holds
        d = _draws(z, "step0_", cuda)
        inner = m.calculate_loss
        m.calculate_loss = lambda inter: inner(inter, draws=d)
    trip = z["step0_triplets"].astype(np.int64)
    losses = []
    for k in range(4):
        losses.append(t.train_step(dev(np.roll(trip, 37 * k, axis=1), cuda), k)[1])
    torch.cuda.synchronize()
    return m, [float(x) for x in losses], t._graph.replays if t._graph is not None else 0


def test_lgmrec_captured_step_equals_eager(cuda, tmp_path):
    z0 = R.load("lgmrec_step0_small.npz")
    a, la, ra = _steps(tmp_path, "graph", z0, cuda, True, True)
    b, lb, rb = _steps(tmp_path, "eager", z0, cuda, False, True)
    assert ra == 3 and rb == 0  # batch 0 eager, batch 1 captured and replayed, batches 2 and 3 replays
    assert_same_run(a, b, la, lb)


def test_lgmrec_hashed_draws_follow_the_seed(cuda, tmp_path):
    """With hashed draws the seed word advances inside the captured step: replays on one batch
    give different losses; two runs from one seed agree bit for bit."""
    from rsx.trainer import Trainer

    z0 = R.load("lgmrec_step0_small.npz")
    a, la, ra = _steps(tmp_path, "a", z0, cuda, True, False)
    b, lb, _ = _steps(tmp_path, "b", z0, cuda, True, False)
    assert ra == 3
    assert_same_run(a, b, la, lb)
    # the same batch twice through the captured step, the optimiser's step size zero
    _, _, c, train, _ = _setup(tmp_path / "c", dict(rsx_graph_step=True, learning_rate=0.0))
    m = _model(c, train)
    t = Trainer(c, m)
    m.train()
    t._gate = False
    batch = dev(z0["step0_triplets"].astype(np.int64), cuda)
    seed0 = int(m._seed.item())
    losses = [float(t.train_step(batch, k)[1]) for k in range(4)]
    assert t._graph.replays == 3 and int(m._seed.item()) == seed0 + 4
    print(f"losses on one batch, fresh draws each: {losses}")
    assert len(set(losses)) == 4


def test_lgmrec_noise_only_draws_advance_the_seed(cuda, tmp_path):
    """`draws` with the four noise tensors alone, in training with keep_rate < 1: the keep bits are
    hashed, so the seed word advances and two calls on one batch drop different entries."""
    z0, z, c, train, _ = _setup(tmp_path)
    m = _model(c, train)
    m.train()
    batch = dev(z0["step0_triplets"].astype(np.int64), cuda)
    noise = _draws(z0, "step0_", cuda)[:4]
    seed0 = int(m._seed.item())
    with torch.no_grad():
        a = m.calculate_loss(batch, draws=noise).item()
        b = m.calculate_loss(batch, draws=noise).item()
        assert int(m._seed.item()) == seed0 + 2 and a != b and np.isfinite(a) and np.isfinite(b)
        full = _draws(z0, "step0_", cuda)  # nothing hashed: the seed stays
        m.calculate_loss(batch, draws=full)
        assert int(m._seed.item()) == seed0 + 2
        m.eval()  # evaluation mode drops nothing: noise alone is every draw
        u1, i1 = m._eval_tables(noise)
        u2, i2 = m._eval_tables(noise)
        assert int(m._seed.item()) == seed0 + 2 and torch.equal(u1, u2) and torch.equal(i1, i2)
