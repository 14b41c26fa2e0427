"""SELFCFED_LGN on the GPU: the per-step edge drop (rsx_selfcf_edge_drop) against numpy / scipy in
replay mode and statistically in hashed mode, the loss kernels (rsx_selfcf_loss_fwd / _bwd,
csrc/selfcf.hip) against the float64 restatement (tests/selfcf_ref.py) with explicit masks and
derived rounding bounds, the hashed target dropout, the evaluation tables, the model's first step
and two Trainer epochs against the reference's own run with its recorded draws replayed
(tests/golden/selfcfed_lgn_step0_small.npz, selfcfed_lgn_small.npz), graph capture, entry points.

Nothing in the step is atomic: two runs of the backward are bit-equal and the captured step equals
the eager one bit for bit.  Observed figures are printed before every assertion (run with -s)."""
import gc
import weakref

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import selfcf_ref as R
from helpers import (assert_same_run, dev, loaders, make_model, metric_dict, quick_start_case, record_batches,
                     train_epochs, write_dataset)

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
NU, NI = 11, 7  # every row repeats many times in a batch
REG = 0.1


# ------------------------------------------------------------------ 1, 2: the edge drop
def _structure(rng, n, nnz):
    """A symmetric structure of exactly nnz entries over n nodes (an odd nnz: one diagonal entry),
    CSR sorted by row then column; node n - 1 has no entry when nnz < 2 n."""
    pairs = set()
    while len(pairs) < nnz // 2:
        a, b = rng.integers(0, n - 1, 2)
        if a != b:
            pairs.add((min(a, b), max(a, b)))
    r = np.array([p[0] for p in pairs] + [p[1] for p in pairs] + ([0] if nnz % 2 else []), dtype=np.int64)
    c = np.array([p[1] for p in pairs] + [p[0] for p in pairs] + ([0] if nnz % 2 else []), dtype=np.int64)
    order = np.lexsort((c, r))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=rowptr[1:])
    return rowptr, r[order], c[order].astype(np.int32)


def _drop(cuda, val0, rev, mask=None, scale=None, seed=None):
    from rsx import selfcf

    val, valT = torch.full_like(val0, 7.0), torch.full_like(val0, 7.0)
    info = torch.zeros(2, device=cuda)
    selfcf.edge_drop(val0, rev, None if seed is None else torch.tensor([seed], dtype=torch.int64, device=cuda),
                     None if mask is None else dev(R.pack_bits(mask).view(np.int32), cuda),
                     None if scale is None else torch.tensor([scale], dtype=torch.float32, device=cuda), val, valT, info)
    torch.cuda.synchronize()
    return val.cpu().numpy(), valT.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("nnz,n,kind", [(1, 3, "rand"), (31, 12, "rand"), (33, 12, "rand"), (6044, 600, "rand"),
                                        (33, 12, "ones"), (6044, 600, "zeros")])
def test_edge_drop_replay_vs_numpy(cuda, nnz, n, kind):
    from rsx import ops, selfcf

    rng = np.random.default_rng(nnz + len(kind))
    rowptr, row, col = _structure(rng, n, nnz)
    assert col.size == nnz and rowptr[n] == nnz and (nnz >= 2 * n or rowptr[n - 1] == rowptr[n])  # an empty row
    val0 = (rng.random(nnz) + 0.1).astype(np.float32)
    keep = {"rand": rng.random(nnz) < 0.6, "ones": np.ones(nnz, bool), "zeros": np.zeros(nnz, bool)}[kind]
    scale = np.float32(1.0) if kind == "ones" else np.float32(1.0 / (1.0 - 0.4))
    rev = selfcf.reverse_slots(dev(rowptr, cuda), dev(col, cuda))
    val, valT, info = _drop(cuda, dev(val0, cuda), rev, keep, scale)
    want = R.dropped(val0, keep, scale)
    assert np.array_equal(val.view(np.int32), want.view(np.int32))  # val0 * scale bit for bit, 0 elsewhere
    assert info[1] == scale and abs(info[0] - (1 - 1 / scale)) <= 4 * U24
    A = sp.csr_matrix((want, col, rowptr), shape=(n, n))
    AT = sp.csr_matrix(A.T)
    AT.sort_indices()
    assert np.array_equal(AT.indptr, rowptr) and np.array_equal(AT.indices, col)
    assert np.array_equal(valT.view(np.int32), AT.data.astype(np.float32).view(np.int32))  # valT as CSR = scipy's transpose
    x = rng.standard_normal((n, 64)).astype(np.float32)
    csr = ops.DeviceCSR(rowptr, dev(col, cuda), dev(valT, cuda), n, cuda)
    y = csr.spmm(dev(x, cuda)).cpu().numpy().astype(np.float64)
    A64 = A.astype(np.float64).toarray()
    ref, mag = A64.T @ x.astype(np.float64), np.abs(A64.T) @ np.abs(x.astype(np.float64))
    K = int(np.diff(rowptr).max())
    ratio = float((np.abs(y - ref) / np.maximum(2 * (K + 1) * U24 * mag, 1e-300)).max())
    print(f"nnz {nnz} {kind}: SpMM over valT vs float64 A^T x, worst error / bound {ratio:.3f}")
    assert np.all(np.abs(y - ref) <= 2 * (K + 1) * U24 * mag)


def test_edge_drop_hashed(cuda):
    """262,144 directed entries (131,072 distinct interactions): the stored rate, the keep share, the
    independence of the two directions, the seed."""
    from rsx import selfcf

    rng = np.random.default_rng(3)
    nu = ni = 2048
    flat = rng.choice(nu * ni, 131072, replace=False)
    u, i = flat // ni, nu + flat % ni
    r, c = np.concatenate([u, i]), np.concatenate([i, u])
    order = np.lexsort((c, r))
    rowptr = np.zeros(nu + ni + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=nu + ni), out=rowptr[1:])
    nnz = r.size
    rev = selfcf.reverse_slots(dev(rowptr, cuda), dev(c[order].astype(np.int32), cuda))
    revh = rev.cpu().numpy()
    val0 = dev((rng.random(nnz) + 0.5).astype(np.float32), cuda)
    seen = []
    for seed in (1234, 1234, 1235, 1236):
        val, valT, info = _drop(cuda, val0, rev, seed=seed)
        rate, scale = float(info[0]), info[1]
        keep = val != 0
        share, dis = keep.mean(), (keep != keep[revh]).mean()
        s1 = np.sqrt(rate * (1 - rate) / nnz)
        p2 = 2 * rate * (1 - rate)
        s2 = np.sqrt(p2 * (1 - p2) / (nnz / 2))
        print(f"seed {seed}: rate {rate:.6f}, keep share {share:.6f} (4 sigma {4 * s1:.6f}), "
              f"directions disagree {dis:.6f} vs {p2:.6f} (4 sigma {4 * s2:.6f})")
        assert 0.0 <= rate < 1.0 and scale == np.float32(1.0) / (np.float32(1.0) - np.float32(rate))
        assert abs(share - (1 - rate)) <= 4 * s1
        assert abs(dis - p2) <= 4 * s2
        assert np.array_equal(val[keep], (val0.cpu().numpy() * scale)[keep])
        assert np.array_equal(valT[revh], val)
        seen.append((rate, keep))
    assert seen[0][0] == seen[1][0] and np.array_equal(seen[0][1], seen[1][1])  # the same seed: the same bits
    for a, b in ((0, 2), (2, 3)):
        assert seen[a][0] != seen[b][0] and not np.array_equal(seen[a][1], seen[b][1])


# ------------------------------------------------------------------ 3: the loss kernels vs float64
def _inputs(d, B, p, seed, nu=NU, ni=NI, zero_row=True):
    """f32 inputs and explicit keep masks keyed on the batch position: Bernoulli(1 - p) (all ones
    at p = 0), and both target rows of batch position 0 all dropped."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    c = dict(E=f(nu + ni, d), P=(f(d, d) / np.sqrt(d)).astype(np.float32), pb=f(d),
             users=rng.integers(0, nu, B).astype(np.int64), items=rng.integers(0, ni, B).astype(np.int64), nu=nu, p=p)
    c["keep"] = rng.random((2, B, d)) >= p
    if zero_row:
        c["keep"][:, 0] = False
    return c


def _args(cuda, c, masks=True, seed=7):
    from rsx import selfcf

    t = {k: dev(c[k], cuda) for k in ("E", "P", "pb", "users", "items")}
    d, B = c["E"].shape[1], len(c["users"])
    t["m"] = dev(R.pack_keep(c["keep"]).view(np.int32), cuda) if masks else None
    t["ws"] = selfcf.workspace(B, d, cuda)
    t["sd"] = torch.tensor([seed], dtype=torch.int64, device=cuda)
    a = selfcf.selfcf_args(t["E"], t["P"], t["pb"], t["users"], t["items"], c["nu"], REG, c["p"], t["sd"], t["m"], t["ws"])
    return a, t  # (the struct holds addresses: the tensors must outlive it)


def _run(cuda, c, masks=True, seed=7, backward=True, raw=False):
    """(out [4], dict of gradients) of the kernels on the inputs `c`."""
    from rsx import selfcf

    a, t = _args(cuda, c, masks, seed)
    out = selfcf.loss_fwd(a, cuda)
    g = {}
    if backward:
        go = torch.ones(1, dtype=torch.float32, device=cuda)
        gE, gP, gpb = selfcf.loss_bwd(a, go, t["E"], t["P"])
        f = (lambda v: v.cpu().numpy()) if raw else (lambda v: v.cpu().numpy().astype(np.float64))
        g = {k: f(v) for k, v in (("gE", gE), ("gP", gP), ("gpb", gpb))}
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64), g


def _ref(c):
    p32 = float(np.float32(c["p"]))
    scale = float(np.float32(1.0 / (1.0 - p32))) if c["p"] > 0 else 1.0
    return R.loss_grad(c["E"], c["P"], c["pb"], c["users"], c["items"], c["nu"], REG, p32, c["keep"], scale=scale)


def _bounds(c, r):
    """First-order rounding bounds of the kernels' results around the float64 restatement `r`:
    tests/test_gpu_bm3.py::_bounds reduced to the two streams (user, item), the batch L2 in place of
    the Frobenius term.  A K-term f32 dot product with a bias is within 2 (K + 1) 2^-24 of
    sum |terms| (tests/test_gpu_mf.py); an input error is carried through the next stage by the
    absolute value of that stage's derivative:
      q = x P^T + pb           dq = 2 (d + 1) u (|x| |P|^T + |pb|)
      c = q . th / n           dc = |dc/dq| . dq + 2 (3 d + 8) u |q| . |th| / n
      term = -mean c / 2       dterm = (mean dc + 2 (B + 1) u mean |c| + 4 u) / 2
      reg = 1/2 sum |x|^2      dreg = 2 (d + B + 8) u reg   (d-long dots, 2 B values added in a fixed order)
      G = w dc/dq, w = 1/(2B)  dG = w |d2c/dq2| dq + 2 (3 d + 8) u |G|mag
      gP = G^T X, gpb = colsum G   the dot bound with K = 2 B, plus dG carried
      gE: a row's occurrences of (G P)_b + reg_weight x_b added: the dot bound with K = d carried,
          plus 2 (count + 1) u sum |terms|."""
    d, B = c["E"].shape[1], len(c["users"])
    aP, apb = np.abs(c["P"].astype(np.float64)), np.abs(c["pb"].astype(np.float64))
    x, q, tg = r["x"], r["q"], r["tg"]
    ax = np.abs(x)
    dq = 2 * (d + 1) * U24 * (ax @ aP.T + apb)
    rc = 2 * (3 * d + 8) * U24
    w = 0.5
    dG, Gmag, dterm = np.zeros_like(x), np.zeros_like(x), np.zeros(2)
    for k, (o, t) in enumerate(((slice(0, B), slice(B, 2 * B)), (slice(B, 2 * B), slice(0, B)))):
        Q, Tt, dqo = q[o], tg[t], dq[o]
        qn = np.linalg.norm(Q, axis=1, keepdims=True)
        assert qn.min() > 1e-3
        th = Tt / np.maximum(np.linalg.norm(Tt, axis=1, keepdims=True), R.EPS)
        cc = (Q * th).sum(1, keepdims=True) / qn
        dc = th / qn - cc / qn * Q / qn
        cmag = (np.abs(Q) * np.abs(th)).sum(1, keepdims=True) / qn
        dcos = (np.abs(dc) * dqo).sum(1, keepdims=True) + rc * cmag
        dterm[k] = w * (dcos.mean() + 2 * (B + 1) * U24 * np.abs(cc).mean() + 4 * U24)
        a = (np.abs(Q) * dqo).sum(1, keepdims=True)
        b = (np.abs(th) * dqo).sum(1, keepdims=True)
        J = (np.abs(th) * a + np.abs(Q) * b) / qn ** 3 + np.abs(cc) * dqo / qn ** 2 + 3 * np.abs(cc) * np.abs(Q) * a / qn ** 4
        gm = w / B * (np.abs(th) / qn + np.abs(cc) * np.abs(Q) / qn ** 2)
        dG[o] = w / B * J + rc * gm
        Gmag[o] = gm
    out = r["out"]
    dreg = 2 * (d + B + 8) * U24 * out[3]
    dtotal = dterm.sum() + REG * dreg + 16 * U24 * (np.abs(out[1:3]).sum() + REG * out[3])
    bounds = dict(out=np.array([dtotal, dterm[0], dterm[1], dreg]))
    n = 2 * B
    bounds["gP"] = dG.T @ ax + 2 * (n + 1) * U24 * (Gmag.T @ ax)
    bounds["gpb"] = dG.sum(0) + 2 * (n + 1) * U24 * Gmag.sum(0)
    ddX = dG @ aP + 2 * (d + 1) * U24 * (Gmag @ aP)
    mag = Gmag @ aP + REG * ax
    idx = np.concatenate([c["users"], c["nu"] + c["items"]])
    acc = np.zeros_like(r["gE"]), np.zeros_like(r["gE"]), np.zeros(r["gE"].shape[0])
    np.add.at(acc[0], idx, ddX)
    np.add.at(acc[1], idx, mag)
    np.add.at(acc[2], idx, 1.0)
    bounds["gE"] = acc[0] + 2 * (acc[2][:, None] + 2) * U24 * acc[1]
    return bounds


@pytest.mark.parametrize("d", [64, 128])
def test_loss_kernels_vs_float64(cuda, d):
    worst = {}
    for B in (1, 63, 65, 200):
        for p in (0.0, 0.3):
            c = _inputs(d, B, p, seed=1000 * d + 10 * B + int(10 * p), zero_row=False)
            r = _ref(c)
            out, g = _run(cuda, c)
            bd = _bounds(c, r)
            assert np.all(np.isfinite(out))
            for key in ("out", "gE", "gP", "gpb"):
                got = out if key == "out" else g[key]
                ratio = np.abs(got - r[key]) / np.maximum(bd[key], 1e-300)
                worst[key] = max(worst.get(key, 0.0), float(ratio.max()))
                k = int(np.argmax(ratio))
                assert np.all(np.abs(got - r[key]) <= bd[key]), (key, B, p, k, got.flat[k], np.asarray(r[key]).flat[k],
                                                                 bd[key].flat[k])
            off = np.setdiff1d(np.arange(NU + NI), np.concatenate([c["users"], NU + c["items"]]))
            assert np.all(g["gE"][off] == 0)
    print(f"d {d}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("d", [64, 128])
def test_all_dropped_target_rows_give_cosine_zero(cuda, d):
    """B = 1 with both target rows all dropped: both cosine terms exactly 0, everything finite, and
    the two rows receive the regulariser's gradient alone."""
    c = _inputs(d, 1, 0.3, seed=5)
    out, g = _run(cuda, c)
    r = _ref(c)
    print(f"terms {out[1:3]} (restatement {r['out'][1:3]}), total {out[0]} vs {r['out'][0]}")
    assert out[1] == 0.0 and out[2] == 0.0 and np.all(np.isfinite(out))
    assert all(np.all(np.isfinite(v)) for v in g.values())
    assert np.all(g["gP"] == 0) and np.all(g["gpb"] == 0)
    for row in (int(c["users"][0]), NU + int(c["items"][0])):
        want = REG * c["E"][row].astype(np.float64)
        assert np.all(np.abs(g["gE"][row] - want) <= 4 * U24 * np.abs(want))


def test_backward_is_bit_reproducible_and_zero_off_the_batch(cuda):
    """Two runs at B = 200 (every row repeats) give the same bits; with users 20.. and items 15..
    absent, their rows of the gradient table are exactly zero."""
    c = _inputs(64, 200, 0.3, seed=9)
    o1, g1 = _run(cuda, c, raw=True)
    o2, g2 = _run(cuda, c, raw=True)
    assert np.array_equal(o1, o2)
    for k in g1:
        assert np.array_equal(g1[k].view(np.int32), g2[k].view(np.int32)), k
    nu, ni = 50, 40
    c = _inputs(128, 65, 0.3, seed=21, nu=nu, ni=ni, zero_row=False)
    c["users"], c["items"] = c["users"] % 20, c["items"] % 15
    _, g = _run(cuda, c, raw=True)
    off = np.concatenate([np.arange(20, nu), nu + np.arange(15, ni)])
    on = np.concatenate([np.unique(c["users"]), nu + np.unique(c["items"])])
    assert np.all(g["gE"][off].view(np.int32) == 0)  # exactly +0.0
    assert np.all(np.any(g["gE"][on] != 0, axis=1))


def test_out_of_table_index_gives_nan_and_writes_nothing_outside(cuda):
    """A pair whose item is outside its table: every loss word NaN; the gradient table stays finite
    and the pair contributes nothing (bm3.hip's contract)."""
    c = _inputs(64, 65, 0.0, seed=31, zero_row=False)
    good = dict(c, users=np.delete(c["users"], 7), items=np.delete(c["items"], 7), keep=np.delete(c["keep"], 7, axis=1))
    c["items"] = c["items"].copy()
    c["items"][7] = NI + 5
    out, g = _run(cuda, c)
    assert np.all(np.isnan(out))
    assert all(np.all(np.isfinite(v)) for v in g.values())
    # the 64 good pairs' gradients: the cosine part carries the mean's 1 / 65, the L2 part is theirs
    r1 = _ref(good)
    r0 = R.loss_grad(good["E"], good["P"], good["pb"], good["users"], good["items"], NU, 0.0, 0.0, good["keep"], scale=1.0)
    bd = _bounds(good, r1)  # (derived at the good pairs' own weight 1 / 64 > 1 / 65)
    want = {"gE": r0["gE"] * 64 / 65 + (r1["gE"] - r0["gE"]), "gP": r1["gP"] * 64 / 65, "gpb": r1["gpb"] * 64 / 65}
    for k in want:
        print(f"  {k}: worst error / bound {float((np.abs(g[k] - want[k]) / np.maximum(bd[k], 1e-300)).max()):.3f}")
        assert np.all(np.abs(g[k] - want[k]) <= bd[k]), k


# ------------------------------------------------------------------ 4: the hashed target dropout
def test_hashed_target_dropout(cuda):
    """p = 0.3, d = 64, 2,048 rows each occurring at batch positions b and b + 2,048 (262,144 draws a
    stream): the keep rate, the scale of the kept values (F.dropout's x * float32(1 / (1 - p))),
    DIFFERENT masks for the two occurrences of a row (agreement p^2 + (1 - p)^2), the two streams,
    consecutive seeds."""
    from rsx import selfcf

    n, d, p = 2048, 64, 0.3
    rng = np.random.default_rng(4)
    E = (rng.standard_normal((2 * n, d)) + 3.0).astype(np.float32)  # no zeros
    E[n:] = E[:n]  # both streams see the same values: the targets differ by their masks only
    idx = np.concatenate([np.arange(n), np.arange(n)]).astype(np.int64)
    B = idx.size
    c = dict(E=E, P=np.eye(d, dtype=np.float32), pb=np.zeros(d, np.float32), users=idx, items=idx, nu=n, p=p)
    outs = []
    for seed in (100, 101):
        a, t = _args(cuda, c, masks=False, seed=seed)
        outs.append(selfcf.targets(a, cuda).cpu().numpy().reshape(2, B, d))
    tg = outs[0]
    p32 = float(np.float32(p))
    scale = np.float32(1.0 / (1.0 - p32))
    x = E[idx]
    sigma = np.sqrt(p32 * (1 - p32) / (B * d))
    masks = []
    for s in range(2):
        keep = tg[s] != 0
        print(f"stream {s}: keep rate {keep.mean():.5f} (0.7 +- 4 sigma = {4 * sigma:.5f})")
        assert abs(keep.mean() - (1 - p32)) <= 4 * sigma
        assert np.array_equal(tg[s][keep], (x * scale)[keep])
        masks.append(keep)
    q = p32 ** 2 + (1 - p32) ** 2
    s4 = 4 * np.sqrt(q * (1 - q) / (n * d))
    for s in range(2):
        agree = (masks[s][:n] == masks[s][n:]).mean()
        print(f"stream {s}: the two occurrences of a row agree on {agree:.5f} (expected {q:.5f} +- {s4:.5f})")
        assert abs(agree - q) <= s4
    s4 = 4 * np.sqrt(q * (1 - q) / (B * d))
    assert abs((masks[0] == masks[1]).mean() - q) <= s4  # the streams are independent
    for s in range(2):
        assert abs(((outs[1][s] != 0) == masks[s]).mean() - q) <= s4  # the next seed: another mask


# ------------------------------------------------------------------ 5: the evaluation tables
@pytest.mark.parametrize("nu,ni", [(5, 3), (67, 130)])
@pytest.mark.parametrize("d", [64, 128])
def test_eval_tables(cuda, nu, ni, d):
    from rsx import ops, selfcf

    rng = np.random.default_rng(nu + d)
    E = rng.standard_normal((nu + ni, d)).astype(np.float32)
    P, pb = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32), rng.standard_normal(d).astype(np.float32)
    UC, IC = selfcf.eval_tables(dev(E, cuda), dev(P, cuda), dev(pb, cuda), nu)
    assert UC.shape == (nu, 2 * d) and IC.shape == (ni, 2 * d)
    E64, P64 = E.astype(np.float64), P.astype(np.float64)
    q = E64 @ P64.T + pb
    dq = 2 * (d + 1) * U24 * (np.abs(E64) @ np.abs(P64).T + np.abs(pb))
    uc, ic = UC.cpu().numpy(), IC.cpu().numpy()
    assert np.array_equal(uc[:, d:], E[:nu]) and np.array_equal(ic[:, :d], E[nu:])  # the placed halves: copies
    assert np.all(np.abs(uc[:, :d] - q[:nu]) <= dq[:nu]) and np.all(np.abs(ic[:, d:] - q[nu:]) <= dq[nu:])
    got = ops.score_dense(UC, None, IC).cpu().numpy()
    want = q[:nu] @ E64[nu:].T + E64[:nu] @ q[nu:].T  # the reference's two-term score
    uc64, ic64 = np.concatenate([q[:nu], E64[:nu]], 1), np.concatenate([E64[nu:], q[nu:]], 1)
    bound = 2 * (2 * d + 1) * U24 * (np.abs(uc64) @ np.abs(ic64).T) + dq[:nu] @ np.abs(E64[nu:]).T + \
        np.abs(E64[:nu]) @ dq[nu:].T
    print(f"({nu}, {ni}) d {d}: worst score error / bound {float((np.abs(got - want) / bound).max()):.3f}")
    assert np.all(np.abs(got - want) <= bound)


# ------------------------------------------------------------------ the model on the fixture data
def _model(tmp_path, extra=None):
    write_dataset(tmp_path, None, None)
    c, train, valid, test = loaders("SELFCFED_LGN", tmp_path, {"n_layers": 1, "dropout": 0.0, "reg_weight": 0.1,
                                                               **(extra or {})})
    return make_model("SELFCFED_LGN", c, train), c, train, valid, test


def _named(m):
    sd = dict(m.named_parameters())
    assert list(sd) == list(R.NAMES)  # the reference's names in its named_parameters() order
    return sd


def _slot_mask(z, packed):
    """A recorded edge keep mask (the reference's nonzero order) in CSR slot order, packed."""
    keep = R.unpack_bits(packed, z["adj_val"].size)
    return R.pack_bits(keep[R.csr_order(z["adj_idx"], 600)]).view(np.int32)


def test_init_graph_and_first_step_vs_reference(cuda, tmp_path):
    z = R.load_fixture("step0")
    m, *_ = _model(tmp_path, dict(n_layers=2, dropout=0.3))
    sd = _named(m)
    for n in R.NAMES:
        assert np.array_equal(sd[n].detach().cpu().numpy().view(np.int32), z["init." + n].view(np.int32)), n
    assert m.drop_ratio == 1.0 and m.drop_flag is True
    from rsx.blocks import _ego

    ego = _ego(*m._tables())  # the two tables are adjacent in one buffer: the ego table is no copy
    assert ego.data_ptr() == sd[R.U_EMB].data_ptr() and ego.shape == (600, 64)
    g = m.graph
    order = R.csr_order(z["adj_idx"], 600)
    rows = np.repeat(np.arange(600), np.diff(g.A0.rowptr_host))
    assert np.array_equal(rows, z["adj_idx"][0][order]) and np.array_equal(g.col.cpu().numpy(), z["adj_idx"][1][order])
    assert np.array_equal(g.val0.cpu().numpy().view(np.int32), z["adj_val"][order].view(np.int32))
    rev = g.rev.cpu().numpy()
    assert np.array_equal(rev[rev], np.arange(6044)) and np.array_equal(g.col.cpu().numpy()[rev], rows)
    # the first step with the draws numpy and torch made
    m.set_replay(_slot_mask(z, z["edge_keep"]), z["scale"])
    masks = dev(np.stack([z["keep_user"], z["keep_item"]]).view(np.int32), cuda)
    m.train()
    loss = m.calculate_loss(dev(z["pairs"].astype(np.int64), cuda), keep_masks=masks)
    assert np.array_equal(g.val.cpu().numpy().view(np.int32), z["drop_val"][order].view(np.int32))  # Â's values
    assert np.array_equal(g.valT.cpu().numpy()[rev].view(np.int32), z["drop_val"][order].view(np.int32))
    loss.backward()
    want = float(z["step0_loss"])
    print(f"loss {loss.item():.8f} vs reference {want:.8f} (rel {abs(loss.item() - want) / want:.2e})")
    assert abs(loss.item() - want) <= 1e-5 * abs(want)
    terms = m.last_terms.cpu().numpy()
    print(f"terms {terms[1:]} vs reference {z['step0_terms']}")
    assert np.all(np.abs(terms[1:] - z["step0_terms"]) <= 1e-5 * np.abs(z["step0_terms"]))
    for n in R.NAMES:
        w = z["step0_grad." + n]
        scale = float(np.abs(w).max())
        bound = max(1e-5 * scale, 4 * float(z["refdiff.grad." + n]))
        err = float(np.abs(sd[n].grad.cpu().numpy() - w).max())
        print(f"  {n}: err {err:.3e}, scale {scale:.3e}, bound {bound:.3e}")
        assert err <= bound, n


def test_trainer_vs_reference_with_recorded_draws(cuda, tmp_path):
    from rsx.trainer import Trainer

    z = R.load_fixture("small")
    m, c, train, valid, test = _model(tmp_path)
    t = Trainer(c, m)
    assert not t.fused and type(t.optimizer).__name__ == "RsxAdam"
    assert len(t.optimizer.param_groups[0]["params"]) == len(R.NAMES)
    rec = record_batches(train)
    masks = [_slot_mask(z, w) for w in z["step_edge_keep"]]
    step, orig = [0], t.train_step

    def replaying(interaction, batch_idx, loss_func=None):  # the step's recorded draw into the persistent buffers
        # the reference draws the rate with np.random.random(), the generator its loader's epoch shuffle
        # reads too: taking the same draw here keeps the batch stream the reference's, and shows it is
        assert np.random.random() == float(z["step_rate"][step[0]])
        m.set_replay(masks[step[0]], z["step_scale"][step[0]])
        step[0] += 1
        return orig(interaction, batch_idx, loss_func)

    t.train_step = replaying
    losses = train_epochs(t, m, train, 2)
    assert step[0] == len(masks) == 12
    want = np.concatenate([z[f"epoch{e}_pairs"] for e in range(2)], axis=1).astype(np.int64)
    got = torch.cat(rec, dim=1).numpy()
    assert got.shape[0] == 2 and np.array_equal(got, want)
    assert t._graph is not None and t._graph.replays > 0  # the captured step ran, in replay mode
    print(f"epoch losses {losses} vs reference {z['epoch_losses']}; {t._graph.replays} replayed batches")
    sd = _named(m)
    for n in R.NAMES:
        bound = max(5e-5, 4 * float(z["refdiff.param." + n]))
        err = float(np.abs(sd[n].detach().cpu().numpy() - z["epoch1_param." + n]).max())
        print(f"{n}: max |param - reference| = {err:.3e} (bound {bound:.1e})")
        assert err <= bound, n
    for split, loader in (("valid", valid), ("test", test)):
        tag = f"epoch1_{split}"
        res = t.evaluate(loader)
        ref = metric_dict(z, tag)
        assert res.keys() == ref.keys()
        for k in ref:
            assert abs(res[k] - ref[k]) <= 1e-4, (k, res[k], ref[k])
        assert np.array_equal(loader.eval_u.cpu().numpy(), z[tag + "_users"])
        _, idx = m.full_sort_topk([loader.eval_u, None], 50, loader)
        same = np.all(idx.cpu().numpy() == z[tag + "_topk_idx"].astype(np.int64), axis=1)
        print(f"{split}: {int(same.sum())} of {same.size} top-50 lists equal, the others recorded as ties")
        assert np.all(same | z[tag + "_inner_tie"] | z[tag + "_boundary_tie"])
    # the evaluation tables are built once per eval() session and dropped by train()
    tabs = m._eval_tables()
    assert m._eval_tables() is tabs and tabs[0].shape == (400, 128) and tabs[1].shape == (200, 128)
    sc = m.full_sort_predict([valid.eval_u[:8], None])
    assert sc.shape == (8, 200) and bool(torch.isfinite(sc).all())
    m.train()
    assert m._eval_cache is None


# ------------------------------------------------------------------ 8: capture
def test_no_autograd_node_outlives_its_step(cuda, tmp_path):
    """Eager, before any capture: with the collector off, every autograd node reachable from the
    loss is dead once backward has run and the loss is dropped (tests/test_gpu_grcn.py's check)."""
    z = R.load_fixture("step0")
    m, *_ = _model(tmp_path, dict(n_layers=2, dropout=0.3))
    m.train()
    pairs = dev(z["pairs"].astype(np.int64), cuda)
    gc.collect()
    on = gc.isenabled()
    gc.disable()
    try:
        loss = m.calculate_loss(pairs)
        refs, names, seen, todo = [], [], set(), [loss.grad_fn]
        while todo:
            fn = todo.pop()
            if fn is None or id(fn) in seen:
                continue
            seen.add(id(fn))
            try:
                refs.append(weakref.ref(fn))
                names.append(type(fn).__name__)
            except TypeError:
                pass
            todo.extend(f for f, _ in fn.next_functions)
        del fn, todo
        assert all(any(k in s for s in names) for k in ("_SelfcfLoss", "_PropMeanRows", "_Joined")), names
        loss.backward()
        del loss
        m.last_terms = None
        alive = [s for r, s in zip(refs, names) if r() is not None]
        assert not alive, alive
    finally:
        if on:
            gc.enable()


def _steps(tmp_path, tag, batches, graph, extra=None):
    from rsx.trainer import Trainer

    m, c, *_ = _model(tmp_path / tag, dict(n_layers=2, dropout=0.3, rsx_graph_step=graph, **(extra or {})))
    t = Trainer(c, m)
    m.train()
    t._gate = False
    losses, rates, seeds = [], [], []
    for k, b in enumerate(batches):
        losses.append(float(t.train_step(b, k)[1]))
        rates.append(float(m.drop_info[0]))
        seeds.append(int(m.drop_seed))
    torch.cuda.synchronize()
    return m, losses, t, rates, seeds


def test_captured_step_equals_eager_bit_for_bit(cuda, tmp_path):
    """Seven steps with the hashed draws (full, full, full, full, short, short, short), captured vs
    eager from the same seed: bit-equal parameters and losses.  Two replays of one batch give
    different losses and different stored rates; the seed word advances once per step."""
    z = R.load_fixture("small")
    full, short = dev(R.epoch_pairs(z, 0)[0], cuda), dev(R.epoch_pairs(z, 0)[-1], cuda)
    seq = [full, full, full, full, short, short, short]
    a, la, ta, ra, sa = _steps(tmp_path, "graph", seq, True)
    b, lb, tb, rb, sb = _steps(tmp_path, "eager", seq, False)
    # batch 0 eager, batch 1 captured, 2 and 3 replays; 4 eager (a new shape), 5 captured, 6 a replay
    assert ta._graph is not None and ta._graph.replays == 5 and tb._graph is None
    print(f"losses {la}\nrates {ra}")
    assert_same_run(a, b, la, lb)
    assert ra == rb and sa == sb
    seed0 = 999 * 1000003 + 41
    assert sa == [seed0 + k for k in range(1, 8)]  # advanced once per step, replays included
    assert len(set(ra)) == 7 and all(0.0 <= r < 1.0 for r in ra)
    assert la[2] != la[3] and ra[2] != ra[3]  # two replays of one batch: fresh draws


# ------------------------------------------------------------------ 9: entry points
def test_quick_start(cuda, tmp_path):
    res = quick_start_case("SELFCFED_LGN", tmp_path, None, None,
                           {"epochs": 1, "n_layers": [2], "reg_weight": [0.1], "dropout": [0.3]})
    assert len(res) == 1 and "recall@20" in res[0][1]
    assert all(np.isfinite(v) for v in res[0][1].values())


def test_dense_propagation_beyond_four_layers_and_none(cuda, tmp_path):
    """n_layers 5 takes the dense propagation (with A^T in the backward), n_layers 0 none: one
    training step each is finite and moves every parameter's gradient."""
    z = R.load_fixture("step0")
    pairs = dev(z["pairs"].astype(np.int64), cuda)
    for k, K in enumerate((5, 0)):
        m, *_ = _model(tmp_path / str(k), dict(n_layers=K, dropout=0.3))
        m.train()
        loss = m.calculate_loss(pairs)
        loss.backward()
        assert np.isfinite(loss.item())
        for n, p in m.named_parameters():
            assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, (K, n)


def test_unsupported_shapes_are_refused(cuda):
    from rsx import _lib as L
    from rsx import selfcf

    z = torch.zeros(64 * 64, device=cuda)
    idx = torch.zeros(8, dtype=torch.int64, device=cuda)
    ws = selfcf.workspace(8, 64, cuda)
    a = selfcf.selfcf_args(z.view(64, 64), z.view(64, 64), z[:64], idx, idx, 32, REG, 0.0, None, None, ws)
    out = torch.zeros(4, device=cuda)
    for d in (16, 32, 48, 256):
        a.d = d
        assert L.lib().rsx_selfcf_loss_fwd(a, out.data_ptr(), None) == L.RSX_ERR_UNSUPPORTED
    a.d, a.batch = 64, 65537
    assert L.lib().rsx_selfcf_loss_fwd(a, out.data_ptr(), None) == L.RSX_ERR_UNSUPPORTED
    a.batch, a.ws_bytes = 8, 16
    assert L.lib().rsx_selfcf_loss_fwd(a, out.data_ptr(), None) == 1003
    a.ws_bytes, a.p_drop = ws.numel(), 0.3  # a hashed stream without a seed
    assert L.lib().rsx_selfcf_loss_fwd(a, out.data_ptr(), None) == 1001
    assert L.lib().rsx_selfcf_targets(a, z.data_ptr(), None) == 1001
    v = torch.zeros(3, 8, device=cuda)
    rev = torch.zeros(8, dtype=torch.int32, device=cuda)
    f = L.lib().rsx_selfcf_edge_drop  # hashed mode without a seed; a replayed mask without its scale
    assert f(v[0].data_ptr(), rev.data_ptr(), 8, None, None, None, v[1].data_ptr(), v[2].data_ptr(), out.data_ptr(), None) == 1001
    assert f(v[0].data_ptr(), rev.data_ptr(), 8, None, rev.data_ptr(), None, v[1].data_ptr(), v[2].data_ptr(),
             out.data_ptr(), None) == 1001
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and bool((v == 0).all())  # nothing was launched
