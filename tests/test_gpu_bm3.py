"""BM3 on the GPU: the bootstrap-loss kernels (rsx_bm3_loss_fwd / _bwd, csrc/bm3.hip) against
the float64 restatement (tests/bm3_ref.py) with explicit masks and derived rounding bounds,
the rows off the batch, the hashed dropout, the model's first step and two Trainer epochs
against the reference's own run (tests/golden/bm3_step0_small.npz, bm3_small.npz), graph
capture, and the entry points.

The repeated rows' gradients are accumulated with f32 atomics, so there
is no run-to-run bit-equality test of the backward; the forward is deterministic and is
checked to be.  Observed figures are printed before every assertion (run with -s)."""
import numpy as np
import pytest
import torch

import bm3_ref as R
from helpers import (dev, loaders, make_model, metric_dict, quick_start_case, record_batches, train_epochs,
                     write_dataset)

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
NU, NI = 11, 7  # every row repeats many times in a batch
REG, CL = 0.1, 2.0
PAIRS = (("user", "item", 1.0), ("item", "user", 1.0), ("text", "item", CL), ("image", "item", CL),
         ("text", "text", CL), ("image", "image", CL))


def _inputs(d, B, has_t, has_v, p, seed, nu=NU, ni=NI, zero_row=True):
    """f32 inputs and explicit keep masks: Bernoulli(1 - p) (all ones at p = 0), and the item
    and user target rows of batch row 0 all dropped."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    c = dict(E=f(nu + ni, d), H=f(ni, d), T=f(ni, d) if has_t else None, V=f(ni, d) if has_v else None,
             P=(f(d, d) / np.sqrt(d)).astype(np.float32), pb=f(d), users=rng.integers(0, nu, B).astype(np.int64),
             items=rng.integers(0, ni, B).astype(np.int64), nu=nu, p=p)
    keep = {}
    for s, rows in (("user", nu), ("item", ni), ("text", ni), ("image", ni)):
        keep[s] = rng.random((rows, d)) >= p
    if zero_row:
        keep["item"][c["items"][0]] = False
        keep["user"][c["users"][0]] = False
    c["keep"] = keep
    return c


def _run(cuda, c, masks=True, seed=7, backward=True):
    """(out [8], dict of gradients) of the kernels on the inputs `c`."""
    from rsx import bm3

    t = {k: dev(c[k], cuda) for k in ("E", "H", "T", "V", "P", "pb", "users", "items")}
    d, B = c["E"].shape[1], len(c["users"])
    m = {s: dev(R.pack_keep(k).view(np.int32), cuda) for s, k in c["keep"].items()} if masks else None
    ws = bm3.workspace(B, d, cuda)
    sd = torch.tensor([seed], dtype=torch.int64, device=cuda)
    a = bm3.bm3_args(t["E"], t["H"], t["T"], t["V"], t["P"], t["pb"], t["users"], t["items"], c["nu"], REG, CL,
                     c["p"], sd, m, ws)
    out = bm3.loss_fwd(a, cuda)
    g = {}
    if backward:
        go = torch.ones(1, dtype=torch.float32, device=cuda)
        gE, gT, gV, gP, gpb = bm3.loss_bwd(a, go, t["E"], t["T"], t["V"], t["P"])
        g = {k: (None if v is None else v.cpu().numpy().astype(np.float64))
             for k, v in (("gE", gE), ("gT", gT), ("gV", gV), ("gP", gP), ("gpb", gpb))}
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64), g


def _bounds(c, r):
    """First-order rounding bounds of the kernels' results around the float64 restatement `r`,
    built from the dot-product bound tests/test_gpu_mf.py derives for lin_rows_fwd: a K-term
    f32 dot product with a bias is within 2 (K + 1) 2^-24 of sum |terms|.  Applied to every
    contraction of the chain, an input error carried through the next stage by the absolute
    value of that stage's derivative:
      q = x P^T + pb            dq = 2 (d + 1) u (|x| |P|^T + |pb|)  [+ u |x| |P|^T: the item row's add]
      c = q . th / n            dc = |dc/dq| . dq + 2 (3 d + 8) u |q| . |th| / n     (three d-long dots,
                                the roots and quotients, the target's own scaling and add)
      term = 1 - mean c         dterm = mean dc + 2 (B + 1) u mean |c| + 4 u
      G = w dc/dq               dG = w |d2c/dq2| dq + 2 (3 d + 8) u |G|mag
      dX = G P, gP = G^T X, gpb = colsum G   the dot bound with K = d, S B, S B, plus dG carried
      gE, gT, gV: a row's occurrences added to the regulariser row: 2 (count + 1) u sum |terms|.
    d2c/dq2 = -(th q^T + q th^T) / n^3 - c I / n^2 + 3 c q q^T / n^4 (no clamp: |q| >> 1e-8 here)."""
    d, B = c["E"].shape[1], len(c["users"])
    aP, apb = np.abs(c["P"].astype(np.float64)), np.abs(c["pb"].astype(np.float64))
    x, q, tg = r["x"], r["q"], r["tg"]
    S = len(x)
    dq, dG, Gmag = {}, {}, {}
    for s in x:
        ax = np.abs(x[s])
        dq[s] = 2 * (d + 1) * U24 * (ax @ aP.T + apb) + (U24 * ax @ aP.T if s == "item" else 0.0)
        dG[s], Gmag[s] = np.zeros_like(x[s]), np.zeros_like(x[s])
    rc = 2 * (3 * d + 8) * U24
    dterm = np.zeros(7)
    for k, (o, t, w) in enumerate(PAIRS):
        if o not in q:
            continue
        Q, Tt = q[o], tg[t]
        qn = np.linalg.norm(Q, axis=1, keepdims=True)
        assert qn.min() > 1e-3
        th = Tt / np.maximum(np.linalg.norm(Tt, axis=1, keepdims=True), R.EPS)
        cc = (Q * th).sum(1, keepdims=True) / qn
        dc = th / qn - cc / qn * Q / qn
        cmag = (np.abs(Q) * np.abs(th)).sum(1, keepdims=True) / qn
        dcos = (np.abs(dc) * dq[o]).sum(1, keepdims=True) + rc * cmag
        dterm[k] = dcos.mean() + 2 * (B + 1) * U24 * np.abs(cc).mean() + 4 * U24
        a = (np.abs(Q) * dq[o]).sum(1, keepdims=True)
        b = (np.abs(th) * dq[o]).sum(1, keepdims=True)
        J = (np.abs(th) * a + np.abs(Q) * b) / qn ** 3 + np.abs(cc) * dq[o] / qn ** 2 + 3 * np.abs(cc) * np.abs(Q) * a / qn ** 4
        gm = w / B * (np.abs(th) / qn + np.abs(cc) * np.abs(Q) / qn ** 2)
        dG[o] += w / B * J + rc * gm
        Gmag[o] += gm
    out = r["out"]
    reg_err = 8 * U24 * out[7]
    dtotal = dterm[0] + dterm[1] + CL * dterm[2:6].sum() + REG * reg_err + \
        16 * U24 * (np.abs(out[1:3]).sum() + CL * np.abs(out[3:7]).sum() + REG * out[7])
    bounds = dict(out=np.concatenate([[dtotal], dterm[:6], [reg_err]]))
    n = S * B
    bounds["gP"] = sum(dG[s].T @ np.abs(x[s]) + (Gmag[s].T @ (U24 * np.abs(x[s])) if s == "item" else 0.0) for s in x) + \
        2 * (n + 1) * U24 * sum(Gmag[s].T @ np.abs(x[s]) for s in x)
    bounds["gpb"] = sum(dG[s].sum(0) for s in x) + 2 * (n + 1) * U24 * sum(Gmag[s].sum(0) for s in x)
    nu = c["nu"]
    reg = np.abs(r["gE_reg"])
    acc = {"gE": (np.zeros_like(reg), np.zeros_like(reg), np.zeros(reg.shape[0])), "gT": None, "gV": None}
    for s in x:
        ddX = dG[s] @ aP + 2 * (d + 1) * U24 * (Gmag[s] @ aP)
        mag = Gmag[s] @ aP
        key = {"user": "gE", "item": "gE", "text": "gT", "image": "gV"}[s]
        if acc[key] is None:
            rows = c["E"].shape[0] - nu
            acc[key] = (np.zeros((rows, d)), np.zeros((rows, d)), np.zeros(rows))
        idx = c["users"] if s == "user" else c["items"] + (nu if s == "item" else 0)
        np.add.at(acc[key][0], idx, ddX)
        np.add.at(acc[key][1], idx, mag)
        np.add.at(acc[key][2], idx, 1.0)
    for key, v in acc.items():
        if v is not None:
            base = reg if key == "gE" else 0.0
            bounds[key] = v[0] + 2 * (v[2][:, None] + 1) * U24 * (v[1] + base) + (8 * U24 * base)
    return bounds


# ------------------------------------------------------------------ 1: the kernels vs float64
@pytest.mark.parametrize("d", [32, 64, 128])
def test_loss_kernels_vs_float64(cuda, d):
    worst = {}
    for B in (1, 63, 65, 200):
        for has_t, has_v in ((True, True), (True, False), (False, True), (False, False)):
            for p in (0.0, 0.3):
                c = _inputs(d, B, has_t, has_v, p, seed=1000 * d + 10 * B + 2 * has_t + has_v)
                r = R.loss_grad(c["E"], c["H"], c["T"], c["V"], c["P"], c["pb"], c["users"], c["items"], NU, REG, CL,
                                float(np.float32(p)), c["keep"])
                out, g = _run(cuda, c)
                bd = _bounds(c, r)
                assert np.all(np.isfinite(out))
                for key in ("out", "gE", "gT", "gV", "gP", "gpb"):
                    got = out if key == "out" else g[key]
                    if r[key] is None:
                        assert got is None
                        continue
                    ratio = np.abs(got - r[key]) / np.maximum(bd[key], 1e-300)
                    worst[key] = max(worst.get(key, 0.0), float(ratio.max()))
                    k = int(np.argmax(ratio))
                    assert np.all(np.abs(got - r[key]) <= bd[key]), (key, B, has_t, has_v, p, k, got.flat[k],
                                                                     np.asarray(r[key]).flat[k], bd[key].flat[k])
                if not has_t:
                    assert out[3] == 0 and out[5] == 0
                if not has_v:
                    assert out[4] == 0 and out[6] == 0
    print(f"d {d}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_all_dropped_target_row_gives_cosine_zero(cuda):
    """B = 1 and the item target row all dropped: cos(q_u, 0) = 0, so the ui term is exactly
    1, finite, and the user row receives the regulariser's gradient alone."""
    c = _inputs(64, 1, False, False, 0.3, seed=5)
    out, g = _run(cuda, c)
    r = R.loss_grad(c["E"], c["H"], None, None, c["P"], c["pb"], c["users"], c["items"], NU, REG, CL,
                    float(np.float32(0.3)), c["keep"])
    print(f"terms {out[1:3]} (restatement {r['out'][1:3]})")
    assert out[1] == 1.0 and out[2] == 1.0 and np.all(np.isfinite(out))
    assert all(np.all(np.isfinite(v)) for v in g.values() if v is not None)
    u = int(c["users"][0])
    assert np.all(np.abs(g["gE"][u] - r["gE_reg"][u]) <= 8 * U24 * np.abs(r["gE_reg"][u]))


def test_forward_is_deterministic_and_hashed_masks_follow_the_seed(cuda):
    c = _inputs(64, 200, True, True, 0.3, seed=9)
    a, _ = _run(cuda, c, backward=False)
    b, _ = _run(cuda, c, backward=False)
    assert np.array_equal(a, b)
    h1, _ = _run(cuda, c, masks=False, seed=11, backward=False)
    h2, _ = _run(cuda, c, masks=False, seed=11, backward=False)
    h3, _ = _run(cuda, c, masks=False, seed=12, backward=False)
    assert np.array_equal(h1, h2) and not np.array_equal(h1[1:7], h3[1:7])
    assert h1[7] == h3[7] == a[7]  # the regulariser sees no dropout


def test_unsupported_shapes_are_refused(cuda):
    from rsx import _lib as L
    from rsx import bm3

    z = torch.zeros(64 * 64, device=cuda)
    idx = torch.zeros(8, dtype=torch.int64, device=cuda)
    ws = bm3.workspace(8, 64, cuda)
    a = bm3.bm3_args(z.view(64, 64), z[: 32 * 64].view(32, 64), None, None, z.view(64, 64), z[:64], idx, idx, 32,
                     REG, CL, 0.0, None, None, ws)
    for d in (16, 48, 256):
        a.d = d
        assert L.lib().rsx_bm3_loss_fwd(a, None, None) == L.RSX_ERR_UNSUPPORTED
    a.d, a.ws_bytes = 64, 16
    out = torch.zeros(8, device=cuda)
    assert L.lib().rsx_bm3_loss_fwd(a, out.data_ptr(), None) == 1003
    a.ws_bytes, a.p_drop = ws.numel(), 0.3  # a hashed stream without a seed
    assert L.lib().rsx_bm3_loss_fwd(a, out.data_ptr(), None) == 1001


# ------------------------------------------------------------------ 2: rows off the batch
def test_rows_off_the_batch(cuda):
    """gT, gV are exactly zero off the batch's items; gE off the batch is the regulariser's
    gradient alone: the same bits whatever the batch, and the restatement's values."""
    nu, ni, d = 50, 40, 64
    c = _inputs(d, 65, True, True, 0.3, seed=21, nu=nu, ni=ni, zero_row=False)
    c["users"], c["items"] = c["users"] % 20, c["items"] % 15  # users 20.., items 15.. never occur
    c2 = dict(c, users=(c["users"] + 7) % 20, items=(c["items"] + 3) % 15)
    r = R.loss_grad(c["E"], c["H"], c["T"], c["V"], c["P"], c["pb"], c["users"], c["items"], nu, REG, CL,
                    float(np.float32(0.3)), c["keep"])
    _, g = _run(cuda, c)
    _, g2 = _run(cuda, c2)
    off_u = np.setdiff1d(np.arange(nu), c["users"])
    off_i = np.setdiff1d(np.arange(ni), c["items"])
    assert off_u.size >= 30 and off_i.size >= 25
    assert np.all(g["gT"][off_i] == 0) and np.all(g["gV"][off_i] == 0)
    assert np.any(g["gT"][c["items"]] != 0) and np.any(g["gV"][c["items"]] != 0)
    off = np.concatenate([off_u, nu + off_i])
    off2 = np.concatenate([np.setdiff1d(np.arange(nu), c2["users"]), nu + np.setdiff1d(np.arange(ni), c2["items"])])
    both = np.intersect1d(off, off2)
    assert np.array_equal(g["gE"][both], g2["gE"][both])  # the batch adds exactly nothing there
    err = np.abs(g["gE"][off] - r["gE_reg"][off])
    print(f"off-batch gE vs regulariser: max err / (8 u |g|) = {float((err / (8 * U24 * np.abs(r['gE_reg'][off]))).max()):.3f}")
    assert np.all(err <= 8 * U24 * np.abs(r["gE_reg"][off]))
    on = np.concatenate([np.unique(c["users"]), nu + np.unique(c["items"])])
    assert np.all(np.any(g["gE"][on] != r["gE_reg"][on].astype(np.float32), axis=1))


# ------------------------------------------------------------------ 3: hashed dropout
def test_hashed_dropout(cuda):
    """p = 0.3, d = 64, 4,096 distinct rows a stream (262,144 draws): the keep rate, the
    scale of the kept values, one mask for two occurrences of a row, four different streams,
    different masks for consecutive seeds."""
    from rsx import bm3

    n, d, p = 4096, 64, 0.3
    rng = np.random.default_rng(4)
    E = (rng.standard_normal((2 * n, d)) + 3.0).astype(np.float32)  # no zeros
    E[n:] = E[:n]  # the four tables hold the same values: targets differ by their masks only
    H = np.zeros((n, d), np.float32)
    t = dict(E=dev(E, cuda), H=dev(H, cuda), T=dev(E[n:], cuda), V=dev(E[n:], cuda),
             P=torch.eye(d, device=cuda), pb=torch.zeros(d, device=cuda))
    idx = np.concatenate([np.arange(n), [5]]).astype(np.int64)  # row 5 occurs twice
    users = items = dev(idx, cuda)
    B = idx.size
    ws = bm3.workspace(B, d, cuda)
    outs = []
    for seed in (100, 101):
        sd = torch.tensor([seed], dtype=torch.int64, device=cuda)
        a = bm3.bm3_args(t["E"], t["H"], t["T"], t["V"], t["P"], t["pb"], users, items, n, REG, CL, p, sd, None, ws)
        outs.append(bm3.targets(a, cuda).cpu().numpy().reshape(4, B, d))
    tg = outs[0]
    p32 = float(np.float32(p))
    scale = np.float32(1.0 / (1.0 - p32))
    sigma = np.sqrt(p32 * (1 - p32) / (n * d))
    x = E[:n]
    for s in range(4):
        keep = tg[s, :n] != 0
        rate = keep.mean()
        print(f"stream {s}: keep rate {rate:.5f} (0.7 +- 4 sigma = {4 * sigma:.5f})")
        assert abs(rate - (1 - p32)) <= 4 * sigma
        assert np.array_equal(tg[s, :n][keep], (x * scale)[keep])  # exactly x / (1 - p) in f32
        assert np.array_equal(tg[s, n], tg[s, 5])  # the second occurrence of row 5: the same mask
    masks = [tg[s, :n] != 0 for s in range(4)]
    for i in range(4):
        for j in range(i + 1, 4):  # independent streams agree on about 0.7^2 + 0.3^2 = 0.58 of the elements
            agree = (masks[i] == masks[j]).mean()
            assert agree < 0.6, (i, j, agree)
    for s in range(4):
        assert ((outs[1][s, :n] != 0) == masks[s]).mean() < 0.6  # the next seed: another mask


# ------------------------------------------------------------------ the model on the fixture data
def _setup(tmp_path, extra):
    z = R.load_fixture("small")
    write_dataset(tmp_path, z["v_feat"], z["t_feat"])
    return loaders("BM3", tmp_path, {"n_layers": 1, "dropout": 0.0, "reg_weight": 0.1, **extra})


def _model(tmp_path, extra=None):
    c, train, valid, test = _setup(tmp_path, extra or {})
    return make_model("BM3", c, train), c, train, valid, test


def _named(m):
    sd = dict(m.named_parameters())
    assert list(sd) == list(R.NAMES)  # the reference's names in its creation order
    return sd


def test_init_graph_and_first_step_vs_reference(cuda, tmp_path):
    z = R.load_fixture("step0")
    m, *_ = _model(tmp_path, dict(n_layers=2, dropout=0.3))
    sd = _named(m)
    for n in R.NAMES:
        assert np.array_equal(sd[n].detach().cpu().numpy().view(np.int32), z["init." + n].view(np.int32)), n
    # the two tables are adjacent in one buffer: the ego table is no copy
    from rsx.blocks import _ego

    ego = _ego(m.user_embedding.weight, m.item_id_embedding.weight)
    assert ego.data_ptr() == m.user_embedding.weight.data_ptr() and ego.shape == (600, 64)
    # the graph: the captured norm_adj
    A = m.norm_adj_csr
    rows = np.repeat(np.arange(600), np.diff(A.rowptr_host))
    order = np.lexsort((z["adj_idx"][1], z["adj_idx"][0]))
    assert np.array_equal(rows, z["adj_idx"][0][order]) and np.array_equal(A.col.cpu().numpy(), z["adj_idx"][1][order])
    assert np.array_equal(A.val.cpu().numpy().view(np.int32), z["adj_val"][order].view(np.int32))
    # the first step with the masks torch drew
    masks = {s: dev(z["keep_" + s].view(np.int32), cuda) for s in R.STREAMS}
    m.train()
    loss = m.calculate_loss(dev(z["pairs"].astype(np.int64), cuda), keep_masks=masks)
    loss.backward()
    want = float(z["step0_loss"])
    print(f"loss {loss.item():.8f} vs reference {want:.8f} (rel {abs(loss.item() - want) / want:.2e})")
    assert abs(loss.item() - want) <= 1e-5 * abs(want)
    terms = m.last_terms.cpu().numpy()
    assert np.all(np.abs(terms[1:] - z["step0_terms"]) <= 1e-5 * np.maximum(np.abs(z["step0_terms"]), 1e-2))
    for n in R.NAMES:
        w = z["step0_grad." + n]
        scale = float(np.abs(w).max())
        err = float(np.abs(sd[n].grad.cpu().numpy() - w).max())
        print(f"  {n}: err {err:.3e}, scale {scale:.3e}, err / scale {err / scale:.2e} (bound 1e-5)")
        assert err <= 1e-5 * scale, n


def _train(tmp_path, extra, epochs, record=False):
    from rsx.trainer import Trainer

    m, c, train, valid, test = _model(tmp_path, extra)
    t = Trainer(c, m)
    assert not t.fused and type(t.optimizer).__name__ == "RsxAdam"
    assert len(t.optimizer.param_groups[0]["params"]) == len(R.NAMES)  # RsxAdam steps every parameter
    rec = record_batches(train) if record else []
    return m, t, valid, test, rec, train_epochs(t, m, train, epochs)


def test_trainer_vs_reference(cuda, tmp_path):
    z = R.load_fixture("small")
    m, t, valid, test, rec, losses = _train(tmp_path, {}, 2, record=True)
    want = np.concatenate([z[f"epoch{e}_pairs"] for e in range(2)], axis=1).astype(np.int64)
    got = torch.cat(rec, dim=1).numpy()
    assert got.shape[0] == 2 and np.array_equal(got, want)
    assert t._graph is not None and t._graph.replays > 0  # the captured step ran, the short last batch included
    print(f"epoch losses {losses} vs reference {z['epoch_losses']}; {t._graph.replays} replayed batches")
    sd = _named(m)
    for n in R.NAMES:
        err = float(np.abs(sd[n].detach().cpu().numpy() - z["epoch1_param." + n]).max())
        print(f"{n}: max |param - reference| = {err:.3e} (bound 5e-5)")
        assert err <= 5e-5, n
    for split, loader in (("valid", valid), ("test", test)):
        tag = f"epoch1_{split}"
        res = t.evaluate(loader)
        ref = metric_dict(z, tag)
        assert res.keys() == ref.keys()
        for k in ref:
            assert abs(res[k] - ref[k]) <= 1e-4 + 1e-12, (k, res[k], ref[k])
        assert np.array_equal(loader.eval_u.cpu().numpy(), z[tag + "_users"])
        _, idx = m.full_sort_topk([loader.eval_u, None], 50, loader)
        same = np.all(idx.cpu().numpy() == z[tag + "_topk_idx"].astype(np.int64), axis=1)
        assert np.all(same | z[tag + "_inner_tie"] | z[tag + "_boundary_tie"])
        sc = m.full_sort_predict([loader.eval_u[:8], None])
        assert sc.shape == (8, int(z["n_items"]))


def test_device_pair_loader(cuda, tmp_path):
    """rsx_sampler: device: the existing epoch shuffle without the negative row: [2, B]
    batches that cover the training interactions once an epoch."""
    z = R.load_fixture("small")
    c, train, *_ = _setup(tmp_path, dict(rsx_sampler="device"))
    got = list(train)
    assert [tuple(b.shape) for b in got] == [(2, 512)] * 5 + [(2, 462)]
    assert all(b.dtype == torch.int64 and b.is_cuda for b in got)
    pairs = torch.cat(got, dim=1).cpu().numpy()
    key = lambda u, i: np.sort(u.astype(np.int64) * 1000 + i)  # noqa: E731
    assert np.array_equal(key(pairs[0], pairs[1]), key(z["train_u"], z["train_i"]))


# ------------------------------------------------------------------ capture
def _steps(tmp_path, tag, dropout, batches, graph):
    """Adam steps over `batches` with the Trainer's train_step (graph: the captured step
    where the Trainer allows it); returns (model, per-batch losses, trainer)."""
    from rsx.trainer import Trainer

    m, c, *_ = _model(tmp_path / tag, dict(dropout=dropout, rsx_graph_step=graph))
    t = Trainer(c, m)
    m.train()
    t._gate = False
    out = []
    for k, b in enumerate(batches):
        _, loss = t.train_step(b, k)
        out.append(loss)
    torch.cuda.synchronize()
    return m, [float(x) for x in out], t


def test_captured_step_replays(cuda, tmp_path):
    """One eager step, the capture and replays against eager steps (dropout 0), a short last
    batch after a captured full one, and with dropout 0.3 two replays of one batch giving
    different losses: the seed advances on the device."""
    z = R.load_fixture("small")
    full = dev(R.epoch_pairs(z, 0)[0], cuda)
    short = dev(R.epoch_pairs(z, 0)[-1], cuda)
    seq = [full, full, full, full, short, short, short]
    a, la, ta = _steps(tmp_path, "graph", 0.0, seq, True)
    b, lb, tb = _steps(tmp_path, "eager", 0.0, seq, False)
    # batch 0 eager, batch 1 captured, 2 and 3 replays; 4 eager (a new shape), 5 captured, 6 a replay
    assert ta._graph is not None and ta._graph.replays == 5 and tb._graph is None
    worst = max(float((p - q).abs().max()) for p, q in zip(a.parameters(), b.parameters()))
    print(f"graph vs eager after 7 steps: {worst:.3e} (bound 5e-5); losses {la} / {lb}")
    assert worst <= 5e-5
    assert np.all(np.abs(np.array(la) - np.array(lb)) <= 1e-5 * np.abs(lb))
    _, ld, td = _steps(tmp_path, "drop", 0.3, [full] * 4, True)
    assert td._graph.replays == 3
    # the parameters move by lr = 1e-3 a step; fresh masks move the loss far more
    print(f"dropout 0.3, one batch replayed: losses {ld}")
    frozen = td.model._drop_seed.clone()
    assert int(frozen) == 999 * 1000003 + 29 + 4  # advanced once per step, replays included
    assert abs(ld[2] - ld[3]) > 1e-3 and abs(ld[2] - ld[1]) > 1e-3


# ------------------------------------------------------------------ entry points
def test_quick_start(cuda, tmp_path):
    z = R.load_fixture("small")
    res = quick_start_case("BM3", tmp_path, z["v_feat"], z["t_feat"],
                           {"epochs": 1, "n_layers": [1], "reg_weight": [0.1], "dropout": [0.3]})
    assert len(res) == 1 and "recall@20" in res[0][1]
    assert all(np.isfinite(v) for v in res[0][1].values())


def test_feature_width_not_a_multiple_of_4_is_refused(cuda, tmp_path):
    from rsx.utils import get_model, init_seed

    c, train, *_ = _setup(tmp_path, {})
    z = R.load_fixture("small")
    np.save(tmp_path / "data" / "baby" / "text_feat_raw.npy", z["t_feat"][:, :22])
    init_seed(999)
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED.*22"):
        get_model("BM3")(c, train)
