"""FREEDOM on the GPU: the fused loss (csrc/freedom.hip, rsx.freedom._FreedomLoss) against the
float64 restatement (tests/freedom_ref.py), the graphs, and the model (rsx.freedom.FREEDOM)
against the reference's own outputs (tests/golden/freedom_step0_small.npz, freedom_small.npz).

Kernel bound (tests/test_gpu_mgcn.py's rule): the forward's four words 1e-5 relative; the
gradients 1e-4 of the tensor's scale, or 4x the error the same formulas composed from
float32 torch ops (freedom.py:182-212, on the CPU, with autograd) make against the same
restatement on the same inputs, whichever is larger.  Rows off the batch are exact zeros,
two calls are bit-equal (repeated rows are summed in an order fixed by the triplets, no
float atomics), and the captured graph step equals the eager one bit for bit.

Model bounds: the CPU tests' (tests/test_freedom_cpu.py) for the first step, the project's
end-to-end bounds for two epochs (parameters 5e-5 of scale, metrics 1e-4, top-50 equal
modulo the recorded ties)."""
import numpy as np
import pytest
import torch

import freedom_ref as R
from helpers import (assert_same_run, check_eval, check_params, check_vs_f32, coo_sorted, csr_to_sorted, dev, loaders,
                     make_model, quick_start_case, record_batches, train_epochs, write_dataset)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ the loss kernel
def _inputs(d, B, nu, ni, seed):
    rng = np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32)  # noqa: E731
    x = dict(E=f32(rng.standard_normal((nu + ni, d)) * 0.3), H=f32(rng.standard_normal((ni, d)) * 0.3),
             T=f32(rng.standard_normal((ni, d)) * 0.3), V=f32(rng.standard_normal((ni, d)) * 0.3))
    trip = np.stack([rng.integers(0, nu, B), rng.integers(0, ni, B), rng.integers(0, ni, B)]).astype(np.int64)
    if B > 1:  # an item that is a positive in one triplet and a negative in another
        trip[2, 1] = trip[1, 0]
        trip[1, B - 1] = trip[2, 0]
    x["trip"] = trip
    return x


def _torch_loss(x, nu, reg, H, T, V):
    """freedom.py:182-212's ops in float32 torch on the CPU, with autograd."""
    t = lambda a: None if a is None else torch.from_numpy(a).clone().requires_grad_(True)  # noqa: E731
    E, H, T, V = t(x["E"]), t(H), t(T), t(V)
    u, p, n = (torch.from_numpy(r) for r in x["trip"])
    ua, ia = E[:nu], (E[nu:] if H is None else E[nu:] + H)

    def bpr(users, pos, neg):
        pos_scores = torch.sum(torch.mul(users, pos), dim=1)
        neg_scores = torch.sum(torch.mul(users, neg), dim=1)
        return -torch.mean(torch.nn.functional.logsigmoid(pos_scores - neg_scores))

    terms = [bpr(ua[u], ia[p], ia[n]), 0.0, 0.0]
    if T is not None:
        terms[1] = bpr(ua[u], T[p], T[n])
    if V is not None:
        terms[2] = bpr(ua[u], V[p], V[n])
    total = terms[0] + reg * (terms[1] + terms[2])
    total.backward()
    g = lambda a: None if a is None else a.grad.numpy()  # noqa: E731
    return np.array([float(total)] + [float(v) for v in terms]), g(E), g(T), g(V)


def _run_loss(x, nu, reg, H, T, V, cuda):
    from rsx import freedom as F

    d, B = x["E"].shape[1], x["trip"].shape[1]
    ws = F.workspace(B, d, cuda)
    E, Hd, Td, Vd = dev(x["E"], cuda, True), dev(H, cuda, True), dev(T, cuda, True), dev(V, cuda, True)
    keep = {}
    loss = F._FreedomLoss.apply((nu, reg, ws, keep), dev(x["trip"], cuda), E, Hd, Td, Vd, None, None)
    loss.backward()
    c = lambda t: None if t is None else t.detach().cpu().numpy()  # noqa: E731
    out = c(keep["terms"])
    assert out[0] == loss.item()
    if Hd is not None:  # the gradient of H is gE's item block, the same values
        assert np.array_equal(c(Hd.grad), c(E.grad)[nu:])
    return out, c(E.grad), c(Td.grad) if Td is not None else None, c(Vd.grad) if Vd is not None else None


@pytest.mark.parametrize("nu,ni", [(5, 7), (400, 200)])
@pytest.mark.parametrize("B", [1, 67, 300, 512])
@pytest.mark.parametrize("d", [64, 128])
def test_loss_kernel_vs_restatement(cuda, d, B, nu, ni):
    x = _inputs(d, B, nu, ni, 100 + d + B + nu)
    trip = x["trip"]
    if B == 512 and nu == 5:  # every row repeats more than a wave's 64 lanes
        assert np.bincount(trip[0], minlength=nu).min() > 64
        assert np.bincount(np.concatenate([trip[1], trip[2]]), minlength=ni).min() > 64
    if B > 1:
        assert np.intersect1d(trip[1], trip[2]).size
    for reg in (0.0, 0.5):
        for has_h in (False, True):
            for mod in ("text", "image", "both"):
                H = x["H"] if has_h else None
                T = x["T"] if mod != "image" else None
                V = x["V"] if mod != "text" else None
                print(f"d={d} B={B} tables=({nu},{ni}) reg={reg} H={has_h} {mod}")
                ref = R.loss_grad(x["E"], H, T, V, trip, nu, reg)
                tor = _torch_loss(x, nu, reg, H, T, V)
                got = _run_loss(x, nu, reg, H, T, V, cuda)
                for k, name in enumerate(("total", "id", "text", "image")):
                    print(f"  {name}: {got[0][k]:.8f} vs {ref[0][k]:.8f}")
                    assert abs(got[0][k] - ref[0][k]) <= 1e-5 * abs(ref[0][k]), name
                for k, name in ((1, "gE"), (2, "gT"), (3, "gV")):
                    if ref[k] is None:
                        assert got[k] is None, name
                        continue
                    check_vs_f32(name, got[k], ref[k], tor[k])
                # rows off the batch are exact zeros
                off_u = np.setdiff1d(np.arange(nu), trip[0])
                off_i = np.setdiff1d(np.arange(ni), np.concatenate([trip[1], trip[2]]))
                assert not got[1][off_u].any() and not got[1][nu + off_i].any()
                for g in got[2:]:
                    assert g is None or not g[off_i].any()
                if reg == 0.0:  # the feature terms switched off: their tables get no gradient
                    assert all(g is None or not g.any() for g in got[2:])
                # deterministic: a second call is bit-equal
                again = _run_loss(x, nu, reg, H, T, V, cuda)
                for a, b in zip(got, again):
                    assert (a is None and b is None) or np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("d", [64, 128])
def test_loss_kernel_saturated_scores(cuda, d):
    """Scores of +-40: softplus and its derivative neither overflow nor lose the answer; the
    loss is 40 per wrong triplet and ~0 per right one, the coefficient -1 / B or 0."""
    nu, ni, B, reg = 8, 2, 8, 0.5
    a = np.full(d, np.sqrt(20.0 / d), dtype=np.float32)
    E = np.concatenate([np.tile(a, (nu, 1)), a[None], -a[None]]).astype(np.float32)
    T = E[nu:].copy()
    b = np.arange(B)
    trip = np.stack([b, b % 2, 1 - b % 2]).astype(np.int64)  # even b: x = +40, odd b: x = -40
    x = dict(E=E, trip=trip)
    ref = R.loss_grad(E, None, T, None, trip, nu, reg)
    got = _run_loss(x, nu, reg, None, T, None, cuda)
    assert np.all(np.isfinite(got[0])) and abs(got[0][1] - 20.0) <= 1e-4 and abs(got[0][0] - 30.0) <= 2e-4
    np.testing.assert_allclose(got[0], ref[0], rtol=1e-5)
    gE = got[1]
    assert np.all(np.isfinite(gE)) and np.all(np.isfinite(got[2]))
    unit = (1.0 + reg) * 2.0 * a / B  # -(-1 / B)(1 + reg)(p - n) with p - n = -2 a
    np.testing.assert_allclose(gE[1:nu:2], np.tile(unit, (nu // 2, 1)), rtol=1e-5)
    assert np.abs(gE[0:nu:2]).max() <= 1e-15
    np.testing.assert_allclose(gE, ref[1], rtol=1e-5, atol=1e-15)
    np.testing.assert_allclose(got[2], ref[2], rtol=1e-5, atol=1e-15)


# ------------------------------------------------------------------------ graphs
def test_item_graph_device_vs_host(cuda):
    from rsx.freedom import freedom_item_graph

    z = R.load_fixture()
    v, t = torch.from_numpy(z["v_feat"]), torch.from_numpy(z["t_feat"])
    ni, k = int(z["n_items"]), R.KNN_K
    hr, hc, hw = freedom_item_graph(v, t, k, R.IMAGE_WEIGHT, mode="host")
    dr, dc, dw = freedom_item_graph(v.to(cuda), t.to(cuda), k, R.IMAGE_WEIGHT, mode="device")
    assert np.unique(dw).size <= 3 and set(np.unique(dw).tolist()) <= set(np.unique(hw).tolist())
    host = dict(zip(zip(hr.tolist(), hc.tolist()), hw.tolist()))
    dev = dict(zip(zip(dr.tolist(), dc.tolist()), dw.tolist()))
    fn = [f.astype(np.float64) / np.linalg.norm(f.astype(np.float64), axis=1, keepdims=True)
          for f in (z["v_feat"], z["t_feat"])]
    bad_rows = set()
    for rc in set(host) ^ set(dev) | {rc for rc in set(host) & set(dev) if host[rc] != dev[rc]}:
        # an edge that differs: its similarity ties with the row's k-th within 1e-5 in a modality
        r, c = rc
        ties = False
        for f in fn:
            sims = f[r] @ f.T
            ties = ties or abs(sims[c] - np.sort(sims)[-k]) <= 1e-5
        assert ties, rc
        bad_rows.add(r)
    assert len(bad_rows) <= max(2, ni // 100)


def _setup(tmp_path, extra=None, feats=None):
    z = R.load_fixture()
    write_dataset(tmp_path, *(feats if feats is not None else (z["v_feat"], z["t_feat"])))
    cfg = dict(rsx_edge_dropout="host", rsx_knn="host", is_multimodal_model=True, dropout=[R.HPARAMS["dropout"]],
               reg_weight=[R.HPARAMS["reg_weight"]])
    cfg.update(extra or {})
    return (z,) + loaders("FREEDOM", tmp_path, cfg)


def _model(c, train):
    return make_model("FREEDOM", c, train)


def _csr_sorted(A):
    return csr_to_sorted(A.rowptr.cpu().numpy(), A.col.cpu().numpy()[: A.nnz], A.val.cpu().numpy()[: A.nnz])


def test_freedom_init_graphs_forward(cuda, tmp_path):
    z, c, train, *_ = _setup(tmp_path)
    m = _model(c, train)
    named = dict(m.named_parameters())
    assert tuple(named) == R.NAMES
    for n, p in named.items():
        assert np.array_equal(p.detach().cpu().numpy().view(np.int32), z["init." + n].view(np.int32)), n
    assert np.array_equal(m.edge_indices.numpy(), z["edge_idx"].astype(np.int64))
    ref = coo_sorted(z["norm_adj_idx"].astype(np.int64), z["norm_adj_val"])
    for a, b in zip(ref, _csr_sorted(m.norm_adj_csr)):
        assert np.array_equal(a, b)
    ref = coo_sorted(z["mm_adj_idx"].astype(np.int64), z["mm_adj_val"])
    for a, b in zip(ref, _csr_sorted(m.mm_adj.A)):
        assert np.array_equal(a, b)
    m.eval()
    with torch.no_grad():
        u, i = m.forward()
        np.testing.assert_allclose(u.cpu().numpy(), z["fwd_user"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(i.cpu().numpy(), z["fwd_item"], rtol=1e-5, atol=1e-6)


def test_freedom_epoch_graph(cuda, tmp_path):
    from rsx import graph

    z, c, train, *_ = _setup(tmp_path, dict(rsx_edge_dropout="device"))
    m = _model(c, train)
    nu, ni = m.n_users, m.n_items
    # the fixture's kept edges: the reference's masked_adj, bit for bit
    for ep in (0, 1):
        A = m.build_epoch_graph(z[f"e{ep}_keep_ids"])
        rows, cols, vals = R.masked_coo(z, ep)
        mine = _csr_sorted(A)
        assert np.array_equal(mine[0], rows) and np.array_equal(mine[1], cols)
        assert np.array_equal(mine[2].view(np.int32), vals.view(np.int32))
    # a device draw: int(E (1 - dropout)) distinct edges, symmetric, the host builder's values
    assert m.edge_dropout_mode == "device"
    keep_len = int(m.edge_values.numel() * (1.0 - m.dropout))
    seen = []
    for _ in range(2):
        m.pre_epoch_processing()
        A = m.train_adj
        rp = A.rowptr.cpu().numpy()
        assert int(rp[-1]) == 2 * keep_len == A.nnz
        r, cidx, v = _csr_sorted(A)
        up = r < nu
        ku, ki = r[up], cidx[up] - nu
        assert ku.size == keep_len and np.unique(ku * ni + ki).size == keep_len
        assert np.isin(ku * ni + ki, z["edge_idx"][0].astype(np.int64) * ni + z["edge_idx"][1]).all()
        hrp, hcol, hval = graph.layergcn_masked_adj(ku, ki, nu, ni)
        assert np.array_equal(hrp, rp) and np.array_equal(hcol.astype(np.int64), cidx)
        assert np.array_equal(hval.view(np.int32), v.view(np.int32))
        seen.append(ku * ni + ki)
    assert not np.array_equal(np.sort(seen[0]), np.sort(seen[1]))  # a fresh draw every epoch
    m.dropout = 0.0
    m.pre_epoch_processing()
    assert m.train_adj is m.norm_adj_csr


# ------------------------------------------------------------------------- model
def test_freedom_first_step(cuda, tmp_path):
    z, c, train, *_ = _setup(tmp_path)
    m = _model(c, train)
    m.train()
    m.build_epoch_graph(z["e0_keep_ids"])
    opt = torch.optim.Adam(m.parameters(), lr=c["learning_rate"])
    trip = dev(z["step0_triplets"].astype(np.int64), cuda)
    loss = m.calculate_loss(trip)
    loss.backward()
    want = float(z["step0_loss"])
    print(f"loss {loss.item():.8f} vs reference {want:.8f}; words {m.last_terms.cpu().numpy()}")
    assert abs(loss.item() - want) <= 1e-5 * abs(want)
    mine = {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters()}
    assert set(mine) == set(R.NAMES)
    for n in R.NAMES:
        w = z["step0_grad." + n]
        scale = max(float(np.abs(w).max()), 1e-30)
        err = float(np.abs(mine[n] - w).max())
        print(f"  grad {n}: err {err:.3e}, scale {scale:.3e}")
        if n in R.BIASES:  # analytically zero: an exact zero tensor here, rounding noise there
            bound = 1e-5 * float(np.abs(z["step0_grad." + n.replace(".bias", ".weight")]).max())
            assert not mine[n].any() and np.abs(w).max() <= bound, n
        else:
            np.testing.assert_allclose(mine[n], w, rtol=1e-3, atol=1e-5 * scale, err_msg=n)
    opt.step()
    check_params(m, z, "step0_param.", 1e-5)
    # Adam's state advanced on the biases too (a zero gradient, not an absent one)
    assert all(len(opt.state[p]) for p in m.parameters())


def _steps(tmp_path, tag, z, cuda, graph):
    from rsx.trainer import Trainer

    _, c, train, *_ = _setup(tmp_path / tag, dict(rsx_graph_step=graph))
    m = _model(c, train)
    t = Trainer(c, m)
    m.train()
    t._gate = False
    losses, replays = [], []
    for ep in (0, 1):
        m.build_epoch_graph(z[f"e{ep}_keep_ids"])  # a new epoch graph: the captures are dropped
        t.reset_graph_step()
        trip = z[f"epoch{ep}_triplets"].astype(np.int64)
        for k in range(3):
            losses.append(t.train_step(dev(trip[:, 512 * k: 512 * (k + 1)], cuda), k)[1])
        replays.append(t._graph.replays if t._graph is not None else 0)
    torch.cuda.synchronize()
    return m, [float(x) for x in losses], replays


def test_freedom_captured_step_equals_eager(cuda, tmp_path):
    z = R.load_fixture()
    a, la, ra = _steps(tmp_path, "graph", z, cuda, True)
    b, lb, rb = _steps(tmp_path, "eager", z, cuda, False)
    # per epoch: batch 0 eager, batch 1 captured and replayed, batch 2 a replay; the second
    # epoch captures again on its own graph
    assert ra[0] >= 1 and ra[1] >= 1 and rb == [0, 0]
    assert_same_run(a, b, la, lb)


def test_freedom_trainer_vs_reference(cuda, tmp_path):
    from rsx.trainer import Trainer

    z, c, train, valid, test = _setup(tmp_path)
    m = _model(c, train)
    t = Trainer(c, m)
    assert not t.fused and type(t.optimizer).__name__ == "RsxAdam"
    rec = record_batches(train)
    kept, build = [], m.build_epoch_graph

    def recording(ids):
        kept.append(np.sort(torch.as_tensor(ids).cpu().numpy()))
        return build(ids)

    m.build_epoch_graph = recording

    def the_draw_first(epoch):  # it pins the order the RNG streams are consumed in
        assert len(kept) == epoch + 1 and np.array_equal(kept[epoch], z[f"e{epoch}_keep_ids"]), epoch

    losses = train_epochs(t, m, train, 2, after_pre_epoch=the_draw_first)
    want = np.concatenate([z[f"epoch{e}_triplets"] for e in range(2)], axis=1).astype(np.int64)
    assert np.array_equal(torch.cat(rec, dim=1).numpy(), want)  # the recorded triplets
    assert t._graph is not None and t._graph.replays > 0
    print(f"epoch losses {losses} vs reference {z['epoch_losses']}")
    check_params(m, z, "epoch1_param.", 5e-5)
    check_eval(t, m, z, (("valid", valid), ("test", test)))
    # training again invalidates the cached evaluation tables
    assert m._eval_cache is not None
    m.train()
    assert m._eval_cache is None


@pytest.mark.parametrize("what", ["embedding_size", "feat_embed_dim", "knn_k", "n_ui_layers", "dropout", "no_features",
                                  "width"])
def test_freedom_unsupported_configurations_raise(cuda, tmp_path, what):
    z = R.load_fixture()
    extra, feats = {}, None
    if what == "embedding_size":
        extra = dict(embedding_size=32, feat_embed_dim=32)
    elif what == "feat_embed_dim":
        extra = dict(feat_embed_dim=128)
    elif what == "knn_k":
        extra = dict(knn_k=33)
    elif what == "n_ui_layers":
        extra = dict(n_ui_layers=0)
    elif what == "dropout":
        extra = dict(dropout=[1.0])
    elif what == "no_features":
        extra = dict(is_multimodal_model=False)
    else:
        feats = (z["v_feat"], z["t_feat"][:, :6])
    _, c, train, *_ = _setup(tmp_path, extra, feats)
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        _model(c, train)


def test_freedom_text_only_model(cuda, tmp_path):
    """One modality alone is supported: the item graph is that modality's, the image term is
    absent, and one step's loss is the restatement's with V = None."""
    from rsx.freedom import freedom_item_graph

    z, c, train, *_ = _setup(tmp_path, feats=(None, R.load_fixture()["t_feat"]))
    m = _model(c, train)
    names = tuple(n for n, _ in m.named_parameters())
    assert names == tuple(n for n in R.NAMES if not n.startswith("image"))
    m.train()
    m.build_epoch_graph(z["e0_keep_ids"])
    trip = z["step0_triplets"].astype(np.int64)
    p = {n: q.detach().cpu().numpy() for n, q in m.named_parameters()}
    loss = m.calculate_loss(dev(trip, cuda))
    loss.backward()
    ni = m.n_items
    r, cc, w = freedom_item_graph(None, torch.from_numpy(z["t_feat"]), R.KNN_K, R.IMAGE_WEIGHT, mode="host")
    _, masked, _ = R.dense_graphs(z, 0)
    want, words, g = R.model_loss_grad(p, masked, R.dense((r, cc), w, (ni, ni)), trip, R.HPARAMS["reg_weight"])
    print(f"loss {loss.item():.8f} vs restatement {want:.8f}; words {m.last_terms.cpu().numpy()} vs {words}")
    assert abs(loss.item() - want) <= 1e-5 * abs(want)
    assert m.last_terms[3].item() == 0.0 and words[3] == 0.0
    gt = m.text_trs.weight.grad.cpu().numpy()
    np.testing.assert_allclose(gt, g["text_trs.weight"], rtol=1e-3, atol=1e-5 * np.abs(g["text_trs.weight"]).max())
    assert not m.text_trs.bias.grad.any().item()


def test_freedom_quick_start(cuda, tmp_path):
    """`main.py -m FREEDOM -d <dataset>`'s path: trains an epoch (device edge dropout, device
    kNN: the defaults) and evaluates on a dataset directory with the .inter file and the
    feature files."""
    z = R.load_fixture()
    res = quick_start_case("FREEDOM", tmp_path, z["v_feat"], z["t_feat"],
                           {"epochs": 1, "dropout": [0.8], "reg_weight": [0.001]})
    assert len(res) == 1 and "recall@20" in res[0][1]
    assert all(np.isfinite(v) for v in res[0][1].values())
