"""MGCN on the GPU: the purifier and fuser kernels (csrc/mgcn.hip, rsx.mgcn_fuse) against
the float64 restatement (tests/mgcn_ref.py), and the model (rsx.mgcn.MGCN) against the
reference's own outputs (tests/golden/mgcn_step0_small.npz, mgcn_small.npz).

Kernel bound: 1e-4 of the tensor's scale (tests/test_gpu_smore_fuse.py's bound for the same
arithmetic), or 4x the error the float32 torch-autograd composition of the reference's ops
(mgcn.py:152-154,187-201, on the CPU) makes against the same restatement on the same
inputs, whichever is larger.  The second term is there for d W1 / d b1 / d w2, which are
sums of nearly cancelling terms wherever the image and the text row nearly agree; it is
measured against the reference's ops, never against the kernel.

The rows form sums repeated rows per occurrence in a fixed order (no float atomics): two
runs are bit-equal, and the captured graph step equals the eager one bit for bit."""
import numpy as np
import pytest
import torch

import mgcn_ref as R
from helpers import (assert_same_run, check_eval, check_params, check_vs_f32, coo_sorted, csr_to_sorted, dev, loaders,
                     make_model, quick_start_case, record_batches, train_epochs, write_dataset)

pytestmark = pytest.mark.gpu
SHAPES = [(64, 5), (64, 65), (128, 37), (64, 1001)]


# ------------------------------------------------------------------ purifier
def _purify_inputs(d, n, seed):
    rng = np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32)  # noqa: E731
    return dict(item=f32(rng.standard_normal((n, d)) * 0.3), feat=[f32(rng.standard_normal((n, d))) for _ in range(2)],
                W=[f32(rng.standard_normal((d, d)) / np.sqrt(d)) for _ in range(2)],
                b=[f32(rng.standard_normal(d) * 0.1) for _ in range(2)],
                go=[f32(rng.standard_normal((n, d))) for _ in range(2)])


def _torch_purify(x):
    t = lambda a: torch.from_numpy(a).clone().requires_grad_(True)  # noqa: E731
    item, feat, W, b = t(x["item"]), [t(a) for a in x["feat"]], [t(a) for a in x["W"]], [t(a) for a in x["b"]]
    out = [torch.multiply(item, torch.sigmoid(torch.nn.functional.linear(feat[m], W[m], b[m]))) for m in range(2)]
    sum((o * torch.from_numpy(g)).sum() for o, g in zip(out, x["go"])).backward()
    n = lambda a: a.detach().numpy()  # noqa: E731
    return dict(out=[n(o) for o in out], g_item=n(item.grad), g_feat=[n(a.grad) for a in feat],
                dW=[n(a.grad) for a in W], db=[n(a.grad) for a in b])


@pytest.mark.parametrize("d,n", SHAPES)
def test_purifier_vs_restatement(cuda, d, n):
    from rsx import mgcn_fuse as MF

    x = _purify_inputs(d, n, 10 + n)
    ref = R.purify(x["item"], x["feat"], x["W"], x["b"], gout=x["go"])
    tor = _torch_purify(x)
    item = dev(x["item"], cuda, True)
    feat, W, b = ([dev(a, cuda, True) for a in x[k]] for k in ("feat", "W", "b"))
    out = MF._Purify.apply(feat[0], feat[1], item, W[0], b[0], W[1], b[1])
    torch.autograd.backward(out, [dev(g, cuda) for g in x["go"]])
    c = lambda t: t.detach().cpu().numpy()  # noqa: E731
    for m in range(2):
        check_vs_f32(f"out[{m}]", c(out[m]), ref["out"][m], tor["out"][m])
        check_vs_f32(f"g_feat[{m}]", c(feat[m].grad), ref["g_feat"][m], tor["g_feat"][m])
        check_vs_f32(f"dW[{m}]", c(W[m].grad), ref["dW"][m], tor["dW"][m])
        check_vs_f32(f"db[{m}]", c(b[m].grad), ref["db"][m], tor["db"][m])
    check_vs_f32("g_item", c(item.grad), ref["g_item"], tor["g_item"])
    # one upstream gradient absent (NULL = zero)
    item.grad = None
    out = MF._Purify.apply(feat[0].detach(), feat[1].detach(), item, W[0].detach(), b[0].detach(), W[1].detach(),
                           b[1].detach())
    out[1].backward(dev(x["go"][1], cuda))
    half = R.purify(x["item"], x["feat"], x["W"], x["b"], gout=[None, x["go"][1]])
    check_vs_f32("g_item (image gradient absent)", c(item.grad), half["g_item"], half["g_item"])


# --------------------------------------------------------------------- fuser
WKEYS = ("W1", "b1", "w2", "Wip", "bip", "Wtp", "btp")
GKEYS = ("dW1", "db1", "dw2", "dWip", "dbip", "dWtp", "dbtp")


def _fuse_inputs(d, N, seed, variant="plain", rows=None):
    rng = np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32)  # noqa: E731
    x = {k: f32(rng.standard_normal((N, d)) * 0.5) for k in ("C", "I", "T")}
    for k in ("W1", "Wip", "Wtp"):
        x[k] = f32(rng.standard_normal((d, d)) / np.sqrt(d))
    for k in ("b1", "bip", "btp"):
        x[k] = f32(rng.standard_normal(d) * 0.1)
    x["w2"] = f32(rng.standard_normal((1, d)) / np.sqrt(d))
    if variant == "saturate":  # the two scores far apart: the softmax saturates
        x["W1"], x["w2"] = x["W1"] * 8, x["w2"] * 8
    if variant == "equal":  # the text row equal to the image row on half the rows
        x["T"][::2] = x["I"][::2]
    n = N if rows is None else len(rows)
    x["rows"] = rows
    x["gA"], x["gS"] = f32(rng.standard_normal((n, d))), f32(rng.standard_normal((n, d)))
    x["gCi"] = None if rows is None else f32(rng.standard_normal((n, d)))
    return x


def _ref_fuse(x):
    return R.fuse(x["C"], x["I"], x["T"], *[x[k] for k in WKEYS], rows=x["rows"], g_all=x["gA"], g_side=x["gS"],
                  g_cin=x["gCi"])


def _torch_fuse(x):
    """The reference's ops (mgcn.py:187-201) in float32 torch on the CPU, with autograd."""
    t = lambda a: torch.from_numpy(a).clone().requires_grad_(True)  # noqa: E731
    C, I, T = t(x["C"]), t(x["I"]), t(x["T"])  # noqa: E741
    W1, b1, w2, Wip, bip, Wtp, btp = (t(x[k]) for k in WKEYS)
    F = torch.nn.functional
    rows = torch.arange(C.shape[0]) if x["rows"] is None else torch.from_numpy(np.asarray(x["rows"], dtype=np.int64))
    content, image, text = C[rows], I[rows], T[rows]
    query = lambda e: F.linear(torch.tanh(F.linear(e, W1, b1)), w2)  # noqa: E731
    weight = torch.softmax(torch.cat([query(image), query(text)], dim=-1), dim=-1)
    common = weight[:, 0].unsqueeze(dim=1) * image + weight[:, 1].unsqueeze(dim=1) * text
    sep_i = torch.multiply(torch.sigmoid(F.linear(content, Wip, bip)), image - common)
    sep_t = torch.multiply(torch.sigmoid(F.linear(content, Wtp, btp)), text - common)
    side = (sep_i + sep_t + common) / 3
    all_ = content + side
    loss = (all_ * torch.from_numpy(x["gA"])).sum() + (side * torch.from_numpy(x["gS"])).sum()
    if x["gCi"] is not None:
        loss = loss + (content * torch.from_numpy(x["gCi"])).sum()
    loss.backward()
    n = lambda a: a.detach().numpy()  # noqa: E731
    r = dict(all=n(all_), side=n(side), content=n(content), gC=n(C.grad), gI=n(I.grad), gT=n(T.grad))
    r.update({g: n(w.grad) for g, w in zip(GKEYS, (W1, b1, w2, Wip, bip, Wtp, btp))})
    return r


def _run_fuse(x, cuda):
    from rsx import mgcn_fuse as MF

    C, I, T = (dev(x[k], cuda, True) for k in ("C", "I", "T"))  # noqa: E741
    w = [dev(x[k], cuda, True) for k in WKEYS]
    rows = None if x["rows"] is None else dev(np.asarray(x["rows"], dtype=np.int64), cuda)
    out = MF._Fuse.apply(C, I, T, rows, *w)
    gs = [dev(x["gA"], cuda), dev(x["gS"], cuda)] + ([] if rows is None else [dev(x["gCi"], cuda)])
    torch.autograd.backward(out, gs)
    c = lambda t: t.detach().cpu().numpy()  # noqa: E731
    r = dict(all=c(out[0]), side=c(out[1]), gC=c(C.grad), gI=c(I.grad), gT=c(T.grad))
    if rows is not None:
        r["content"] = c(out[2])
    r.update({g: c(t.grad) for g, t in zip(GKEYS, w)})
    return r


def _check_fuse(got, ref, tor, keys):
    for k in keys:
        check_vs_f32(k, got[k], ref[k], tor[k])


@pytest.mark.parametrize("variant", ["plain", "saturate", "equal"])
@pytest.mark.parametrize("d,n", SHAPES)
def test_fuser_full_vs_restatement(cuda, d, n, variant):
    x = _fuse_inputs(d, n, 20 + n, variant)
    got = _run_fuse(x, cuda)
    _check_fuse(got, _ref_fuse(x), _torch_fuse(x), ("all", "side", "gC", "gI", "gT") + GKEYS)


@pytest.mark.parametrize("d", [64, 128])
def test_fuser_equal_views_weights_are_one_half(cuda, d):
    """T = I on every row: both softmax weights are exactly 1/2, so common = I, side = I / 3,
    and d aI = -d aT = 0 exactly: the query MLP's three gradients are exact zeros."""
    x = _fuse_inputs(d, 37, 5)
    x["T"] = x["I"].copy()
    got = _run_fuse(x, cuda)
    np.testing.assert_allclose(got["side"], x["I"] / np.float32(3), rtol=2e-7, atol=0)
    for k in ("dW1", "db1", "dw2"):
        assert not got[k].any(), k
    assert np.all(np.isfinite(got["gI"])) and np.all(np.isfinite(got["gT"]))


def _rows_cases():
    rng = np.random.default_rng(8)
    many = rng.integers(0, 50, 192)
    hot = rng.integers(0, 50, 64)
    hot[rng.permutation(64)[:40]] = 17
    return {"repeats": many, "seven": rng.integers(0, 50, 7), "hot": hot}


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("case", ["repeats", "seven", "hot"])
def test_fuser_rows_form(cuda, d, case):
    rows = _rows_cases()[case]
    if case == "hot":
        assert (rows == 17).sum() >= 40
    x = _fuse_inputs(d, 50, 31, "equal" if case == "hot" else "plain", rows=rows)
    got = _run_fuse(x, cuda)
    # compact outputs: the full form's rows, bit for bit (the same arithmetic per row)
    full = _run_fuse(dict(x, rows=None, gA=np.zeros((50, d), np.float32), gS=np.zeros((50, d), np.float32), gCi=None), cuda)
    for k, src in (("all", full["all"]), ("side", full["side"]), ("content", x["C"])):
        assert np.array_equal(got[k].view(np.int32), src[rows].view(np.int32)), k
    _check_fuse(got, _ref_fuse(x), _torch_fuse(x), ("gC", "gI", "gT") + GKEYS)
    # rows no occurrence names keep an exact zero gradient
    untouched = np.setdiff1d(np.arange(50), rows)
    for k in ("gC", "gI", "gT"):
        assert not got[k][untouched].any(), k
    # deterministic sums: a second run is bit-equal
    again = _run_fuse(x, cuda)
    for k in got:
        assert np.array_equal(got[k].view(np.int32), again[k].view(np.int32)), k


# --------------------------------------------------------------------- model
def _setup(tmp_path, extra=None, feats=None):
    z = R.load_fixture()
    write_dataset(tmp_path, *(feats if feats is not None else (z["v_feat"], z["t_feat"])))
    cfg = dict(is_multimodal_model=True, cl_loss=[0.01])
    cfg.update(extra or {})
    return (z,) + loaders("MGCN", tmp_path, cfg)


def _model(c, train):
    return make_model("MGCN", c, train)


def test_mgcn_init_graphs_forward(cuda, tmp_path):
    z, c, train, *_ = _setup(tmp_path)
    m = _model(c, train)
    named = dict(m.named_parameters())
    assert tuple(named) == R.NAMES and m.tau == 0.5
    for n, p in named.items():
        assert np.array_equal(p.detach().cpu().numpy().view(np.int32), z["init." + n].view(np.int32)), n
    A = m.norm_adj_csr
    ref = coo_sorted(z["norm_adj_idx"].astype(np.int64), z["norm_adj_val"])
    for a, b in zip(ref, csr_to_sorted(A.rowptr.cpu().numpy(), A.col.cpu().numpy(), A.val.cpu().numpy())):
        assert np.array_equal(a, b)
    for name, g in (("image_original_adj", m.image_graph), ("text_original_adj", m.text_graph), ("R", m.R)):
        ref = coo_sorted(z[name + "_idx"].astype(np.int64), z[name + "_val"])
        mine = csr_to_sorted(g.A.rowptr.cpu().numpy(), g.A.col.cpu().numpy(), g.A.val.cpu().numpy())
        assert np.array_equal(ref[0], mine[0]) and np.array_equal(ref[1], mine[1]), name
        if name == "R":
            assert np.array_equal(ref[2], mine[2])
        else:
            np.testing.assert_allclose(mine[2], ref[2], rtol=3e-6, atol=0, err_msg=name)
    m.eval()
    with torch.no_grad():
        u, i = m.forward(None)
        np.testing.assert_allclose(u.cpu().numpy(), z["fwd_user"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(i.cpu().numpy(), z["fwd_item"], rtol=1e-5, atol=1e-6)
        _, _, side, content = m.forward(None, train=True)
        np.testing.assert_allclose(side.cpu().numpy(), z["fwd_side"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(content.cpu().numpy(), z["fwd_content"], rtol=1e-5, atol=1e-6)


def test_mgcn_first_step(cuda, tmp_path):
    z, c, train, *_ = _setup(tmp_path)
    m = _model(c, train)
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=c["learning_rate"])
    trip = dev(z["step0_triplets"].astype(np.int64), cuda)
    loss = m.calculate_loss(trip)
    loss.backward()
    want = float(z["step0_loss"])
    print(f"loss {loss.item():.8f} vs reference {want:.8f}")
    assert abs(loss.item() - want) <= 1e-5 * abs(want)
    _, g64 = R.step0(z)
    mine = {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters()}
    assert set(mine) == set(R.NAMES)
    for n in R.NAMES:
        w = z["step0_grad." + n]
        scale = max(float(np.abs(w).max()), 1e-12)
        if n in R.QUERY:
            # cancelling sums: against the f64 restatement, within 4x the f32 reference's own error
            ref = g64[n].reshape(w.shape)
            bound = 4 * float(np.abs(w - ref).max())
            err = float(np.abs(mine[n] - ref).max())
            print(f"  {n}: err {err:.3e} vs f64, reference's own {bound / 4:.3e}, scale {scale:.3e}")
            assert err <= bound, n
        else:
            np.testing.assert_allclose(mine[n], w, rtol=1e-3, atol=1e-5 * scale, err_msg=n)
    opt.step()
    lr = c["learning_rate"]
    for n, p in m.named_parameters():
        got, want = p.detach().cpu().numpy(), z["step0_param." + n]
        # Adam's first step is -lr * g / (|g| + eps): it differs from the reference's by at most
        # lr * |s(g_mine) - s(g_ref)| (plus rounding), large only where |g| is rounding noise
        sgn = lambda g: g / (np.abs(g) + 1e-8)  # noqa: E731
        bound = lr * np.abs(sgn(mine[n]) - sgn(z["step0_grad." + n])) + 2e-6
        assert np.all(np.abs(got - want) <= bound), n


def test_mgcn_batch_rows_loss_equals_full_tables(cuda, tmp_path):
    z, c, train, *_ = _setup(tmp_path)
    m = _model(c, train)
    m.train()
    trip = dev(z["step0_triplets"].astype(np.int64), cuda)
    trip[0, :40] = trip[0, 0]
    trip[1, 100:140] = trip[2, 7]
    out = []
    for rows in (True, False):
        m.batch_rows = rows
        m.zero_grad(set_to_none=True)
        loss = m.calculate_loss(trip)
        loss.backward()
        out.append((loss.item(), {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters()}))
    (la, ga), (lb, gb) = out
    assert abs(la - lb) <= 1e-5 * abs(lb)
    for n in R.NAMES:
        scale = max(float(np.abs(gb[n]).max()), 1e-30)
        err = float(np.abs(ga[n] - gb[n]).max())
        print(f"  {n}: batch rows vs full tables {err:.3e}, scale {scale:.3e}")
        assert err <= 1e-5 * scale, n


def _steps(tmp_path, tag, batches, graph):
    from rsx.trainer import Trainer

    _, c, train, *_ = _setup(tmp_path / tag, dict(rsx_graph_step=graph))
    m = _model(c, train)
    t = Trainer(c, m)
    m.train()
    t._gate = False
    losses = [t.train_step(b, k)[1] for k, b in enumerate(batches)]
    torch.cuda.synchronize()
    return m, [float(x) for x in losses], t


def test_mgcn_captured_step_equals_eager(cuda, tmp_path):
    z = R.load_fixture()
    trip = z["epoch0_triplets"].astype(np.int64)
    seq = [dev(trip[:, 512 * k: 512 * (k + 1)], cuda) for k in range(3)]
    a, la, ta = _steps(tmp_path, "graph", seq, True)
    b, lb, tb = _steps(tmp_path, "eager", seq, False)
    # batch 0 eager, batch 1 captured, batch 2 a replay
    assert ta._graph is not None and ta._graph.replays >= 1 and tb._graph is None
    assert_same_run(a, b, la, lb)


def test_mgcn_trainer_vs_reference(cuda, tmp_path):
    from rsx.trainer import Trainer

    z, c, train, valid, test = _setup(tmp_path)
    m = _model(c, train)
    t = Trainer(c, m)
    assert not t.fused and type(t.optimizer).__name__ == "RsxAdam"
    rec = record_batches(train)
    losses = train_epochs(t, m, train, 2)
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


@pytest.mark.parametrize("what", ["embedding_size", "knn_k", "no_text", "width"])
def test_mgcn_unsupported_configurations_raise(cuda, tmp_path, what):
    z = R.load_fixture()
    extra, feats = {}, None
    if what == "embedding_size":
        extra = dict(embedding_size=32)
    elif what == "knn_k":
        extra = dict(knn_k=33)
    elif what == "no_text":
        feats = (z["v_feat"], None)
    else:
        feats = (z["v_feat"], z["t_feat"][:, :6])
    _, c, train, *_ = _setup(tmp_path, extra, feats)
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        _model(c, train)


def test_mgcn_quick_start(cuda, tmp_path):
    """`main.py -m MGCN -d <dataset>`'s path: trains an epoch and evaluates on a dataset
    directory with the .inter file and the two feature files."""
    z = R.load_fixture()
    res = quick_start_case("MGCN", tmp_path, z["v_feat"], z["t_feat"], {"epochs": 1, "cl_loss": [0.01]})
    assert len(res) == 1 and "recall@20" in res[0][1]
    assert all(np.isfinite(v) for v in res[0][1].values())
