"""DualGNN on the GPU: the kernels of csrc/dualgnn.hip (rsx.dualgnn's wrappers) against the float64
restatement (tests/dualgnn_ref.py), and the model (rsx.dualgnn.DualGNN) against the reference's
own run (tests/golden/dualgnn_step0_small.npz, dualgnn_small.npz).

Kernel bound: helpers.check_vs_f32 — 1e-4 of the tensor's scale, or 4x the error the float32
torch composition of the same ops (on the CPU) makes against the same float64 values, whichever
is larger.  Every sum is in a fixed order (no float atomics): two runs are bit-equal, and a run
with captured graph steps equals the eager one bit for bit."""
import os
import types

import numpy as np
import pytest
import torch

import dualgnn_ref as R
from helpers import (LOSS_BATCHES, assert_same_run, check_eval, check_params, check_vs_f32, dev, loaders, loss_triplets,
                     make_model, quick_start_case, train_epochs, write_dataset)

pytestmark = pytest.mark.gpu
c = lambda t: t.detach().cpu().numpy()  # noqa: E731
D = 64


def _randn(seed, *shape):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)).float()


def _lists(nu, k, seed):
    """idx int32 [nu, k], W float32 [nu, k] with the rows the kernel must get right: zero weights
    at index 0, one user k times, a row naming itself, an out-of-range index."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, nu, (nu, k)).astype(np.int32)
    W = torch.softmax(_randn(seed + 1, nu, k), dim=1).numpy().copy()
    idx[0], W[0] = 0, 0.0
    if nu > 3:
        idx[1] = nu - 1
        idx[2] = 2
        idx[3, 0] = nu  # outside the table: contributes nothing
        if k > 1:
            idx[3, k - 1] = -1
    return idx, W


def _ugraph_ref(x, idx, W):
    """The restatement with the out-of-range entries' weights zeroed (they contribute nothing)."""
    nu = x.shape[0]
    ok = (idx >= 0) & (idx < nu)
    return R.ugraph(x, np.where(ok, idx, 0), torch.from_numpy(np.where(ok, W, 0.0)).to(x.dtype))


# ---------------------------------------------------------------- user graph
@pytest.mark.parametrize("k", [1, 40, 64])
@pytest.mark.parametrize("nu", [1, 15, 16, 17, 130])
def test_ugraph_fwd_vs_restatement(cuda, nu, k):
    from rsx import dualgnn as M

    x = _randn(nu * 100 + k, nu, D)
    idx, W = _lists(nu, k, nu + k)
    out = torch.full((nu + 3, D), 7.0, device=cuda)  # rows past nu stay as they are
    M.ugraph_fwd(x.to(cuda), dev(idx, cuda), dev(W, cuda), out=out)
    check_vs_f32("out", c(out[:nu]), _ugraph_ref(x.double(), idx, W), _ugraph_ref(x, idx, W))
    assert torch.equal(out[nu:], torch.full((3, D), 7.0, device=cuda))
    if nu > 3:
        assert np.array_equal(c(out[0]), x[0].numpy())  # zero weights: the row itself
    again = M.ugraph_fwd(x.to(cuda), dev(idx, cuda), dev(W, cuda))
    assert torch.equal(again, out[:nu])


def test_ugraph_fwd_refusals(cuda):
    from rsx import dualgnn as M

    x = _randn(1, 5, D).to(cuda)
    with pytest.raises(RuntimeError, match="rsx_dualgnn_ugraph_fwd failed"):  # k = 0
        M.ugraph_fwd(x, torch.zeros(5, 0, dtype=torch.int32, device=cuda), torch.zeros(5, 0, device=cuda))
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED|1002"):  # k = 65
        M.ugraph_fwd(x, torch.zeros(5, 65, dtype=torch.int32, device=cuda), torch.zeros(5, 65, device=cuda))
    x32 = _randn(1, 5, 32).to(cuda)
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED|1002"):
        M.ugraph_fwd(x32, torch.zeros(5, 4, dtype=torch.int32, device=cuda), torch.zeros(5, 4, device=cuda))
    with pytest.raises(RuntimeError):
        M.ugraph_fwd(x, torch.zeros(5, 4, dtype=torch.int32, device=cuda), torch.zeros(5, 4, device=cuda), out=x)


def test_ugraph_backward_on_the_spmm(cuda):
    """g_user_rep = g + P^T g through the transposed lists: 120 of 130 users all name user 7 (a
    hub row past chunk 32, several chunks), user 9 is named by nobody (an empty row)."""
    from rsx import dualgnn as M
    from rsx import ops

    nu, ni, k = 130, 6, 40
    rng = np.random.default_rng(11)
    idx = rng.integers(0, nu, (nu, k)).astype(np.int32)
    idx[idx == 9] = 10
    idx[:120, 5] = 7
    W = torch.softmax(_randn(12, nu, k), dim=1).numpy().copy()
    W[3] = 0.0  # zero-weight entries stay in the lists
    rp, col, val = M.transposed_lists(idx, W)
    assert rp[-1] == nu * k and rp[10] - rp[9] == 0 and rp[8] - rp[7] >= 120
    PT = ops.DeviceCSR(rp, col, val, nu, cuda, 32)
    assert PT.n_long >= 1
    g = _randn(13, nu + ni, D)
    got = M.ugraph_bwd(PT, g.to(cuda), nu)
    Wt = torch.from_numpy(W)
    check_vs_f32("g_user_rep", c(got), R.ugraph_backward(g[:nu].double(), idx, Wt.double()), R.ugraph_backward(g[:nu], idx, Wt))
    assert np.array_equal(c(got[9]), g[9].numpy())
    # the same gradient by autograd through the restatement's forward
    x = _randn(14, nu, D).double().requires_grad_()
    (R.ugraph(x, idx, Wt.double()) * g[:nu].double()).sum().backward()
    check_vs_f32("g_user_rep (autograd)", c(got), x.grad, R.ugraph_backward(g[:nu], idx, Wt))
    assert torch.equal(M.ugraph_bwd(PT, g.to(cuda), nu), got)


# ----------------------------------------------------------------------- mix
@pytest.mark.parametrize("mods", ["vt", "v", "t"])
@pytest.mark.parametrize("ni", [1, 33])
@pytest.mark.parametrize("nu", [1, 15, 16, 17, 130])
def test_mix_fwd_bwd_vs_restatement(cuda, nu, ni, mods):
    from rsx import dualgnn as M

    n, reg = nu + ni, 0.01
    seed = nu * 1000 + ni * 10 + len(mods)
    xv = _randn(seed, n, D) if "v" in mods else None
    xt = _randn(seed + 1, n, D) if "t" in mods else None
    w = torch.softmax(_randn(seed + 2, nu, 2, 1), dim=1)
    gu, gr = _randn(seed + 3, nu, D), _randn(seed + 4, n, D)
    result = torch.full((n, D), 7.0, device=cuda)
    dv = lambda t: None if t is None else t.to(cuda)  # noqa: E731
    user_rep = M.mix_fwd(dv(xv), dv(xt), w.to(cuda), nu, result)
    res = {}
    for dt in (torch.float64, torch.float32):
        a, b, ww = (None if t is None else t.to(dt).clone().requires_grad_() for t in (xv, xt, w))
        u, i = R.mix(a, b, ww, nu)
        ((u * gu.to(dt)).sum() + (i * gr[nu:].to(dt)).sum() + reg * (ww ** 2).mean()).backward()
        res[dt] = (u.detach(), i.detach(), None if a is None else a.grad, None if b is None else b.grad, ww.grad)
    r64, r32 = res[torch.float64], res[torch.float32]
    check_vs_f32("user_rep", c(user_rep), r64[0], r32[0])
    check_vs_f32("item rows", c(result[nu:]), r64[1], r32[1])
    assert torch.equal(result[:nu], torch.full((nu, D), 7.0, device=cuda))  # the user rows are the user graph's
    go = torch.ones(1, device=cuda)
    g_v, g_t, g_w = M.mix_bwd(gu.to(cuda), gr.to(cuda), dv(xv), dv(xt), w.to(cuda), go, reg, nu)
    for name, got, j in (("g_v", g_v, 2), ("g_t", g_t, 3)):
        assert (got is None) == (r64[j] is None), name
        if got is not None:
            check_vs_f32(name, c(got), r64[j], r32[j])
    assert g_w.shape == (nu, 2, 1)
    check_vs_f32("g_weight_u", c(g_w), r64[4], r32[4])
    if len(mods) == 1:  # one modality: the regulariser alone
        check_vs_f32("g_weight_u (reg)", c(g_w), 2 * reg / (2 * nu) * w.double(), 2 * reg / (2 * nu) * w)
    g2 = M.mix_bwd(gu.to(cuda), gr.to(cuda), dv(xv), dv(xt), w.to(cuda), go, reg, nu)
    assert all(torch.equal(a, b) for a, b in zip((g_v, g_t, g_w), g2) if a is not None)


# ---------------------------------------------------------------------- loss
def _loss_inputs(nu, ni, seed):
    return dict(result=_randn(seed, nu + ni, D) * 0.3, pref_v=_randn(seed + 1, nu, D) * 0.2, pref_t=_randn(seed + 2, nu, D) * 0.2,
                weight_u=torch.softmax(_randn(seed + 3, nu, 2, 1), dim=1), weight_i=torch.softmax(_randn(seed + 4, ni, 2, 1), dim=1))


def _run_loss(cuda, x, trip, nu, reg, mods):
    from rsx import dualgnn as M

    t = {k: v.to(cuda) for k, v in x.items()}
    pv, pt = (t["pref_v"] if "v" in mods else None), (t["pref_t"] if "t" in mods else None)
    ws = M.loss_workspace(trip.shape[1], D, cuda)
    trip_dev = dev(trip, cuda)  # held to the end: the argument struct keeps addresses, not tensors
    a = M.loss_args(t["result"], pv, pt, t["weight_u"], t["weight_i"], trip_dev, nu, reg)
    terms = M.loss_fwd(a, ws)
    g, gpv, gpt, gwi = M.loss_bwd(a, torch.ones(1, device=cuda), ws, pv, pt, t["weight_i"])
    return c(terms), {"result": c(g), "pref_v": None if gpv is None else c(gpv), "pref_t": None if gpt is None else c(gpt),
                      "weight_i": c(gwi)}


def _ref_loss(x, trip, nu, reg, mods, dt):
    leaves = {k: v.to(dt).clone().requires_grad_() for k, v in x.items()}
    P = {"v_gcn.preference": leaves["pref_v"], "t_gcn.preference": leaves["pref_t"], "weight_u": leaves["weight_u"],
         "weight_i": leaves["weight_i"]}
    terms = R.loss(P, {m: 0 for m in mods}, leaves["result"], torch.from_numpy(trip), nu, reg)
    # weight_u's own term is the mix kernel's: leave it out of the gradients compared here
    (terms[0] - reg * (leaves["weight_u"] ** 2).mean()).backward()
    return [float(t) for t in terms], {k: (None if v.grad is None else v.grad) for k, v in leaves.items()}


@pytest.mark.parametrize("mods", ["vt", "v", "t"])
@pytest.mark.parametrize("B", LOSS_BATCHES)
def test_loss_vs_restatement(cuda, B, mods):
    nu, ni, reg = 50, 40, 0.01
    trip = loss_triplets(np.random.default_rng(B + (B == 192)), nu, ni, B)  # (a seed its own assertions hold at)
    x = _loss_inputs(nu, ni, B)
    terms, grads = _run_loss(cuda, x, trip, nu, reg, mods)
    t64, g64 = _ref_loss(x, trip, nu, reg, mods, torch.float64)
    t32, g32 = _ref_loss(x, trip, nu, reg, mods, torch.float32)
    for j, name in enumerate(("total", "bpr", "reg")):
        check_vs_f32(name, terms[j], np.float64(t64[j]), t32[j])
    check_vs_f32("g_result", grads["result"], g64["result"], g32["result"])
    rows = np.unique(np.concatenate([trip[0], nu + trip[1], nu + trip[2]]))
    untouched = np.setdiff1d(np.arange(nu + ni), rows)
    assert untouched.size > 0 and not grads["result"][untouched].any()
    counts = np.bincount(trip[0], minlength=nu)
    for m in "vt":
        k = "pref_" + m
        if m not in mods:
            assert grads[k] is None
            continue
        check_vs_f32("g_" + k, grads[k], g64[k], g32[k])
        # the preference gradient carries the repeat counts: 2 reg / (B 64) count(u) pref[u]
        want = (2 * reg / (B * D)) * counts[:, None] * x[k].double().numpy()
        check_vs_f32("g_" + k + " (counts)", grads[k], want, want.astype(np.float32))
        assert not grads[k][counts == 0].any()
    check_vs_f32("g_weight_i", grads["weight_i"], g64["weight_i"], g32["weight_i"])
    terms2, grads2 = _run_loss(cuda, x, trip, nu, reg, mods)
    assert np.array_equal(terms.view(np.int32), terms2.view(np.int32))
    for k, v in grads.items():
        assert v is None or np.array_equal(v.view(np.int32), grads2[k].view(np.int32)), k


def test_loss_refuses_what_it_is_not_built_for(cuda):
    from rsx import dualgnn as M

    for B, d in ((65537, 64), (512, 32), (0, 64)):
        with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
            M.loss_workspace(B, d, cuda)
    nu, ni = 20, 10
    x = {k: v.to(cuda) for k, v in _loss_inputs(nu, ni, 1).items()}
    ws = M.loss_workspace(8, D, cuda)
    for B in (0, 65537):
        trip = torch.zeros(3, B, dtype=torch.int64, device=cuda)
        a = M.loss_args(x["result"], x["pref_v"], x["pref_t"], x["weight_u"], x["weight_i"], trip, nu, 0.01)
        with pytest.raises(RuntimeError):
            M.loss_fwd(a, ws)
    r32 = torch.zeros(nu + ni, 32, device=cuda)
    trip = torch.zeros(3, 8, dtype=torch.int64, device=cuda)
    a = M.loss_args(r32, x["pref_v"], x["pref_t"], x["weight_u"], x["weight_i"], trip, nu, 0.01)
    with pytest.raises(RuntimeError):
        M.loss_fwd(a, ws)


# ---------------------------------------------------------------------- model
def _write_graph(tmp_path, z):
    d = tmp_path / "data" / "baby"
    d.mkdir(parents=True, exist_ok=True)
    np.save(d / "user_graph_dict.npy", R.lists_of(z["ug_ptr"], z["ug_nbr"], z["ug_cnt"]), allow_pickle=True)


def _setup(tmp_path, extra=None, feats=None, graph_file=True):
    z = R.load("dualgnn_small.npz")
    write_dataset(tmp_path, *(feats if feats is not None else (z["v_feat"], z["t_feat"])))
    if graph_file:
        _write_graph(tmp_path, z)
    cfg = dict(is_multimodal_model=True, learning_rate=[0.001], reg_weight=[0.001])
    cfg.update(extra or {})
    return (z,) + loaders("DualGNN", tmp_path, cfg)


def _model(c_, train):
    return make_model("DualGNN", c_, train)


def flat2(a):
    return a.reshape(a.shape[0], -1) if a.ndim > 2 else a


def _strided(m, k):
    """The model as check_params sees it: every parameter at the fixture's row stride."""
    return types.SimpleNamespace(named_parameters=lambda: [(n, R.rows(flat2(p.detach()), k)) for n, p in m.named_parameters()])


def test_dualgnn_init_and_initial_evaluation(cuda, tmp_path):
    from rsx.trainer import Trainer

    z, c_, train, valid, _ = _setup(tmp_path)
    m = _model(c_, train)
    S = R.strides(z)
    named = dict(m.named_parameters())
    assert tuple(named) == R.names() and m.user_graph_source == "file"
    for n, p in named.items():
        assert np.array_equal(R.rows(flat2(c(p)), S["param"]).view(np.int32), z["init." + n].view(np.int32)), n
    assert np.array_equal(c(m.result)[::S["const"]].view(np.int32), z["const.result_embed"].view(np.int32))
    assert "result" not in m.state_dict() and not m.result.requires_grad and m.result_embed is m.result
    g = m.user_graph
    assert np.array_equal(g.ptr, z["ug_ptr"]) and np.array_equal(g.nbr, z["ug_nbr"]) and np.array_equal(g.cnt, z["ug_cnt"])
    # before any training the scores are those of the random table (dualgnn.py:129, 199-205)
    check_eval(Trainer(c_, m), m, z, (("valid", valid),), tag_prefix="init_")
    m.pre_epoch_processing()
    assert np.array_equal(c(m.epoch_idx), z["epoch0_idx"].astype(np.int32))
    assert np.array_equal(c(m.epoch_W).view(np.int32), z["epoch0_W"].view(np.int32))


def test_dualgnn_first_two_steps(cuda, tmp_path):
    z, c_, train, *_ = _setup(tmp_path)
    z0 = R.load("dualgnn_step0_small.npz")
    S = R.strides(z0)
    m = _model(c_, train)
    m.train()
    m.pre_epoch_processing()
    lr = c_["learning_rate"]
    live = [p for n, p in m.named_parameters() if n not in R.UNUSED]
    opt = torch.optim.Adam(live, lr=lr)
    names = R.trained()
    dgs, grefs = {n: [] for n in names}, {n: [] for n in names}
    for step in range(2):
        pre = f"step{step}_"
        opt.zero_grad()
        trip = dev(z0[pre + "triplets"].astype(np.int64), cuda)
        if step == 0:
            with torch.no_grad():
                xs = {k: m._modal(g, f) for k, g, f in m._mods()}
            for k in "vt":
                np.testing.assert_allclose(c(xs[k])[::S["rep"]], z0["step0_x_hat_" + k], rtol=1e-5, atol=1e-6)
        rep = m.forward().clone()  # without autograd: the same kernels, the same bits, `result` itself
        assert not rep.requires_grad and m.forward().data_ptr() == m.result.data_ptr()
        m.result.zero_()
        loss = m.calculate_loss(trip)
        loss.backward()
        assert torch.equal(rep, m.result)
        terms = c(m.last_terms)
        for j, name in enumerate(("loss", "bpr", "reg")):
            want = float(z0[pre + name])
            print(f"step {step} {name} {terms[j]:.8f} vs reference {want:.8f}")
            assert abs(terms[j] - want) <= 1e-5 * abs(want), (step, name)
        assert loss.item() == terms[0]
        if step == 0:
            np.testing.assert_allclose(c(m.last_user_rep)[::S["rep"]], z0["step0_user_rep"], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(c(m.result)[::S["rep"]], z0["step0_result"], rtol=1e-5, atol=1e-6)
        mine = {}
        for n, p in m.named_parameters():
            if n in R.UNUSED:  # nothing reads them: no gradient at all, not a zero one
                assert p.grad is None, n
            else:
                mine[n] = flat2(c(p.grad)).copy()
        if step == 0:
            for n in names:
                w = z0[pre + "grad." + n]
                scale = max(float(np.abs(w).max()), 1e-12)
                np.testing.assert_allclose(R.rows(mine[n], S["grad"]), w, rtol=1e-3, atol=1e-5 * scale, err_msg=n)
        opt.step()
        for n, p in m.named_parameters():
            got, want = R.rows(flat2(c(p)), S["param"]), z0[pre + "param." + n]
            if n in R.UNUSED:
                assert np.array_equal(got, want), n
                continue
            gref = z0[pre + "grad." + n]
            if gref.ndim == 2 and p.shape[0] >= 64:
                gref = gref[::S["param"] // S["grad"]]
            gmine = R.rows(mine[n], S["param"])
            grefs[n].append(gref.astype(np.float64))
            dgs[n].append(gmine.astype(np.float64) - gref)
            # 1e-5 of scale plus what Adam turns the gradient differences into (grcn_ref.adam_tolerance)
            scale = float(np.abs(want).max())
            extra = R.adam_tolerance(dgs[n], grefs[n], lr)
            err = np.abs(got - want)
            print(f"  step {step} {n}: err {err.max():.3e}, scale {scale:.3e}")
            assert np.all(err <= 1e-5 * scale + extra + 2e-6 * (step == 0)), n


def _run(tmp_path, tag, graph, epochs=2):
    from rsx.trainer import Trainer

    _, c_, train, *_ = _setup(tmp_path / tag, dict(rsx_graph_step=graph))
    m = _model(c_, train)
    t = Trainer(c_, m)
    seen = []
    losses = train_epochs(t, m, train, epochs, after_pre_epoch=lambda e: seen.append((m.epoch_idx.clone(), m.epoch_W.clone())))
    return m, losses, t, seen


def test_dualgnn_captured_run_equals_eager_across_an_epoch_boundary(cuda, tmp_path):
    z = R.load("dualgnn_small.npz")
    a, la, ta, sa = _run(tmp_path, "graph", True)
    b, lb, tb, sb = _run(tmp_path, "eager", False)
    assert ta._graph is not None and ta._graph.replays >= 1 and tb._graph is None
    assert_same_run(a, b, la, lb)
    assert torch.equal(a.result, b.result)
    for e in range(2):  # both runs trained on the reference's lists of either epoch
        for s in (sa, sb):
            assert np.array_equal(c(s[e][0]), z[f"epoch{e}_idx"].astype(np.int32))
            assert np.array_equal(c(s[e][1]).view(np.int32), z[f"epoch{e}_W"].view(np.int32))


def test_dualgnn_trainer_vs_reference(cuda, tmp_path):
    from rsx.trainer import Trainer

    z, c_, train, valid, test = _setup(tmp_path)
    m = _model(c_, train)
    t = Trainer(c_, m)
    assert not t.fused and type(t.optimizer).__name__ == "RsxAdam"
    S = R.strides(z)
    snaps = {}

    def snap(e):  # copies: the parameters move on
        snaps[e] = [(n, p.cpu().clone()) for n, p in _strided(m, S["epoch" if e == 0 else "last"]).named_parameters()]

    losses = train_epochs(t, m, train, 2, after_epoch=snap)
    print(f"epoch losses {losses} vs reference {z['epoch_losses']}")
    for e in range(2):
        check_params(types.SimpleNamespace(named_parameters=lambda e=e: snaps[e]), z, f"epoch{e}_param.", 5e-5)
    for n in R.UNUSED:  # skipped by the optimiser, not updated with zeros
        p = dict(m.named_parameters())[n]
        assert p.grad is None and np.array_equal(R.rows(flat2(c(p)), S["param"]), z["init." + n]), n
    # `result` is the last training forward's, one optimiser step stale
    check_eval(t, m, z, (("valid", valid), ("test", test)))


@pytest.mark.parametrize("only", ["v", "t"])
def test_dualgnn_one_modality_vs_restatement(cuda, tmp_path, only):
    z = R.load("dualgnn_small.npz")
    z0 = R.load("dualgnn_step0_small.npz")
    feats = (z["v_feat"], None) if only == "v" else (None, z["t_feat"])
    _, c_, train, *_ = _setup(tmp_path, feats=feats)
    m = _model(c_, train)
    assert tuple(n for n, _ in m.named_parameters()) == R.names((only,))
    m.train()
    m.pre_epoch_processing()
    trip = z0["step0_triplets"].astype(np.int64)
    loss = m.calculate_loss(dev(trip, cuda))
    loss.backward()
    nu, ni = int(z["n_users"]), int(z["n_items"])
    idx, W = c(m.epoch_idx).astype(np.int64), m.epoch_W.cpu()
    res = {}
    for dtype in (torch.float64, torch.float32):
        P = R.cast({n: p.detach().cpu() for n, p in m.named_parameters()}, dtype)
        A = R.sym_operator(z["train_u"].astype(np.int64), z["train_i"].astype(np.int64), nu, ni, dtype)
        f = {only: torch.from_numpy(z[only + "_feat"]).to(dtype)}
        res[dtype] = R.step(P, f, A, idx, W.to(dtype), torch.from_numpy(trip), nu, 0.001)
    (rep64, u64, _, t64, g64), (rep32, u32, _, t32, g32) = res[torch.float64], res[torch.float32]
    terms = c(m.last_terms)
    for j, name in enumerate(("loss", "bpr", "reg")):
        assert abs(terms[j] - float(t64[j])) <= 1e-5 * abs(float(t64[j])), name
    check_vs_f32("user_rep", c(m.last_user_rep), u64, u32)
    check_vs_f32("result", c(m.result), rep64, rep32)
    for n, p in m.named_parameters():
        if n in R.UNUSED:
            assert p.grad is None and g64[n] is None, n
        else:
            check_vs_f32(n, c(p.grad), g64[n], g32[n])


def test_dualgnn_builds_its_own_graph_without_the_file(cuda, tmp_path):
    from rsx.dualgnn import CACHE_NAME
    from rsx.trainer import Trainer

    z, c_, train, *_ = _setup(tmp_path, graph_file=False)
    m = _model(c_, train)
    assert m.user_graph_source == "built"
    assert os.path.isfile(tmp_path / "data" / "baby" / CACHE_NAME)
    assert np.array_equal(np.diff(m.user_graph.ptr), np.diff(z["ug_ptr"]))  # the generator's lengths; ties may order otherwise
    losses = train_epochs(Trainer(c_, m), m, train, 1)
    assert np.isfinite(losses[0]) and torch.isfinite(m.result).all()


@pytest.mark.parametrize("what", ["embedding_size", "no_features", "width", "aggr_mode"])
def test_dualgnn_unsupported_configurations_raise(cuda, tmp_path, what):
    z = R.load("dualgnn_small.npz")
    extra, feats = {}, None
    if what == "embedding_size":
        extra = dict(embedding_size=128)
    elif what == "no_features":
        feats = (None, None)
    elif what == "width":
        feats = (z["v_feat"][:, :6], z["t_feat"])
    else:
        extra = dict(aggr_mode=["mean"])
    _, c_, train, *_ = _setup(tmp_path, extra, feats)
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        _model(c_, train)


def test_dualgnn_quick_start(cuda, tmp_path):
    """`main.py -m DualGNN -d <dataset>`'s path: trains an epoch and evaluates on a dataset
    directory with the .inter file, the two feature files and the user graph file."""
    z = R.load("dualgnn_small.npz")
    _write_graph(tmp_path, z)
    res = quick_start_case("DualGNN", tmp_path, z["v_feat"], z["t_feat"],
                           {"epochs": 1, "learning_rate": [0.001], "reg_weight": [0.001]})
    assert len(res) == 1 and "recall@20" in res[0][1]
    assert all(np.isfinite(v) for v in res[0][1].values())
