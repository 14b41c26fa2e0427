"""DRAGON on the GPU: the kernels of csrc/dragon.hip (rsx.dragon's wrappers) against the float64
restatement (tests/dragon_ref.py), and the model (rsx.dragon.DRAGON) against the reference's own
run (tests/golden/dragon_step0_small.npz, dragon_small.npz).

Kernel bound: helpers.check_vs_f32 — 1e-4 of the tensor's scale, or 4x the error the float32
torch composition of the same ops (on the CPU) makes against the same float64 values, whichever
is larger.  Every sum is in a fixed order (no float atomics): two runs are bit-equal, and a run
with captured graph steps equals the eager one bit for bit.

Model bounds are those of tests/test_gpu_dualgnn.py: 1e-5 relative on the loss terms, rtol 1e-3
and atol 1e-5 of the scale on step-0 gradients, grcn_ref.adam_tolerance on the parameters after a
step.  The parameters after an epoch: max(5e-5 of the scale, 4 x epoch{e}_f32_dist.<name>), the
fixture's record of how far the reference's own float32 run strays from the float64 restatement
trained on the same batches (the factor 4 is check_vs_f32's)."""
import os
import types

import numpy as np
import pytest
import torch

import dragon_ref as R
from helpers import (LOSS_BATCHES, assert_same_run, check_eval, check_vs_f32, dev, loaders, loss_triplets, make_model,
                     quick_start_case, train_epochs, write_dataset)
from test_gpu_dualgnn import _lists, _randn, _ugraph_ref

pytestmark = pytest.mark.gpu
c = lambda t: t.detach().cpu().numpy()  # noqa: E731
DM, DC = 64, 128
FEAT_TABLE = {"image_embedding.weight": "v_feat", "text_embedding.weight": "t_feat"}


# ----------------------------------------------------------------------- cat
@pytest.mark.parametrize("ni", [1, 33])
@pytest.mark.parametrize("nu", [1, 7, 8, 9, 130])
def test_cat_fwd_bwd_vs_restatement(cuda, nu, ni):
    """8 rows a block: nu on either side of a block's edge, the user / item boundary inside a block."""
    from rsx import dragon as M

    n = nu + ni
    seed = nu * 1000 + ni * 10
    xv, xt = _randn(seed, n, DM), _randn(seed + 1, n, DM)
    w = torch.softmax(_randn(seed + 2, nu, 2, 1), dim=1)
    gu, gi = _randn(seed + 3, nu, DC), _randn(seed + 4, ni, DC)
    user_rep, item_rep = M.cat_fwd(xv.to(cuda), xt.to(cuda), w.to(cuda), nu)
    assert user_rep.shape == (nu, DC) and item_rep.shape == (ni, DC)
    res = {}
    for dt in (torch.float64, torch.float32):
        a, b, ww = (t.to(dt).clone().requires_grad_() for t in (xv, xt, w))
        u, i = R.cat(a, b, ww, nu)
        ((u * gu.to(dt)).sum() + (i * gi.to(dt)).sum()).backward()
        res[dt] = (u.detach(), i.detach(), a.grad, b.grad, ww.grad)
    r64, r32 = res[torch.float64], res[torch.float32]
    check_vs_f32("user_rep", c(user_rep), r64[0], r32[0])
    assert np.array_equal(c(item_rep), torch.cat((xv[nu:], xt[nu:]), dim=1).numpy())  # the item rows are copies
    g_v, g_t, g_w = M.cat_bwd(gu.to(cuda), gi.to(cuda), xv.to(cuda), xt.to(cuda), w.to(cuda), nu)
    check_vs_f32("g_v", c(g_v), r64[2], r32[2])
    check_vs_f32("g_t", c(g_t), r64[3], r32[3])
    assert g_w.shape == (nu, 2, 1)
    check_vs_f32("g_weight_u", c(g_w), r64[4], r32[4])
    hand = R.cat_backward(gu.double(), gi.double(), xv.double(), xt.double(), w.double(), nu)
    check_vs_f32("g_weight_u (by hand)", c(g_w), hand[2], r32[4])
    u2, i2 = M.cat_fwd(xv.to(cuda), xt.to(cuda), w.to(cuda), nu)
    assert torch.equal(u2, user_rep) and torch.equal(i2, item_rep)
    g2 = M.cat_bwd(gu.to(cuda), gi.to(cuda), xv.to(cuda), xt.to(cuda), w.to(cuda), nu)
    assert all(torch.equal(a, b) for a, b in zip((g_v, g_t, g_w), g2))


def test_cat_refusals(cuda):
    from rsx import dragon as M

    xv, xt, w = _randn(1, 9, DM).to(cuda), _randn(2, 9, DM).to(cuda), torch.ones(5, 2, 1, device=cuda)
    with pytest.raises(RuntimeError):  # a 32-wide table
        M.cat_fwd(xv[:, :32].contiguous(), xt[:, :32].contiguous(), w, 5)
    with pytest.raises(RuntimeError):  # weight_u of another user count
        M.cat_fwd(xv, xt, w, 4)
    with pytest.raises(RuntimeError):  # a 64-wide gradient
        M.cat_bwd(xv[:5].contiguous(), xt[5:].contiguous(), xv, xt, w, 5)


# ---------------------------------------------------------------- user graph
UGRAPH_CASES = [(DC, nu) for nu in (1, 7, 8, 9, 130)] + [(DM, nu) for nu in (1, 15, 16, 17)]


@pytest.mark.parametrize("k", [1, 32, 33, 40, 64])
@pytest.mark.parametrize("d,nu", UGRAPH_CASES)
def test_ugraph_fwd_vs_restatement(cuda, d, nu, k):
    from rsx import dragon as M

    x = _randn(nu * 100 + k + d, nu, d)
    idx, W = _lists(nu, k, nu + k)
    out = torch.full((nu + 3, d), 7.0, device=cuda)  # rows past nu stay as they are
    M.ugraph_fwd(x.to(cuda), dev(idx, cuda), dev(W, cuda), out=out)
    check_vs_f32("out", c(out[:nu]), _ugraph_ref(x.double(), idx, W), _ugraph_ref(x, idx, W))
    assert torch.equal(out[nu:], torch.full((3, d), 7.0, device=cuda))
    if nu > 3:
        assert np.array_equal(c(out[0]), x[0].numpy())  # zero weights: the row itself
    again = M.ugraph_fwd(x.to(cuda), dev(idx, cuda), dev(W, cuda))
    assert torch.equal(again, out[:nu])


@pytest.mark.parametrize("nu,k", [(17, 40), (130, 64)])
def test_ugraph_fwd_at_64_is_dualgnns(cuda, nu, k):
    """The template at D = 64 gives rsx_dualgnn_ugraph_fwd's bits."""
    from rsx import dragon as M
    from rsx import dualgnn as G

    x = _randn(nu + k, nu, DM).to(cuda)
    idx, W = _lists(nu, k, nu + k)
    assert torch.equal(M.ugraph_fwd(x, dev(idx, cuda), dev(W, cuda)), G.ugraph_fwd(x, dev(idx, cuda), dev(W, cuda)))


def test_ugraph_fwd_refusals(cuda):
    from rsx import dragon as M

    x = _randn(1, 5, DC).to(cuda)
    with pytest.raises(RuntimeError, match="rsx_dragon_ugraph_fwd failed"):  # k = 0
        M.ugraph_fwd(x, torch.zeros(5, 0, dtype=torch.int32, device=cuda), torch.zeros(5, 0, device=cuda))
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED|1002"):  # k = 65
        M.ugraph_fwd(x, torch.zeros(5, 65, dtype=torch.int32, device=cuda), torch.zeros(5, 65, device=cuda))
    x32 = _randn(1, 5, 32).to(cuda)
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED|1002"):
        M.ugraph_fwd(x32, torch.zeros(5, 4, dtype=torch.int32, device=cuda), torch.zeros(5, 4, device=cuda))
    with pytest.raises(RuntimeError):
        M.ugraph_fwd(x, torch.zeros(5, 4, dtype=torch.int32, device=cuda), torch.zeros(5, 4, device=cuda), out=x)


def test_ugraph_backward_on_the_spmm_at_128(cuda):
    """g_user_rep = g + P^T g through the transposed lists, 128 wide: 120 of 130 users all name
    user 7 (a hub row past chunk 32, several chunks), user 9 is named by nobody (an empty row)."""
    from rsx import dragon as M
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
    g = _randn(13, nu + ni, DC)
    got = M.ugraph_bwd(PT, g.to(cuda), nu)
    assert got.shape == (nu, DC)
    Wt = torch.from_numpy(W)
    check_vs_f32("g_user_rep", c(got), R.ugraph_backward(g[:nu].double(), idx, Wt.double()), R.ugraph_backward(g[:nu], idx, Wt))
    assert np.array_equal(c(got[9]), g[9].numpy())
    # the same gradient by autograd through the restatement's forward
    x = _randn(14, nu, DC).double().requires_grad_()
    (R.ugraph(x, idx, Wt.double()) * g[:nu].double()).sum().backward()
    check_vs_f32("g_user_rep (autograd)", c(got), x.grad, R.ugraph_backward(g[:nu], idx, Wt))
    assert torch.equal(M.ugraph_bwd(PT, g.to(cuda), nu), got)


# ---------------------------------------------------------------- item graph
@pytest.mark.parametrize("layers", [0, 1, 2])
def test_item_graph_fwd_bwd_at_128(cuda, layers):
    """x + A^L x written into the item rows of a taller table, and g + (A^T)^L g, on a 40-item graph
    whose pattern is not symmetric."""
    from rsx import dragon as M
    from rsx.blocks import _DevGraph

    ni, nu, k = 40, 5, 5
    rng = np.random.default_rng(21)
    rows = np.repeat(np.arange(ni), k).astype(np.int64)
    cols = np.concatenate([rng.permutation(ni)[:k] for _ in range(ni)]).astype(np.int64)
    vals = (rng.random(ni * k) * 0.5 + 0.1).astype(np.float32)
    pairs = set(zip(rows.tolist(), cols.tolist()))
    assert any((b, a) not in pairs for a, b in pairs)
    A32 = torch.zeros(ni, ni)
    A32[torch.from_numpy(rows), torch.from_numpy(cols)] = torch.from_numpy(vals)
    A64 = A32.double()
    G = _DevGraph(rows, cols, vals, ni, ni, cuda, 64)
    x, g = _randn(22, ni, DC), _randn(23, ni, DC)
    table = torch.full((nu + ni, DC), 7.0, device=cuda)
    M.graph_residual(G.A, x.to(cuda), layers, out=table[nu:])
    check_vs_f32("x + A^L x", c(table[nu:]), R.item_prop(x.double(), A64, layers), R.item_prop(x, A32, layers))
    assert torch.equal(table[:nu], torch.full((nu, DC), 7.0, device=cuda))
    got = M.graph_residual(G.AT, g.to(cuda), layers)
    check_vs_f32("g + (A^T)^L g", c(got), R.item_prop(g.double(), A64.t(), layers), R.item_prop(g, A32.t(), layers))
    xa = x.double().requires_grad_()
    (R.item_prop(xa, A64, layers) * g.double()).sum().backward()
    check_vs_f32("g + (A^T)^L g (autograd)", c(got), xa.grad, R.item_prop(g, A32.t(), layers))
    assert torch.equal(M.graph_residual(G.AT, g.to(cuda), layers), got)
    if layers == 0:
        assert np.array_equal(c(got), (g + g).numpy())


# ---------------------------------------------------------------------- loss
def _loss_inputs(nu, ni, d, seed):
    return dict(result=_randn(seed, nu + ni, d) * 0.3, pref_v=_randn(seed + 1, nu, DM) * 0.2, pref_t=_randn(seed + 2, nu, DM) * 0.2,
                weight_u=torch.softmax(_randn(seed + 3, nu, 2, 1), dim=1))


def _run_loss(cuda, x, trip, nu, reg, mods):
    from rsx import dragon as M

    t = {k: v.to(cuda) for k, v in x.items()}
    pv, pt = (t["pref_v"] if "v" in mods else None), (t["pref_t"] if "t" in mods else None)
    ws = M.loss_workspace(trip.shape[1], x["result"].shape[1], cuda)
    trip_dev = dev(trip, cuda)  # held to the end: the argument struct keeps addresses, not tensors
    a = M.loss_args(t["result"], pv, pt, t["weight_u"], trip_dev, nu, reg)
    terms = M.loss_fwd(a, ws)
    g, gpv, gpt, gwu = M.loss_bwd(a, torch.ones(1, device=cuda), ws, pv, pt, t["weight_u"])
    return c(terms), {"result": c(g), "pref_v": None if gpv is None else c(gpv), "pref_t": None if gpt is None else c(gpt),
                      "weight_u": c(gwu)}


def _ref_loss(x, trip, nu, reg, mods, dt):
    leaves = {k: v.to(dt).clone().requires_grad_() for k, v in x.items()}
    P = {"v_gcn.preference": leaves["pref_v"], "t_gcn.preference": leaves["pref_t"], "weight_u": leaves["weight_u"]}
    terms = R.loss(P, {m: 0 for m in mods}, leaves["result"], torch.from_numpy(trip), nu, reg)
    terms[0].backward()
    return [float(t) for t in terms], {k: (None if v.grad is None else v.grad) for k, v in leaves.items()}


@pytest.mark.parametrize("d,mods", [(DC, "vt"), (DC, "v"), (DC, "t"), (DM, "v"), (DM, "t")])
@pytest.mark.parametrize("B", LOSS_BATCHES)
def test_loss_vs_restatement(cuda, B, d, mods):
    nu, ni, reg = 50, 40, 0.01
    trip = loss_triplets(np.random.default_rng(B + (B == 192)), nu, ni, B)  # (a seed its own assertions hold at)
    x = _loss_inputs(nu, ni, d, B + d)
    terms, grads = _run_loss(cuda, x, trip, nu, reg, mods)
    t64, g64 = _ref_loss(x, trip, nu, reg, mods, torch.float64)
    t32, g32 = _ref_loss(x, trip, nu, reg, mods, torch.float32)
    for j, name in enumerate(("total", "bpr", "reg")):
        check_vs_f32(name, terms[j], np.float64(t64[j]), t32[j])
    assert grads["result"].shape == (nu + ni, d)
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
        assert grads[k].shape == (nu, DM)
        check_vs_f32("g_" + k, grads[k], g64[k], g32[k])
        # the preference gradient carries the repeat counts: 2 reg / (B 64) count(u) pref[u]
        want = (2 * reg / (B * DM)) * counts[:, None] * x[k].double().numpy()
        check_vs_f32("g_" + k + " (counts)", grads[k], want, want.astype(np.float32))
        assert not grads[k][counts == 0].any()
    # the loss owns weight_u's regulariser: 2 reg / (2 nu) weight_u, and there is no weight_i anywhere
    check_vs_f32("g_weight_u", grads["weight_u"], g64["weight_u"], g32["weight_u"])
    want = 2 * reg / (2 * nu) * x["weight_u"].double().numpy()
    check_vs_f32("g_weight_u (closed form)", grads["weight_u"], want, want.astype(np.float32))
    terms2, grads2 = _run_loss(cuda, x, trip, nu, reg, mods)
    assert np.array_equal(terms.view(np.int32), terms2.view(np.int32))
    for k, v in grads.items():
        assert v is None or np.array_equal(v.view(np.int32), grads2[k].view(np.int32)), k


def test_loss_refuses_what_it_is_not_built_for(cuda):
    from rsx import dragon as M

    for B, d in ((65537, 64), (65537, 128), (512, 32), (0, 64), (0, 128)):
        with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
            M.loss_workspace(B, d, cuda)
    nu, ni = 20, 10
    x = {k: v.to(cuda) for k, v in _loss_inputs(nu, ni, DC, 1).items()}
    ws = M.loss_workspace(8, DC, cuda)
    for B in (0, 65537):
        trip = torch.zeros(3, B, dtype=torch.int64, device=cuda)
        a = M.loss_args(x["result"], x["pref_v"], x["pref_t"], x["weight_u"], trip, nu, 0.01)
        with pytest.raises(RuntimeError):
            M.loss_fwd(a, ws)
    r32 = torch.zeros(nu + ni, 32, device=cuda)
    trip = torch.zeros(3, 8, dtype=torch.int64, device=cuda)
    a = M.loss_args(r32, x["pref_v"], x["pref_t"], x["weight_u"], trip, nu, 0.01)
    with pytest.raises(RuntimeError):
        M.loss_fwd(a, ws)
    # 64 wide is one modality: both preference tables are refused
    r64 = torch.zeros(nu + ni, DM, device=cuda)
    a = M.loss_args(r64, x["pref_v"], x["pref_t"], x["weight_u"], trip, nu, 0.01)
    with pytest.raises(RuntimeError):
        M.loss_fwd(a, ws)
    with pytest.raises(RuntimeError):  # a workspace sized for a smaller batch
        trip = torch.zeros(3, 64, dtype=torch.int64, device=cuda)
        M.loss_fwd(M.loss_args(x["result"], x["pref_v"], x["pref_t"], x["weight_u"], trip, nu, 0.01), ws)


# ---------------------------------------------------------------------- model
def _write_graph(tmp_path, z):
    d = tmp_path / "data" / "baby"
    d.mkdir(parents=True, exist_ok=True)
    np.save(d / "user_graph_dict.npy", R.lists_of(z["ug_ptr"], z["ug_nbr"], z["ug_cnt"]), allow_pickle=True)


def _write_mm_adj(tmp_path, z, k=10):
    """The reference's cache file (dragon.py:61, :83: torch.save of the sparse mm_adj), from the fixture's COO."""
    d = tmp_path / "data" / "baby"
    d.mkdir(parents=True, exist_ok=True)
    ni = int(z["n_items"])
    idx = torch.from_numpy(np.stack([z["mm_adj_row"], z["mm_adj_col"]]).astype(np.int64))
    torch.save(torch.sparse_coo_tensor(idx, torch.from_numpy(z["mm_adj_val"]), (ni, ni)), d / f"mm_adj_{k}.pt")


def _setup(tmp_path, extra=None, feats=None, graph_file=True, mm_file=False):
    z = R.load("dragon_small.npz")
    write_dataset(tmp_path, *(feats if feats is not None else (z["v_feat"], z["t_feat"])))
    if graph_file:
        _write_graph(tmp_path, z)
    if mm_file:
        _write_mm_adj(tmp_path, z)
    # the device kNN, as a run without rsx_sampler: host takes it
    cfg = dict(is_multimodal_model=True, learning_rate=[0.001], reg_weight=[0.001], rsx_knn="device")
    cfg.update(extra or {})
    return (z,) + loaders("DRAGON", tmp_path, cfg)


def _model(c_, train):
    return make_model("DRAGON", c_, train)


def flat2(a):
    return a.reshape(a.shape[0], -1) if a.ndim > 2 else a


def _initial(z, n, stride):
    return R.rows(z[FEAT_TABLE[n]], stride) if n in FEAT_TABLE else z["init." + n]


def _mm_coo(m):
    """(rows, cols, vals) of the model's item graph, in coalesced order."""
    A = m.mm_adj.A
    rp, col, val = c(A.rowptr).astype(np.int64), c(A.col).astype(np.int64), c(A.val)
    return np.repeat(np.arange(rp.size - 1), np.diff(rp)), col, val


def test_dragon_init_and_initial_evaluation(cuda, tmp_path):
    from rsx.trainer import Trainer

    z, c_, train, valid, _ = _setup(tmp_path)
    m = _model(c_, train)
    S = R.strides(z)
    named = dict(m.named_parameters())
    assert tuple(named) == R.names() and m.user_graph_source == "file" and m.mm_adj_source == "built"
    for n, p in named.items():  # UNUSED included
        assert np.array_equal(R.rows(flat2(c(p)), S["param"]).view(np.int32), _initial(z, n, S["param"]).view(np.int32)), n
    assert m.result.shape == (600, 64)
    assert np.array_equal(c(m.result)[::S["const"]].view(np.int32), z["const.result_embed"].view(np.int32))
    assert "result" not in m.state_dict() and not m.result.requires_grad and m.result_embed is m.result
    g = m.user_graph
    assert np.array_equal(g.ptr, z["ug_ptr"]) and np.array_equal(g.nbr, z["ug_nbr"]) and np.array_equal(g.cnt, z["ug_cnt"])
    # the device kNN names the reference's neighbours (the capture's margin): the same mm_adj
    r, col, val = _mm_coo(m)
    assert np.array_equal(r, z["mm_adj_row"].astype(np.int64)) and np.array_equal(col, z["mm_adj_col"].astype(np.int64))
    assert np.array_equal(val.view(np.int32), z["mm_adj_val"].view(np.int32))
    # before any training the scores are those of the random table (dragon.py:155-156, 279-285)
    check_eval(Trainer(c_, m), m, z, (("valid", valid),), tag_prefix="init_")
    m.pre_epoch_processing()
    assert np.array_equal(c(m.epoch_idx), z["epoch0_idx"].astype(np.int32))
    assert np.array_equal(c(m.epoch_W).view(np.int32), z["epoch0_W"].view(np.int32))


def test_dragon_first_two_steps(cuda, tmp_path):
    z, c_, train, *_ = _setup(tmp_path)
    z0 = R.load("dragon_step0_small.npz")
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
        assert rep.shape == (600, DC) and not rep.requires_grad and m.forward().data_ptr() == m.result.data_ptr()
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
            got = R.rows(flat2(c(p)), S["param"])
            if n in R.UNUSED:  # the fixture keeps their initial value: they never move
                assert np.array_equal(got, _initial(z, n, S["param"])), n
                continue
            want = z0[pre + "param." + n]
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


def test_dragon_captured_run_equals_eager_across_an_epoch_boundary(cuda, tmp_path):
    z = R.load("dragon_small.npz")
    a, la, ta, sa = _run(tmp_path, "graph", True)
    b, lb, tb, sb = _run(tmp_path, "eager", False)
    assert ta._graph is not None and ta._graph.replays >= 1 and tb._graph is None
    assert_same_run(a, b, la, lb)
    assert a.result.shape == (600, DC) and torch.equal(a.result, b.result)
    for e in range(2):  # both runs trained on the reference's lists of either epoch
        for s in (sa, sb):
            assert np.array_equal(c(s[e][0]), z[f"epoch{e}_idx"].astype(np.int32))
            assert np.array_equal(c(s[e][1]).view(np.int32), z[f"epoch{e}_W"].view(np.int32))


def test_dragon_trainer_vs_reference(cuda, tmp_path):
    from rsx.trainer import Trainer

    z, c_, train, valid, test = _setup(tmp_path)
    m = _model(c_, train)
    t = Trainer(c_, m)
    assert not t.fused and type(t.optimizer).__name__ == "RsxAdam"
    S = R.strides(z)
    snaps = {}

    def snap(e):  # copies: the parameters move on
        k = S["epoch" if e == 0 else "last"]
        snaps[e] = {n: R.rows(flat2(c(p)), k).copy() for n, p in m.named_parameters() if n not in R.UNUSED}

    losses = train_epochs(t, m, train, 2, after_epoch=snap)
    print(f"epoch losses {losses} vs reference {z['epoch_losses']}")
    for e in range(2):
        for n, got in snaps[e].items():
            w = z[f"epoch{e}_param.{n}"]
            scale = float(np.abs(w).max())
            dist = float(z[f"epoch{e}_f32_dist.{n}"])
            bound = max(5e-5 * scale, 4 * dist)
            err = float(np.abs(got - w).max())
            print(f"  epoch {e} {n}: err {err:.3e}, scale {scale:.3e}, reference f32 vs f64 {dist:.3e}, bound {bound:.3e}")
            assert err <= bound, (e, n)
    for n in R.UNUSED:  # skipped by the optimiser, not updated with zeros
        p = dict(m.named_parameters())[n]
        assert p.grad is None and np.array_equal(R.rows(flat2(c(p)), S["param"]), _initial(z, n, S["param"])), n
    # `result` is the last training forward's, one optimiser step stale
    check_eval(t, m, z, (("valid", valid), ("test", test)))


@pytest.mark.parametrize("only", ["v", "t"])
def test_dragon_one_modality_vs_restatement(cuda, tmp_path, only):
    from rsx.freedom import freedom_item_graph

    z = R.load("dragon_small.npz")
    z0 = R.load("dragon_step0_small.npz")
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
    assert m.result.shape == (nu + ni, DM)
    # one modality: mm_adj is that modality's graph alone (dragon.py:73-78)
    tf = lambda a: None if a is None else torch.from_numpy(a)  # noqa: E731
    r, col, val = freedom_item_graph(tf(feats[0]), tf(feats[1]), 10, 0.1, "host")
    mr, mc, mv = _mm_coo(m)
    assert np.array_equal(mr, r) and np.array_equal(mc, col) and np.array_equal(mv.view(np.int32), val.view(np.int32))
    idx, W = c(m.epoch_idx).astype(np.int64), m.epoch_W.cpu()
    res = {}
    for dtype in (torch.float64, torch.float32):
        P = R.cast({n: p.detach().cpu() for n, p in m.named_parameters()}, dtype)
        A = R.sym_operator(z["train_u"].astype(np.int64), z["train_i"].astype(np.int64), nu, ni, dtype)
        mm = R.mm_adj_dense(dict(mm_adj_row=r, mm_adj_col=col, mm_adj_val=val), ni, dtype)
        f = {only: torch.from_numpy(z[only + "_feat"]).to(dtype)}
        res[dtype] = R.step(P, f, A, mm, 1, idx, W.to(dtype), torch.from_numpy(trip), nu, 0.001)
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


def test_dragon_builds_its_graphs_without_the_files(cuda, tmp_path):
    from rsx.dualgnn import CACHE_NAME
    from rsx.trainer import Trainer

    z, c_, train, *_ = _setup(tmp_path, graph_file=False)
    m = _model(c_, train)
    assert m.user_graph_source == "built" and m.mm_adj_source == "built"
    assert os.path.isfile(tmp_path / "data" / "baby" / CACHE_NAME)
    assert not [f for f in os.listdir(tmp_path / "data" / "baby") if f.startswith("mm_adj_")]
    assert np.array_equal(np.diff(m.user_graph.ptr), np.diff(z["ug_ptr"]))  # the generator's lengths; ties may order otherwise
    losses = train_epochs(Trainer(c_, m), m, train, 1)
    assert np.isfinite(losses[0]) and torch.isfinite(m.result).all() and m.result.shape == (600, DC)


def test_dragon_reads_the_references_mm_adj_file(cuda, tmp_path):
    """A `mm_adj_{knn_k}.pt` the reference wrote is the graph the run trains on: here the fixture's
    with one row's values doubled, which no build from the features gives."""
    from rsx.trainer import Trainer

    z = dict(R.load("dragon_small.npz"))
    z["mm_adj_val"] = z["mm_adj_val"].copy()
    z["mm_adj_val"][z["mm_adj_row"] == 3] *= 2.0
    write_dataset(tmp_path, z["v_feat"], z["t_feat"])
    _write_graph(tmp_path, z)
    _write_mm_adj(tmp_path, z)
    c_, train, *_ = loaders("DRAGON", tmp_path, dict(is_multimodal_model=True, learning_rate=[0.001], reg_weight=[0.001]))
    m = _model(c_, train)
    assert m.mm_adj_source == "file" and m.user_graph_source == "file"
    r, col, val = _mm_coo(m)
    assert np.array_equal(r, z["mm_adj_row"].astype(np.int64)) and np.array_equal(col, z["mm_adj_col"].astype(np.int64))
    assert np.array_equal(val.view(np.int32), z["mm_adj_val"].view(np.int32))
    losses = train_epochs(Trainer(c_, m), m, train, 1)
    assert np.isfinite(losses[0]) and torch.isfinite(m.result).all()


def test_dragon_zero_item_layers_double_the_item_rows(cuda, tmp_path):
    _, c_, train, *_ = _setup(tmp_path, dict(n_mm_layers=0))
    m = _model(c_, train)
    m.pre_epoch_processing()
    with torch.no_grad():
        xs = {k: m._modal(g, f) for k, g, f in m._mods()}
    rep = m.forward()
    assert torch.equal(rep[400:], 2 * torch.cat((xs["v"][400:], xs["t"][400:]), dim=1))


@pytest.mark.parametrize("what", ["embedding_size", "no_features", "width", "aggr_mode", "knn_k", "n_mm_layers"])
def test_dragon_unsupported_configurations_raise(cuda, tmp_path, what):
    z = R.load("dragon_small.npz")
    extra, feats = {}, None
    if what == "embedding_size":
        extra = dict(embedding_size=128)
    elif what == "no_features":
        feats = (None, None)
    elif what == "width":
        feats = (z["v_feat"][:, :6], z["t_feat"])
    elif what == "aggr_mode":
        extra = dict(aggr_mode=["mean"])
    elif what == "knn_k":
        extra = dict(knn_k=33)
    else:
        extra = dict(n_mm_layers=-1)
    _, c_, train, *_ = _setup(tmp_path, extra, feats)
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        _model(c_, train)


def test_dragon_quick_start(cuda, tmp_path):
    """`main.py -m DRAGON -d <dataset>`'s path: trains an epoch and evaluates on a dataset
    directory with the .inter file, the two feature files and the user graph file."""
    z = R.load("dragon_small.npz")
    _write_graph(tmp_path, z)
    res = quick_start_case("DRAGON", tmp_path, z["v_feat"], z["t_feat"],
                           {"epochs": 1, "learning_rate": [0.001], "reg_weight": [0.001]})
    assert len(res) == 1 and "recall@20" in res[0][1]
    assert all(np.isfinite(v) for v in res[0][1].values())
