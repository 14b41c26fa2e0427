"""BPR / VBPR on the GPU: the two row-gathered Linear kernels against numpy f64 with derived
rounding bounds, the fused loss's gradients against the f64 restatement (tests/mf_ref.py),
the dense Adam, fused = autograd, the Trainer end to end against the reference's own run
(tests/golden/{bpr,vbpr}_small.npz), the NaN halt, graph capture and quick_start.

Observed figures are printed before every assertion (run with -s to see them)."""
import ctypes as C
import numpy as np
import pytest
import torch

import mf_ref as R
from helpers import dev, loaders, make_model, metric_dict, quick_start_case, record_batches, write_dataset

pytestmark = pytest.mark.gpu

MODELS = ("BPR", "VBPR")
REG = 2.0
U24 = 2.0 ** -24
NS = (1, 33, 1029)
INS = (4, 72, 100, 1028)
N_SRC = 57  # fewer table rows than the largest n: repeated, unsorted row indices


# ------------------------------------------------------------------ 1, 2: the Linear kernels
@pytest.fixture(scope="module")
def lin_cases():
    """Per (n, in_dim, out_dim): inputs and the f64 results, computed once."""
    rng = np.random.default_rng(3)
    cases = {}
    for o in (32, 64, 128):
        for i in INS:
            W = rng.standard_normal((o, i)).astype(np.float32)
            b = rng.standard_normal(o).astype(np.float32)
            for n in NS:
                x = rng.standard_normal((max(n, N_SRC), i)).astype(np.float32)
                rows = rng.integers(0, N_SRC, n).astype(np.int64)
                g = rng.standard_normal((n, 2 * o)).astype(np.float32)  # gradient rows: the left o columns
                cases[(n, i, o)] = dict(W=W, b=b, x=x, rows=rows, g=g)
    return cases


def _fwd_ref(x, W, b):
    x64, W64 = x.astype(np.float64), W.astype(np.float64)
    want = x64 @ W64.T + b
    mag = np.abs(x64) @ np.abs(W64).T + np.abs(b)
    return want, 2 * (x.shape[1] + 1) * U24 * mag


@pytest.mark.parametrize("o", [32, 64, 128])
def test_linear_rows_fwd(cuda, lin_cases, o):
    from rsx import ops

    worst = 0.0
    for i in INS:
        for n in NS:
            c = lin_cases[(n, i, o)]
            x, W, b = dev(c["x"], cuda), dev(c["W"], cuda), dev(c["b"], cuda)
            for rows in (c["rows"], None):
                src = c["x"][rows] if rows is not None else c["x"][:n]
                want, bound = _fwd_ref(src, c["W"], c["b"])
                out = torch.full((n, 2 * o), 7.5, dtype=torch.float32, device=cuda)  # ld_out = 2 out_dim
                xin = x if rows is not None else x[:n].contiguous()
                ops.linear_rows_fwd(xin, W, b, None if rows is None else dev(rows, cuda), out=out, col0=o)
                got = out.cpu().numpy()
                assert np.all(got[:, :o] == 7.5), (n, i, o)  # the sentinel half survives
                err = np.abs(got[:, o:] - want)
                worst = max(worst, float((err / bound).max()))
                assert np.all(err <= bound), (n, i, o, rows is None, float((err / bound).max()))
            # no bias
            want, bound = _fwd_ref(c["x"][c["rows"]], c["W"], np.zeros(o, np.float32))
            got = ops.linear_rows_fwd(x, W, None, dev(c["rows"], cuda)).cpu().numpy()
            assert np.all(np.abs(got - want) <= bound)
    print(f"linear_rows_fwd out_dim {o}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("row_tiles,o,ot", [(1.0, 64, 2), (1.0, 128, 4), (0.5, 128, 2)])
def test_linear_rows_fwd_wide_strips(cuda, row_tiles, o, ot):
    """The launch takes 32 x 32 OT output tiles with OT from the shapes: narrow strips until
    the blocks fill the CUs, so the grid above only launches OT = 1.  Enough row tiles (one
    per CU: the item-table projection of evaluation; half as many at out_dim 128) reach the
    OT = 2 and OT = 4 kernels."""
    from rsx import ops

    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    n, i = int(32 * cus * row_tiles) + 5, 72  # a ragged last row tile
    tiles = -(-n // 32)
    t = o // 32
    while t > 1 and tiles * (o // 32 // t) < cus:
        t //= 2
    assert t == ot  # the plan rsx_linear_rows_fwd documents
    rng = np.random.default_rng(17)
    x = rng.standard_normal((N_SRC, i)).astype(np.float32)
    W = rng.standard_normal((o, i)).astype(np.float32)
    b = rng.standard_normal(o).astype(np.float32)
    rows = rng.integers(0, N_SRC, n).astype(np.int64)
    want, bound = _fwd_ref(x[rows], W, b)
    out = torch.full((n, 2 * o), 7.5, dtype=torch.float32, device=cuda)
    ops.linear_rows_fwd(dev(x, cuda), dev(W, cuda), dev(b, cuda), dev(rows, cuda), out=out, col0=o)
    got = out.cpu().numpy()
    assert np.all(got[:, :o] == 7.5)
    assert np.all(np.abs(got[:, o:] - want) <= bound), (n, o)


def test_linear_rows_unsupported_shapes(cuda):
    from rsx import _lib as L

    lib = L.lib()
    z = torch.zeros(64 * 64, device=cuda)
    p = C.c_void_p(z.data_ptr())
    for i, o in ((16, 48), (16, 256), (18, 64), (6, 32)):
        assert lib.rsx_linear_rows_fwd(p, p, None, None, 8, i, o, p, o, None) == 1002
        assert lib.rsx_linear_rows_wgrad(p, o, p, None, 8, o, i, p, None, p, 1 << 12, None) == 1002


@pytest.mark.parametrize("o", [32, 64, 128])
def test_linear_rows_wgrad(cuda, lin_cases, o):
    from rsx import ops

    worst = 0.0
    for i in INS:
        for n in NS:
            c = lin_cases[(n, i, o)]
            x, g, rows = dev(c["x"], cuda), dev(c["g"], cuda), dev(c["rows"], cuda)
            g64, x64 = c["g"][:, :o].astype(np.float64), c["x"][c["rows"]].astype(np.float64)
            want = g64.T @ x64
            bound = 2 * n * U24 * (np.abs(g64).T @ np.abs(x64))
            dw, db = ops.linear_rows_wgrad(g, x, rows, out_dim=o)  # ld_g = 2 out_dim
            dw2, db2 = ops.linear_rows_wgrad(g, x, rows, out_dim=o)
            assert torch.equal(dw, dw2) and torch.equal(db, db2)  # deterministic
            err = np.abs(dw.cpu().numpy() - want)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert np.all(err <= bound), (n, i, o)
            assert np.all(np.abs(db.cpu().numpy() - g64.sum(0)) <= 2 * n * U24 * np.abs(g64).sum(0))
            # rows = NULL: rsx_linear_wgrad's result
            gc, xc = g[:, :o].contiguous(), x[:n].contiguous()
            dw0, _ = ops.linear_rows_wgrad(gc, xc, None)
            old = ops.linear_wgrad(gc, xc)
            b0 = 2 * n * U24 * (np.abs(g64).T @ np.abs(c["x"][:n].astype(np.float64)))
            assert np.all(np.abs((dw0 - old).cpu().numpy()) <= b0)
            assert torch.equal(dw0, old)  # the same plan and kernels: rsx_linear_wgrad's bits
            assert np.all(np.abs(dw0.cpu().numpy() - g64.T @ c["x"][:n].astype(np.float64)) <= b0)
    print(f"linear_rows_wgrad out_dim {o}: worst error / bound = {worst:.3f}")


# ------------------------------------------------------------------ models on the fixture data
def _feats(model):
    """(image, text) feature tables of the model's dataset directory: VBPR's, none for BPR."""
    if model != "VBPR":
        return None, None
    z = R.load_fixture("VBPR")
    return z["v_feat"], z["t_feat"]


def _setup(tmp_path, model, extra):
    write_dataset(tmp_path, *_feats(model))
    return loaders(model, tmp_path, {"is_multimodal_model": model == "VBPR", **extra})


def _model(tmp_path, name, extra=None):
    c, train, valid, test = _setup(tmp_path, name, extra or {})
    return make_model(name, c, train), c, train, valid, test


def _named(m, name):
    sd = dict(m.named_parameters())
    return [sd[n] for n in R.NAMES[name]]


def _hand_batch():
    """462 triplets (the fixture's tail size): user 7 fills 64 slots, item 5 is the positive
    of 100 triplets and the negative of 40 others."""
    rng = np.random.default_rng(11)
    t = np.stack([rng.integers(0, 400, 462), rng.integers(0, 200, 462), rng.integers(0, 200, 462)]).astype(np.int64)
    t[0, 100:164] = 7
    t[1, :100] = 5
    t[1, 300:340] = 9
    t[2, 300:340] = 5
    return torch.from_numpy(t)


@pytest.mark.parametrize("name", MODELS)
def test_model_init_and_batch_gradients(cuda, tmp_path, name):
    z = R.load_fixture(name)
    m, *_ = _model(tmp_path, name)
    ps = _named(m, name)
    for p, n in zip(ps, R.NAMES[name]):
        assert np.array_equal(p.detach().cpu().numpy().view(np.int32), z["init." + n].view(np.int32)), n
    init = R.fixture_params(z, name, "init.")
    X = R.features(z)
    ref64 = R.MFRef(init, REG, X, dtype=torch.float64)
    ref32 = R.MFRef(init, REG, X, dtype=torch.float32)
    for tag, trip in (("fixture batch 0", R.epoch_batches(z, 0)[0]), ("hand-made 462", _hand_batch())):
        l64, g64 = ref64.loss_grad(trip)
        _, g32 = ref32.loss_grad(trip)
        for p in ps:
            p.grad = None
        loss = m.calculate_loss(trip.cuda())
        loss.backward()
        got = float(loss.item())
        print(f"{name} {tag}: loss {got:.8f} vs f64 {l64:.8f} (rel {abs(got - l64) / abs(l64):.2e})")
        assert abs(got - l64) <= 1e-6 * abs(l64)
        for p, a, b, n in zip(ps, g64, g32, R.NAMES[name]):
            a = a.numpy()
            e32 = float(np.abs(b.numpy().astype(np.float64) - a).max())
            tol = max(4 * e32, 8 * U24 * float(np.abs(a).max()))
            err = float(np.abs(p.grad.cpu().numpy().astype(np.float64) - a).max())
            print(f"  {n}: err {err:.3e}, e32 {e32:.3e}, tol {tol:.3e}, err/tol {err / tol:.3f}")
            assert err <= tol, (n, err, tol)


# ------------------------------------------------------------------ 4: dense Adam
def _engine(name, cuda, z=None):
    from rsx.mf import MFEngine

    z = z or R.load_fixture(name)
    init = R.fixture_params(z, name, "init.")
    X = R.features(z)
    kw = {} if X is None else dict(W=init[2], b=init[3], features=X)
    eng = MFEngine(z["train_u"], z["train_i"], int(z["n_users"]), int(z["n_items"]), 64, REG, 1e-3, cuda,
                   init[0], init[1], batch=512, **kw)
    return eng, R.MFRef(init, REG, X), z


def _disjoint(lo, n=50):
    a = np.arange(lo, lo + n)
    return torch.from_numpy(np.stack([a, a, a + n]).astype(np.int64))


@pytest.mark.parametrize("name", MODELS)
def test_dense_adam_moves_rows_outside_the_batch(cuda, name):
    eng, ref, _ = _engine(name, cuda)
    b1, b2 = _disjoint(0), _disjoint(100)
    b3 = torch.flip(b2, dims=[1]).contiguous()
    snaps = []
    for b in (b1, b2, b3):
        eng.step(triplets=b.cuda())
        ref.step(b)
        snaps.append([t.clone() for t in (eng.U, eng.I)])
    # rows only step 1 touched (users 0..49, items 0..99) keep moving on their moments
    for a, b in zip(snaps[:-1], snaps[1:]):
        assert bool((a[0][:50] != b[0][:50]).any(dim=1).all())
        assert bool((a[1][:100] != b[1][:100]).any(dim=1).all())
    assert all(bool((g == 0).all()) for g in eng.g[:2])  # the scatter scratch is zero again
    worst = 0.0
    for t, r in zip(eng.params, ref.numpy()):
        worst = max(worst, float(np.abs(t.cpu().numpy() - r).max()))
    print(f"{name}: max |param - restatement| after 3 dense Adam steps = {worst:.3e} (bound 2e-6)")
    assert worst <= 2e-6


# ------------------------------------------------------------------ 5: fused = autograd
@pytest.mark.parametrize("name", MODELS)
def test_fused_path_equals_autograd_path(cuda, tmp_path, name):
    z = R.load_fixture(name)
    a, *_ = _model(tmp_path / "a", name)
    b, *_ = _model(tmp_path / "b", name)
    opt = torch.optim.Adam(b.parameters(), lr=1e-3)
    for trip in R.epoch_batches(z, 0):
        t = trip.cuda()
        a.fused_step(t, 1e-3)
        opt.zero_grad()
        b.calculate_loss(t).backward()
        opt.step()
    worst = max(float((p - q).abs().max()) for p, q in zip(_named(a, name), _named(b, name)))
    print(f"{name}: fused vs autograd after one epoch: {worst:.3e} (bound 5e-5)")
    assert worst <= 5e-5


# ------------------------------------------------------------------ 6: Trainer end to end
def _train(tmp_path, name, extra, epochs, record=False):
    from rsx.trainer import Trainer

    m, c, train, valid, test = _model(tmp_path, name, extra)
    t = Trainer(c, m)
    assert t.fused
    rec = record_batches(train) if record else []
    for epoch in range(epochs):
        m.cur_epoch = epoch
        m.pre_epoch_processing()
        loss, _ = t._train_epoch(train, epoch)
        assert not torch.is_tensor(loss) and np.isfinite(loss)
        t._epoch_for_lr += 1
    torch.cuda.synchronize()
    return m, t, valid, test, rec


@pytest.mark.parametrize("name", MODELS)
def test_trainer_vs_reference(cuda, tmp_path, name):
    z = R.load_fixture(name)
    epochs = R.FIXTURE[name][1]
    last = epochs - 1
    m, t, valid, test, rec = _train(tmp_path, name, {}, epochs, record=True)
    want = np.concatenate([z[f"epoch{e}_triplets"] for e in range(epochs)], axis=1).astype(np.int64)
    assert np.array_equal(torch.cat(rec, dim=1).numpy(), want)
    for p, n in zip(_named(m, name), R.NAMES[name]):
        err = float(np.abs(p.detach().cpu().numpy() - z[f"epoch{last}_param." + n]).max())
        print(f"{name} {n}: max |param - reference| = {err:.3e} (bound 5e-5)")
        assert err <= 5e-5, n
    for split, loader in (("valid", valid), ("test", test)):
        tag = f"epoch{last}_{split}"
        res = t.evaluate(loader)
        ref = metric_dict(z, tag)
        assert res.keys() == ref.keys()
        for k in ref:
            assert abs(res[k] - ref[k]) <= 1e-4 + 1e-12, (k, res[k], ref[k])
        assert np.array_equal(loader.eval_u.cpu().numpy(), z[tag + "_users"])
        _, idx = m.full_sort_topk([loader.eval_u, None], 50, loader)
        same = np.all(idx.cpu().numpy() == z[tag + "_topk_idx"].astype(np.int64), axis=1)
        assert np.all(same | z[tag + "_inner_tie"] | z[tag + "_boundary_tie"])
        # the dense scores (full_sort_predict) rank the same items first
        sc = m.full_sort_predict([loader.eval_u[:8], None])
        assert sc.shape == (8, int(z["n_items"]))


@pytest.mark.parametrize("name", MODELS)
def test_trainer_device_sampler(cuda, tmp_path, name):
    z = R.load_fixture(name)
    epochs = R.FIXTURE[name][1]
    m, t, valid, _, _ = _train(tmp_path, name, dict(rsx_sampler="device"), epochs)
    res = t.evaluate(valid)
    for k, want in metric_dict(z, f"epoch{epochs - 1}_valid").items():
        assert np.isfinite(res[k]) and abs(res[k] - want) <= 0.05 + 0.5 * want, (k, res[k], want)


# ------------------------------------------------------------------ 7: NaN halt
@pytest.mark.parametrize("name", MODELS)
def test_nan_loss_halts_the_step(cuda, name):
    eng, _, z = _engine(name, cuda)
    b0, b1 = (t.cuda() for t in R.epoch_batches(z, 0)[:2])
    eng.step(triplets=b0)  # moments are non-zero now
    eng.U[int(b1[0, 3])].fill_(float("nan"))
    state = [t.clone() for t in (*eng.params, *eng.m, *eng.v)]
    eng.step(triplets=b1)
    torch.cuda.synchronize()
    assert eng.halt.cpu().tolist() == [1, 2]
    assert bool(torch.isnan(eng.loss_out).all())
    for a, b in zip(state, (*eng.params, *eng.m, *eng.v)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    eng.step(triplets=b0)  # halted from then on
    for a, b in zip(state, (*eng.params, *eng.m, *eng.v)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert all(bool((g == 0).all()) for g in eng.g[:2])


# ------------------------------------------------------------------ 8: capture
@pytest.mark.parametrize("name", MODELS)
def test_captured_step_replays(cuda, name):
    eng, _, z = _engine(name, cuda)
    ref, _, _ = _engine(name, cuda)
    trip = R.epoch_batches(z, 0)[0].cuda()
    for _ in range(3):
        ref.step(triplets=trip)
    eng.step(triplets=trip)  # eager step 1
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # one stream, no side branches
        eng.step(triplets=trip)
    g.replay()  # steps 2 and 3
    g.replay()
    torch.cuda.synchronize()
    assert eng.sync_step_count() == 3
    worst = max(float((a - b).abs().max()) for a, b in zip(eng.params, ref.params))
    print(f"{name}: eager + 2 replays vs 3 eager steps: {worst:.3e} (bound 5e-5)")
    assert worst <= 5e-5


# ------------------------------------------------------------------ 9: quick_start
@pytest.mark.parametrize("name", MODELS)
def test_quick_start(cuda, tmp_path, name):
    res = quick_start_case(name, tmp_path, *_feats(name), {"epochs": 2, "reg_weight": [1e-2]})
    assert len(res) == 1 and "recall@20" in res[0][1]


def test_vbpr_without_features_is_refused(cuda, tmp_path):
    from rsx.utils import get_model, init_seed

    c, train, *_ = _setup(tmp_path, "BPR", {})  # a data directory without feature files
    c["is_multimodal_model"] = True
    init_seed(999)
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):
        get_model("VBPR")(c, train)


def test_vbpr_feature_width_not_a_multiple_of_4_is_refused(cuda, tmp_path):
    from rsx.utils import get_model, init_seed

    c, train, *_ = _setup(tmp_path, "VBPR", {})
    z = R.load_fixture("VBPR")
    np.save(tmp_path / "data" / "baby" / "text_feat_raw.npy", z["t_feat"][:, :22])  # 48 + 22 = 70
    init_seed(999)
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED.*70"):
        get_model("VBPR")(c, train)


# ------------------------------------------------------------------ tail batches, device draw
def _synth_engine(cuda, d, F, batch, nu=300, ni=150, n_inter=5000):
    from rsx.mf import MFEngine, bpr_init, vbpr_init

    rng = np.random.default_rng(23)
    tu, ti = rng.integers(0, nu, n_inter).astype(np.int64), rng.integers(0, ni, n_inter).astype(np.int64)
    torch.manual_seed(4)
    if F:
        X = rng.standard_normal((ni, F)).astype(np.float32)
        init = [t.numpy() for t in vbpr_init(nu, ni, d, F)]
        kw = dict(W=init[2], b=init[3], features=X)
    else:
        X, init, kw = None, [t.numpy() for t in bpr_init(nu, ni, d)], {}
    eng = MFEngine(tu, ti, nu, ni, d, 1e-2, 1e-3, cuda, init[0], init[1], batch=batch, seed=3, **kw)
    refs = {dt: R.MFRef(init, 1e-2, X, dtype=dt) for dt in (torch.float32, torch.float64)}
    return eng, refs, rng


@pytest.mark.parametrize("d,F,b", [(64, 384, 2016), (32, 384, 609), (64, 72, 1500), (128, 384, 2000)])
def test_tail_batch_fits_the_engine_workspace(cuda, d, F, b):
    """An engine built for batches of 2048 steps a shorter one, of sizes at which the
    weight gradient's exact split plan needs more partial slots than at 2048 (the workspace
    query is a bound that does not decrease with the batch).  loss_grad, then the fused
    step, against the f64 restatement."""
    eng, refs, rng = _synth_engine(cuda, d, F, 2048)
    ref, ref64 = refs[torch.float32], refs[torch.float64]
    t = torch.from_numpy(np.stack([rng.integers(0, 300, b), rng.integers(0, 150, b), rng.integers(0, 150, b)]))
    loss, g = eng.loss_grad(t.cuda())
    l64, g64 = ref64.loss_grad(t)
    _, g32 = ref.loss_grad(t)
    assert abs(float(loss) - l64) <= 1e-6 * abs(l64)
    tols = []
    for a, r64, r32 in zip(g, g64, g32):  # the bound of test_model_init_and_batch_gradients
        e32 = float((r32.double() - r64).abs().max())
        tols.append(max(4 * e32, 8 * U24 * float(r64.abs().max())))
        assert float((a.cpu().double() - r64).abs().max()) <= tols[-1]
    # The step itself, against the f64 restatement's.  Adam's first step moves an element by
    # lr g / (|g| + eps), whose slope in g is lr eps / (|g| + eps)^2: up to lr / eps = 1e5 where
    # |g| is near eps = 1e-8 (the f32 and f64 restatements themselves differ by 1.5e-6 there
    # on this batch), so a flat atol would measure those few elements' gradient noise.  With
    # the gradient within `tol` of g64 (asserted above) the update is within
    # lr tol eps / (max(|g64| - tol, 0) + eps)^2, plus the f32 rounding of the update itself.
    # Elements with g = 0 (rows outside the batch) do not move at all in the first step.
    init = [p.clone() for p in eng.params]
    eng.step(triplets=t.cuda())
    ref64.step(t)
    lr, eps, worst = 1e-3, 1e-8, 0.0
    for p, p0, r, r64, gt in zip(eng.params, init, ref64.numpy(), g64, tols):
        ga = r64.abs().numpy()
        # f32 roundings of the kernel's update (rsx_adam.hpp): v 3, sqrt (halving v's) 1, the
        # two bias-correction constants 2, / and + eps 2, m 1, m / denom 1, step size 1 and
        # its product 1: under 12 units of 2^-24 relative to the move (<= lr); the final add
        # one unit relative to the parameter (4 allowed)
        bound = lr * gt * eps / (np.maximum(ga - gt, 0) + eps) ** 2 + U24 * (4 * np.abs(r) + 12 * lr)
        err = np.abs(p.cpu().numpy().astype(np.float64) - r)
        zero = ga == 0
        assert np.array_equal(p.cpu().numpy()[zero], p0.cpu().numpy()[zero])
        worst = max(worst, float((err[~zero] / bound[~zero]).max()))
        k = int(np.argmax(np.where(zero, 0, err / bound)))
        assert np.all(err[~zero] <= bound[~zero]), (k, err.flat[k], bound.flat[k], ga.flat[k], gt)
    print(f"d {d} F {F} batch {b}: worst |param - f64 restatement| / bound after the step = {worst:.3f}")
    assert int(eng.halt[0]) == 0


@pytest.mark.parametrize("F", [0, 72])
def test_step_draws_its_own_triplets(cuda, F):
    """rsx_mf_step with `sample` set: the batch is drawn in the same call, rsx_sample_triplets'
    contract, the last one of the epoch shorter; the step is the one of those triplets."""
    a, _, _ = _synth_engine(cuda, 64, F, 512)
    b, _, _ = _synth_engine(cuda, 64, F, 512)
    for start in (0, 512, 4608):  # 5000 interactions: the last batch has 392
        want = b.sampler.sample(0, start, 512)
        got = a.step_draw(0, start)
        assert got.shape == want.shape == (3, min(512, 5000 - start)) and torch.equal(got, want)
        b.step(triplets=want)
        assert abs(float(a.loss_out) - float(b.loss_out)) <= 1e-6 * abs(float(b.loss_out))
    worst = max(float((p - q).abs().max()) for p, q in zip(a.params, b.params))
    assert worst <= 2e-6 and a.step_count == b.step_count == 3  # f32 atomics: the order of the adds differs


def test_item_table_follows_a_torch_optimiser(cuda, tmp_path):
    """The cached evaluation table is rebuilt after an in-place torch update of the
    parameters (the autograd path: no train() / eval() call in between)."""
    z = R.load_fixture("VBPR")
    m, *_ = _model(tmp_path, "VBPR")
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    before = m.engine.item_table().clone()
    opt.zero_grad()
    m.calculate_loss(R.epoch_batches(z, 0)[0].cuda()).backward()
    assert torch.equal(m.engine.item_table(), before)  # nothing moved yet
    opt.step()
    after = m.engine.item_table()
    ps = [p.detach().cpu().double() for p in _named(m, "VBPR")]
    want = torch.cat((ps[1], torch.from_numpy(R.features(z)).double() @ ps[2].t() + ps[3]), -1)
    assert not torch.equal(after, before)
    assert float((after.cpu().double() - want).abs().max()) <= 1e-5
