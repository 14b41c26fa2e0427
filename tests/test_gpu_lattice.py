"""LATTICE on the GPU: the fused loss, the learned item graph and its backward
(csrc/lattice.hip, rsx.lattice) against the float64 restatement (tests/lattice_ref.py), and the
model (rsx.lattice.LATTICE) against the reference's own run (tests/golden/lattice_step0_small.npz,
lattice_small.npz).

Bounds.
* Loss kernel (tests/test_gpu_freedom.py's rule): the forward's three words 1e-5 relative; the
  gradients 1e-4 of the tensor's scale, or 4x the error the same formulas in float32 torch on
  the CPU make against the restatement on the same inputs, whichever is larger.
* Graph forward and propagation: 1e-5 of sum_j |M_ij| |x_j| per element, the quantity a float32
  sum's error is proportional to (it is |y_i| itself where a row's terms share a sign, which
  makes this rtol 1e-5; where they cancel no float32 sum can keep 1e-5 of the result).
* Graph backward: 4x the error of the restatement's own float32 CPU autograd against its
  float64 run on the same inputs (GPU sums reassociate), per tensor, in max-norm; the float32
  error counts as no less than half a unit in the last place of the tensor's largest value.
  Measured on an MI355X: test_graph_backward_vs_autograd's docstring.
* Model: the first two steps' gradients rtol 1e-3, atol 1e-5 of the tensor's scale; two epochs
  5e-5 of the parameter's scale, metrics 1e-4, top-50 equal modulo the recorded ties.
"""
import numpy as np
import pytest
import torch

import lattice_ref as R
from helpers import (assert_same_run, check_eval, check_params, check_vs_f32, coo_sorted, csr_to_sorted, dev, loaders,
                     make_model, quick_start_case, record_batches, train_epochs, write_dataset)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1. the loss kernel
def _loss_inputs(d, B, nu, ni, seed):
    rng = np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32)  # noqa: E731
    x = dict(E=f32(rng.standard_normal((nu + ni, d)) * 0.3), H=f32(rng.standard_normal((ni, d)) * 0.3))
    trip = np.stack([rng.integers(0, nu, B), rng.integers(0, ni, B), rng.integers(0, ni, B)]).astype(np.int64)
    if B > 1:  # an item that is a positive in one triplet and a negative in another
        trip[2, 1] = trip[1, 0]
        trip[1, B - 1] = trip[2, 0]
    x["trip"] = trip
    return x


def _run_loss(x, nu, reg, bs, cuda):
    from rsx import lattice as LT

    d, B = x["E"].shape[1], x["trip"].shape[1]
    ws = LT.workspace(B, d, cuda)
    E, H = dev(x["E"], cuda, True), dev(x["H"], cuda, True)
    keep = {}
    loss = LT._LatticeLoss.apply((nu, reg, bs, ws, keep), dev(x["trip"], cuda), E, H)
    loss.backward()
    out = keep["terms"].detach().cpu().numpy()
    assert out[0] == loss.item() or (np.isnan(out[0]) and np.isnan(loss.item()))
    return out, E.grad.cpu().numpy(), H.grad.cpu().numpy()


@pytest.mark.parametrize("nu,ni", [(5, 7), (400, 200)])
@pytest.mark.parametrize("B", [1, 67, 300, 512])
@pytest.mark.parametrize("d", [64, 128])
def test_loss_kernel_vs_restatement(cuda, d, B, nu, ni):
    x = _loss_inputs(d, B, nu, ni, 300 + d + B + nu)
    trip = x["trip"]
    if B == 512 and nu == 5:  # every row repeats more than a wave's 64 lanes
        assert np.bincount(trip[0], minlength=nu).min() > 64
        assert np.bincount(np.concatenate([trip[1], trip[2]]), minlength=ni).min() > 64
    bs = 2048.0  # the configured batch size, not the batch's length
    for reg in (0.0, 0.05):
        print(f"d={d} B={B} tables=({nu},{ni}) reg={reg}")
        ref = R.loss_grad(x["E"], x["H"], trip, nu, reg, bs)
        tor = R.loss_grad(x["E"], x["H"], trip, nu, reg, bs, dtype=torch.float32)
        got = _run_loss(x, nu, reg, bs, cuda)
        for k, name in enumerate(("total", "mf", "emb")):
            print(f"  {name}: {got[0][k]:.8f} vs {ref[0][k]:.8f}")
            assert abs(got[0][k] - ref[0][k]) <= 1e-5 * abs(ref[0][k]), name
        check_vs_f32("gE", got[1], ref[1], tor[1])
        check_vs_f32("gH", got[2], ref[2], tor[2])
        off_u = np.setdiff1d(np.arange(nu), trip[0])
        off_i = np.setdiff1d(np.arange(ni), np.concatenate([trip[1], trip[2]]))
        assert not got[1][off_u].any() and not got[1][nu + off_i].any() and not got[2][off_i].any()
        again = _run_loss(x, nu, reg, bs, cuda)  # deterministic: a second call is bit-equal
        for a, b in zip(got, again):
            assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("d", [64, 128])
def test_loss_kernel_saturated_scores(cuda, d):
    """Scores of +-40: softplus and its derivative neither overflow nor lose the answer."""
    nu, ni, B, reg, bs = 8, 2, 8, 0.01, 16.0
    e = np.full(d, 1.0 / np.sqrt(d), dtype=np.float32)
    E = np.concatenate([np.tile(20.0 * e, (nu, 1)), np.zeros((ni, d), dtype=np.float32)]).astype(np.float32)
    H = np.stack([3.0 * e, -0.5 * e]).astype(np.float32)  # normalised: +e and -e
    b = np.arange(B)
    trip = np.stack([b, b % 2, 1 - b % 2]).astype(np.int64)  # even b: x = +40, odd b: x = -40
    x = dict(E=E, H=H, trip=trip)
    ref = R.loss_grad(E, H, trip, nu, reg, bs)
    got = _run_loss(x, nu, reg, bs, cuda)
    assert np.all(np.isfinite(got[0])) and abs(got[0][1] - 20.0) <= 1e-4
    np.testing.assert_allclose(got[0], ref[0], rtol=1e-5)
    assert np.all(np.isfinite(got[1])) and np.all(np.isfinite(got[2]))
    np.testing.assert_allclose(got[1], ref[1], rtol=1e-5, atol=1e-6 * np.abs(ref[1]).max())
    np.testing.assert_allclose(got[2], ref[2], rtol=1e-5, atol=1e-6 * np.abs(ref[1]).max())


def test_loss_kernel_bad_index_and_batch_cap(cuda):
    from rsx import lattice as LT

    x = _loss_inputs(64, 8, 5, 7, 1)
    x["trip"][1, 3] = 7  # an item outside its table
    out, gE, gH = _run_loss(x, 5, 0.1, 8.0, cuda)
    assert np.isnan(out[0]) and np.all(np.isfinite(gE)) and np.all(np.isfinite(gH))
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):
        LT.workspace(65537, 64, cuda)


# ------------------------------------------------- 2 / 3. the graph against the dense operator
_CASES = {}


def _graph_case(N, k, M, L):
    """Inputs of one graph case (made once): projected tables, kept columns from the
    restatement, original graphs, modal_weight, h, an output gradient; the dense float64
    operator; the float64 and float32 autograd of sum(G * M^L h)."""
    key = (N, k, M, L)
    if key in _CASES:
        return _CASES[key]
    f, d = (64, 128) if M == 2 else (128, 64)
    rng = np.random.default_rng(1000 * N + 10 * k + M)
    c = dict(N=N, k=k, M=M, L=L, f=f, d=d, lam=0.9)
    c["F"] = [(rng.standard_normal((N, f)) + 0.5).astype(np.float32) for _ in range(M)]
    raws = [rng.standard_normal((N, 12)).astype(np.float32) for _ in range(M)]
    og = [R.original_graph(r, k) for r in raws]
    c["oidx"], c["oval"] = [o[0].numpy() for o in og], [o[1].numpy().astype(np.float32) for o in og]
    c["idx"] = [R.topk_ids(R.t64(F), k).numpy() for F in c["F"]]
    c["mw"] = np.array([0.3, -0.4], dtype=np.float32) if M == 2 else None
    c["h"] = (rng.standard_normal((N, d)) * 0.3).astype(np.float32)
    c["G"] = rng.standard_normal((N, d)).astype(np.float32)

    def autograd(dt):
        cast = lambda a: torch.as_tensor(a, dtype=dt).clone().requires_grad_(True)  # noqa: E731
        Fs, h = [cast(F) for F in c["F"]], cast(c["h"])
        mw = cast(c["mw"]) if M == 2 else None
        Os = [R.dense_lists(i, v, N).to(dt) for i, v in zip(c["oidx"], c["oval"])]
        A = R.item_adj(Fs, [torch.from_numpy(i) for i in c["idx"]], Os, mw, c["lam"])
        y = R.propagate(A, h, L)
        (y * torch.as_tensor(c["G"], dtype=dt)).sum().backward()
        g = dict(h=h.grad.numpy(), **{f"F{m}": Fs[m].grad.numpy() for m in range(M)})
        if M == 2:
            g["mw"] = mw.grad.numpy()
        return A.detach().numpy(), y.detach().numpy(), g

    c["A"], c["y"], c["g64"] = autograd(torch.float64)
    _, _, c["g32"] = autograd(torch.float32)
    _CASES[key] = c
    return c


def _device_graph(c, cuda):
    from rsx.lattice import ItemGraph

    Fs = [dev(F, cuda, True) for F in c["F"]]
    mw = dev(c["mw"], cuda, True)
    g = ItemGraph(Fs, [dev(i, cuda) for i in c["idx"]], [dev(i, cuda) for i in c["oidx"]],
                  [dev(v, cuda) for v in c["oval"]], mw, c["lam"])
    return g, Fs, mw


GRAPH_SHAPES = [(7, 3, 2, 1), (7, 1, 1, 2), (200, 10, 2, 1), (200, 32, 1, 2), (200, 1, 2, 2), (300, 10, 2, 2),
                (300, 32, 2, 1), (300, 1, 1, 1), (300, 10, 1, 1)]


@pytest.mark.parametrize("N,k,M,L", GRAPH_SHAPES)
def test_graph_forward_and_propagation_vs_dense(cuda, N, k, M, L):
    c = _graph_case(N, k, M, L)
    g, _, _ = _device_graph(c, cuda)
    A = c["A"]
    # the operator's own pieces
    w = np.exp(c["mw"] - c["mw"].max()) / np.exp(c["mw"] - c["mw"].max()).sum() if M == 2 else np.array([1.0, 0.0])
    np.testing.assert_allclose(g.w.cpu().numpy(), w, rtol=1e-5)
    col, val = g.col.cpu().numpy().astype(np.int64), g.val.cpu().numpy().astype(np.float64)
    dense = np.zeros((N, N))
    np.add.at(dense, (np.repeat(np.arange(N), g.K), col.reshape(-1)), val.reshape(-1))
    np.testing.assert_allclose(dense, A, rtol=1e-5, atol=1e-5 * np.abs(A).max())
    # the transpose index is the stable sort of the columns
    te, tp = g.tedge.cpu().numpy().astype(np.int64), g.tptr.cpu().numpy()
    assert np.array_equal(te, np.argsort(col.reshape(-1), kind="stable"))
    assert np.array_equal(tp, np.concatenate([[0], np.cumsum(np.bincount(col.reshape(-1), minlength=N))]))
    x, gr = dev(c["h"], cuda), dev(c["G"], cuda)
    y, yt = x, gr
    want, want_t = c["h"].astype(np.float64), c["G"].astype(np.float64)
    mag, mag_t = np.abs(want), np.abs(want_t)
    for _ in range(L):
        y, yt = g.prop(y), g.prop(yt, transpose=True)
        want, want_t = A @ want, A.T @ want_t
        mag, mag_t = np.abs(A) @ mag, np.abs(A.T) @ mag_t
    for name, got, ref, m in (("item_adj^L x", y, want, mag), ("(item_adj^T)^L g", yt, want_t, mag_t)):
        err = np.abs(got.cpu().numpy() - ref)
        print(f"  {name}: worst err / (1e-5 sum|terms|) = {(err / (1e-5 * m + 1e-300)).max():.3f}")
        assert np.all(err <= 1e-5 * m), name
    again = x
    for _ in range(L):
        again = g.prop(again)
    assert torch.equal(y, again)  # bit-identical from run to run


@pytest.mark.parametrize("N,k,M,L", GRAPH_SHAPES)
def test_graph_backward_vs_autograd(cuda, N, k, M, L):
    """d sum(G * item_adj^L h) / d (F_m, modal_weight, h) against the restatement's float64
    autograd; bound: 4x the restatement's own float32 CPU autograd error, per tensor.
    Measured on an MI355X, error / float32 autograd error per tensor over the k in {3, 10, 32}
    cases: 0.48 .. 2.00 (h 1.28 .. 1.94, F_m 0.90 .. 1.85, modal_weight 0.48 .. 2.00), the errors
    themselves 6e-10 .. 1e-6 on tensors of scale 1e-3 .. 5.  The k = 1 cases are degenerate (the
    operator is the identity): h's gradient has float32 error 0 on the CPU and 7e-7 here (2.65
    half-units in the last place of its largest value), the other gradients are analytically
    zero and 2e-7 (modal_weight) and 2e-15 (F_m) here; see the two notes in the loop."""
    from rsx.lattice import _ItemProp

    c = _graph_case(N, k, M, L)
    runs = []
    for _ in range(2):
        g, Fs, mw = _device_graph(c, cuda)
        h = dev(c["h"], cuda, True)
        H = _ItemProp.apply(h, g, L, True, mw, *Fs)
        (H * dev(c["G"], cuda)).sum().backward()
        got = dict(h=h.grad.cpu().numpy(), **{f"F{m}": Fs[m].grad.cpu().numpy() for m in range(M)})
        if M == 2:
            got["mw"] = mw.grad.cpu().numpy()
        runs.append(got)
    np.testing.assert_allclose(H.detach().cpu().numpy(), c["y"], rtol=1e-4, atol=1e-5 * np.abs(c["y"]).max())
    for name, ref in c["g64"].items():
        # the float32 run's error, and no less than half a unit in the last place of the tensor's
        # largest value: with k = 1 the operator is the identity, the CPU's float32 gradient of h is
        # exact (error 0.0) and the rule "4x the float32 error" would ask for float64's bits
        err32 = max(float(np.abs(c["g32"][name] - ref).max()), 2.0 ** -24 * float(np.abs(ref).max()))
        err = float(np.abs(runs[0][name] - ref).max())
        if k == 1 and name != "h":
            # k = 1: every list is the self loop, item_adj is the identity whatever F and
            # modal_weight are, and their gradients are analytically zero: both runs hold only
            # what is left of terms that cancel, of which neither is a measure of the other.
            # The terms are those of sum(G * y), so the bound is a float32 sum's over them
            err32 = 2.0 ** -24 * float(np.abs(c["G"].astype(np.float64) * c["y"]).sum())
        print(f"  N={N} k={k} M={M} L={L} {name}: err {err:.3e}, float32 autograd err {err32:.3e}, "
              f"ratio {err / max(err32, 1e-300):.2f}, scale {np.abs(ref).max():.3e}")
        assert np.all(np.isfinite(runs[0][name])), name
        assert err <= 4 * err32, name
        assert np.array_equal(runs[0][name].view(np.int32), runs[1][name].view(np.int32)), name  # bit-identical


# ------------------------------------------------------------------------- the model
def _setup(tmp_path, extra=None, feats="both"):
    z = R.load_fixture()
    # narrow: a text table whose width is no multiple of 4
    text = {"both": z["t_feat"], "text": z["t_feat"], "narrow": z["t_feat"][:, :6]}.get(feats)
    write_dataset(tmp_path, z["v_feat"] if feats != "text" else None, text)
    cfg = dict(is_multimodal_model=True, reg_weight=[R.HPARAMS["reg_weight"]],
               learning_rate=[R.HPARAMS["learning_rate"]])
    cfg.update(extra or {})
    return (z,) + loaders("LATTICE", tmp_path, cfg)


def _model(c, train):
    return make_model("LATTICE", c, train)


def _load_params(m, z, prefix):
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(torch.from_numpy(z[prefix + n]).to(p.device))


def _same_sets(got, want, gap):
    """Rows whose neighbour sets differ, among the rows whose recorded gap exceeds 1e-5."""
    use = gap > 1e-5
    same = (np.sort(got, 1) == np.sort(want.astype(np.int64), 1)).all(1)
    return int((use & ~same).sum()), int((~use).sum())


def test_lattice_neighbours_vs_fixture(cuda, tmp_path):
    z, c, train, *_ = _setup(tmp_path)
    m = _model(c, train)
    ni = m.n_items
    for ep, prefix in ((0, "init."), (1, "epoch0_param.")):
        _load_params(m, z, prefix)
        g = m.build_graph()
        for mod, idx in zip(m.mods, g.idx):
            bad, left_out = _same_sets(idx.cpu().numpy(), z[f"build{ep}_{mod}_idx"], z[f"build{ep}_{mod}_gap"])
            print(f"build {ep} {mod}: {bad} rows differ, {left_out} rows left out")
            assert bad == 0 and left_out <= 0.02 * ni, (ep, mod)


def test_lattice_init_graphs_forward(cuda, tmp_path):
    z, c, train, *_ = _setup(tmp_path)
    m = _model(c, train)
    named = dict(m.named_parameters())
    assert tuple(named) == R.NAMES
    for n, p in named.items():
        assert np.array_equal(p.detach().cpu().numpy().view(np.int32), z["init." + n].view(np.int32)), n
    ref = coo_sorted(z["norm_adj_idx"].astype(np.int64), z["norm_adj_val"])
    A, AT = m.norm_adj_csr, m.norm_adj_t_csr
    mine = csr_to_sorted(A.rowptr.cpu().numpy(), A.col.cpu().numpy()[: A.nnz], A.val.cpu().numpy()[: A.nnz])
    for a, b in zip(ref, mine):
        assert np.array_equal(a, b)
    # the transpose operand: the same structure, the transposed values
    n = m.n_nodes
    D = np.zeros((n, n), dtype=np.float32)
    D[mine[0], mine[1]] = mine[2]
    t = csr_to_sorted(AT.rowptr.cpu().numpy(), AT.col.cpu().numpy()[: AT.nnz], AT.val.cpu().numpy()[: AT.nnz])
    assert np.array_equal(t[0], mine[0]) and np.array_equal(t[1], mine[1]) and np.array_equal(t[2], D.T[t[0], t[1]])
    # the original graphs' lists
    for mod in m.mods:
        idx, val = (t.cpu().numpy() for t in m._orig[mod])
        bad, left_out = _same_sets(idx, z[f"orig_{mod}_idx"], z[f"orig_{mod}_gap"])
        assert bad == 0 and left_out <= 0.02 * m.n_items, mod
        want = R.dense_lists(z[f"orig_{mod}_idx"], z[f"orig_{mod}_val"], m.n_items).numpy()
        np.testing.assert_allclose(R.dense_lists(idx, val, m.n_items).numpy(), want, rtol=1e-5, atol=1e-6)
    m.eval()
    with torch.no_grad():
        u, i = m.forward(build_item_graph=True)
        np.testing.assert_allclose(u.cpu().numpy(), z["fwd_user"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(i.cpu().numpy(), z["fwd_item"], rtol=1e-5, atol=1e-6)
        u2, i2 = m._eval_tables()
        np.testing.assert_allclose(i2.cpu().numpy(), z["fwd_item"], rtol=1e-5, atol=1e-6)
        assert torch.equal(u2, u.contiguous())


def test_lattice_first_two_steps(cuda, tmp_path):
    from rsx.optim import RsxAdam

    z, c, train, *_ = _setup(tmp_path)
    m = _model(c, train)
    m.train()
    m.pre_epoch_processing()
    opt = RsxAdam(list(m.parameters()), lr=c["learning_rate"])
    trip = z["epoch0_triplets"].astype(np.int64)
    for s in (0, 1):
        opt.zero_grad(set_to_none=True)
        assert m.graph_step_eager() == (s == 0)
        loss = m.calculate_loss(dev(trip[:, 512 * s: 512 * (s + 1)], cuda))
        loss.backward()
        want = float(z[f"step{s}_loss"])
        print(f"step {s}: loss {loss.item():.8f} vs reference {want:.8f}; words {m.last_terms.cpu().numpy()}")
        assert abs(loss.item() - want) <= 1e-5 * abs(want)
        none = {n for n, p in m.named_parameters() if p.grad is None}
        assert none == set(z[f"step{s}_none"].tolist()), (s, none)
        for n, p in m.named_parameters():
            if p.grad is None:
                continue
            w = z[f"step{s}_grad.{n}"]
            g = p.grad.detach().cpu().numpy()
            scale = max(float(np.abs(w).max()), 1e-30)
            print(f"  step {s} grad {n}: err {np.abs(g - w).max():.3e}, scale {scale:.3e}")
            np.testing.assert_allclose(g, w, rtol=1e-3, atol=1e-5 * scale, err_msg=f"step {s} {n}")
        opt.step()
        check_params(m, z, f"step{s}_param.", 1e-5)
    # Adam skipped the graph-only parameters on the steady batch: one step taken, as the reference's
    for n, p in m.named_parameters():
        assert int(opt.state[p]["step"].item()) == (1 if n in R.GRAPH_ONLY else 2), n


def _steps(tmp_path, tag, z, cuda, graph):
    from rsx.trainer import Trainer

    _, c, train, *_ = _setup(tmp_path / tag, dict(rsx_graph_step=graph))
    m = _model(c, train)
    t = Trainer(c, m)
    m.train()
    t._gate = False
    losses, replays, dropped = [], [], []
    for ep in (0, 1):
        m.pre_epoch_processing()
        t.reset_graph_step()
        dropped.append(t._graph is None)
        trip = z[f"epoch{ep}_triplets"].astype(np.int64)
        for k in range(4):
            losses.append(t.train_step(dev(trip[:, 512 * k: 512 * (k + 1)], cuda), k)[1])
        replays.append(t._graph.replays if t._graph is not None else 0)
    torch.cuda.synchronize()
    return m, [float(x) for x in losses], replays, dropped


def test_lattice_captured_step_equals_eager(cuda, tmp_path):
    z = R.load_fixture()
    a, la, ra, da = _steps(tmp_path, "graph", z, cuda, True)
    b, lb, rb, _ = _steps(tmp_path, "eager", z, cuda, False)
    # per epoch: batch 0 (the build) eager, batch 1 eager (the first steady one), batch 2 captured
    # and replayed, batch 3 a replay; the epoch boundary drops the capture
    assert ra == [2, 2] and rb == [0, 0] and da == [True, True]
    assert_same_run(a, b, la, lb)


def test_lattice_trainer_vs_reference(cuda, tmp_path):
    from rsx.trainer import Trainer

    z, c, train, valid, test = _setup(tmp_path)
    m = _model(c, train)
    t = Trainer(c, m)
    assert not t.fused and type(t.optimizer).__name__ == "RsxAdam"
    rec = record_batches(train)

    def epochs_build(epoch):  # the neighbours the epoch's build chose
        for mod, idx in zip(m.mods, m.item_graph.idx):
            bad, _ = _same_sets(idx.cpu().numpy(), z[f"build{epoch}_{mod}_idx"], z[f"build{epoch}_{mod}_gap"])
            assert bad == 0, (epoch, mod)

    losses = train_epochs(t, m, train, 2, after_epoch=epochs_build)
    want = np.concatenate([z[f"epoch{e}_triplets"] for e in range(2)], axis=1).astype(np.int64)
    assert np.array_equal(torch.cat(rec, dim=1).numpy(), want)  # the recorded triplets
    assert t._graph is not None and t._graph.replays > 0
    print(f"epoch losses {losses} vs reference {z['epoch_losses']}")
    np.testing.assert_allclose(losses, z["epoch_losses"], rtol=1e-5)
    check_params(m, z, "epoch1_param.", 5e-5)
    check_eval(t, m, z, (("valid", valid), ("test", test)))
    # the evaluation tables are cached until train() is called
    assert m._eval_cache is not None
    m.train()
    assert m._eval_cache is None


# ----------------------------------------------------------------------- variants
def _one_step_vs_restatement(m, z, cuda, mods, cf_model):
    trip = z["epoch0_triplets"].astype(np.int64)[:, :512]
    p = {n: q.detach().cpu().numpy() for n, q in m.named_parameters()}
    ref = R.Model(p, R.ui_dense(z), R.orig_dense(z), cf_model=cf_model)
    want, g = ref.loss_backward(trip)
    m.train()
    m.pre_epoch_processing()
    loss = m.calculate_loss(dev(trip, cuda))
    loss.backward()
    print(f"loss {loss.item():.8f} vs restatement {want:.8f}")
    assert abs(loss.item() - want) <= 1e-5 * abs(want)
    for n, q in m.named_parameters():
        if g[n] is None:
            assert q.grad is None, n
            continue
        scale = float(np.abs(g[n]).max())
        print(f"  grad {n}: err {np.abs(q.grad.cpu().numpy() - g[n]).max():.3e}, scale {scale:.3e}")
        np.testing.assert_allclose(q.grad.cpu().numpy(), g[n], rtol=1e-3, atol=1e-5 * scale, err_msg=n)


def test_lattice_text_only_model(cuda, tmp_path):
    """One modality: the graph is that modality's, there is no weight, modal_weight has no gradient."""
    z, c, train, *_ = _setup(tmp_path, feats="text")
    m = _model(c, train)
    names = tuple(n for n, _ in m.named_parameters())
    assert names == tuple(n for n in R.NAMES if not n.startswith("image"))
    _one_step_vs_restatement(m, z, cuda, ("text",), "lightgcn")
    assert m.modal_weight.grad is None and m.text_trs.weight.grad is not None


def test_lattice_mf_backbone(cuda, tmp_path):
    z, c, train, *_ = _setup(tmp_path, dict(cf_model="mf"))
    m = _model(c, train)
    _one_step_vs_restatement(m, z, cuda, R.MODS, "mf")


@pytest.mark.parametrize("what", ["ngcf", "embedding_size", "feat_embed_dim", "knn_k", "no_features", "width"])
def test_lattice_unsupported_configurations_raise(cuda, tmp_path, what):
    extra, feats = {}, "both"
    if what == "ngcf":
        extra = dict(cf_model="ngcf")
    elif what == "embedding_size":
        extra = dict(embedding_size=32)
    elif what == "feat_embed_dim":
        extra = dict(feat_embed_dim=48)
    elif what == "knn_k":
        extra = dict(knn_k=33)
    elif what == "no_features":
        extra = dict(is_multimodal_model=False)
    elif what == "width":
        feats = "narrow"
    _, c, train, *_ = _setup(tmp_path, extra, feats)
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        _model(c, train)


def test_lattice_quick_start(cuda, tmp_path):
    """`main.py -m LATTICE -d <dataset>`'s path: trains an epoch and evaluates on a dataset
    directory with the .inter file and the feature files."""
    z = R.load_fixture()
    res = quick_start_case("LATTICE", tmp_path, z["v_feat"], z["t_feat"],
                           {"epochs": 1, "reg_weight": [0.001], "learning_rate": [0.001]})
    assert len(res) == 1 and "recall@20" in res[0][1]
    assert all(np.isfinite(v) for v in res[0][1].values())
