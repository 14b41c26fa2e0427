"""MMGCN on the GPU: the kernels of csrc/mmgcn.hip (rsx.mmgcn's wrappers) against the float64
restatement (tests/mmgcn_ref.py) and numpy float64, and the model (rsx.mmgcn.MMGCN) against the
reference's own run (tests/golden/mmgcn_step0_small.npz, mmgcn_small.npz).  The shared dense
blocks (the wide product, normalise, the column sum) are tests/test_gpu_dense.py's.

Kernel bound: helpers.check_vs_f32 — 1e-4 of the tensor's scale, or 4x the error the float32
torch composition of the same ops (on the CPU) makes against the same float64 values, whichever
is larger.  leaky_relu's slope is discontinuous at zero, so a test flags the rows where the
float64 run has any pre-activation within 1e-5 of that tensor's scale of zero (about 7x the
rounding of a <= 512-term float32 dot product), zeroes the upstream gradient on those rows for
kernel and restatement alike, and asserts that at most 5 % of the rows are flagged.

Every sum is in a fixed order (no float atomics): two runs are bit-equal, and the captured graph
step equals the eager one bit for bit."""
import types

import numpy as np
import pytest
import torch

import mmgcn_ref as R
from helpers import (LOSS_BATCHES, assert_same_run, check_eval, check_params, check_vs_f32, coo_sorted, csr_to_sorted, dev,
                     loaders, loss_triplets, make_model, quick_start_case, record_batches, train_epochs, unflagged,
                     write_dataset)

pytestmark = pytest.mark.gpu
SHAPES = [(64, 5), (64, 65), (128, 37), (64, 1001)]
c = lambda t: t.detach().cpu().numpy()  # noqa: E731


# ------------------------------------------------------------- the fused layer
@pytest.mark.parametrize("d,n", SHAPES)
def test_fused_layer_vs_restatement(cuda, d, n):
    from rsx import mmgcn as M

    x64 = R.layer_inputs(d, d, n, 100 + n)
    x32 = {k: v.float() for k, v in x64.items()}
    x64 = {k: v.double() for k, v in x32.items()}  # the float32 inputs, exactly
    k = {}
    out64 = R.layer(**x64, keep=k)
    keep = unflagged([k["ph"], k["pu"], k["po"]], n)
    go = torch.randn(n, d, dtype=torch.float64, generator=torch.Generator().manual_seed(7)).float().double() * keep
    ref = R.layer_backward(go, **x64)
    kt = {}
    out32 = R.layer(**x32, keep=kt)
    tor = R.layer_backward(go.float(), **x32)
    a, x = (dev(x32[s].numpy(), cuda, True) for s in ("a", "x"))
    E = dev(x32["E"].numpy(), cuda)
    W = [dev(x32[s].numpy(), cuda, True) for s in ("Wc", "Wl", "bl", "Wg", "bg")]
    h, u, _ = M.layer_fwd(a.detach(), x.detach(), E, *(w.detach() for w in W))
    check_vs_f32("h", c(h), k["h"], kt["h"])
    check_vs_f32("u", c(u), k["u"], kt["u"])
    out = M._Layer.apply(None, a, x, E, *W)
    check_vs_f32("out", c(out), out64, out32)
    out.backward(dev(go.float().numpy(), cuda))
    for name, t in (("g_a", a), ("g_x", x), ("dWc", W[0]), ("dWl", W[1]), ("dbl", W[2]), ("dWg", W[3]), ("dbg", W[4])):
        check_vs_f32(name, c(t.grad), ref[name], tor[name])


# ----------------------------------------------------------------------- loss
def _loss_case(d, mods, B, seed=3):
    rng = np.random.default_rng(seed)
    nu, ni = 70, 50
    trip = loss_triplets(rng, nu, ni, B)
    tabs = {m: (rng.standard_normal((nu + ni, d)) * 0.4).astype(np.float32) for m in mods}
    E = (rng.standard_normal((nu + ni, d)) * 0.3).astype(np.float32)
    return nu, ni, trip, tabs, E


def _run_loss(cuda, nu, trip, tabs, E, reg_weight, pref_term, result=None):
    from rsx import mmgcn as M

    t = {m: dev(a, cuda, True) for m, a in tabs.items()}
    keep = {}
    ws = M.loss_workspace(trip.shape[1], E.shape[1], cuda)
    loss = M._Loss.apply((nu, reg_weight, pref_term, dev(E, cuda), result, ws, keep), dev(trip, cuda), t.get("v"), t.get("t"))
    loss.backward()
    return loss.item(), c(keep["terms"]), {m: c(x.grad) for m, x in t.items()}


LOSS_CASES = [(mods, d, B) for B in LOSS_BATCHES for d in (64, 128) for mods in (("v", "t"), ("v",), ("t",))]


# (the cases at B = 192 keep the ids they had before the batch became a parameter)
@pytest.mark.parametrize("mods,d,B", LOSS_CASES,
                         ids=["".join(m) + f"-{d}" + ("" if B == 192 else f"-{B}") for m, d, B in LOSS_CASES])
def test_loss_value_gradients_and_result(cuda, d, mods, B):
    nu, ni, trip, tabs, E = _loss_case(d, mods, B)
    pref = np.random.default_rng(1).standard_normal((nu, 8)).astype(np.float32)
    res = {}
    for dtype in (torch.float64, torch.float32):
        T = {m: torch.from_numpy(a).to(dtype).requires_grad_(True) for m, a in tabs.items()}
        C = {"id_embedding": torch.from_numpy(E).to(dtype), "v_gcn.preference": torch.from_numpy(pref).to(dtype)}
        rep = sum(T.values()) / len(T)
        terms = R.loss(C, {m: 0 for m in mods}, rep, torch.from_numpy(trip), nu, 0.01)
        terms[0].backward()
        res[dtype] = ([float(t) for t in terms], {m: x.grad for m, x in T.items()}, rep.detach())
    (w64, g64, rep64), (w32, g32, rep32) = res[torch.float64], res[torch.float32]
    pref_term = float((pref.astype(np.float64) ** 2).mean()) if "v" in mods else 0.0
    result = torch.full((nu + ni, d), 7.0, dtype=torch.float32, device=cuda)
    loss, terms, grads = _run_loss(cuda, nu, trip, tabs, E, 0.01, pref_term, result)
    for j, name in enumerate(("loss", "bpr", "reg")):
        print(f"  {name}: {terms[j]:.8f} vs {w64[j]:.8f}")
        assert abs(terms[j] - w64[j]) <= 1e-5 * abs(w64[j]), name
    assert loss == terms[0]
    check_vs_f32("result", c(result), rep64, rep32)
    rows = np.unique(np.concatenate([trip[0], nu + trip[1], nu + trip[2]]))
    untouched = np.setdiff1d(np.arange(nu + ni), rows)
    assert untouched.size > 0
    for m in mods:
        check_vs_f32(f"g_x{m}", grads[m], g64[m], g32[m])
        assert not grads[m][untouched].any()
    # deterministic: a second run is bit-equal
    _, terms2, grads2 = _run_loss(cuda, nu, trip, tabs, E, 0.01, pref_term)
    assert np.array_equal(terms.view(np.int32), terms2.view(np.int32))
    for m in mods:
        assert np.array_equal(grads[m].view(np.int32), grads2[m].view(np.int32))


def test_loss_refuses_what_it_is_not_built_for(cuda):
    from rsx import mmgcn as M

    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        M.loss_workspace(65537, 64, cuda)
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        M.loss_workspace(512, 32, cuda)


# -------------------------------------------------------------- mean operator
def test_mean_operator_on_the_device(cuda):
    from rsx.blocks import _DevGraph
    from rsx.mmgcn import mean_operator, spmm_wide

    z = R.load("mmgcn_small.npz")
    nu, ni = int(z["n_users"]), int(z["n_items"])
    G = _DevGraph(*mean_operator(z["train_u"], z["train_i"], nu, ni), nu + ni, nu + ni, cuda, 32)
    ref = coo_sorted(z["mean_adj_idx"].astype(np.int64), z["mean_adj_val"])
    mine = csr_to_sorted(G.A.rowptr.cpu().numpy(), G.A.col.cpu().numpy(), G.A.val.cpu().numpy())
    for a, b in zip(ref, mine):
        assert np.array_equal(a, b)
    # a duplicate interaction counts twice; user 2 and item 1 (node 4) have no edge: zero rows
    G = _DevGraph(*mean_operator([0, 0, 1, 0], [0, 0, 2, 2], 3, 3), 6, 6, cuda, 32)
    A = R.mean_operator([0, 0, 1, 0], [0, 0, 2, 2], 3, 3)
    assert float(A[0, 3]) == 2 / 3 and float(A[0, 5]) == 1 / 3
    for w in (64, 32, 96):
        x = torch.from_numpy(np.random.default_rng(w).standard_normal((6, w)).astype(np.float32))
        y = c(spmm_wide(G.A, x.to(cuda)))
        check_vs_f32(f"A x, width {w}", y, A @ x.double(), A.float() @ x)
        assert not y[2].any() and not y[4].any()
        yt = c(spmm_wide(G.AT, x.to(cuda)))
        check_vs_f32(f"A^T x, width {w}", yt, A.t() @ x.double(), A.float().t() @ x)


# ---------------------------------------------------------------------- model
def _setup(tmp_path, extra=None, feats=None):
    z = R.load("mmgcn_small.npz")
    write_dataset(tmp_path, *(feats if feats is not None else (z["v_feat"], z["t_feat"])))
    cfg = dict(is_multimodal_model=True, learning_rate=[0.001], reg_weight=[0.001])
    cfg.update(extra or {})
    return (z,) + loaders("MMGCN", tmp_path, cfg)


def _model(c_, train):
    return make_model("MMGCN", c_, train)


def _consts(m):
    out = {"id_embedding": m.id_embedding, "result": m.result}
    for k in ("v", "t"):
        if hasattr(m, k + "_gcn"):
            out[f"{k}_gcn.preference"] = getattr(m, k + "_gcn").preference
    return out


def _strided(m, k):
    """The model as check_params sees it: every parameter at the fixture's row stride."""
    return types.SimpleNamespace(named_parameters=lambda: [(n, R.rows(p.detach(), k)) for n, p in m.named_parameters()])


def _check_consts(m, z):
    S = R.strides(z)
    own = {id(p) for p in m.parameters()}
    for k, v in _consts(m).items():
        assert id(v) not in own and not v.requires_grad and v.is_contiguous(), k
        if k != "result":
            assert np.array_equal(c(v)[::S["const"]].view(np.int32), z["const." + k].view(np.int32)), k


def test_mmgcn_init_and_initial_evaluation(cuda, tmp_path):
    from rsx.trainer import Trainer

    z, c_, train, valid, _ = _setup(tmp_path)
    m = _model(c_, train)
    S = R.strides(z)
    named = dict(m.named_parameters())
    assert tuple(named) == R.names()
    for n, p in named.items():
        assert np.array_equal(R.rows(c(p), S["param"]).view(np.int32), z["init." + n].view(np.int32)), n
    _check_consts(m, z)
    assert np.array_equal(c(m.result)[::S["const"]].view(np.int32), z["const.result"].view(np.int32))
    assert not any(k in m.state_dict() for k in ("id_embedding", "result", "v_gcn.preference", "t_gcn.preference"))
    ref = coo_sorted(z["mean_adj_idx"].astype(np.int64), z["mean_adj_val"])
    A = m.graph.A
    for a, b in zip(ref, csr_to_sorted(A.rowptr.cpu().numpy(), A.col.cpu().numpy(), A.val.cpu().numpy())):
        assert np.array_equal(a, b)
    # before any training the scores are those of the random `result` (mmgcn.py:56, 99-105)
    check_eval(Trainer(c_, m), m, z, (("valid", valid),), tag_prefix="init_")


def test_mmgcn_first_two_steps(cuda, tmp_path):
    z, c_, train, *_ = _setup(tmp_path)
    z0 = R.load("mmgcn_step0_small.npz")
    S = R.strides(z0)
    m = _model(c_, train)
    m.train()
    lr = c_["learning_rate"]
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    dgs, grefs = {n: [] for n in R.names()}, {n: [] for n in R.names()}
    for step in range(2):
        pre = f"step{step}_"
        opt.zero_grad()
        loss = m.calculate_loss(dev(z0[pre + "triplets"].astype(np.int64), cuda))
        loss.backward()
        terms = c(m.last_terms)
        for j, name in enumerate(("loss", "bpr", "reg")):
            want = float(z0[pre + name])
            print(f"step {step} {name} {terms[j]:.8f} vs reference {want:.8f}")
            assert abs(terms[j] - want) <= 1e-5 * abs(want), (step, name)
        assert loss.item() == terms[0]
        np.testing.assert_allclose(c(m.result)[::S["rep"]], z0[pre + "representation"], rtol=1e-5, atol=1e-6)
        mine = {n: c(p.grad).copy() for n, p in m.named_parameters()}
        assert set(mine) == set(R.names())
        if step == 0:
            for n in R.names():
                w = z0[pre + "grad." + n]
                scale = max(float(np.abs(w).max()), 1e-12)
                np.testing.assert_allclose(R.rows(mine[n], S["grad"]), w, rtol=1e-3, atol=1e-5 * scale, err_msg=n)
        opt.step()
        for n, p in m.named_parameters():
            got, want = R.rows(c(p), S["param"]), z0[pre + "param." + n]
            gref = R.rows(z0[pre + "grad." + n], S["param"] // S["grad"])
            gmine = R.rows(mine[n], S["param"])
            if step == 0:
                # Adam's first step is -lr * g / (|g| + eps): it differs from the reference's by at most
                # lr * |s(g_mine) - s(g_ref)| (plus rounding), large only where |g| is rounding noise
                sgn = lambda g: g / (np.abs(g) + 1e-8)  # noqa: E731
                bound = lr * np.abs(sgn(gmine) - sgn(gref)) + 2e-6
                assert np.all(np.abs(got - want) <= bound), n
            grefs[n].append(gref.astype(np.float64))
            dgs[n].append(gmine.astype(np.float64) - gref)
            if step == 1:
                # The second update: 1e-5 of scale plus what Adam turns the two gradient differences
                # into (grcn_ref.adam_tolerance).  Step 0's differences are pinned above (rtol 1e-3);
                # step 1 has no pre-activation margin (the capture asserts one for step 0 only), so a
                # pre-activation may sit on the other side of leaky_relu's kink here than in the
                # reference, which changes one column of that layer's conv weight gradient or one row
                # of its Linears' (max(shape) elements) by a slope ratio of 100.  An update is at most
                # about lr, so an element's check says nothing once its allowance reaches a tenth of
                # lr (|dg| / |g| of a few percent): that may happen on the rounding-noise elements
                # (1e-3 of the tensor, the CPU test's cap) plus two such rows or columns, no more.
                scale = float(np.abs(want).max())
                extra = R.adam_tolerance(dgs[n], grefs[n], lr)
                share = float((extra > 0.1 * lr).mean())
                cap = 1e-3 + 2 * (max(got.shape) if got.ndim == 2 else 1) / got.size  # (a bias: one element a flip)
                err = np.abs(got - want)
                print(f"  step 1 {n}: err {err.max():.3e}, scale {scale:.3e}, allowance above lr / 10 on {share:.4f} (cap {cap:.4f})")
                assert np.all(err <= 1e-5 * scale + extra), n
                assert share <= cap, n
    _check_consts(m, z)


def _steps(tmp_path, tag, batches, graph):
    from rsx.trainer import Trainer

    _, c_, train, *_ = _setup(tmp_path / tag, dict(rsx_graph_step=graph))
    m = _model(c_, train)
    t = Trainer(c_, m)
    m.train()
    t._gate = False
    losses = [t.train_step(b, k)[1] for k, b in enumerate(batches)]
    torch.cuda.synchronize()
    return m, [float(x) for x in losses], t


def test_mmgcn_captured_step_equals_eager(cuda, tmp_path):
    z = R.load("mmgcn_small.npz")
    trip = z["epoch0_triplets"].astype(np.int64)
    seq = [dev(trip[:, 512 * k: 512 * (k + 1)], cuda) for k in range(3)]
    a, la, ta = _steps(tmp_path, "graph", seq, True)
    b, lb, tb = _steps(tmp_path, "eager", seq, False)
    # batch 0 eager, batch 1 captured, batch 2 a replay
    assert ta._graph is not None and ta._graph.replays >= 1 and tb._graph is None
    assert_same_run(a, b, la, lb)
    assert torch.equal(a.result, b.result)


def test_mmgcn_trainer_vs_reference(cuda, tmp_path):
    from rsx.trainer import Trainer

    z, c_, train, valid, test = _setup(tmp_path)
    m = _model(c_, train)
    t = Trainer(c_, m)
    assert not t.fused and type(t.optimizer).__name__ == "RsxAdam"
    rec = record_batches(train)
    losses = train_epochs(t, m, train, 2)
    want = np.concatenate([z[f"epoch{e}_triplets"] for e in range(2)], axis=1).astype(np.int64)
    assert np.array_equal(torch.cat(rec, dim=1).numpy(), want)  # the recorded triplets
    assert t._graph is not None and t._graph.replays > 0
    print(f"epoch losses {losses} vs reference {z['epoch_losses']}")
    S = R.strides(z)
    check_params(_strided(m, S["last"]), z, "epoch1_param.", 5e-5)
    # `result` is the last training forward's, one optimiser step stale: a fresh forward scores otherwise
    check_eval(t, m, z, (("valid", valid), ("test", test)))
    _check_consts(m, z)


@pytest.mark.parametrize("only", ["v", "t"])
def test_mmgcn_one_modality_vs_restatement(cuda, tmp_path, only):
    z = R.load("mmgcn_small.npz")
    z0 = R.load("mmgcn_step0_small.npz")
    feats = (z["v_feat"], None) if only == "v" else (None, z["t_feat"])
    _, c_, train, *_ = _setup(tmp_path, feats=feats)
    m = _model(c_, train)
    assert m.num_modal == 1 and tuple(n for n, _ in m.named_parameters()) == R.names((only,))
    m.train()
    trip = z0["step0_triplets"].astype(np.int64)
    loss = m.calculate_loss(dev(trip, cuda))
    loss.backward()
    nu, ni = int(z["n_users"]), int(z["n_items"])
    res = {}
    for dtype in (torch.float64, torch.float32):
        P = R.cast({n: p.detach().cpu() for n, p in m.named_parameters()}, dtype)
        C = R.consts({k: v.cpu() for k, v in _consts(m).items() if k != "result"}, dtype)
        A = R.mean_operator(z["train_u"].astype(np.int64), z["train_i"].astype(np.int64), nu, ni, dtype)
        f = {only: torch.from_numpy(z[only + "_feat"]).to(dtype)}
        res[dtype] = R.step(P, C, f, A, torch.from_numpy(trip), nu, 0.001)
    (rep64, t64, g64), (rep32, t32, g32) = res[torch.float64], res[torch.float32]
    terms = c(m.last_terms)
    for j, name in enumerate(("loss", "bpr", "reg")):
        assert abs(terms[j] - float(t64[j])) <= 1e-5 * abs(float(t64[j])), name
    check_vs_f32("result", c(m.result), rep64, rep32)
    for n, p in m.named_parameters():
        check_vs_f32(n, c(p.grad), g64[n], g32[n])


@pytest.mark.parametrize("what", ["embedding_size", "no_features", "width", "text_width"])
def test_mmgcn_unsupported_configurations_raise(cuda, tmp_path, what):
    z = R.load("mmgcn_small.npz")
    extra, feats = {}, None
    if what == "embedding_size":
        extra = dict(embedding_size=32)
    elif what == "no_features":
        feats = (None, None)
    elif what == "width":
        feats = (z["v_feat"][:, :6], z["t_feat"])
    else:
        feats = (z["v_feat"], z["t_feat"][:, :24])
    _, c_, train, *_ = _setup(tmp_path, extra, feats)
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        _model(c_, train)


def test_mmgcn_quick_start(cuda, tmp_path):
    """`main.py -m MMGCN -d <dataset>`'s path: trains an epoch and evaluates on a dataset
    directory with the .inter file and the two feature files."""
    z = R.load("mmgcn_small.npz")
    res = quick_start_case("MMGCN", tmp_path, z["v_feat"], z["t_feat"],
                           {"epochs": 1, "learning_rate": [0.001], "reg_weight": [0.001]})
    assert len(res) == 1 and "recall@20" in res[0][1]
    assert all(np.isfinite(v) for v in res[0][1].values())
