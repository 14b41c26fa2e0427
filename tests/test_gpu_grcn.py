"""GRCN on the GPU: the kernels of csrc/grcn.hip (rsx.grcn's wrappers) against their float64
contracts (tests/grcn_kernels_ref.py), and the model (rsx.grcn.GRCN) against the reference's own
run (tests/golden/grcn_step0_small.npz, grcn_small.npz) and the restatement (tests/grcn_ref.py).

Kernel bound: helpers.check_vs_f32 — 1e-4 of the tensor's scale, or 4x the error the same
formulas make in float32 torch on the CPU against the same float64 values, whichever is larger.

The refined weight takes the larger of two products, and its gradient goes to the winner: a test
that runs the refine first asserts, on the float64 values of ITS INPUTS, that on every edge with
w > 0 the two products differ by more than 1e-4 of the larger.  A condition on the inputs; no edge
is excluded from any comparison.

Every sum is in a fixed order (no float atomics): two runs are bit-equal, and the captured graph
step equals the eager one bit for bit."""
import gc
import types
import weakref

import numpy as np
import pytest
import torch

import grcn_kernels_ref as K
import grcn_ref as R
import test_grcn_cpu as T
from helpers import (LOSS_BATCHES, assert_same_run, check_eval, check_params, check_vs_f32, dev, loaders, loss_triplets,
                     make_model, quick_start_case, record_batches, train_epochs, write_dataset)

pytestmark = pytest.mark.gpu
NAMES = T.NAMES
c = lambda t: t.detach().cpu().numpy()  # noqa: E731
_cache = {}


# ------------------------------------------------------------------ the two graphs
def _hub_edges(H):
    """40 items, 3 H + 105 users: item 0 with 3 H + 5 in-edges (user 0 twice), item 1 with H + 1,
    item 2 with exactly H; the users H + 1 .. 3 H + 3 have item 0 alone (alpha = 1); the last user
    and item 39 are isolated; the rest interact with items 3 .. 38."""
    nu, ni = 3 * H + 105, 40
    rng = np.random.default_rng(11)
    u = [np.arange(3 * H + 4), [0], np.arange(H + 1), np.arange(H)]
    i = [np.zeros(3 * H + 4), [0], np.ones(H + 1), np.full(H, 2)]
    for user in range(3 * H + 4, nu - 1):
        k = int(rng.integers(1, 5))
        u.append(np.full(k, user))
        i.append(rng.choice(np.arange(3, 39), k, replace=False))
    u, i = np.concatenate(u).astype(np.int64), np.concatenate(i).astype(np.int64)
    perm = rng.permutation(u.size)
    return u[perm], i[perm], nu, ni


def _graphs(cuda):
    """{name: (EdgeGraph on the device, K.Graph, n_users)}, built once."""
    if "graphs" not in _cache:
        from rsx import _lib as L
        from rsx.grcn import EdgeGraph, target_csr

        H = int(L.lib().rsx_grcn_hub_degree())
        z = T.load("grcn_small.npz")
        out = {}
        for name, (u, i, nu, ni) in (("fixture", (z["train_u"], z["train_i"], int(z["n_users"]), int(z["n_items"]))),
                                     ("hub", _hub_edges(H))):
            s = target_csr(u, i, nu, ni)
            out[name] = (EdgeGraph(*s, cuda), K.Graph(*s[:3]), nu)
        deg = np.diff(out["hub"][1].rowptr.numpy())
        nu = out["hub"][2]
        assert (deg[nu], deg[nu + 1], deg[nu + 2]) == (3 * H + 5, H + 1, H) and deg[nu + 39] == 0 and deg[nu - 1] == 0
        assert np.all(deg[H + 1: 3 * H + 4] == 1) and out["fixture"][1].nnz == 6044
        _cache["graphs"] = out
    return _cache["graphs"]


def _unit(n, d, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.normalize(torch.randn(n, d, dtype=torch.float64, generator=g)) * scale
    return x.float()


def _randn(shape, seed, scale=1.0):
    return (torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)) * scale).float()


GRAPHS = ["fixture", "hub"]


# ------------------------------------------------------------------ attention
@pytest.mark.parametrize("norm", [1.0, 10.0])
@pytest.mark.parametrize("dc", [64, 128])
@pytest.mark.parametrize("graph", GRAPHS)
def test_attention_forward_and_backward(cuda, graph, dc, norm):
    from rsx import grcn as G

    g, kg, nu = _graphs(cuda)[graph]
    x = _unit(kg.n, dc, 5 + dc, norm)
    g_rep, dext = _randn((kg.n, dc), 6), _randn((kg.nnz,), 7)
    a64, rep64 = K.attn_fwd(kg, x.double())
    a32, rep32 = K.attn_fwd(kg, x)
    assert norm == 1.0 or float((x.double() ** 2).sum(1).max()) > 99  # scores reach 100: the max must be subtracted
    X = dev(x.numpy(), cuda)
    alpha, rep = G.attn_fwd(g, X)
    check_vs_f32("alpha", c(alpha), a64, a32)
    check_vs_f32("rep", c(rep), rep64, rep32)
    deg = np.diff(kg.rowptr.numpy())
    single = np.nonzero(deg == 1)[0]
    assert single.size and np.all(c(alpha)[kg.rowptr.numpy()[single]] == 1.0)  # one in-edge: alpha = 1
    lone = np.nonzero(deg == 0)[0]
    assert graph == "fixture" or lone.size >= 2
    assert torch.equal(rep[lone], X[lone])  # no in-edge: rep = x
    sums = np.add.reduceat(c(alpha).astype(np.float64), kg.rowptr.numpy()[:-1][deg > 0])
    assert np.abs(sums - 1).max() < 1e-5
    dx64 = K.attn_bwd(kg, g_rep.double(), dext.double(), x.double(), a64)
    dx32 = K.attn_bwd(kg, g_rep, dext, x, a32)
    Gd, Dd = dev(g_rep.numpy(), cuda), dev(dext.numpy(), cuda)
    dx = G.attn_bwd(g, Gd, Dd, X, alpha)
    check_vs_f32("dx", c(dx), dx64, dx32)
    # deterministic: a second run is bit-equal
    alpha2, rep2 = G.attn_fwd(g, X)
    assert torch.equal(alpha, alpha2) and torch.equal(rep, rep2) and torch.equal(dx, G.attn_bwd(g, Gd, Dd, X, alpha))


# ------------------------------------------------------------------ refine, SDDMM
def _refine_inputs(kg, dc, seed):
    """(alphas float32 [2 x nnz], conf float32 [n, 2]) with the gap condition asserted on their float64 values."""
    alphas = [K.attn_fwd(kg, _unit(kg.n, dc, seed + m))[0] for m in range(2)]
    conf = _randn((kg.n, 2), seed + 2, (2.0 / (kg.n + 2)) ** 0.5)
    gap = K.min_relative_gap(kg, [a.double() for a in alphas], conf.double())
    print(f"  smallest relative gap of the two products on edges with w > 0: {gap:.3e}")
    assert gap > 1e-4
    return alphas, conf


@pytest.mark.parametrize("graph", GRAPHS)
def test_refine_forward_and_backward(cuda, graph):
    from rsx import grcn as G

    g, kg, nu = _graphs(cuda)[graph]
    alphas, conf = _refine_inputs(kg, 64, 20)
    dw = _randn((kg.nnz,), 23)
    A, Cf, DW = [dev(a.numpy(), cuda) for a in alphas], dev(conf.numpy(), cuda), dev(dw.numpy(), cuda)
    for M in (2, 1):
        a_, cf_ = alphas[:M], conf[:, :M].contiguous()
        A_, Cf_ = A[:M], Cf[:, :M].contiguous()
        v64, vT64 = K.refine_fwd(kg, [a.double() for a in a_], cf_.double())
        v32, vT32 = K.refine_fwd(kg, a_, cf_)
        val = G.refine_fwd(g, A_, Cf_)
        check_vs_f32(f"val (M={M})", c(val), v64, v32)
        check_vs_f32(f"valT (M={M})", c(g.valT), vT64, vT32)
        assert torch.equal(g.valT[g.rev.long()], val)
        assert np.array_equal(c(val) > 0, v64.numpy() > 0) and 0.05 < float((val > 0).float().mean()) < 0.95
        das64, dc64 = K.refine_bwd(kg, [a.double() for a in a_], cf_.double(), dw.double())
        das32, dc32 = K.refine_bwd(kg, a_, cf_, dw)
        das, dconf = G.refine_bwd(g, A_, Cf_, DW)
        check_vs_f32(f"dconf (M={M})", c(dconf), dc64, dc32)
        for m in range(M):
            check_vs_f32(f"dalpha_{m} (M={M})", c(das[m]), das64[m], das32[m])
        first = val.clone()
        das2, dconf2 = G.refine_bwd(g, A_, Cf_, DW)
        assert torch.equal(G.refine_fwd(g, A_, Cf_), first) and torch.equal(dconf, dconf2)
        assert all(torch.equal(a, b) for a, b in zip(das, das2))


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("graph", GRAPHS)
def test_edge_dots(cuda, graph, d):
    from rsx import grcn as G

    g, kg, nu = _graphs(cuda)[graph]
    t = [_randn((kg.n, d), 30 + k, 0.5) for k in range(4)]
    want64 = K.edge_dots(kg, *(x.double() for x in t))
    want32 = K.edge_dots(kg, *t)
    T_ = [dev(x.numpy(), cuda) for x in t]
    dw = G.edge_dots(g, *T_)
    check_vs_f32("dw", c(dw), want64, want32)
    assert torch.equal(dw, G.edge_dots(g, *T_))


def test_kernels_refuse_what_they_are_not_built_for(cuda):
    from rsx import grcn as G

    g, kg, nu = _graphs(cuda)["fixture"]
    x32 = dev(_unit(kg.n, 32, 1).numpy(), cuda)
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):
        G.attn_fwd(g, x32)
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):
        G.edge_dots(g, x32, x32, x32, x32)
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):
        G.attn_bwd(g, x32, None, x32, g.alpha[0])
    a = [torch.zeros(kg.nnz, device=cuda)] * 3
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):
        G.refine_fwd(g, a, torch.zeros(kg.n, 3, device=cuda))
    with pytest.raises(RuntimeError, match="grcn:"):  # a table of another graph's size never reaches a launch
        G.attn_fwd(g, dev(_unit(kg.n - 1, 64, 1).numpy(), cuda))
    with pytest.raises(RuntimeError, match="grcn:"):
        G.refine_fwd(g, [torch.zeros(kg.nnz - 1, device=cuda)], torch.zeros(kg.n, 1, device=cuda))
    for batch, width in ((65537, 192), (512, 320), (512, 64), (512, 160)):
        assert G.loss_ws_bytes(batch, width) == 0
        with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
            G.loss_workspace(batch, width, cuda)


# ------------------------------------------------------------------ the chain of a step
@pytest.mark.parametrize("dc,M", [(64, 2), (128, 1)])
def test_step_chain_on_the_hub_graph(cuda, dc, M):
    """_Step (every kernel of a step, forward and backward) from given x_m, conf, normalize(E) on the
    hub graph against the chained contracts: two modalities at dc = 64, the image alone at 128."""
    from rsx import grcn as G

    g, kg, nu = _graphs(cuda)["hub"]
    dx = 64
    xs = [_unit(kg.n, dc, 40 + m) for m in range(M)]
    conf = _randn((kg.n, M), 42, (2.0 / (kg.n + 2)) ** 0.5)
    xn, E = _unit(kg.n, dx, 43), _randn((kg.n, dx), 44, 0.1)
    prefs = [_randn((nu, dc), 45 + m, 0.1) for m in range(M)]
    gap = K.min_relative_gap(kg, [K.attn_fwd(kg, x.double())[0] for x in xs], conf.double())
    print(f"  smallest relative gap: {gap:.3e}")
    assert gap > 1e-4
    rng = np.random.default_rng(4)
    B = 256
    trip = np.stack([rng.integers(0, nu, B), rng.integers(0, 40, B), rng.integers(0, 40, B)]).astype(np.int64)
    trip[0, :40], trip[1, 20:80] = 0, 0  # the hub's user and item, repeated
    trip_t = torch.from_numpy(trip)
    keys = ("x_v", "x_t")[:M] + ("conf", "xn", "E") + ("pv", "pt")[:M]

    def chain(dtype):
        x_, cf, xn_, E_, p_ = [x.to(dtype) for x in xs], conf.to(dtype), xn.to(dtype), E.to(dtype), [p.to(dtype) for p in prefs]
        al, reps = zip(*(K.attn_fwd(kg, x) for x in x_))
        val, valT = K.refine_fwd(kg, list(al), cf)
        h1, id_rep = K.id_gcn_fwd(kg, val, xn_)
        terms, rep = K.loss_fwd(id_rep, list(reps), E_, p_, trip_t, nu, 0.01)
        Gi, g_reps, gE, gp = K.loss_bwd(id_rep, list(reps), E_, p_, trip_t, nu, 0.01)
        dxn, dw = K.id_gcn_bwd(kg, val, valT, Gi, h1, xn_)
        das, dconf = K.refine_bwd(kg, list(al), cf, dw)
        dxs = [K.attn_bwd(kg, g_reps[m], das[m], x_[m], al[m]) for m in range(M)]
        return dict(zip(keys, (*dxs, dconf, dxn, gE, *gp)), terms=terms, rep=rep)

    r64, r32 = chain(torch.float64), chain(torch.float32)
    leaves = dict(zip(keys, (dev(v.numpy(), cuda, True) for v in (*xs, conf, xn, E, *prefs))))
    result = torch.zeros(kg.n, 256, device=cuda)
    keep = {}
    W = dx + M * dc
    loss = G._Step.apply((g, nu, 0.01, result, G.loss_workspace(B, W, cuda), keep), dev(trip, cuda),
                         *(leaves.get(k) for k in ("x_v", "x_t", "conf", "xn", "E", "pv", "pt")))
    loss.backward()
    terms = c(keep["terms"])
    for j, name in enumerate(("loss", "bpr", "reg")):
        print(f"  {name}: {terms[j]:.8f} vs {float(r64['terms'][j]):.8f}")
        assert abs(terms[j] - float(r64["terms"][j])) <= 1e-5 * abs(float(r64["terms"][j])), name
    check_vs_f32("result", c(result)[:, :W], r64["rep"], r32["rep"])
    assert not result[:, W:].any()
    for k, t in leaves.items():
        check_vs_f32("grad " + k, c(t.grad), r64[k], r32[k])


# ----------------------------------------------------------------------- loss
LOSS_SHAPES = [(64, 64, 2, 256), (64, 64, 1, 128), (64, 64, 1, 256), (128, 64, 2, 256), (64, 128, 1, 256)]


LOSS_CASES = [s + (B,) for B in LOSS_BATCHES for s in LOSS_SHAPES]


# (the cases at B = 192 keep the ids they had before the batch became a parameter)
@pytest.mark.parametrize("dx,dc,M,ld,B", LOSS_CASES,
                         ids=["-".join(map(str, k[:4] if k[4] == 192 else k)) for k in LOSS_CASES])
def test_loss_value_gradients_and_result(cuda, dx, dc, M, ld, B):
    from rsx import grcn as G

    rng = np.random.default_rng(3)
    nu, ni = 70, 50
    trip = loss_triplets(rng, nu, ni, B)
    n = nu + ni
    f32 = lambda shape, s: (rng.standard_normal(shape) * s).astype(np.float32)  # noqa: E731
    tabs = dict(id=f32((n, dx), 0.4), E=f32((n, dx), 0.3))
    for m in range(M):
        tabs[f"rep{m}"], tabs[f"pref{m}"] = f32((n, dc), 0.4), f32((nu, dc), 0.3)
    W = dx + M * dc

    def run(dtype):
        t = {k: torch.from_numpy(v).to(dtype) for k, v in tabs.items()}
        reps, prefs = [t[f"rep{m}"] for m in range(M)], [t[f"pref{m}"] for m in range(M)]
        terms, rep = K.loss_fwd(t["id"], reps, t["E"], prefs, torch.from_numpy(trip), nu, 0.01)
        Gi, g_reps, gE, gp = K.loss_bwd(t["id"], reps, t["E"], prefs, torch.from_numpy(trip), nu, 0.01, go=0.5)
        out = dict(terms=terms, rep=rep, id=Gi, E=gE)
        for m in range(M):
            out[f"rep{m}"], out[f"pref{m}"] = g_reps[m], gp[m]
        return out

    r64, r32 = run(torch.float64), run(torch.float32)
    # the contract's own loss against autograd of the restatement's
    P = {"id_gcn.id_embedding": torch.from_numpy(tabs["E"]).double(), "v_gcn.preference": torch.from_numpy(tabs["pref0"]).double()}
    if M == 2:
        P["t_gcn.preference"] = torch.from_numpy(tabs["pref1"]).double()
    want = R.loss(P, {m: 0 for m in ("v", "t")[:M]}, r64["rep"], torch.from_numpy(trip), nu, 0.01)
    assert all(abs(float(a) - float(b)) <= 1e-12 for a, b in zip(want, r64["terms"]))
    d = {k: dev(v, cuda) for k, v in tabs.items()}
    trip_d = dev(trip, cuda)  # (the argument struct holds addresses: the tensors must outlive it)
    a = G.loss_args(d["id"], d["rep0"], d.get("rep1"), d["E"], d["pref0"], d.get("pref1"), trip_d, nu, 0.01)
    ws = G.loss_workspace(B, W, cuda)
    out = torch.empty(3, device=cuda)
    result = torch.full((n, ld), 7.0, device=cuda)
    G.loss_fwd(a, out, result, ws)
    terms = c(out)
    for j, name in enumerate(("loss", "bpr", "reg")):
        print(f"  {name}: {terms[j]:.8f} vs {float(r64['terms'][j]):.8f}")
        assert abs(terms[j] - float(r64["terms"][j])) <= 1e-5 * abs(float(r64["terms"][j])), name
    check_vs_f32("result", c(result)[:, :W], r64["rep"], r32["rep"])
    assert torch.all(result[:, W:] == 7.0)  # the padding columns are left alone
    go = torch.full((), 0.5, device=cuda)
    grads = G.loss_bwd(a, go, d["id"], d["rep0"], d.get("rep1"), d["pref0"], ws)
    names = ("id", "rep0", "rep1", "E", "pref0", "pref1")
    rows = np.unique(np.concatenate([trip[0], nu + trip[1], nu + trip[2]]))
    untouched = np.setdiff1d(np.arange(n), rows)
    assert untouched.size > 0
    for name, t in zip(names, grads):
        if t is None:
            assert name not in r64
            continue
        check_vs_f32("g_" + name, c(t), r64[name], r32[name])
        if name != "pref0":  # (the whole-table term reaches every row of pref_v)
            assert not c(t)[untouched[untouched < t.shape[0]]].any(), name
    grads2 = G.loss_bwd(a, go, d["id"], d["rep0"], d.get("rep1"), d["pref0"], ws)
    out2 = torch.empty(3, device=cuda)
    G.loss_fwd(a, out2, None, ws)
    assert torch.equal(out, out2) and all(x is None or torch.equal(x, y) for x, y in zip(grads, grads2))


# ---------------------------------------------------------------------- model
def _setup(tmp_path, extra=None, feats=None):
    z = T.load("grcn_small.npz")
    write_dataset(tmp_path, *(feats if feats is not None else (z["v_feat"], z["t_feat"])))
    cfg = dict(is_multimodal_model=True, learning_rate=[0.001], reg_weight=[0.001])
    cfg.update(extra or {})
    return (z,) + loaders("GRCN", tmp_path, cfg)


def _model(c_, train):
    return make_model("GRCN", c_, train)


def _fixture_slots(z):
    """target_csr of the fixture's edges in the reference's own order: its edge_slot carries the
    fixture's [2 E] arrays to slots."""
    from rsx.grcn import target_csr

    s = target_csr(z["train_u"], z["train_i"], int(z["n_users"]), int(z["n_items"]))
    key = np.repeat(np.arange(s[0].size - 1), np.diff(s[0])) * 600 + s[1]
    assert np.all(np.diff(key) > 0)  # no interaction repeats
    return s


def _strided(m, k):
    """The model as check_params sees it: the tables at the fixture's row stride."""
    return types.SimpleNamespace(named_parameters=lambda: [(n, T.rows(p.detach(), n, k)) for n, p in m.named_parameters()])


def test_grcn_init_and_initial_evaluation(cuda, tmp_path):
    from rsx.trainer import Trainer

    z, c_, train, valid, _ = _setup(tmp_path)
    m = _model(c_, train)
    named = dict(m.named_parameters())
    assert tuple(named) == NAMES
    for n, p in named.items():
        assert np.array_equal(c(p).view(np.int32), z["init." + n].view(np.int32)), n
    assert m.result.shape == (600, 64) and np.array_equal(c(m.result).view(np.int32), z["init.result"].view(np.int32))
    assert m._result.shape == (600, 256) and not m._result[:, 64:].any()
    assert "result" not in m.state_dict() and "_result" not in m.state_dict()
    # the model's graph is the fixture's (the loader lists the interactions in another order than the
    # reference's edge_index; no interaction repeats, so the slots are the same)
    g = m.graph
    rowptr, col, rev, _ = _fixture_slots(z)
    assert np.array_equal(c(g.rowptr), rowptr) and np.array_equal(c(g.col), col) and np.array_equal(c(g.rev), rev)
    assert np.array_equal(np.sort(c(m.edge_slot)), np.arange(g.nnz))
    # before any training the scores are those of the random `result` (grcn.py:214, 335-341)
    check_eval(Trainer(c_, m), m, z, (("valid", valid),), tag_prefix="init_")


def test_grcn_first_two_steps(cuda, tmp_path):
    z, c_, train, *_ = _setup(tmp_path)
    z0 = T.load("grcn_step0_small.npz")
    S = T.strides(z0)
    m = _model(c_, train)
    m.train()
    lr = c_["learning_rate"]
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    dgs, grefs = {n: [] for n in NAMES}, {n: [] for n in NAMES}
    slot = _fixture_slots(z)[3]
    k = S["param"] // S["grad"]
    for step in range(2):
        pre = f"step{step}_"
        opt.zero_grad()
        loss = m.calculate_loss(dev(z0[pre + "triplets"].astype(np.int64), cuda))
        loss.backward()
        for name, got in (("alpha_v", m.alpha_v), ("alpha_t", m.alpha_t), ("weight", m.edge_weight)):
            T.close(c(got)[slot], z0[pre + name])
        terms = c(m.last_terms)
        for j, name in enumerate(("loss", "bpr", "reg")):
            want = float(z0[pre + name])
            print(f"step {step} {name} {terms[j]:.8f} vs reference {want:.8f}")
            assert abs(terms[j] - want) <= 1e-5 * abs(want), (step, name)
        assert loss.item() == terms[0]
        assert m.result.shape == (600, 192)
        np.testing.assert_allclose(c(m.result)[::S["rep"]], z0[pre + "representation"], rtol=1e-5, atol=1e-6)
        mine = {n: c(p.grad).copy() for n, p in m.named_parameters()}
        assert set(mine) == set(NAMES)
        if step == 0:
            for n in NAMES:
                w = z0[pre + "grad." + n]
                scale = max(float(np.abs(w).max()), 1e-12)
                np.testing.assert_allclose(T.rows(mine[n], n, S["grad"]), w, rtol=1e-3, atol=1e-5 * scale, err_msg=n)
        opt.step()
        for n, p in m.named_parameters():
            got, want = T.rows(c(p), n, S["param"]).astype(np.float64), z0[pre + "param." + n].astype(np.float64)
            gref = T.rows(z0[pre + "grad." + n].astype(np.float64), n, k)
            grefs[n].append(gref)
            dgs[n].append(T.rows(mine[n], n, S["param"]).astype(np.float64) - gref)
            # test_grcn_cpu's bound: 1e-5 of scale plus what Adam turns the gradient differences into,
            # and that allowance above 1e-5 of scale on fewer than 1e-3 of the elements
            scale = float(np.abs(want).max())
            extra = R.adam_tolerance(dgs[n], grefs[n], lr)
            err = np.abs(got - want)
            share = float((extra > 1e-5 * scale).mean())
            print(f"  step {step} param {n}: err {err.max():.3e}, scale {scale:.3e}, Adam term above 1e-5 of scale on {share:.4f}")
            assert np.all(err <= 1e-5 * scale + extra), (step, n, float((err - 1e-5 * scale - extra).max()))
            assert share < 1e-3, (step, n, share)


def test_no_autograd_node_outlives_its_step(cuda, tmp_path):
    """Eager, before any capture: with the collector off, every autograd node reachable from the
    loss is dead once backward has run and the loss is dropped.  A Function that keeps its own
    output on ctx (ctx -> output -> grad_fn -> ctx) fails this; save_for_backward passes."""
    z, c_, train, *_ = _setup(tmp_path)
    z0 = T.load("grcn_step0_small.npz")
    m = _model(c_, train)
    m.train()
    trip = dev(z0["step0_triplets"].astype(np.int64), cuda)
    gc.collect()
    on = gc.isenabled()
    gc.disable()
    try:
        loss = m.calculate_loss(trip)
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
        # (the nodes of torch's own ops take no weak reference; the Functions' nodes, which are their ctx, do)
        assert all(any(k in s for s in names) for k in ("_Step", "_Normalize", "_Gemm")), names
        loss.backward()
        del loss
        m.last_terms = None
        alive = [s for r, s in zip(refs, names) if r() is not None]
        assert not alive, alive
    finally:
        if on:
            gc.enable()


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


def test_grcn_captured_step_equals_eager(cuda, tmp_path):
    z = T.load("grcn_small.npz")
    trip = z["epoch0_triplets"].astype(np.int64)
    seq = [dev(trip[:, 512 * k: 512 * (k + 1)], cuda) for k in range(3)]
    a, la, ta = _steps(tmp_path, "graph", seq, True)
    b, lb, tb = _steps(tmp_path, "eager", seq, False)
    # batch 0 eager, batch 1 captured, batch 2 a replay
    assert ta._graph is not None and ta._graph.replays >= 1 and tb._graph is None
    assert_same_run(a, b, la, lb)
    assert torch.equal(a.result, b.result)
    assert torch.equal(a.alpha_v, b.alpha_v) and torch.equal(a.edge_weight, b.edge_weight)


def test_grcn_trainer_vs_reference(cuda, tmp_path):
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
    check_params(_strided(m, T.strides(z)["last"]), z, "epoch1_param.", 5e-5)
    # `result` is the last training forward's, one optimiser step stale: a fresh forward scores otherwise
    check_eval(t, m, z, (("valid", valid), ("test", test)))
    assert not torch.equal(m.forward(), m.result)


def test_grcn_image_alone_vs_restatement(cuda, tmp_path):
    """One modality: no argmax exists.  Loss words, `result` and every gradient against the
    restatement in float64 / float32 on the model's own initial parameters."""
    z = T.load("grcn_small.npz")
    z0 = T.load("grcn_step0_small.npz")
    _, c_, train, *_ = _setup(tmp_path, feats=(z["v_feat"], None))
    m = _model(c_, train)
    names = tuple(n for n in NAMES if not n.startswith("t_gcn"))
    assert m.num_modal == 1 and tuple(n for n, _ in m.named_parameters()) == names and m.alpha_t is None
    assert m.model_specific_conf.shape == (600, 1) and m._result.shape == (600, 128)
    m.train()
    trip = z0["step0_triplets"].astype(np.int64)
    loss = m.calculate_loss(dev(trip, cuda))
    loss.backward()
    nu = int(z["n_users"])
    ei = R.edge_index(z["train_u"].astype(np.int64), z["train_i"].astype(np.int64), nu)
    res = {}
    for dtype in (torch.float64, torch.float32):
        P = R.cast({n: p.detach().cpu() for n, p in m.named_parameters()}, dtype)
        f = {"v": torch.from_numpy(z["v_feat"]).to(dtype)}
        res[dtype] = R.step(P, f, ei, torch.from_numpy(trip), nu, 3, 0.001)
    (fw64, t64, g64), (fw32, t32, g32) = res[torch.float64], res[torch.float32]
    terms = c(m.last_terms)
    for j, name in enumerate(("loss", "bpr", "reg")):
        assert abs(terms[j] - float(t64[j])) <= 1e-5 * abs(float(t64[j])), name
    check_vs_f32("result", c(m.result), fw64["representation"].detach(), fw32["representation"].detach())
    check_vs_f32("forward()", c(m.forward()), fw64["representation"].detach(), fw32["representation"].detach())
    slot = _fixture_slots(z)[3]
    check_vs_f32("alpha_v", c(m.alpha_v)[slot], fw64["alphas"][0].detach(), fw32["alphas"][0].detach())
    check_vs_f32("weight", c(m.edge_weight)[slot], fw64["weight"].detach(), fw32["weight"].detach())
    for n, p in m.named_parameters():
        check_vs_f32(n, c(p.grad), g64[n], g32[n])


@pytest.mark.parametrize("what", ["embedding_size", "latent_embedding", "too_wide", "no_features", "text_alone",
                                  "width", "n_layers"])
def test_grcn_unsupported_configurations_raise(cuda, tmp_path, what):
    z = T.load("grcn_small.npz")
    extra, feats = {}, None
    if what == "embedding_size":
        extra = dict(embedding_size=32)
    elif what == "latent_embedding":
        extra = dict(latent_embedding=256)
    elif what == "too_wide":
        extra = dict(embedding_size=128, latent_embedding=128)
    elif what == "no_features":
        feats = (None, None)
    elif what == "text_alone":
        feats = (None, z["t_feat"])
    elif what == "width":
        feats = (z["v_feat"][:, :6], z["t_feat"])
    else:
        extra = dict(n_layers=-1)
    _, c_, train, *_ = _setup(tmp_path, extra, feats)
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        _model(c_, train)


def test_grcn_quick_start(cuda, tmp_path):
    """`main.py -m GRCN -d <dataset>`'s path: trains an epoch and evaluates on a dataset
    directory with the .inter file and the two feature files."""
    z = T.load("grcn_small.npz")
    res = quick_start_case("GRCN", tmp_path, z["v_feat"], z["t_feat"],
                           {"epochs": 1, "learning_rate": [0.001], "reg_weight": [0.001]})
    assert len(res) == 1 and "recall@20" in res[0][1]
    assert all(np.isfinite(v) for v in res[0][1].values())
