"""DualGNN without a GPU: the user graph (loader, builder, sampler) and the float64 restatement
(tests/dualgnn_ref.py) against the reference's own run (tests/golden/dualgnn_step0_small.npz,
dualgnn_small.npz), the initial draws, the in-place alias, the hand-derived backward of the mix
and the user graph, the one-modality forms, configuration and refusals."""
import os
import pickle
import types

import numpy as np
import pytest
import torch

import dualgnn_ref as R
from test_mmgcn_cpu import close

NAMES = R.names()


def flat2(a):
    return a.reshape(a.shape[0], -1) if a.ndim > 2 else a


def init(z):
    """(P float32 by name, result_embed float64) of seed 999 through the model's own draws."""
    from rsx.dualgnn import dualgnn_init
    from rsx.utils import init_seed

    init_seed(999)
    host = torch.nn.Module()
    result = dualgnn_init(host, int(z["n_users"]), int(z["n_items"]), 64, z["v_feat"].shape[1], z["t_feat"].shape[1])
    return {n: p.detach() for n, p in host.named_parameters()}, result


def graph_of(z):
    from rsx.dualgnn import UserGraph

    return UserGraph(z["ug_ptr"], z["ug_nbr"], z["ug_cnt"])


def setup(dtype=torch.float64):
    z0, z = R.load("dualgnn_step0_small.npz"), R.load("dualgnn_small.npz")
    nu, ni = int(z["n_users"]), int(z["n_items"])
    P = R.cast(init(z)[0], dtype)
    feats = {"v": torch.from_numpy(z["v_feat"]).to(dtype), "t": torch.from_numpy(z["t_feat"]).to(dtype)}
    A = R.sym_operator(z["train_u"].astype(np.int64), z["train_i"].astype(np.int64), nu, ni, dtype)
    idx, W = z["epoch0_idx"].astype(np.int64), torch.from_numpy(z["epoch0_W"]).to(dtype)
    return z0, z, nu, P, feats, A, idx, W


def test_fixture_sizes_hparams_and_margin():
    for f in ("dualgnn_small.npz", "dualgnn_step0_small.npz"):
        assert os.path.getsize(os.path.join(R.GOLD, f)) < (1 << 20), f
    z0, z = R.load("dualgnn_step0_small.npz"), R.load("dualgnn_small.npz")
    hp = R.hparams(z0)
    assert float(hp["learning_rate"]) == 0.001 and float(hp["reg_weight"]) == 0.001 and int(hp["seed"]) == 999
    assert (int(hp["embedding_size"]), int(hp["n_layers"])) == (64, 2)
    assert (int(z["n_users"]), int(z["n_items"]), z["train_u"].size) == (400, 200, 3022)
    assert (z["v_feat"].shape[1], z["t_feat"].shape[1]) == (48, 32)
    keys = [k for k in z0.files if k.startswith("step0_preact_min.")]
    assert len(keys) == 2
    for k in keys:
        assert float(z0[k]) > float(z0[k.replace("_min.", "_thr.")]) > 0, k
    # the graph exercises the padding draws and the generator's cut; no list is empty
    length = np.diff(z["ug_ptr"])
    assert int((length < 40).sum()) == 13 and int((length == 200).sum()) >= 262 and length.min() > 0
    assert int(z["ug_cnt"].max()) == 12
    assert tuple(z0["no_grad"]) == R.UNUSED


def test_initial_draws_follow_the_reference():
    z = R.load("dualgnn_small.npz")
    S = R.strides(z)
    P, result = init(z)
    assert tuple(P) == NAMES
    for n in NAMES:
        got = R.rows(flat2(P[n].numpy()), S["param"])
        assert np.array_equal(got.view(np.int32), z["init." + n].view(np.int32)), n
    assert result.dtype == torch.float64
    got = result.to(torch.float32).numpy()[::S["const"]]
    assert np.array_equal(got.view(np.int32), z["const.result_embed"].view(np.int32))
    w = P["weight_u"]
    assert w.shape == (400, 2, 1) and torch.allclose(w.sum(1), torch.ones(400, 1))


def test_sampler_reproduces_both_epochs(tmp_path):
    """topk_sample on the fixture's lists after the constructor's draws gives epoch 0's lists and
    weights exactly; after the loader's epoch of draws, epoch 1's."""
    from helpers import loaders, write_dataset
    from rsx.dualgnn import topk_sample
    from rsx.utils import init_seed

    z = R.load("dualgnn_small.npz")
    write_dataset(tmp_path, z["v_feat"], z["t_feat"])
    c, train, _, _ = loaders("DualGNN", tmp_path, dict(use_gpu=False, learning_rate=0.001, reg_weight=0.001))
    g = graph_of(z)
    init_seed(c["seed"])
    train.pretrain_setup()
    from rsx.dualgnn import dualgnn_init

    dualgnn_init(torch.nn.Module(), 400, 200, 64, 48, 32)
    for epoch in range(2):
        idx, W = topk_sample(g, 40)
        assert idx.dtype == np.int32 and W.dtype == np.float32 and idx.shape == W.shape == (400, 40)
        assert np.array_equal(idx, z[f"epoch{epoch}_idx"].astype(np.int32)), epoch
        assert np.array_equal(W.view(np.int32), z[f"epoch{epoch}_W"].view(np.int32)), epoch
        n = sum(1 for _ in train)
        assert n == int(z[f"epoch{epoch}_nbatch"])
    assert not np.array_equal(z["epoch0_idx"], z["epoch1_idx"])  # the padding draws moved on


def test_sampler_equals_the_literal_loop_and_edge_rows():
    from rsx.dualgnn import UserGraph, topk_sample

    rng = np.random.default_rng(3)
    lens = [0, 3, 39, 40, 41, 200, 1, 0]
    nbr = [rng.integers(0, 8, n) for n in lens]
    cnt = [np.sort(rng.integers(1, 6, n))[::-1].astype(np.float32) for n in lens]
    ptr = np.concatenate([[0], np.cumsum(lens)])
    g = UserGraph(ptr, np.concatenate(nbr), np.concatenate(cnt))
    np.random.seed(5)
    idx, W = topk_sample(g, 40)
    np.random.seed(5)
    ridx, rW = R.topk_sample_ref(R.lists_of(g.ptr, g.nbr, g.cnt), 40)
    assert np.array_equal(idx, ridx) and np.array_equal(W.view(np.int32), rW.view(np.int32))
    # an empty list: index row [0] * 40 and an all-zero weight row
    for u in (0, 7):
        assert not idx[u].any() and not W[u].any()
    # three neighbours: 40 entries, the first three the list, the rest drawn from it
    assert np.array_equal(idx[1, :3], nbr[1]) and set(idx[1]) <= set(nbr[1].tolist())
    assert abs(float(W[1].sum()) - 1.0) < 1e-6 and np.array_equal(idx[5], nbr[5][:40])


def test_loader_round_trip_and_refusals(tmp_path):
    from rsx.dualgnn import load_user_graph

    z = R.load("dualgnn_small.npz")
    g = graph_of(z)
    d = R.lists_of(g.ptr, g.nbr, g.cnt)
    path = str(tmp_path / "user_graph_dict.npy")
    np.save(path, d, allow_pickle=True)
    got = load_user_graph(path, 400)
    assert got is not None and got.nbr.dtype == np.int32 and got.cnt.dtype == np.float32
    assert np.array_equal(got.ptr, g.ptr) and np.array_equal(got.nbr, g.nbr) and np.array_equal(got.cnt, g.cnt)
    assert load_user_graph(path, 399) is None  # not a dict of n_users lists
    assert load_user_graph(str(tmp_path / "absent.npy"), 400) is None
    # a pickle that names any other global is refused, not executed
    raw = open(path, "rb").read()
    with open(path, "rb") as f:
        np.lib.format.read_magic(f)
        np.lib.format.read_array_header_1_0(f)
        head = f.tell()
    import builtins

    class Says:
        def __reduce__(self):
            return builtins.print, ("hello",)

    said = []
    bad = str(tmp_path / "bad.npy")
    payload = pickle.dumps(Says(), protocol=3)
    assert b"builtins" in payload and b"print" in payload
    with open(bad, "wb") as f:
        f.write(raw[:head] + payload)

    orig = builtins.print
    builtins.print = lambda *a, **k: said.append(a)
    try:
        assert load_user_graph(bad, 400) is None
    finally:
        builtins.print = orig
    assert not said
    # a truncated file
    cut = str(tmp_path / "cut.npy")
    with open(cut, "wb") as f:
        f.write(raw[: len(raw) // 2])
    assert load_user_graph(cut, 400) is None
    with open(cut, "wb") as f:
        f.write(raw[:6])
    assert load_user_graph(cut, 400) is None
    # a malformed entry
    d2 = dict(d)
    d2[3] = [[1, 2], [1.0]]
    np.save(path, d2, allow_pickle=True)
    assert load_user_graph(path, 400) is None


def test_builder_matches_the_generator_modulo_ties():
    from rsx.dualgnn import build_user_graph

    z = R.load("dualgnn_small.npz")
    tu, ti = z["train_u"].astype(np.int64), z["train_i"].astype(np.int64)
    ref = graph_of(z)
    g = build_user_graph(tu, ti, 400)
    Bm = np.zeros((400, 200))
    Bm[tu, ti] = 1.0
    Cm = Bm @ Bm.T
    np.fill_diagonal(Cm, 0)
    for u in range(400):
        nb, ct = g.lists(u)
        rnb, rct = ref.lists(u)
        assert nb.size == rnb.size, u
        assert np.array_equal(np.sort(ct), np.sort(rct)), u
        assert np.array_equal(Cm[u, nb], ct) and np.array_equal(Cm[u, rnb], rct), u
        if nb.size:
            above = np.flatnonzero(Cm[u] > ct[-1])
            assert set(above) <= set(nb.tolist()), u
        key = list(zip((-ct).tolist(), nb.tolist()))
        assert key == sorted(key) and len(set(nb.tolist())) == nb.size, u
    assert np.diff(g.ptr).max() == 200


def test_cached_graph_round_trip(tmp_path):
    from rsx.dualgnn import CACHE_NAME, cached_user_graph

    z = R.load("dualgnn_small.npz")
    tu, ti = z["train_u"].astype(np.int64), z["train_i"].astype(np.int64)
    a = cached_user_graph(str(tmp_path), tu, ti, 400)
    assert os.path.isfile(tmp_path / CACHE_NAME)
    b = cached_user_graph(str(tmp_path), tu, ti, 400)
    assert np.array_equal(a.ptr, b.ptr) and np.array_equal(a.nbr, b.nbr) and np.array_equal(a.cnt, b.cnt)
    c = cached_user_graph(str(tmp_path), tu[:-1], ti[:-1], 400)  # other interactions: rebuilt
    assert c.nbr.size != a.nbr.size or not np.array_equal(c.cnt, a.cnt)


def test_sym_operator_and_transposed_lists_host():
    from rsx.dualgnn import sym_operator, transposed_lists

    z = R.load("dualgnn_small.npz")
    nu, ni = int(z["n_users"]), int(z["n_items"])
    r, c, v = sym_operator(z["train_u"], z["train_i"], nu, ni)
    dense = np.zeros((nu + ni, nu + ni))
    dense[r, c] = v
    want = R.sym_operator(z["train_u"].astype(np.int64), z["train_i"].astype(np.int64), nu, ni).numpy()
    assert np.abs(dense - want).max() <= 1e-7 and np.array_equal(dense != 0, want != 0)
    assert np.array_equal(dense, dense.T)
    # a duplicate interaction counts twice; a node without edges has no entry
    r, c, v = sym_operator([0, 0, 1], [0, 0, 2], 3, 3)
    got = dict(zip(zip(r.tolist(), c.tolist()), v.tolist()))
    assert got == {(0, 3): 1.0, (3, 0): 1.0, (1, 5): 1.0, (5, 1): 1.0}
    r, c, v = sym_operator([0, 0, 0], [0, 0, 1], 1, 2)
    got = dict(zip(zip(r.tolist(), c.tolist()), v.tolist()))
    assert got[(0, 1)] == np.float32(2 / np.sqrt(6)) and got[(0, 2)] == np.float32(1 / np.sqrt(3))
    # the transposed lists against the dense P^T
    idx, W = z["epoch0_idx"].astype(np.int32), z["epoch0_W"]
    rp, col, val = transposed_lists(idx, W)
    assert rp[-1] == idx.size == col.size == val.size
    PT = np.zeros((nu, nu))
    np.add.at(PT, (idx.reshape(-1), np.repeat(np.arange(nu), 40)), W.reshape(-1).astype(np.float64))
    got = np.zeros((nu, nu))
    np.add.at(got, (np.repeat(np.arange(nu), np.diff(rp)), col), val.astype(np.float64))
    assert np.array_equal(got, PT)


def test_restatement_first_step_vs_fixture_and_the_alias():
    """Step 0's tensors, loss words and every gradient in float64 within 1e-5 of each tensor's
    scale of the reference's; without the in-place alias user_rep misses by more than that."""
    z0, z, nu, P, feats, A, idx, W = setup()
    hp, S = R.hparams(z0), R.strides(z0)
    trip = torch.from_numpy(z0["step0_triplets"].astype(np.int64))
    result, user_rep, xs, terms, grads = R.step(P, feats, A, idx, W, trip, nu, float(hp["reg_weight"]))
    close(xs["v"][::S["rep"]], z0["step0_x_hat_v"])
    close(xs["t"][::S["rep"]], z0["step0_x_hat_t"])
    close(user_rep[::S["rep"]], z0["step0_user_rep"])
    close(result[::S["rep"]], z0["step0_result"])
    for j, name in enumerate(("loss", "bpr", "reg")):
        want = float(z0["step0_" + name])
        assert abs(float(terms[j]) - want) <= 1e-5 * abs(want), (name, float(terms[j]), want)
    for n in NAMES:
        if n in R.UNUSED:
            assert grads[n] is None and "step0_grad." + n not in z0.files, n
        else:
            close(R.rows(flat2(grads[n].numpy()), S["grad"]), z0["step0_grad." + n])
    # weight_i receives its regulariser's gradient alone
    wi = P["weight_i"].detach()
    close(grads["weight_i"], 2 * float(hp["reg_weight"]) / wi.numel() * wi)
    # the alias cannot silently be "fixed": w0 v + w1 t is not what the reference computes
    with torch.no_grad():
        _, plain, _ = R.forward(P, feats, A, idx, W, nu, alias=False)
    want = z0["step0_user_rep"].astype(np.float64)
    miss = np.abs(plain.numpy()[::S["rep"]] - want).max()
    assert miss > 1e-5 * np.abs(want).max() * 100, miss


def test_restatement_second_step_parameters():
    z0, z, nu, P, feats, A, idx, W = setup()
    hp, S = R.hparams(z0), R.strides(z0)
    lr = float(hp["learning_rate"])
    live = {n: P[n] for n in R.trained()}
    adam = R.Adam(live, lr)
    dgs, grefs = {n: [] for n in live}, {n: [] for n in live}
    for step in range(2):
        pre = f"step{step}_"
        trip = torch.from_numpy(z0[pre + "triplets"].astype(np.int64))
        *_, terms, grads = R.step(P, feats, A, idx, W, trip, nu, float(hp["reg_weight"]))
        want = float(z0[pre + "loss"])
        assert abs(float(terms[0]) - want) <= 1e-5 * abs(want)
        adam.step({n: grads[n] for n in live})
        for n in NAMES:
            want = z0[pre + "param." + n].astype(np.float64)
            got = R.rows(flat2(P[n].detach().numpy()), S["param"])
            if n in R.UNUSED:  # never updated: the initial draw, bit for bit
                assert np.array_equal(got, z["init." + n].astype(np.float64)) and np.array_equal(got, want), n
                continue
            gref = z0[pre + "grad." + n].astype(np.float64)
            if gref.ndim == 2 and P[n].shape[0] >= 64:  # a table R.rows strides: from the gradients' stride to the parameters'
                gref = gref[::S["param"] // S["grad"]]
            grefs[n].append(gref)
            dgs[n].append(R.rows(flat2(grads[n].numpy()), S["param"]) - gref)
            extra = R.adam_tolerance(dgs[n], grefs[n], lr)
            tol = 1e-5 * np.abs(want).max() + extra
            share = float((extra > 1e-5 * np.abs(want).max()).mean())
            print(f"  step {step} param {n}: share of elements whose Adam allowance exceeds 1e-5 of the scale {share:.4f}")
            assert (np.abs(got - want) <= tol).all(), (step, n)


def test_hand_backward_of_mix_and_user_graph():
    g = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    nu, ni, k = 9, 5, 4
    xv, xt, w = r(nu + ni, 8).requires_grad_(), r(nu + ni, 8).requires_grad_(), r(nu, 2, 1).requires_grad_()
    gu, gi = r(nu, 8), r(ni, 8)
    user_rep, item_rep = R.mix(xv, xt, w, nu)
    ((user_rep * gu).sum() + (item_rep * gi).sum()).backward()
    g_v, g_t, g_w = R.mix_backward(gu, gi, xv.detach(), xt.detach(), w.detach(), nu)
    assert torch.allclose(g_v, xv.grad) and torch.allclose(g_t, xt.grad) and torch.allclose(g_w, w.grad.reshape(nu, 2))
    idx = torch.randint(0, nu, (nu, k), generator=g)
    idx[2] = 2  # a row naming itself
    idx[3] = 7  # a row naming one user k times
    W = torch.softmax(r(nu, k), dim=1)
    W[0] = 0
    x = r(nu, 8).requires_grad_()
    go = r(nu, 8)
    (R.ugraph(x, idx, W) * go).sum().backward()
    assert torch.allclose(R.ugraph_backward(go, idx, W), x.grad)


@pytest.mark.parametrize("only", ["v", "t"])
def test_one_modality_forms(only):
    z0, z, nu, P, feats, A, idx, W = setup()
    feats = {only: feats[only]}
    other = "t" if only == "v" else "v"
    P = {k: v for k, v in P.items() if not k.startswith(other + "_gcn.")}
    trip = torch.from_numpy(z0["step0_triplets"].astype(np.int64))
    result, user_rep, xs, terms, grads = R.step(P, feats, A, idx, W, trip, nu, 0.001)
    assert result.shape == (nu + int(z["n_items"]), 64) and all(torch.isfinite(t) for t in terms)
    # the user rows are the modality's own rows; weight_u is not applied and is still regularised
    assert torch.equal(user_rep, xs[only][:nu])
    wu = P["weight_u"].detach()
    close(grads["weight_u"], 2 * 0.001 / wu.numel() * wu)
    assert all(grads[n] is not None and grads[n].abs().max() > 0 for n in R.trained((only,)))


def test_yaml_config_and_registry():
    from rsx.config import Config
    from rsx.dualgnn import DualGNN
    from rsx.utils import MODELS, get_model

    c = Config("DualGNN", "baby", {"use_gpu": False})
    assert c["embedding_size"] == 64 and c["n_layers"] == 2 and c["aggr_mode"] == ["add"]
    assert c["reg_weight"] == [0.1, 0.01, 0.001, 0.0001, 0.00001] == c["learning_rate"]
    assert set(c["hyper_parameters"]) >= {"aggr_mode", "reg_weight", "learning_rate"} and c["is_multimodal_model"] is True
    assert c["user_graph_dict_file"] == "user_graph_dict.npy"
    assert MODELS["dualgnn"] == ("rsx.dualgnn", "DualGNN") and get_model("DualGNN") is DualGNN
    assert DualGNN.supports_graph_step and not DualGNN.graph_step_persistent
    with pytest.raises(ValueError, match="DualGNN"):  # the message lists the models, the new one included
        get_model("NoSuchModel")


def _config(**over):
    c = dict(use_gpu=True, device="cuda", embedding_size=64, aggr_mode="add")
    c.update(over)
    return c


@pytest.mark.parametrize("over", [dict(use_gpu=False), dict(device="cpu"), dict(embedding_size=32), dict(embedding_size=128),
                                  dict(aggr_mode="mean")], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_refused_configurations(over):
    from rsx.dualgnn import DualGNN

    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        DualGNN.check_config(_config(**over))
    DualGNN.check_config(_config())


def test_cpu_configuration_and_more_than_one_rank_are_refused(monkeypatch):
    import torch.distributed as dist

    from rsx.config import Config
    from rsx.dualgnn import DualGNN
    from rsx.utils import get_model

    c = Config("DualGNN", "baby", {"use_gpu": False})
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        get_model("DualGNN")(c, None)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda: 2)
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        DualGNN.check_config(_config())


@pytest.mark.parametrize("v_dim,t_dim", [(None, None), (10, None), (48, 6)])
def test_feature_tables_are_refused(v_dim, t_dim):
    from rsx import dualgnn as M

    def stub(v, t):
        s = types.SimpleNamespace(v_feat=None if v is None else torch.zeros(5, v), t_feat=None if t is None else torch.zeros(5, t))
        s.require_features = types.MethodType(M.DualGNN.require_features, s)
        return s

    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        M.DualGNN.check_features(stub(v_dim, t_dim))
    for ok in ((48, 32), (48, None), (None, 384), (4096, 384), (48, 36)):
        M.DualGNN.check_features(stub(*ok))


def test_library_symbols_and_limits():
    from rsx import _lib as L

    lib = L.lib()
    for name in ("rsx_dualgnn_mix_fwd", "rsx_dualgnn_mix_bwd", "rsx_dualgnn_ugraph_fwd", "rsx_dualgnn_loss_ws_bytes",
                 "rsx_dualgnn_loss_fwd", "rsx_dualgnn_loss_bwd"):
        assert hasattr(lib, name) and name in L.EXPORTED, name
    f = lib.rsx_dualgnn_loss_ws_bytes
    assert f(512, 64) > 0 and f(65536, 64) > 0
    assert [f(0, 64), f(65537, 64), f(512, 32), f(512, 128)] == [0, 0, 0, 0]
