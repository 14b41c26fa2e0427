"""DRAGON without a GPU: the float64 restatement (tests/dragon_ref.py) against the reference's own
run (tests/golden/dragon_step0_small.npz, dragon_small.npz), the initial draws, the frozen item
graph, the hand-derived backward of the concatenation, the registry, the configuration checks and
the library's host-side entry points."""
import os
import types

import numpy as np
import pytest
import torch

import dragon_ref as R
from test_mmgcn_cpu import close

NAMES = R.names()
FEAT_TABLE = {"image_embedding.weight": "v_feat", "text_embedding.weight": "t_feat"}


def flat2(a):
    return a.reshape(a.shape[0], -1) if a.ndim > 2 else a


def initial(z, n, stride):
    """The fixture's initial value of parameter n at `stride`: the embedding tables are the
    feature tables, which the fixture holds whole."""
    return R.rows(z[FEAT_TABLE[n]], stride) if n in FEAT_TABLE else z["init." + n]


def init(z):
    """(P float32 by name, result_embed float64) of seed 999 through the model's own draws."""
    from rsx.dragon import dragon_init
    from rsx.utils import init_seed

    init_seed(999)
    host = torch.nn.Module()
    result = dragon_init(host, int(z["n_users"]), int(z["n_items"]), 64, 64, torch.from_numpy(z["v_feat"]),
                         torch.from_numpy(z["t_feat"]))
    return {n: p.detach() for n, p in host.named_parameters()}, result


def setup(dtype=torch.float64):
    z0, z = R.load("dragon_step0_small.npz"), R.load("dragon_small.npz")
    nu, ni = int(z["n_users"]), int(z["n_items"])
    P = R.cast(init(z)[0], dtype)
    feats = {"v": torch.from_numpy(z["v_feat"]).to(dtype), "t": torch.from_numpy(z["t_feat"]).to(dtype)}
    A = R.sym_operator(z["train_u"].astype(np.int64), z["train_i"].astype(np.int64), nu, ni, dtype)
    mm = R.mm_adj_dense(z, ni, dtype)
    idx, W = z["epoch0_idx"].astype(np.int64), torch.from_numpy(z["epoch0_W"]).to(dtype)
    return z0, z, nu, P, feats, A, mm, idx, W


def test_fixture_sizes_hparams_and_margins():
    limit = os.path.getsize(os.path.join(R.GOLD, "dualgnn_step0_small.npz"))
    for f in ("dragon_small.npz", "dragon_step0_small.npz"):
        assert os.path.getsize(os.path.join(R.GOLD, f)) < limit, f
    z0, z = R.load("dragon_step0_small.npz"), R.load("dragon_small.npz")
    hp = R.hparams(z0)
    assert float(hp["learning_rate"]) == 0.001 and float(hp["reg_weight"]) == 0.001 and int(hp["seed"]) == 999
    assert (int(hp["embedding_size"]), int(hp["n_mm_layers"]), int(hp["knn_k"])) == (64, 1, 10)
    assert float(hp["mm_image_weight"]) == 0.1
    assert (int(z["n_users"]), int(z["n_items"]), z["train_u"].size) == (400, 200, 3022)
    assert (z["v_feat"].shape[1], z["t_feat"].shape[1]) == (48, 32)
    for kind in ("step0_preact", "knn_gap"):  # the two margins the capture insists on
        keys = [k for k in z0.files if k.startswith(kind + "_min.")]
        assert len(keys) == 2, kind
        for k in keys:
            assert float(z0[k]) > float(z0[k.replace("_min.", "_thr.")]) > 0, k
    assert sorted(z0["no_grad"]) == sorted(R.UNUSED)
    assert z0["step0_result"].shape[1] == 128 and z["const.result_embed"].shape[1] == 64
    for e in range(2):
        for n in R.trained():
            assert 0 <= float(z[f"epoch{e}_f32_dist.{n}"]) < 1e-3, (e, n)


def test_names_and_initial_draws_follow_the_reference():
    z0, z = R.load("dragon_step0_small.npz"), R.load("dragon_small.npz")
    S = R.strides(z)
    P, result = init(z)
    assert tuple(P) == NAMES
    stored = [k[len("init."):] for k in z.files if k.startswith("init.")]
    assert stored == [n for n in NAMES if n not in FEAT_TABLE]
    assert set(R.trained()) == {k[len("step0_grad."):] for k in z0.files if k.startswith("step0_grad.")}
    assert set(R.trained()) | set(R.UNUSED) == set(NAMES) and "weight_i" in R.UNUSED
    assert P["MLP_user.weight"].shape == (64, 128)
    for n in NAMES:
        got = R.rows(flat2(P[n].numpy()), S["param"])
        assert np.array_equal(got.view(np.int32), initial(z, n, S["param"]).view(np.int32)), n
    assert result.dtype == torch.float64 and result.shape == (600, 64)
    got = result.to(torch.float32).numpy()[::S["const"]]
    assert np.array_equal(got.view(np.int32), z["const.result_embed"].view(np.int32))
    assert R.names(("v",))[4:7] == ("image_embedding.weight", "image_trs.weight", "image_trs.bias")
    assert not any(n.startswith(("text_", "t_gcn.")) for n in R.names(("v",)))


def test_item_graph_is_the_fixtures_mm_adj():
    """freedom_item_graph on the host builds the reference's mm_adj: the same entries in coalesced
    order, the same float32 values; the pattern is not symmetric."""
    from rsx.freedom import freedom_item_graph

    z0, z = R.load("dragon_step0_small.npz"), R.load("dragon_small.npz")
    hp = R.hparams(z0)
    r, c_, v = freedom_item_graph(torch.from_numpy(z["v_feat"]), torch.from_numpy(z["t_feat"]), int(hp["knn_k"]),
                                  float(hp["mm_image_weight"]), "host")
    assert np.array_equal(r, z["mm_adj_row"].astype(np.int64)) and np.array_equal(c_, z["mm_adj_col"].astype(np.int64))
    assert np.array_equal(v.view(np.int32), z["mm_adj_val"].view(np.int32))
    pairs = set(zip(r.tolist(), c_.tolist()))
    assert any((b, a) not in pairs for a, b in pairs)
    # one modality: that modality's graph alone, knn_k entries a row
    r1, _, _ = freedom_item_graph(torch.from_numpy(z["v_feat"]), None, 10, 0.1, "host")
    assert np.array_equal(np.bincount(r1), np.full(200, 10))


def test_reference_mm_adj_cache_is_read(tmp_path):
    """The reference's `mm_adj_{knn_k}.pt` (dragon.py:83: torch.save of the sparse graph) through
    the loader that executes nothing from the file; a file of another size is not trusted."""
    from rsx.blocks import load_reference_knn

    z = R.load("dragon_small.npz")
    ni = int(z["n_items"])
    idx = torch.from_numpy(np.stack([z["mm_adj_row"], z["mm_adj_col"]]).astype(np.int64))
    torch.save(torch.sparse_coo_tensor(idx, torch.from_numpy(z["mm_adj_val"]), (ni, ni)), tmp_path / "mm_adj_10.pt")
    r, c_, v = load_reference_knn(str(tmp_path / "mm_adj_10.pt"), ni)
    assert np.array_equal(r, z["mm_adj_row"]) and np.array_equal(c_, z["mm_adj_col"])
    assert np.array_equal(v.view(np.int32), z["mm_adj_val"].view(np.int32))
    assert load_reference_knn(str(tmp_path / "mm_adj_10.pt"), ni + 1) is None
    assert load_reference_knn(str(tmp_path / "mm_adj_20.pt"), ni) is None


def test_restatement_first_step_vs_fixture():
    """Step 0's tensors, loss words and every gradient in float64 within 1e-5 of each tensor's
    scale of the reference's."""
    z0, z, nu, P, feats, A, mm, idx, W = setup()
    hp, S = R.hparams(z0), R.strides(z0)
    trip = torch.from_numpy(z0["step0_triplets"].astype(np.int64))
    result, user_rep, xs, terms, grads = R.step(P, feats, A, mm, int(hp["n_mm_layers"]), idx, W, trip, nu,
                                                float(hp["reg_weight"]))
    assert result.shape == (600, 128) and user_rep.shape == (400, 128)
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
    # the item graph is in the step: without it the item rows miss by far more than the bound
    with torch.no_grad():
        plain, _, _ = R.forward(P, feats, A, mm, 0, idx, W, nu)
    want = z0["step0_result"].astype(np.float64)
    assert np.abs(plain.numpy()[::S["rep"]] - want).max() > 1e-3 * np.abs(want).max()


def test_restatement_second_step_parameters():
    z0, z, nu, P, feats, A, mm, idx, W = setup()
    hp, S = R.hparams(z0), R.strides(z0)
    lr = float(hp["learning_rate"])
    live = {n: P[n] for n in R.trained()}
    adam = R.Adam(live, lr)
    dgs, grefs = {n: [] for n in live}, {n: [] for n in live}
    for step in range(2):
        pre = f"step{step}_"
        trip = torch.from_numpy(z0[pre + "triplets"].astype(np.int64))
        *_, terms, grads = R.step(P, feats, A, mm, int(hp["n_mm_layers"]), idx, W, trip, nu, float(hp["reg_weight"]))
        want = float(z0[pre + "loss"])
        assert abs(float(terms[0]) - want) <= 1e-5 * abs(want)
        adam.step({n: grads[n] for n in live})
        for n in live:
            want = z0[pre + "param." + n].astype(np.float64)
            got = R.rows(flat2(P[n].detach().numpy()), S["param"])
            gref = z0[pre + "grad." + n].astype(np.float64)
            if gref.ndim == 2 and P[n].shape[0] >= 64:  # a table R.rows strides: from the gradients' stride to the parameters'
                gref = gref[::S["param"] // S["grad"]]
            grefs[n].append(gref)
            dgs[n].append(R.rows(flat2(grads[n].numpy()), S["param"]) - gref)
            tol = 1e-5 * np.abs(want).max() + R.adam_tolerance(dgs[n], grefs[n], lr)
            assert (np.abs(got - want) <= tol).all(), (step, n)
        for n in R.UNUSED:  # never updated; the fixture keeps their initial value only
            assert pre + "param." + n not in z0.files, n


def test_hand_backward_of_cat_and_item_prop():
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    nu, ni, h = 9, 5, 8
    xv, xt, w = r(nu + ni, h).requires_grad_(), r(nu + ni, h).requires_grad_(), r(nu, 2, 1).requires_grad_()
    gu, gi = r(nu, 2 * h), r(ni, 2 * h)
    user_rep, item_rep = R.cat(xv, xt, w, nu)
    assert user_rep.shape == (nu, 2 * h) and item_rep.shape == (ni, 2 * h)
    assert torch.equal(item_rep[:, :h], xv[nu:]) and torch.equal(user_rep[:, h:], w[:, 1] * xt[:nu])
    ((user_rep * gu).sum() + (item_rep * gi).sum()).backward()
    g_v, g_t, g_w = R.cat_backward(gu, gi, xv.detach(), xt.detach(), w.detach(), nu)
    assert torch.allclose(g_v, xv.grad) and torch.allclose(g_t, xt.grad) and torch.allclose(g_w, w.grad.reshape(nu, 2))
    # the item graph's residual: its gradient is the same residual on the transpose
    A = r(ni, ni)
    for layers in (0, 1, 2):
        x = r(ni, h).requires_grad_()
        (R.item_prop(x, A, layers) * gi[:, :h]).sum().backward()
        assert torch.allclose(x.grad, R.item_prop(gi[:, :h], A.t(), layers))
    assert torch.equal(R.item_prop(gi, A, 0), 2 * gi)


@pytest.mark.parametrize("only", ["v", "t"])
def test_one_modality_forms(only):
    z0, z, nu, P, feats, A, mm, idx, W = setup()
    feats = {only: feats[only]}
    keep = set(R.names((only,)))
    P = {k: v for k, v in P.items() if k in keep}
    trip = torch.from_numpy(z0["step0_triplets"].astype(np.int64))
    result, user_rep, xs, terms, grads = R.step(P, feats, A, mm, 1, idx, W, trip, nu, 0.001)
    assert result.shape == (nu + int(z["n_items"]), 64) and all(torch.isfinite(t) for t in terms)
    # the user rows are the modality's own rows; weight_u is not applied and is still regularised
    assert torch.equal(user_rep, xs[only][:nu])
    wu = P["weight_u"].detach()
    close(grads["weight_u"], 2 * 0.001 / wu.numel() * wu)
    assert all(grads[n] is not None and grads[n].abs().max() > 0 for n in R.trained((only,)))
    assert all(grads[n] is None for n in R.names((only,)) if n in R.UNUSED)


def test_yaml_config_and_registry():
    from rsx.config import Config
    from rsx.dragon import DRAGON
    from rsx.utils import MODELS, get_model

    c = Config("DRAGON", "baby", {"use_gpu": False})
    assert (c["embedding_size"], c["feat_embed_dim"], c["n_mm_layers"], c["n_layers"], c["knn_k"]) == (64, 64, 1, 2, 10)
    assert c["mm_image_weight"] == 0.1 and c["aggr_mode"] == ["add"]
    assert c["reg_weight"] == [0.1, 0.01, 0.001, 0.0001, 0.00001] == c["learning_rate"]
    assert set(c["hyper_parameters"]) >= {"aggr_mode", "reg_weight", "learning_rate"} and c["is_multimodal_model"] is True
    assert MODELS["dragon"] == ("rsx.dragon", "DRAGON") and get_model("DRAGON") is DRAGON
    assert DRAGON.supports_graph_step and not DRAGON.graph_step_persistent
    with pytest.raises(ValueError, match="DRAGON"):  # the message lists the models, the new one included
        get_model("NoSuchModel")


def _config(**over):
    c = dict(use_gpu=True, device="cuda", embedding_size=64, aggr_mode="add", knn_k=10, n_mm_layers=1)
    c.update(over)
    return c


@pytest.mark.parametrize("over", [dict(use_gpu=False), dict(device="cpu"), dict(embedding_size=32), dict(embedding_size=128),
                                  dict(aggr_mode="mean"), dict(knn_k=33), dict(n_mm_layers=-1)],
                         ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_refused_configurations(over):
    from rsx.dragon import DRAGON

    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        DRAGON.check_config(_config(**over))
    DRAGON.check_config(_config())
    DRAGON.check_config(_config(n_mm_layers=0, knn_k=32))


def test_cpu_configuration_and_more_than_one_rank_are_refused(monkeypatch):
    import torch.distributed as dist

    from rsx.config import Config
    from rsx.dragon import DRAGON
    from rsx.utils import get_model

    c = Config("DRAGON", "baby", {"use_gpu": False})
    for k in c["hyper_parameters"]:
        if isinstance(c[k], list):
            c[k] = c[k][0]
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        get_model("DRAGON")(c, None)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda: 2)
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        DRAGON.check_config(_config())


@pytest.mark.parametrize("v_dim,t_dim", [(None, None), (10, None), (48, 6)])
def test_feature_tables_are_refused(v_dim, t_dim):
    from rsx import dragon as M

    def stub(v, t):
        s = types.SimpleNamespace(v_feat=None if v is None else torch.zeros(5, v), t_feat=None if t is None else torch.zeros(5, t))
        s.require_features = types.MethodType(M.DRAGON.require_features, s)
        return s

    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        M.DRAGON.check_features(stub(v_dim, t_dim))
    for ok in ((48, 32), (48, None), (None, 384), (4096, 384)):
        M.DRAGON.check_features(stub(*ok))


def test_library_symbols_and_limits():
    from rsx import _lib as L

    lib = L.lib()
    for name in ("rsx_dragon_cat_fwd", "rsx_dragon_cat_bwd", "rsx_dragon_ugraph_fwd", "rsx_dragon_loss_ws_bytes",
                 "rsx_dragon_loss_fwd", "rsx_dragon_loss_bwd"):
        assert hasattr(lib, name) and name in L.EXPORTED, name
    f = lib.rsx_dragon_loss_ws_bytes
    assert [f(0, 64), f(0, 128), f(65537, 64), f(65537, 128), f(512, 32)] == [0, 0, 0, 0, 0]
    assert 0 < f(512, 64) < f(512, 128) and 0 < f(65536, 64) < f(65536, 128)
    assert f(1, 64) > 0 and f(1, 128) > 0
    # the user-graph functions are DualGNN's own, imported and unchanged
    from rsx import dragon, dualgnn

    for name in ("load_user_graph", "cached_user_graph", "topk_sample", "transposed_lists", "sym_operator", "GCN", "_Prop"):
        assert getattr(dragon, name) is getattr(dualgnn, name), name
