"""FREEDOM without a GPU: the float64 restatement (tests/freedom_ref.py) against the
reference's own forward and first step (tests/golden/freedom_step0_small.npz,
freedom_small.npz; tools/capture_golden.py --only freedom), the host item-graph and
epoch-graph builders against the reference's graphs bit for bit, model resolution, the
YAML, the refusal of a CPU configuration and the library's new symbols.

Bounds.  The reference ran in float32 and the restatement is float64, so the difference is
the reference's own rounding: forward rtol 1e-5 / atol 1e-6 and loss 1e-5 relative (what
the GPU tests ask of the model against the same arrays), the six non-bias gradients rtol
1e-3 with atol 1e-5 of the tensor's scale (tests/test_mgcn_cpu.py's bound).  The two
projection-bias gradients are analytically zero (the bias enters T[pos] - T[neg] with both
signs); what either side holds is rounding noise, so they are held absolutely:
|g_bias| <= 1e-5 max|g_weight| of the same layer."""
import os

import numpy as np
import pytest
import torch

import freedom_ref as R


def test_fixture_files_are_small_and_complete():
    for f in ("freedom_small.npz", "freedom_step0_small.npz"):
        assert os.path.getsize(os.path.join(R.GOLD, f)) < (1 << 20), f
    z = R.load_fixture()
    for n in R.NAMES:
        for pre in ("init.", "step0_grad.", "step0_param.", "epoch1_param."):
            assert z[pre + n].shape == z["init." + n].shape and z[pre + n].dtype == np.float32, pre + n
    assert z["step0_triplets"].shape == (3, 512)
    assert np.array_equal(z["step0_triplets"], z["epoch0_triplets"][:, :512])
    assert list(z["hparams"]) == ["seed=999", "dropout=0.8", "reg_weight=0.001"]
    assert "init_valid_topk_idx" not in z
    n_edges = z["edge_idx"].shape[1]
    assert n_edges == 3022 and z["train_u"].size == n_edges
    for e in (0, 1):
        assert z[f"e{e}_keep_ids"].size == int(n_edges * 0.2) == 604
        assert z[f"e{e}_masked_val"].size == 2 * 604
    assert not np.array_equal(z["e0_keep"], z["e1_keep"])  # a fresh draw every epoch
    # the item graph: k = 10, three distinct float32 values (image only, text only, both)
    assert z["mm_adj_val"].size == 3722
    vals = np.unique(z["mm_adj_val"])
    assert vals.size == 3
    np.testing.assert_allclose(vals, [0.01, 0.09, 0.1], rtol=1e-6)


def test_restatement_reproduces_the_reference_forward():
    z = R.load_fixture()
    norm, _, mm = R.dense_graphs(z)
    u, i = R.forward(R.init_params(z), norm, mm)
    np.testing.assert_allclose(u, z["fwd_user"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(i, z["fwd_item"], rtol=1e-5, atol=1e-6)


def test_restatement_reproduces_the_reference_first_step():
    z = R.load_fixture()
    loss, words, g = R.step0(z)
    want = float(z["step0_loss"])
    print(f"loss {loss:.9f} vs reference {want:.9f}; words {words}")
    assert abs(loss - want) <= 1e-5 * abs(want)
    assert set(g) == set(R.NAMES)
    for n in R.NAMES:
        w = z["step0_grad." + n]
        scale = float(np.abs(w).max())
        err = float(np.abs(g[n].reshape(w.shape) - w).max())
        print(f"  {n}: err {err:.3e}, scale {scale:.3e}")
        if n in R.BIASES:
            bound = 1e-5 * float(np.abs(z["step0_grad." + n.replace(".bias", ".weight")]).max())
            assert np.abs(w).max() <= bound and np.abs(g[n]).max() <= bound, (n, np.abs(w).max(), np.abs(g[n]).max())
        else:
            np.testing.assert_allclose(g[n].reshape(w.shape), w, rtol=1e-3, atol=1e-5 * scale, err_msg=n)


def test_restatement_against_finite_differences():
    """The analytic gradients at a tiny shape whose batch repeats users and items (an item
    both a positive and a negative) against central differences of the loss."""
    rng = np.random.default_rng(5)
    nu, ni, d, fv, ft, B = 4, 5, 6, 7, 3, 12
    p = {"user_embedding.weight": rng.standard_normal((nu, d)), "item_id_embedding.weight": rng.standard_normal((ni, d)),
         "image_embedding.weight": rng.standard_normal((ni, fv)), "image_trs.weight": rng.standard_normal((d, fv)) * 0.5,
         "image_trs.bias": rng.standard_normal(d), "text_embedding.weight": rng.standard_normal((ni, ft)),
         "text_trs.weight": rng.standard_normal((d, ft)) * 0.5, "text_trs.bias": rng.standard_normal(d)}
    A = rng.random((nu + ni, nu + ni)) * 0.3
    A = A + A.T
    M = rng.random((ni, ni)) * 0.4  # not symmetric
    trip = np.stack([rng.integers(0, nu, B), rng.integers(0, ni, B), rng.integers(0, ni, B)])
    assert np.intersect1d(trip[1], trip[2]).size and np.unique(trip[0]).size < B
    reg = 0.7
    _, _, g = R.model_loss_grad(p, A, M, trip, reg)
    eps = 1e-6
    for name in R.NAMES:
        x = p[name]
        for _ in range(3):
            idx = tuple(rng.integers(0, s) for s in x.shape)
            hi, lo = dict(p), dict(p)
            hi[name], lo[name] = x.copy(), x.copy()
            hi[name][idx] += eps
            lo[name][idx] -= eps
            fd = (R.model_loss_grad(hi, A, M, trip, reg)[0] - R.model_loss_grad(lo, A, M, trip, reg)[0]) / (2 * eps)
            assert abs(fd - g[name][idx]) <= 1e-7 * max(1.0, abs(fd)) + 1e-9, (name, idx, fd, g[name][idx])
    # the bias gradients are zero to rounding
    for b in R.BIASES:
        assert np.abs(g[b]).max() <= 1e-12
    # one modality only, and the kernel-level contract with H = None
    q = {k: v for k, v in p.items() if not k.startswith("image")}
    loss_t, words, gq = R.model_loss_grad(q, A, M, trip, reg)
    assert words[3] == 0.0 and "image_trs.weight" not in gq and loss_t == words[1] + reg * words[2]
    out, gE, gT, gV = R.loss_grad(rng.standard_normal((nu + ni, d)), None, rng.standard_normal((ni, d)), None, trip, nu, reg)
    assert gV is None and not gE[np.setdiff1d(np.arange(nu), trip[0])].any()


def test_item_graph_host_matches_the_fixture_bit_for_bit():
    from rsx.freedom import freedom_item_graph

    z = R.load_fixture()
    v, t = torch.from_numpy(z["v_feat"]), torch.from_numpy(z["t_feat"])
    r, c, w = freedom_item_graph(v, t, R.KNN_K, R.IMAGE_WEIGHT, mode="host")
    assert np.array_equal(np.stack([r, c]), z["mm_adj_idx"].astype(np.int64))
    assert np.array_equal(w.view(np.int32), z["mm_adj_val"].view(np.int32))
    # the restatement's values, from its own float64 top-k
    ni = int(z["n_items"])
    g = R.item_graph(R.topk_ids(z["v_feat"], R.KNN_K), R.topk_ids(z["t_feat"], R.KNN_K), ni, R.IMAGE_WEIGHT)
    idx = z["mm_adj_idx"].astype(np.int64)
    ref = dict(zip(zip(idx[0].tolist(), idx[1].tolist()), z["mm_adj_val"]))
    common = set(g) & set(ref)
    assert len(common) >= 0.99 * len(ref)  # near-ties of the float32 top-k may swap a neighbour
    assert max(abs(float(g[k]) - float(ref[k])) for k in common) <= 1e-8
    # one modality alone: that modality's graph, k entries a row at 1 / k
    r1, c1, w1 = freedom_item_graph(None, t, R.KNN_K, R.IMAGE_WEIGHT, mode="host")
    assert r1.size == ni * R.KNN_K and np.all(np.bincount(r1) == R.KNN_K)
    np.testing.assert_allclose(w1, 1.0 / R.KNN_K, rtol=1e-6)
    with pytest.raises(ValueError):
        freedom_item_graph(v, t, R.KNN_K, R.IMAGE_WEIGHT, mode="gpu")


def test_masked_adj_of_the_kept_edges_matches_the_fixture_bit_for_bit():
    from rsx import graph

    z = R.load_fixture()
    nu, ni = int(z["n_users"]), int(z["n_items"])
    e = z["edge_idx"].astype(np.int64)
    # the model's edge list is the training interactions (in the order its edge ids count in)
    assert np.array_equal(np.sort(e[0] * ni + e[1]), np.sort(z["train_u"] * ni + z["train_i"]))
    for ep in (0, 1):
        k = e[:, z[f"e{ep}_keep_ids"]]
        rp, col, val = graph.layergcn_masked_adj(k[0], k[1], nu, ni)
        rows, cols, want = R.masked_coo(z, ep)
        assert np.array_equal(np.repeat(np.arange(nu + ni), np.diff(rp)), rows)
        assert np.array_equal(col.astype(np.int64), cols)
        assert np.array_equal(val.view(np.int32), want.view(np.int32))


def test_model_resolves_and_config_loads():
    from rsx.config import Config
    from rsx.utils import MODELS, get_model

    cls = get_model("FREEDOM")
    assert cls.__name__ == "FREEDOM" and cls.supports_graph_step and not cls.graph_step_persistent
    assert not cls.supports_fused_step
    assert MODELS["freedom"] == ("rsx.freedom", "FREEDOM")
    c = Config("FREEDOM", "baby", {"use_gpu": False})
    assert c["embedding_size"] == 64 and c["feat_embed_dim"] == 64 and c["weight_size"] == [64, 64]
    assert c["n_mm_layers"] == 1 and c["n_ui_layers"] == 2 and c["knn_k"] == 10
    assert c["mm_image_weight"] == 0.1 and c["lambda_coeff"] == 0.9
    assert c["reg_weight"] == [0.0, 1e-05, 1e-04, 1e-03] and all(isinstance(x, float) for x in c["reg_weight"])
    assert c["dropout"] == [0.8, 0.9]
    assert "dropout" in c["hyper_parameters"] and "reg_weight" in c["hyper_parameters"]
    with pytest.raises(ValueError, match="FREEDOM"):  # the message lists the models, the new one included
        get_model("NoSuchModel")


def test_cpu_configuration_is_refused():
    from rsx.config import Config
    from rsx.utils import get_model

    c = Config("FREEDOM", "baby", {"use_gpu": False})
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        get_model("FREEDOM")(c, None)


def test_unsupported_configurations_are_refused(monkeypatch):
    import torch.distributed as dist

    from rsx.freedom import FREEDOM

    ok = {"use_gpu": True, "device": torch.device("cuda", 0), "embedding_size": 64, "feat_embed_dim": 64, "knn_k": 10,
          "n_ui_layers": 2, "dropout": 0.8}
    FREEDOM.check_config(ok)
    for key, bad, what in (("embedding_size", 32, "embedding_size 32"), ("feat_embed_dim", 128, "feat_embed_dim 128"),
                           ("knn_k", 33, "knn_k 33"), ("n_ui_layers", 0, "n_ui_layers 0"), ("dropout", 1.0, "dropout 1.0")):
        with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED.*" + what):
            FREEDOM.check_config(dict(ok, **{key: bad}))
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED.*world size 2"):
        FREEDOM.check_config(ok)


def test_library_symbols_and_refusals():
    import ctypes as C

    from rsx import _lib as L

    lib = L.lib()
    for sym in ("rsx_freedom_ws_bytes", "rsx_freedom_loss_fwd", "rsx_freedom_loss_bwd"):
        assert sym in L.EXPORTED and hasattr(lib, sym)
    assert lib.rsx_freedom_ws_bytes(512, 64) >= 512 * 64 * 4 + 3 * 512 * 4 + 3 * 512 * 4
    assert lib.rsx_freedom_ws_bytes(513, 128) > lib.rsx_freedom_ws_bytes(512, 128) >= 512 * 128 * 4
    assert lib.rsx_freedom_ws_bytes(0, 64) == 0 and lib.rsx_freedom_ws_bytes(512, 32) == 0

    # refused before any launch (no GPU needed; the pointers are never read)
    def call(d=64, batch=8, T=16, V=16, E=16, ws=16, ws_bytes=1 << 30):
        a = L.FreedomArgs(E, 16, T, V, 16, 5, 7, batch, d, 0.5)
        return lib.rsx_freedom_loss_fwd(C.byref(a), C.c_void_p(16), C.c_void_p(ws) if ws else None, ws_bytes, None)

    assert call(d=32) == L.RSX_ERR_UNSUPPORTED and call(d=256) == L.RSX_ERR_UNSUPPORTED
    assert call(batch=0) == 1001
    assert call(T=None, V=None) == 1001
    assert call(E=None) == 1001 and call(ws=None) == 1001
    assert call(E=20) == 1001  # float4 lanes: 16-byte aligned tables
    assert call(ws_bytes=64) == 1003
    a = L.FreedomArgs(16, 16, 16, None, 16, 5, 7, 8, 64, 0.5)
    assert lib.rsx_freedom_loss_bwd(C.byref(a), None, C.c_void_p(16), C.c_void_p(16), None, C.c_void_p(16), 1 << 30,
                                    None) == 1001  # no upstream gradient
    assert lib.rsx_freedom_loss_bwd(C.byref(a), C.c_void_p(16), C.c_void_p(16), None, None, C.c_void_p(16), 1 << 30,
                                    None) == 1001  # T without gT
