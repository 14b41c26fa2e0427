"""MGCN without a GPU: the float64 restatement (tests/mgcn_ref.py) against the reference's
own forward and first step (tests/golden/mgcn_step0_small.npz, mgcn_small.npz; tools/
capture_golden.py --only mgcn), model resolution, the YAML, the refusal of a CPU
configuration and the library's new symbols.

Bounds.  The reference ran in float32 and the restatement is float64, so the difference is
the reference's own rounding: forward rtol 1e-5 / atol 1e-6 and loss 1e-5 relative (what
the GPU tests ask of the model against the same arrays), gradients rtol 1e-3 with atol
1e-5 of the tensor's scale (tests/test_gpu_smore.py's first-step bound).  The three
query_common gradients are sums of nearly cancelling terms at initialisation (both
purified views are about item / 2, so the image and the text row nearly agree and
d aT = -d aI): a float64 rerun of the reference itself moved them by up to 2.3e-4 of scale
(query_common.0.bias; 1.3e-6 and 3.7e-6 for the two weights), so they are held to 4x that,
1e-3 of scale."""
import numpy as np
import pytest
import torch

import mgcn_ref as R


def test_fixture_files_are_small_and_complete():
    import os

    for f in ("mgcn_small.npz", "mgcn_step0_small.npz"):
        assert os.path.getsize(os.path.join(R.GOLD, f)) < (1 << 20), f
    z = R.load_fixture()
    for n in R.NAMES:
        for pre in ("init.", "step0_grad.", "step0_param.", "epoch1_param."):
            assert z[pre + n].shape == z["init." + n].shape and z[pre + n].dtype == np.float32, pre + n
    assert z["step0_triplets"].shape == (3, 512)
    assert np.array_equal(z["step0_triplets"], z["epoch0_triplets"][:, :512])
    assert list(z["hparams"]) == ["seed=999", "cl_loss=0.01"]


def test_restatement_reproduces_the_reference_forward():
    z = R.load_fixture()
    nu = int(z["n_users"])
    all_, side, content, _ = R.forward(R.init_params(z), R.dense_graphs(z), 2, 1)
    for got, key in ((all_[:nu], "fwd_user"), (all_[nu:], "fwd_item"), (side, "fwd_side"), (content, "fwd_content")):
        np.testing.assert_allclose(got, z[key], rtol=1e-5, atol=1e-6, err_msg=key)


def test_restatement_reproduces_the_reference_first_step():
    z = R.load_fixture()
    loss, g = R.step0(z)
    want = float(z["step0_loss"])
    print(f"loss {loss:.9f} vs reference {want:.9f}")
    assert abs(loss - want) <= 1e-5 * abs(want)
    assert set(g) == set(R.NAMES)
    for n in R.NAMES:
        w = z["step0_grad." + n]
        scale = float(np.abs(w).max())
        err = float(np.abs(g[n].reshape(w.shape) - w).max())
        print(f"  {n}: err {err:.3e}, scale {scale:.3e}, err / scale {err / scale:.2e}")
        if n in R.QUERY:
            assert err <= 1e-3 * scale, n
        else:
            np.testing.assert_allclose(g[n].reshape(w.shape), w, rtol=1e-3, atol=1e-5 * scale, err_msg=n)


def test_restatement_blocks_against_finite_differences():
    """The purifier's and the fuser's analytic gradients (repeated rows, g_side and g_cin
    included) against central differences of a random linear functional."""
    rng = np.random.default_rng(3)
    N, n, d = 9, 14, 8
    C, I, T = (rng.standard_normal((N, d)) for _ in range(3))
    W = [rng.standard_normal((d, d)) * 0.4 for _ in range(3)]
    b = [rng.standard_normal(d) * 0.1 for _ in range(3)]
    w2 = rng.standard_normal((1, d))
    rows = rng.integers(0, N, n)
    gA, gS, gCi = (rng.standard_normal((n, d)) for _ in range(3))

    def val(C_, I_, T_, W1, w2_):
        r = R.fuse(C_, I_, T_, W1, b[0], w2_, W[1], b[1], W[2], b[2], rows=rows)
        return (r["all"] * gA).sum() + (r["side"] * gS).sum() + (r["content"] * gCi).sum()

    r = R.fuse(C, I, T, W[0], b[0], w2, W[1], b[1], W[2], b[2], rows=rows, g_all=gA, g_side=gS, g_cin=gCi)
    eps = 1e-6
    for k, (x, g) in enumerate(((C, r["gC"]), (I, r["gI"]), (T, r["gT"]), (W[0], r["dW1"]), (w2, r["dw2"]))):
        for _ in range(4):
            i, j = rng.integers(0, x.shape[0]), rng.integers(0, x.shape[1])
            args = [C, I, T, W[0], w2]
            hi, lo = x.copy(), x.copy()
            hi[i, j] += eps
            lo[i, j] -= eps
            args[k] = hi
            vh = val(*args)
            args[k] = lo
            fd = (vh - val(*args)) / (2 * eps)
            assert abs(fd - g[i, j]) <= 1e-6 * max(1.0, abs(fd)), (k, i, j, fd, g[i, j])
    # I = T on a row: the softmax weights are exactly 1/2 and the query gradients' row terms vanish
    r2 = R.fuse(C, I, I, W[0], b[0], w2, W[1], b[1], W[2], b[2], g_all=rng.standard_normal((N, d)))
    assert np.all(r2["wI"] == 0.5) and not r2["dW1"].any() and not r2["dw2"].any() and not r2["db1"].any()
    item, f0, f1 = (rng.standard_normal((N, d)) for _ in range(3))
    go = [rng.standard_normal((N, d)) for _ in range(2)]
    p = R.purify(item, [f0, f1], W[:2], b[:2], gout=go)
    for x, g, k in ((item, p["g_item"], 0), (f0, p["g_feat"][0], 1), (W[1], p["dW"][1], 2)):
        i, j = 2, 5
        hi, lo = x.copy(), x.copy()
        hi[i, j] += eps
        lo[i, j] -= eps

        def v(y):
            a = [item, f0, list(W[:2])]
            a[k] = y if k < 2 else [W[0], y]
            o = R.purify(a[0], [a[1], f1], a[2], b[:2])["out"]
            return (o[0] * go[0]).sum() + (o[1] * go[1]).sum()

        fd = (v(hi) - v(lo)) / (2 * eps)
        assert abs(fd - g[i, j]) <= 1e-6 * max(1.0, abs(fd)), (k, fd, g[i, j])


def test_model_resolves_and_config_loads():
    from rsx.config import Config
    from rsx.utils import MODELS, get_model

    cls = get_model("MGCN")
    assert cls.__name__ == "MGCN" and cls.supports_graph_step and cls.graph_step_persistent
    assert not cls.supports_fused_step and not hasattr(cls, "mg_enable")
    assert MODELS["mgcn"] == ("rsx.mgcn", "MGCN")
    c = Config("MGCN", "baby", {"use_gpu": False})
    assert c["embedding_size"] == 64 and c["n_ui_layers"] == 2 and c["n_layers"] == 1
    assert c["learning_rate_scheduler"] == [0.96, 50] and c["lambda_coeff"] == 0.9
    assert c["reg_weight"] == 1e-4 and isinstance(c["reg_weight"], float)
    assert c["knn_k"] == 10 and c["learning_rate"] == 0.001
    assert c["cl_loss"] == [0.001, 0.01, 0.1] and "cl_loss" in c["hyper_parameters"]
    with pytest.raises(ValueError, match="MGCN"):  # the message lists the models, the new one included
        get_model("NoSuchModel")


def test_cpu_configuration_is_refused():
    from rsx.config import Config
    from rsx.utils import get_model

    c = Config("MGCN", "baby", {"use_gpu": False})
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        get_model("MGCN")(c, None)


def test_unsupported_width_k_and_world_size_are_refused(monkeypatch):
    import torch.distributed as dist

    from rsx.mgcn import MGCN

    cfg = {"use_gpu": True, "device": torch.device("cuda", 0), "embedding_size": 32, "knn_k": 10}
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED.*embedding_size 32"):
        MGCN.check_config(cfg)
    cfg.update(embedding_size=64, knn_k=33)
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED.*knn_k 33"):
        MGCN.check_config(cfg)
    cfg["knn_k"] = 10
    MGCN.check_config(cfg)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED.*world size 2"):
        MGCN.check_config(cfg)


def test_library_symbols_and_refusals():
    import ctypes as C

    from rsx import _lib as L

    lib = L.lib()
    for sym in ("rsx_mgcn_purify", "rsx_mgcn_fuse", "rsx_mgcn_fuse_ws_bytes"):
        assert sym in L.EXPORTED and hasattr(lib, sym)
    # refused before any launch (no GPU needed)
    two = (C.c_void_p * 2)(1, 1)
    four = (C.c_void_p * 4)(1, 1, 1, 1)
    one = C.c_void_p(1)
    assert lib.rsx_mgcn_purify(0, two, one, two, two, 5, 48, two, None, None, None, None, None) == L.RSX_ERR_UNSUPPORTED
    assert lib.rsx_mgcn_purify(0, None, one, two, two, 5, 64, two, None, None, None, None, None) == 1001
    assert lib.rsx_mgcn_purify(0, two, one, two, two, 0, 64, two, None, None, None, None, None) == 0
    fuse = lambda d, n, c: lib.rsx_mgcn_fuse(0, four, four, c, one, one, None, n, n, d, one, one, None, None, None,  # noqa: E731
                                             None, None, None, None, None, None, None, None, None, 0, None)
    assert fuse(256, 5, one) == L.RSX_ERR_UNSUPPORTED
    assert fuse(64, 5, None) == 1001
    assert fuse(64, 0, one) == 0
    # the backward's scratch: the d w2 partial rows, plus in the rows form the per-occurrence
    # rows and two words a table row
    assert lib.rsx_mgcn_fuse_ws_bytes(65, 65, 64, 0) == 2 * 64 * 4
    assert lib.rsx_mgcn_fuse_ws_bytes(65, 50, 64, 1) == (2 * 64 + 3 * 65 * 64 + 2 * 50) * 4
    assert lib.rsx_mgcn_fuse_ws_bytes(0, 50, 64, 1) == 0
