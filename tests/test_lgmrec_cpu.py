"""LGMRec without a GPU: the float64 restatement (tests/lgmrec_ref.py) against the reference's own
run (tests/golden/lgmrec_step0_small.npz, lgmrec_small.npz), the initial draws, the host graph
builders, the refused configurations and the library's new symbols."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lgmrec_ref as R
from helpers import coo_sorted, csr_to_sorted

HP = R.HPARAMS


def test_fixture_sizes():
    for f in ("lgmrec_small.npz", "lgmrec_step0_small.npz"):
        assert os.path.getsize(os.path.join(R.GOLD, f)) < (1 << 20), f


def _setup(dtype=torch.float64, grad=False):
    z0, z = R.load("lgmrec_step0_small.npz"), R.load("lgmrec_small.npz")
    nu, ni = int(z["n_users"]), int(z["n_items"])
    tu, ti = z["train_u"].astype(np.int64), z["train_i"].astype(np.int64)
    graphs = R.dense_graphs(tu, ti, nu, ni, dtype)
    feats = (R.tt(z["v_feat"], dtype), R.tt(z["t_feat"], dtype))
    p = {n: R.tt(z0["init." + n], dtype, grad) for n in R.NAMES}
    return z0, z, nu, ni, graphs, feats, p


def test_hparams_recorded():
    z0 = R.load("lgmrec_step0_small.npz")
    got = dict(s.split("=", 1) for s in z0["hparams"])
    for k in ("hyper_num", "n_hyper_layer", "keep_rate", "alpha", "n_ui_layers", "n_mm_layers", "cl_weight",
              "reg_weight", "seed"):
        assert float(got[k]) == float(HP[k]), k


def test_restatement_eval_forward_vs_fixture():
    z0, _, nu, ni, graphs, feats, p = _setup()
    draws = R.fixture_draws(z0, "fwd_")
    with torch.no_grad():
        ts = R.tables(p, feats, graphs, HP, draws, training=False)
        all_ = R.combine(*ts, HP["alpha"]).numpy()
    np.testing.assert_allclose(all_[:nu], z0["fwd_user"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(all_[nu:], z0["fwd_item"], rtol=1e-5, atol=1e-6)
    Gv, Gt = ts[3].numpy(), ts[4].numpy()
    for name, t in (("uv", Gv[:nu]), ("iv", Gv[nu:]), ("ut", Gt[:nu]), ("it", Gt[nu:])):
        want = z0["fwd_hyper_" + name]
        np.testing.assert_allclose(t[::8], want, rtol=1e-5, atol=1e-6 * np.abs(want).max())


def test_restatement_two_steps_vs_fixture():
    """Loss terms and gradients of the first two steps in float64, within 1e-5 of each tensor's
    scale, and the parameters after Adam."""
    z0, _, nu, ni, graphs, feats, p = _setup(grad=True)
    m = {n: torch.zeros_like(t) for n, t in p.items()}
    v = {n: torch.zeros_like(t) for n, t in p.items()}
    for step in range(2):
        pre = f"step{step}_"
        draws = R.fixture_draws(z0, pre)
        trip = z0[pre + "triplets"].astype(np.int64)
        loss, terms = R.model_loss(p, feats, graphs, HP, draws, trip)
        want = z0[pre + "terms"]  # bpr, ssl_u, ssl_i, reg (the norms' sum over B, unweighted)
        assert abs(float(terms["bpr"]) - want[0]) <= 1e-5 * abs(want[0])
        assert abs(float(terms["ssl_u"]) - want[1]) <= 1e-5 * abs(want[1])
        assert abs(float(terms["ssl_i"]) - want[2]) <= 1e-5 * abs(want[2])
        assert abs(float(terms["reg"]) - HP["reg_weight"] * want[3]) <= 1e-5 * HP["reg_weight"] * abs(want[3])
        assert abs(float(loss) - float(z0[pre + "loss"])) <= 1e-5 * abs(float(z0[pre + "loss"]))
        grads = torch.autograd.grad(loss, [p[n] for n in R.NAMES])
        assert sorted(set(z0[pre + "no_grad"])) == ["image_embedding.weight", "text_embedding.weight"]
        new = {}
        for n, g in zip(R.NAMES, grads):
            want = z0[pre + "grad." + n].astype(np.float64)
            err = np.abs(g.numpy() - want).max()
            assert err <= 1e-5 * np.abs(want).max(), (n, err, np.abs(want).max())
            # Adam from the reference's float32 gradient, as its optimiser saw it
            q, m[n], v[n] = R.adam_step(p[n].detach(), R.tt(want), m[n], v[n], step + 1, HP["learning_rate"])
            after = (z0[pre + "param_xor." + n] ^ z0["init." + n].view(np.int32)).view(np.float32)
            assert np.abs(q.numpy() - after).max() <= 1e-5 * np.abs(after).max(), n
            new[n] = R.tt(after, grad=True)
        p = new


def test_init_is_bit_equal_to_the_fixture():
    from rsx.lgmrec import lgmrec_init
    from rsx.utils import init_seed

    z0, z = R.load("lgmrec_step0_small.npz"), R.load("lgmrec_small.npz")
    init_seed(HP["seed"])
    init = lgmrec_init(int(z["n_users"]), int(z["n_items"]), 64, 64, HP["hyper_num"], z["v_feat"].shape[1],
                       z["t_feat"].shape[1])
    assert sorted(init) == sorted(R.NAMES)
    for n in R.NAMES:
        assert np.array_equal(init[n].numpy().view(np.int32), z0["init." + n].view(np.int32)), n


def test_host_graphs_are_bit_exact():
    from rsx.lgmrec import lgmrec_graphs

    z0, z = R.load("lgmrec_step0_small.npz"), R.load("lgmrec_small.npz")
    nu, ni = int(z["n_users"]), int(z["n_items"])
    tu, ti = z["train_u"].astype(np.int64), z["train_i"].astype(np.int64)
    (rp, col, val), (rrp, rcol, rval), ninv = lgmrec_graphs(tu, ti, nu, ni)
    # R: the binary [n_users, n_items] interaction matrix (lgmrec.py:40-41)
    rr, rc, rv = csr_to_sorted(rrp, rcol, rval)
    o = np.lexsort((rc, rr))
    w = np.lexsort((ti, tu))
    assert rrp.size == nu + 1 and np.array_equal(rr[o], tu[w]) and np.array_equal(rc[o], ti[w])
    assert rv.dtype == np.float32 and (rv == 1.0).all() and rc.max() < ni
    r, c, v = csr_to_sorted(rp, col, val)
    order = np.lexsort((c, r))
    wr, wc, wv = coo_sorted(z0["norm_adj_idx"].astype(np.int64), z0["norm_adj_val"])
    assert np.array_equal(r[order], wr) and np.array_equal(c[order], wc)
    assert np.array_equal(np.asarray(v)[order].view(np.int32), wv.view(np.int32))
    want = np.asarray(z0["num_inters"]).reshape(-1)
    assert np.array_equal(ninv.view(np.int32), want.view(np.int32))


def _config(**over):
    c = dict(use_gpu=True, device="cuda", cf_model="lightgcn", embedding_size=64, feat_embed_dim=64, hyper_num=4,
             n_hyper_layer=1, keep_rate=0.5, n_mm_layers=2, n_ui_layers=2)
    c.update(over)
    return c


@pytest.mark.parametrize("over", [
    dict(use_gpu=False), dict(device="cpu"), dict(cf_model="ngcf"), dict(embedding_size=32, feat_embed_dim=32),
    dict(feat_embed_dim=128), dict(hyper_num=6), dict(hyper_num=0), dict(hyper_num=68), dict(n_hyper_layer=0),
    dict(n_hyper_layer=5), dict(keep_rate=0.0), dict(keep_rate=1.5), dict(n_mm_layers=5), dict(n_ui_layers=0),
    dict(n_ui_layers=5)], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_refused_configurations(over):
    from rsx.lgmrec import LGMRec

    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):
        LGMRec.check_config(_config(**over))


@pytest.mark.parametrize("v_dim,t_dim", [(48, None), (None, 24), (48, 6), (10, 24)])
def test_feature_tables_are_refused(v_dim, t_dim):
    """Fewer than both modalities, and a feature width that is no multiple of 4: the check the
    constructor runs (GeneralRecommender.require_features with need=2), on a stub that holds
    only the two tables, so that it needs no device."""
    import types

    from rsx import lgmrec as LG

    stub = types.SimpleNamespace(v_feat=None if v_dim is None else torch.zeros(5, v_dim),
                                 t_feat=None if t_dim is None else torch.zeros(5, t_dim))
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):
        LG.LGMRec.require_features(stub, LG.unsupported, need=2)
    LG.LGMRec.require_features(types.SimpleNamespace(v_feat=torch.zeros(5, 48), t_feat=torch.zeros(5, 24)),
                               LG.unsupported, need=2)


def test_hashed_gumbel_is_finite_at_both_ends():
    """The 32-bit draw -> u -> g map (rsx_lgm_gumbel_of_bits, the function the kernel calls): u stays
    inside (0, 1) and g finite for every draw, the all-zeros and all-ones draws included.  (With
    24 bits of the draw, k + 1/2 is no float32 at k = 2^24 - 1: it rounds to 2^24, u = 1, g = inf.)"""
    from rsx import _lib as L

    f = L.lib().rsx_lgm_gumbel_of_bits
    ends = [0, 1, 0x1FF, 0x200, 0x7FFFFFFF, 0x80000000, 0xFFFFFDFF, 0xFFFFFE00, 0xFFFFFFFE, 0xFFFFFFFF]
    rng = np.random.default_rng(0)
    bits = np.concatenate([ends, rng.integers(0, 1 << 32, 4096, dtype=np.uint64)]).astype(np.uint64)
    u, want = R.gumbel_of_bits(bits)
    assert u.dtype == np.float32 and u.min() == np.float32(2.0 ** -24) and u.max() == np.float32(1 - 2.0 ** -24)
    assert 0.0 < u.min() and u.max() < 1.0 and np.all(np.isfinite(want))
    got = np.array([f(int(b)) for b in bits], dtype=np.float64)
    assert np.all(np.isfinite(got)) and got.min() >= -2.82 and got.max() <= 16.64
    # float32 logs against the float64 map: the outer log's argument carries the inner one's rounding
    assert np.abs(got - want).max() <= 1e-5
    assert got[0] == got.min() and got[len(ends) - 1] == got.max() and np.all(np.diff(got[np.argsort(bits)]) >= 0)
    # the 24-bit form this replaces does reach u = 1
    assert (np.float32(2 ** 24 - 1) + np.float32(0.5)) * np.float32(2.0 ** -24) == np.float32(1.0)


def test_more_than_one_rank_is_refused(monkeypatch):
    import torch.distributed as dist

    from rsx.lgmrec import LGMRec

    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda: 2)
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):
        LGMRec.check_config(_config())


def test_accepted_configuration_and_registry():
    from rsx.lgmrec import LGMRec
    from rsx.utils import MODELS, get_model

    LGMRec.check_config(_config())
    LGMRec.check_config(_config(cf_model="mf", hyper_num=64, n_hyper_layer=4, keep_rate=1.0, embedding_size=128,
                                feat_embed_dim=128))
    assert MODELS["lgmrec"] == ("rsx.lgmrec", "LGMRec") and get_model("LGMRec") is LGMRec
    assert LGMRec.supports_graph_step


def test_library_symbols_and_limits():
    from rsx import _lib as L

    lib = L.lib()
    for name in ("rsx_lgm_ssl_ws_bytes", "rsx_lgm_ssl_fwd", "rsx_lgm_ssl_bwd", "rsx_lgm_assign_fwd",
                 "rsx_lgm_assign_bwd", "rsx_lgm_gumbel_of_bits", "rsx_lgm_hgnn_ws_bytes", "rsx_lgm_hgnn_reduce", "rsx_lgm_hgnn_expand",
                 "rsx_lgm_hgnn_rowdots", "rsx_lgm_loss_ws_bytes", "rsx_lgm_loss_fwd", "rsx_lgm_loss_bwd"):
        assert hasattr(lib, name) and name in L.EXPORTED, name
    # no B x N array: the workspace is the normalised table, the batch rows and the parts
    n, B, d = 19445, 2048, 64
    assert n * d * 4 <= lib.rsx_lgm_ssl_ws_bytes(n, B, d) < n * B * 4
    assert lib.rsx_lgm_ssl_ws_bytes(n, B, 32) == 0 and lib.rsx_lgm_ssl_ws_bytes(n, 65537, d) == 0
    assert lib.rsx_lgm_loss_ws_bytes(512, 64) > 0 and lib.rsx_lgm_loss_ws_bytes(512, 32) == 0
    assert lib.rsx_lgm_loss_ws_bytes(65537, 64) == 0 and lib.rsx_lgm_hgnn_ws_bytes(100, 0, 68, 64) == 0
    # unsupported shapes are refused before anything is launched (no GPU here)
    a = L.LgmSslArgs()
    a.T1 = a.T2 = a.idx = 16
    a.n, a.batch, a.d, a.tau = 10, 4, 48, 0.2
    assert lib.rsx_lgm_ssl_fwd(C.byref(a), C.c_void_p(16), C.c_void_p(16), 1 << 30, None) == L.RSX_ERR_UNSUPPORTED
    s = L.LgmAssignArgs()
    s.x = s.seed = 16
    s.n, s.H, s.ld, s.tau, s.keep_rate = 4, 6, 32, 0.2, 1.0
    assert lib.rsx_lgm_assign_fwd(C.byref(s), C.c_void_p(16), C.c_void_p(16), None, None) == L.RSX_ERR_UNSUPPORTED
    assert lib.rsx_lgm_hgnn_expand(C.c_void_p(16), 32, 4, C.c_void_p(16), 8, 48, C.c_void_p(16), None) \
        == L.RSX_ERR_UNSUPPORTED
    q = L.LgmLossArgs()
    q.C = q.Mv = q.Mt = q.Gv = q.Gt = q.triplets = 16
    q.n_users, q.n_items, q.batch, q.d = 5, 7, 8, 32
    assert lib.rsx_lgm_loss_fwd(C.byref(q), C.c_void_p(16), C.c_void_p(16), 1 << 30, None) == L.RSX_ERR_UNSUPPORTED
