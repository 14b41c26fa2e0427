"""MMGCN without a GPU: the float64 restatement (tests/mmgcn_ref.py) against the reference's own
run (tests/golden/mmgcn_step0_small.npz, mmgcn_small.npz), the initial draws, the mean operator,
the layer's hand-derived backward, the one-modality forms, configuration and refusals."""
import os
import types

import numpy as np
import pytest
import torch

import mmgcn_ref as R

NAMES = R.names()


def close(got, want, tol=1e-5):
    """Within `tol` of the tensor's scale (its largest magnitude)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = np.abs(want).max()
    err = np.abs(got - want).max() if want.size else 0.0
    assert err <= tol * scale, (err, scale)


def init(z):
    """(P float32 by name, C float32 constants) of seed 999 through the model's own draws."""
    from rsx.mmgcn import mmgcn_init
    from rsx.utils import init_seed

    init_seed(999)
    v, t, E, result = mmgcn_init(int(z["n_users"]), int(z["n_items"]), 64, z["v_feat"].shape[1], z["t_feat"].shape[1])
    P = {f"{m}_gcn.{n}": p.detach() for m, g in (("v", v), ("t", t)) for n, p in g.named_parameters()}
    C = {"id_embedding": E, "v_gcn.preference": v.preference, "t_gcn.preference": t.preference, "result": result}
    return P, C


def setup(dtype=torch.float64):
    z0, z = R.load("mmgcn_step0_small.npz"), R.load("mmgcn_small.npz")
    nu, ni = int(z["n_users"]), int(z["n_items"])
    P32, C32 = init(z)
    P = R.cast(P32, dtype)
    C = R.consts({k: v for k, v in C32.items() if k != "result"}, dtype)
    feats = {"v": torch.from_numpy(z["v_feat"]).to(dtype), "t": torch.from_numpy(z["t_feat"]).to(dtype)}
    A = R.mean_operator(z["train_u"].astype(np.int64), z["train_i"].astype(np.int64), nu, ni, dtype)
    return z0, z, nu, P, C, feats, A


def test_fixture_sizes_hparams_and_margin():
    for f in ("mmgcn_small.npz", "mmgcn_step0_small.npz"):
        assert os.path.getsize(os.path.join(R.GOLD, f)) < (1 << 20), f
    z0, z = R.load("mmgcn_step0_small.npz"), R.load("mmgcn_small.npz")
    hp = R.hparams(z0)
    assert float(hp["learning_rate"]) == 0.001 and float(hp["reg_weight"]) == 0.001 and int(hp["seed"]) == 999
    assert (int(hp["embedding_size"]), int(hp["n_layers"])) == (64, 2)
    assert (z["v_feat"].shape[1], z["t_feat"].shape[1]) == (48, 32)
    # the capture's own condition: every pre-activation the feature seeds reach is farther from
    # zero than twice the reference-vs-restatement difference on its tensor
    keys = [k for k in z0.files if k.startswith("step0_preact_min.")]
    assert len(keys) == 18
    for k in keys:
        assert float(z0[k]) > float(z0[k.replace("_min.", "_thr.")]) > 0, k
    # what the seeds cannot move (rows that read the preferences alone) is listed, not hidden
    assert len(z0["step0_preact_seed_fixed_inside"]) <= 1


def test_initial_draws_follow_the_reference():
    z = R.load("mmgcn_small.npz")
    S = R.strides(z)
    P, C = init(z)
    assert tuple(P) == NAMES
    for n in NAMES:
        assert np.array_equal(R.rows(P[n].numpy(), S["param"]).view(np.int32), z["init." + n].view(np.int32)), n
    for k in R.CONSTS:
        assert np.array_equal(C[k].numpy()[::S["const"]].view(np.int32), z["const." + k].view(np.int32)), k
        assert not C[k].requires_grad


def test_mean_operator_host():
    from rsx.mmgcn import mean_operator
    from helpers import coo_sorted

    z = R.load("mmgcn_small.npz")
    nu, ni = int(z["n_users"]), int(z["n_items"])
    r, c, v = mean_operator(z["train_u"], z["train_i"], nu, ni)
    wr, wc, wv = coo_sorted(z["mean_adj_idx"].astype(np.int64), z["mean_adj_val"])
    assert np.array_equal(r, wr) and np.array_equal(c, wc) and np.array_equal(v.view(np.int32), wv.view(np.int32))
    # a duplicate interaction counts twice; user 2 and item 1 have no edge: no entry, a zero row
    r, c, v = mean_operator([0, 0, 1], [0, 0, 2], 3, 3)
    dense = np.zeros((6, 6))
    dense[r, c] = v
    want = R.mean_operator([0, 0, 1], [0, 0, 2], 3, 3).numpy()
    assert np.array_equal(dense, want.astype(np.float32))
    assert dense[0, 3] == 1.0 and dense[3, 0] == 1.0 and not dense[2].any() and not dense[4].any()
    r, c, v = mean_operator([0, 0, 0], [0, 0, 1], 1, 2)
    assert dict(zip(zip(r.tolist(), c.tolist()), v.tolist())) == {(0, 1): np.float32(2 / 3), (0, 2): np.float32(1 / 3),
                                                                 (1, 0): 1.0, (2, 0): 1.0}


def test_restatement_two_steps_vs_fixture():
    """Representation, per-layer x, loss words and every gradient of the first step, loss words and
    parameters of the second, in float64, at tests/test_grcn_cpu.py's bounds: 1e-5 of the tensor's
    scale (the loss words 1e-5 relative), the parameters after the restatement's own Adam within
    that plus what Adam turns the gradient difference into (grcn_ref.adam_tolerance), on fewer
    than one element in a thousand."""
    z0, z, nu, P, C, feats, A = setup()
    hp, S = R.hparams(z0), R.strides(z0)
    lr = float(hp["learning_rate"])
    adam = R.Adam(P, lr)
    dgs, grefs = {n: [] for n in NAMES}, {n: [] for n in NAMES}
    for step in range(2):
        pre = f"step{step}_"
        trip = torch.from_numpy(z0[pre + "triplets"].astype(np.int64))
        keep = {}
        rep, terms, grads = R.step(P, C, feats, A, trip, nu, float(hp["reg_weight"]), keep)
        close(rep[::S["rep"]], z0[pre + "representation"])
        for m in R.MODS:
            for k in (1, 2, 3):
                close(keep[m][f"x{k}"].detach()[::S["rep"]], z0[f"{pre}x.{m}.{k}"])
        for j, name in enumerate(("loss", "bpr", "reg")):
            want = float(z0[pre + name])
            assert abs(float(terms[j]) - want) <= 1e-5 * abs(want), (name, float(terms[j]), want)
        for n in NAMES:
            close(R.rows(grads[n].numpy(), S["grad"]), z0[pre + "grad." + n])
        adam.step(grads)
        for n in NAMES:
            gref = R.rows(z0[pre + "grad." + n].astype(np.float64), S["param"] // S["grad"])
            grefs[n].append(gref)
            dgs[n].append(R.rows(grads[n].numpy(), S["param"]) - gref)
            want = z0[pre + "param." + n].astype(np.float64)
            err = np.abs(R.rows(P[n].detach().numpy(), S["param"]) - want)
            extra = R.adam_tolerance(dgs[n], grefs[n], lr)
            tol = 1e-5 * np.abs(want).max() + extra
            share = float((extra > 1e-5 * np.abs(want).max()).mean())
            print(f"  step {step} param {n}: err {err.max():.3e}, scale {np.abs(want).max():.3e}, share {share:.4f}")
            assert (err <= tol).all(), (step, n, float((err - tol).max()))
            assert share < 1e-3, (step, n, share)


@pytest.mark.parametrize("d,w,n", [(8, 8, 7), (8, 12, 5)])
def test_layer_backward_by_finite_differences_and_autograd(d, w, n):
    x = R.layer_inputs(d, w, n, 3)
    go = torch.randn(n, d, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    got = R.layer_backward(go, **x)
    leaves = {k: v.clone().requires_grad_(True) for k, v in x.items()}
    (R.layer(**leaves) * go).sum().backward()
    for k, name in (("a", "g_a"), ("x", "g_x"), ("E", "g_E"), ("Wc", "dWc"), ("Wl", "dWl"), ("bl", "dbl"), ("Wg", "dWg"),
                    ("bg", "dbg")):
        assert torch.allclose(got[name], leaves[k].grad, rtol=1e-12, atol=1e-14), name
    f = lambda **kw: float((R.layer(**kw) * go).sum())  # noqa: E731
    eps = 1e-6
    rng = np.random.default_rng(0)
    for k, name in (("a", "g_a"), ("x", "g_x"), ("Wc", "dWc"), ("Wl", "dWl"), ("Wg", "dWg"), ("bg", "dbg")):
        for _ in range(6):
            idx = tuple(int(rng.integers(0, s)) for s in x[k].shape)
            hi, lo = {kk: v.clone() for kk, v in x.items()}, {kk: v.clone() for kk, v in x.items()}
            hi[k][idx] += eps
            lo[k][idx] -= eps
            fd = (f(**hi) - f(**lo)) / (2 * eps)
            assert abs(fd - float(got[name][idx])) <= 1e-6 * max(1.0, abs(fd)), (name, idx, fd, float(got[name][idx]))


def test_flagged_rows_rate_of_the_gpu_tests_inputs():
    """The GPU tests' layer inputs (tests/test_gpu_mmgcn.py builds them through the same function and
    seeds) flag about one row in a hundred; at most 5 % is what those tests allow."""
    assert R.layer_inputs(8, 8, 3, 1)["Wg"].shape == (8, 16)
    for d, n in ((64, 5), (64, 65), (128, 37), (64, 1001)):
        x = R.layer_inputs(d, d, n, 100 + n)
        k = {}
        R.layer(**x, keep=k)
        share = float(R.near_zero_rows([k["ph"], k["pu"], k["po"]]).float().mean())
        assert share <= 0.05, (d, n, share)


@pytest.mark.parametrize("only", ["v", "t"])
def test_one_modality_forms_run(only):
    z0, z, nu, P, C, feats, A = setup()
    feats = {only: feats[only]}
    P = {k: v for k, v in P.items() if k.startswith(only + "_gcn.")}
    trip = torch.from_numpy(z0["step0_triplets"].astype(np.int64))
    rep, terms, grads = R.step(P, C, feats, A, trip, nu, 0.001)
    assert rep.shape == (nu + int(z["n_items"]), 64) and all(torch.isfinite(t) for t in terms)
    assert set(grads) == set(R.names((only,))) and all(g.abs().max() > 0 for g in grads.values())
    both = R.loss(C, {"v": 0, "t": 0}, rep, trip, nu, 0.001)[2]
    # the preference word of the regulariser is the image branch's alone (mmgcn.py:94-95)
    assert (float(both) == float(terms[2])) == (only == "v")


def test_yaml_config_and_registry():
    from rsx.config import Config
    from rsx.mmgcn import MMGCN
    from rsx.utils import MODELS, get_model

    c = Config("MMGCN", "baby", {"use_gpu": False})
    assert c["embedding_size"] == 64 and c["n_layers"] == 2
    assert c["reg_weight"] == [0, 1e-05, 1e-04, 1e-03, 1e-02, 0.1]
    assert c["learning_rate"] == [0.0001, 0.0005, 0.001, 0.005, 0.01]
    assert set(c["hyper_parameters"]) >= {"reg_weight", "learning_rate"} and c["is_multimodal_model"] is True
    assert MODELS["mmgcn"] == ("rsx.mmgcn", "MMGCN") and get_model("MMGCN") is MMGCN
    assert MMGCN.supports_graph_step and MMGCN.graph_step_persistent
    with pytest.raises(ValueError, match="MMGCN"):  # the message lists the models, the new one included
        get_model("NoSuchModel")


def test_cpu_configuration_is_refused():
    from rsx.config import Config
    from rsx.utils import get_model

    c = Config("MMGCN", "baby", {"use_gpu": False})
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        get_model("MMGCN")(c, None)


def _config(**over):
    c = dict(use_gpu=True, device="cuda", embedding_size=64)
    c.update(over)
    return c


@pytest.mark.parametrize("over", [dict(use_gpu=False), dict(device="cpu"), dict(embedding_size=32), dict(embedding_size=256)],
                         ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_refused_configurations(over):
    from rsx.mmgcn import MMGCN

    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        MMGCN.check_config(_config(**over))
    MMGCN.check_config(_config())
    MMGCN.check_config(_config(embedding_size=128))


def test_more_than_one_rank_is_refused(monkeypatch):
    import torch.distributed as dist

    from rsx.mmgcn import MMGCN

    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda: 2)
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        MMGCN.check_config(_config())


@pytest.mark.parametrize("v_dim,t_dim", [(None, None), (10, None), (48, 6), (48, 48), (None, 40)])
def test_feature_tables_are_refused(v_dim, t_dim):
    """No table at all, a width that is no multiple of 4, a text width that is no multiple of 32:
    the check the constructor runs, on a stub that holds only the two tables."""
    from rsx import mmgcn as M

    def stub(v, t):
        s = types.SimpleNamespace(v_feat=None if v is None else torch.zeros(5, v), t_feat=None if t is None else torch.zeros(5, t))
        s.require_features = types.MethodType(M.MMGCN.require_features, s)
        return s

    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        M.MMGCN.check_features(stub(v_dim, t_dim))
    for ok in ((48, 32), (48, None), (None, 384), (4096, 384)):
        M.MMGCN.check_features(stub(*ok))


def test_library_symbols_and_limits():
    from rsx import _lib as L

    lib = L.lib()
    for name in ("rsx_mmgcn_layer_fwd", "rsx_mmgcn_layer_bwd", "rsx_mmgcn_loss_ws_bytes", "rsx_mmgcn_loss_fwd",
                 "rsx_mmgcn_loss_bwd"):
        assert hasattr(lib, name) and name in L.EXPORTED, name
    assert lib.rsx_mmgcn_loss_ws_bytes(512, 64) > 0 and lib.rsx_mmgcn_loss_ws_bytes(65536, 128) > 0
    assert lib.rsx_mmgcn_loss_ws_bytes(65537, 64) == 0 and lib.rsx_mmgcn_loss_ws_bytes(512, 32) == 0
