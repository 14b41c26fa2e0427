"""GRCN's model layer without a GPU: the host graph structure (rsx.grcn.target_csr), the initial
draws (rsx.grcn.grcn_init) against the reference's own, the kernels' float64 contracts
(tests/grcn_kernels_ref.py: explicit formulas, no autograd) against autograd of the restatement
(tests/grcn_ref.py), the registry entry and the configuration."""
import os

import numpy as np
import pytest
import torch

import grcn_kernels_ref as K
import grcn_ref as R
import test_grcn_cpu as T

NAMES, load = T.NAMES, T.load


def _check_structure(tu, ti, nu, ni):
    from rsx.grcn import target_csr

    tu, ti = np.asarray(tu, dtype=np.int64), np.asarray(ti, dtype=np.int64)
    rowptr, col, rev, edge_slot = target_csr(tu, ti, nu, ni)
    n, E = nu + ni, tu.size
    assert rowptr.dtype == np.int64 and col.dtype == np.int32 and rev.dtype == np.int32
    assert rowptr.shape == (n + 1,) and rowptr[0] == 0 and rowptr[-1] == 2 * E and np.all(np.diff(rowptr) >= 0)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    # the three identities of rev
    assert np.array_equal(rev[rev], np.arange(2 * E))
    assert np.array_equal(col[rev], row)
    assert np.array_equal(row[rev], col)
    # edge_slot is a permutation that carries the reference's edges (both_ways order) to their slots
    assert np.array_equal(np.sort(edge_slot), np.arange(2 * E))
    ei2 = R.both_ways(R.edge_index(tu, ti, nu)).numpy()
    assert np.array_equal(col[edge_slot], ei2[0]) and np.array_equal(row[edge_slot], ei2[1])
    # rows sorted by source, copies by occurrence; the k-th copy pairs with the k-th copy
    key = row.astype(np.int64) * n + col
    assert np.all(np.diff(key) >= 0)
    inv = np.empty(2 * E, dtype=np.int64)
    inv[edge_slot] = np.arange(2 * E)  # the reference's edge of a slot
    same = np.diff(key) == 0
    assert np.all(np.diff(inv)[same] > 0)
    assert np.array_equal(inv[rev], (inv + E) % (2 * E))
    return rowptr, col, rev, edge_slot


def test_target_csr_on_the_fixture_edges():
    z = load("grcn_small.npz")
    rowptr, *_ = _check_structure(z["train_u"], z["train_i"], int(z["n_users"]), int(z["n_items"]))
    assert rowptr[-1] == 6044


def test_target_csr_on_a_hand_graph():
    """3 users, 3 items; (0, 0) twice; user 2 and item 1 (node 4) isolated."""
    rowptr, col, rev, edge_slot = _check_structure([0, 0, 1, 0], [0, 0, 2, 2], 3, 3)
    assert rowptr.tolist() == [0, 3, 4, 4, 6, 6, 8]
    assert col.tolist() == [3, 3, 5, 5, 0, 0, 0, 1]
    assert rev.tolist() == [4, 5, 6, 7, 0, 1, 2, 3]
    assert edge_slot.tolist() == [4, 5, 7, 6, 0, 1, 3, 2]


def test_grcn_init_is_the_reference_draw():
    from rsx.grcn import grcn_init
    from rsx.utils import init_seed

    z = load("grcn_small.npz")
    init_seed(999)
    id_gcn, v, t, conf, result = grcn_init(int(z["n_users"]), int(z["n_items"]), 64, 64, z["v_feat"].shape[1],
                                           z["t_feat"].shape[1])
    m = torch.nn.Module()
    m.id_gcn, m.v_gcn, m.t_gcn, m.model_specific_conf = id_gcn, v, t, conf
    named = dict(m.named_parameters())
    assert tuple(named) == NAMES
    for n, p in named.items():
        assert np.array_equal(p.detach().numpy().view(np.int32), z["init." + n].view(np.int32)), n
    assert np.array_equal(result.numpy().view(np.int32), z["init.result"].view(np.int32))
    assert not result.requires_grad


def _graph(z, nu):
    from rsx.grcn import target_csr

    rowptr, col, rev, edge_slot = target_csr(z["train_u"], z["train_i"], nu, int(z["n_items"]))
    return K.Graph(rowptr, col, rev), torch.from_numpy(edge_slot)


@pytest.mark.parametrize("mods", [("v", "t"), ("v",)], ids="".join)
def test_kernel_contracts_chain_to_the_restatement(mods):
    """grcn_kernels_ref.step (explicit forward and backward formulas, slot order, the preferences
    normalised once) against autograd of grcn_ref.step (the literal routing loop): alphas, weights,
    representation, the loss words and all eight gradients within 1e-9 of scale."""
    z0, z, nu, P, feats, ei = T.setup()
    feats = {m: feats[m] for m in mods}
    names = [n for n in NAMES if n[0] not in "vt" or n[0] in mods]
    P = {n: (P[n] if n != "model_specific_conf" else P[n].detach()[:, :len(mods)].clone().requires_grad_(True))
         for n in names}
    trip = torch.from_numpy(z0["step0_triplets"].astype(np.int64))
    g, slot = _graph(z, nu)
    fw, terms, grads = R.step(P, feats, ei, trip, nu, 3, 0.001)
    with torch.no_grad():
        kfw, kterms, kgrads = K.step({n: p.detach() for n, p in P.items()}, feats, g, trip, nu, 0.001)

    def close(name, got, want):
        scale = float(want.abs().max())
        err = float((got - want).abs().max())
        print(f"  {name}: err {err:.3e}, scale {scale:.3e}")
        assert err <= 1e-9 * scale, name

    for j, m in enumerate(mods):
        close("alpha_" + m, kfw["alpha"][j][slot], fw["alphas"][j].detach())
    close("weight", kfw["weight"][slot], fw["weight"].detach())
    close("representation", kfw["representation"], fw["representation"].detach())
    for j, name in enumerate(("loss", "bpr", "reg")):
        assert abs(float(kterms[j]) - float(terms[j])) <= 1e-9 * abs(float(terms[j])), name
    assert set(kgrads) == set(names)
    for n in names:
        close("grad " + n, kgrads[n], grads[n])
    if len(mods) == 2:
        assert K.min_relative_gap(g, kfw["alpha"], P["model_specific_conf"].detach()) > 1e-5


def test_each_contract_against_autograd_on_general_rows():
    """The attention on rows of norm 10 (scores reach 100), its backward with an external alpha
    gradient, the refine and the id GCN, each against autograd of grcn_ref's own functions."""
    z0, z, nu, _, _, ei = T.setup()
    g, slot = _graph(z, nu)
    ei2 = R.both_ways(ei)
    gen = torch.Generator().manual_seed(3)
    x = torch.nn.functional.normalize(torch.randn(g.n, 16, dtype=torch.float64, generator=gen)) * 10
    x.requires_grad_(True)
    h, a = R.gat(x, ei2)
    g_rep = torch.randn(g.n, 16, dtype=torch.float64, generator=gen)
    dext = torch.randn(g.nnz, dtype=torch.float64, generator=gen)
    ((x + h) * g_rep).sum().add((a * dext[slot]).sum()).backward()
    alpha, rep = K.attn_fwd(g, x.detach())
    assert float((x.detach() * x.detach()).sum(1).max()) > 99
    assert torch.allclose(alpha[slot], a.detach(), rtol=1e-12, atol=1e-300)
    assert torch.allclose(rep, (x + h).detach(), rtol=1e-12, atol=1e-13)
    dx = K.attn_bwd(g, g_rep, dext, x.detach(), alpha)
    assert float((dx - x.grad).abs().max()) <= 1e-11 * float(x.grad.abs().max())
    # refine + id GCN
    conf = (torch.randn(g.n, 2, dtype=torch.float64, generator=gen) * 0.06).requires_grad_(True)
    a2 = torch.rand(g.nnz, dtype=torch.float64, generator=gen)
    alphas = [alpha.clone().requires_grad_(True), a2.requires_grad_(True)]
    E = torch.randn(g.n, 16, dtype=torch.float64, generator=gen).requires_grad_(True)
    w, arg = R.refined_weight([t[slot] for t in alphas], conf, ei)
    G = torch.randn(g.n, 16, dtype=torch.float64, generator=gen)
    (R.egcn(E, ei2, w) * G).sum().backward()
    with torch.no_grad():
        val, valT = K.refine_fwd(g, [t.detach() for t in alphas], conf.detach())
        assert torch.equal(val[slot], w) and torch.equal(valT[g.rev], val) and float((val > 0).double().mean()) > 0.2
        xn, den = K.normalize_fwd(E.detach())
        h1, id_rep = K.id_gcn_fwd(g, val, xn)
        dxn, dw = K.id_gcn_bwd(g, val, valT, G, h1, xn)
        das, dconf = K.refine_bwd(g, [t.detach() for t in alphas], conf.detach(), dw)
        dE = K.normalize_bwd(dxn, xn, den)
    for got, want in ((dE, E.grad), (dconf, conf.grad), (das[0], alphas[0].grad), (das[1], alphas[1].grad)):
        assert float((got - want).abs().max()) <= 1e-11 * float(want.abs().max())


def test_registry_and_configuration():
    import yaml

    from rsx.utils import MODELS

    assert MODELS["grcn"] == ("rsx.grcn", "GRCN")
    import rsx

    path = os.path.join(os.path.dirname(os.path.dirname(rsx.__file__)), "configs", "model", "GRCN.yaml")
    c = yaml.safe_load(open(path))
    assert c["embedding_size"] in (64, 128) and c["latent_embedding"] in (64, 128) and c["n_layers"] >= 0
    assert isinstance(c["reg_weight"], list) and isinstance(c["learning_rate"], list)
    assert set(c["hyper_parameters"]) == {"reg_weight", "learning_rate"}
    from rsx.config import Config

    cfg = Config("GRCN", "baby", {})
    assert cfg["latent_embedding"] == 64 and cfg["n_layers"] == 3
    from rsx.grcn import GRCN, unsupported

    assert GRCN.supports_graph_step and GRCN.graph_step_persistent
    assert str(unsupported("x")).startswith("RSX_ERR_UNSUPPORTED")


def test_cpu_configuration_widths_and_world_size_are_refused(monkeypatch):
    import torch.distributed as dist

    from rsx.config import Config
    from rsx.grcn import GRCN
    from rsx.utils import get_model

    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):
        get_model("GRCN")(Config("GRCN", "baby", {"use_gpu": False}), None)
    cfg = {"use_gpu": True, "device": torch.device("cuda", 0), "embedding_size": 32, "latent_embedding": 64, "n_layers": 3}
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED.*embedding_size 32"):
        GRCN.check_config(cfg)
    cfg.update(embedding_size=64, latent_embedding=256)
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED.*latent_embedding 256"):
        GRCN.check_config(cfg)
    cfg.update(latent_embedding=128, n_layers=0)
    GRCN.check_config(cfg)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED.*world size 2"):
        GRCN.check_config(cfg)


def test_library_refuses_shapes_without_a_gpu():
    """The argument checks run before any launch: they answer here too."""
    import ctypes as C

    from rsx import _lib as L

    lib = L.lib()
    assert lib.rsx_grcn_hub_degree() >= 32
    assert lib.rsx_grcn_loss_ws_bytes(512, 192) > 0 and lib.rsx_grcn_loss_ws_bytes(65536, 256) > 0
    for batch, width in ((65537, 192), (0, 192), (512, 320), (512, 64), (512, 160)):
        assert lib.rsx_grcn_loss_ws_bytes(batch, width) == 0
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.rsx_grcn_attn_fwd(p, p, p, 4, 8, 32, p, p, None) == L.RSX_ERR_UNSUPPORTED
    assert lib.rsx_grcn_attn_fwd(p, p, p, 4, 1 << 31, 64, p, p, None) == L.RSX_ERR_UNSUPPORTED
    assert lib.rsx_grcn_refine_fwd(3, p, p, p, p, p, 4, 8, p, p, None) == L.RSX_ERR_UNSUPPORTED
    assert lib.rsx_grcn_edge_dots(p, p, p, p, p, p, 4, 8, 256, p, None) == L.RSX_ERR_UNSUPPORTED
    assert lib.rsx_grcn_attn_fwd(None, p, p, 4, 8, 64, p, p, None) == 1001
