"""LATTICE without a GPU: the float64 restatement (tests/lattice_ref.py) against the reference's
own run (tests/golden/lattice_step0_small.npz, lattice_small.npz), the library's new symbols
and struct layouts, the host-built UI graph, and the refusals.

Bounds: the restatement is float64, the reference float32, so they differ by the reference's
own rounding: losses 1e-5 relative, gradients rtol 1e-3 with atol 1e-5 of the tensor's scale
(the GPU first-step test's bound), parameters after two epochs 5e-5 of scale (the project's
end-to-end bound)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import lattice_ref as R


def test_fixture_files_are_small_and_complete():
    for f in ("lattice_small.npz", "lattice_step0_small.npz"):
        assert os.path.getsize(os.path.join(R.GOLD, f)) < (1 << 20), f
    z = R.load_fixture()
    assert tuple(n for n in R.NAMES if "init." + n in z) == R.NAMES
    assert z["v_feat"].shape == (int(z["n_items"]), 48) and z["t_feat"].shape == (int(z["n_items"]), 24)
    for s in (0, 1):
        have = {n for n in R.NAMES if f"step{s}_grad.{n}" in z}
        assert have | set(z[f"step{s}_none"].tolist()) == set(R.NAMES) and not have & set(z[f"step{s}_none"].tolist())
    # the build batch reaches every parameter, the steady batch only the two id tables
    assert z["step0_none"].size == 0
    assert set(z["step1_none"].tolist()) == set(R.GRAPH_ONLY)
    for ep in (0, 1):
        assert f"epoch{ep}_param.modal_weight" in z
        for m in R.MODS:
            assert z[f"build{ep}_{m}_idx"].shape == (int(z["n_items"]), R.HPARAMS["knn_k"])
            assert z[f"build{ep}_{m}_gap"].min() >= 1e-4  # the capture's condition
    total = sum(int(z[f"epoch{e}_nbatch"]) for e in (0, 1))
    assert z["epoch_losses"].shape == (2,) and total == len(R.batches(z, 0)) + len(R.batches(z, 1))
    assert R.batches(z, 0)[-1].shape[1] < R.HPARAMS["train_batch_size"]  # the last batch is shorter


def test_original_graphs_and_forward_match_the_fixture():
    z = R.load_fixture()
    k = R.HPARAMS["knn_k"]
    for m, feat in (("image", z["v_feat"]), ("text", z["t_feat"])):
        idx, val, _ = R.original_graph(feat, k)
        assert np.array_equal(np.sort(idx.numpy(), 1), np.sort(z[f"orig_{m}_idx"].astype(np.int64), 1)), m
        want = R.dense_lists(z[f"orig_{m}_idx"], z[f"orig_{m}_val"], feat.shape[0])
        np.testing.assert_allclose(R.dense_lists(idx, val, feat.shape[0]).numpy(), want.numpy(), rtol=1e-5, atol=1e-7)
    model = R.Model(R.init_params(z), R.ui_dense(z), R.orig_dense(z))
    u, i = model.eval_tables()
    np.testing.assert_allclose(u, z["fwd_user"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(i, z["fwd_item"], rtol=1e-5, atol=1e-6)
    for m, idx in zip(R.MODS, model.idx):
        assert np.array_equal(np.sort(idx.numpy(), 1), np.sort(z[f"build0_{m}_idx"].astype(np.int64), 1)), m


def test_restatement_reproduces_the_reference_run():
    z = R.load_fixture()
    run = R.two_epochs(z)
    n0 = int(z["epoch0_nbatch"])
    for s in (0, 1):
        want = float(z[f"step{s}_loss"])
        print(f"step {s}: loss {run['losses'][s]:.8f} vs reference {want:.8f}")
        assert abs(run["losses"][s] - want) <= 1e-5 * abs(want)
        g = run["grads"][s]
        assert {n for n in R.NAMES if g[n] is None} == set(z[f"step{s}_none"].tolist())
        for n in R.NAMES:
            if g[n] is None:
                continue
            w = z[f"step{s}_grad.{n}"]
            scale = float(np.abs(w).max())
            print(f"  step {s} grad {n}: err {np.abs(g[n] - w).max():.3e}, scale {scale:.3e}")
            np.testing.assert_allclose(g[n], w, rtol=1e-3, atol=1e-5 * scale, err_msg=f"step {s} {n}")
    sums = [sum(run["losses"][:n0]), sum(run["losses"][n0:])]
    print(f"epoch losses {sums} vs reference {z['epoch_losses']}")
    np.testing.assert_allclose(sums, z["epoch_losses"], rtol=1e-5)
    for ep in (0, 1):
        for m, idx in zip(R.MODS, run["idx"][ep]):
            assert np.array_equal(np.sort(idx, 1), np.sort(z[f"build{ep}_{m}_idx"].astype(np.int64), 1)), (ep, m)
        for n in R.NAMES:
            w = z[f"epoch{ep}_param.{n}"]
            scale = float(np.abs(w).max())
            err = float(np.abs(run["epoch_params"][ep][n] - w).max())
            print(f"  epoch {ep} {n}: err / scale {err / scale:.2e} (bound 5e-5)")
            assert err <= 5e-5 * scale, (ep, n)


def test_ui_graph_host_matches_the_fixture():
    from rsx import graph

    z = R.load_fixture()
    nu, ni = int(z["n_users"]), int(z["n_items"])
    rp, col, val, val_t = graph.lattice_norm_adj(z["train_u"], z["train_i"], nu, ni)
    idx = z["norm_adj_idx"].astype(np.int64)
    order = np.lexsort((idx[1], idx[0]))
    rows = np.repeat(np.arange(nu + ni), np.diff(rp))
    assert np.array_equal(rows, idx[0][order]) and np.array_equal(col.astype(np.int64), idx[1][order])
    assert np.array_equal(val.view(np.int32), z["norm_adj_val"][order].view(np.int32))
    # val_t: the transpose's values on the same structure
    A = np.zeros((nu + ni, nu + ni), dtype=np.float32)
    A[rows, col] = val
    assert np.array_equal(val_t, A.T[rows, col])
    assert np.allclose(A.sum(1), 1.0, atol=1e-6)  # row-normalised, self loops included


def test_model_resolves_and_config_loads():
    from rsx.config import Config
    from rsx.utils import MODELS, get_model

    cls = get_model("LATTICE")
    assert cls.__name__ == "LATTICE" and cls.supports_graph_step and not cls.graph_step_persistent
    assert MODELS["lattice"] == ("rsx.lattice", "LATTICE")
    c = Config("LATTICE", "baby", {"use_gpu": False})
    assert c["embedding_size"] == 64 and c["feat_embed_dim"] == 64 and c["weight_size"] == [64, 64]
    assert c["n_layers"] == 1 and c["knn_k"] == 10 and c["lambda_coeff"] == 0.9 and c["cf_model"] == "lightgcn"
    assert c["reg_weight"] == [0.0, 1e-05, 1e-04, 1e-03] and all(isinstance(x, float) for x in c["reg_weight"])
    assert "reg_weight" in c["hyper_parameters"] and "learning_rate" in c["hyper_parameters"]
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED"):  # no GPU in this configuration
        cls(c, None)


def test_unsupported_configurations_are_refused(monkeypatch):
    import torch.distributed as dist

    from rsx.lattice import LATTICE

    ok = {"use_gpu": True, "device": torch.device("cuda", 0), "embedding_size": 64, "feat_embed_dim": 64, "knn_k": 10,
          "cf_model": "lightgcn", "n_layers": 1}
    LATTICE.check_config(ok)
    LATTICE.check_config(dict(ok, cf_model="mf", embedding_size=128, feat_embed_dim=128, knn_k=32, n_layers=0))
    for key, bad, what in (("cf_model", "ngcf", "cf_model 'ngcf'"), ("embedding_size", 32, "embedding_size 32"),
                           ("feat_embed_dim", 48, "feat_embed_dim 48"), ("knn_k", 33, "knn_k 33"),
                           ("n_layers", 5, "n_layers 5"), ("use_gpu", False, "use_gpu"),
                           ("device", torch.device("cpu"), "no ROCm GPU")):
        with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED.*" + what):
            LATTICE.check_config(dict(ok, **{key: bad}))
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(RuntimeError, match="^RSX_ERR_UNSUPPORTED.*world size 2"):
        LATTICE.check_config(ok)


NEW_SYMBOLS = ("rsx_lattice_ws_bytes", "rsx_lattice_loss_fwd", "rsx_lattice_loss_bwd", "rsx_lattice_graph",
               "rsx_lattice_prop", "rsx_lattice_graph_bwd_ws_bytes", "rsx_lattice_graph_bwd")


def test_library_symbols_and_refusals():
    from rsx import _lib as L

    lib = L.lib()
    for sym in NEW_SYMBOLS:
        assert sym in L.EXPORTED and hasattr(lib, sym), sym
    assert lib.rsx_lattice_ws_bytes(512, 64) >= 512 * 64 * 4 + 512 * 4 + 3 * 512 * 4
    assert lib.rsx_lattice_ws_bytes(513, 128) > lib.rsx_lattice_ws_bytes(512, 128)
    assert lib.rsx_lattice_ws_bytes(0, 64) == 0 and lib.rsx_lattice_ws_bytes(512, 32) == 0
    assert lib.rsx_lattice_ws_bytes(65536, 64) > 0 and lib.rsx_lattice_ws_bytes(65537, 64) == 0
    assert lib.rsx_lattice_graph_bwd_ws_bytes(200, 10, 2) >= 200 * 40 * 4
    assert lib.rsx_lattice_graph_bwd_ws_bytes(200, 33, 2) == 0 and lib.rsx_lattice_graph_bwd_ws_bytes(200, 10, 3) == 0

    # refused before any launch (no GPU needed; the pointers are never read)
    def loss(d=64, batch=8, E=16, H=16, ws=16, ws_bytes=1 << 30, bs=512.0):
        a = L.LatticeArgs(E, H, 16, 5, 7, batch, d, 0.5, bs, 0)
        return lib.rsx_lattice_loss_fwd(C.byref(a), C.c_void_p(16), C.c_void_p(ws) if ws else None, ws_bytes, None)

    assert loss(d=32) == L.RSX_ERR_UNSUPPORTED and loss(batch=65537) == L.RSX_ERR_UNSUPPORTED
    assert loss(batch=0) == 1001 and loss(E=None) == 1001 and loss(H=None) == 1001 and loss(ws=None) == 1001
    assert loss(E=20) == 1001 and loss(bs=0.0) == 1001
    assert loss(ws_bytes=64) == 1003
    a = L.LatticeArgs(16, 16, 16, 5, 7, 8, 64, 0.5, 512.0, 0)
    assert lib.rsx_lattice_loss_bwd(C.byref(a), None, C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), 1 << 30,
                                    None) == 1001  # no upstream gradient

    def graph(n=200, k=10, n_mod=2, f=64, mw=16):
        g = L.LatticeGraph()
        g.n, g.k, g.n_mod, g.f, g.lam = n, k, n_mod, f, 0.9
        for m in range(2):
            g.F[m] = g.idx[m] = g.oidx[m] = g.oval[m] = g.invn[m] = g.a[m] = 16
        g.modal_weight = mw
        g.w = g.r = g.dis = g.col = g.val = 16
        return g

    assert lib.rsx_lattice_graph(C.byref(graph(k=33)), None) == L.RSX_ERR_UNSUPPORTED
    assert lib.rsx_lattice_graph(C.byref(graph(n=7, k=8)), None) == L.RSX_ERR_UNSUPPORTED
    assert lib.rsx_lattice_graph(C.byref(graph(f=48)), None) == L.RSX_ERR_UNSUPPORTED
    assert lib.rsx_lattice_graph(C.byref(graph(n_mod=3)), None) == 1001
    assert lib.rsx_lattice_graph(C.byref(graph(mw=None)), None) == 1001
    # the transposed product needs the transpose index
    assert lib.rsx_lattice_prop(C.byref(graph()), C.c_void_p(16), C.c_void_p(32), 64, 1, None) == 1001
    assert lib.rsx_lattice_prop(C.byref(graph()), C.c_void_p(16), C.c_void_p(32), 32, 0, None) == L.RSX_ERR_UNSUPPORTED


def test_new_struct_layouts_match_header(tmp_path):
    """The two new ctypes mirrors have the sizes and field offsets gcc gives the C structs."""
    from rsx import _lib as L

    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    inc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
    src = tmp_path / "sz.c"
    src.write_text('#include "rsx.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu %zu %zu",'
                   ' sizeof(rsx_lattice_args), offsetof(rsx_lattice_args, batch_size), sizeof(rsx_lattice_graph_args),'
                   ' offsetof(rsx_lattice_graph_args, F), offsetof(rsx_lattice_graph_args, modal_weight),'
                   ' offsetof(rsx_lattice_graph_args, tedge)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run([cc, "-I", inc, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(L.LatticeArgs), L.LatticeArgs.batch_size.offset, C.sizeof(L.LatticeGraph),
                   L.LatticeGraph.F.offset, L.LatticeGraph.modal_weight.offset, L.LatticeGraph.tedge.offset]
