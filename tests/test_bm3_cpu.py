"""BM3 without a GPU: the float64 restatement (tests/bm3_ref.py) against the reference's own
first step (tests/golden/bm3_step0_small.npz, tools/capture_golden.py --only bm3), the pair
loader against the reference's batch streams (bm3_small.npz), the initial draws, model
resolution and refusals, the ctypes struct and the workspace query.

Bounds.  The reference ran in float32; the restatement is float64, so the difference is the
reference's own rounding: loss 1e-6 relative (tests/test_mf_cpu.py's bound for the same
kind of quantity), gradients 1e-5 of the tensor's largest magnitude (the bound
tests/test_gpu_smore.py puts on a first step, relative to scale)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import bm3_ref as R

GOLD = R.GOLD


def _keep(z):
    return {s: R.unpack_keep(z["keep_" + s], 64) for s in R.STREAMS}


def test_mask_packing_round_trips():
    rng = np.random.default_rng(0)
    k = rng.random((13, 96)) < 0.7
    w = R.pack_keep(k)
    assert w.shape == (13, 3) and w.dtype == np.uint32
    assert np.array_equal(R.unpack_keep(w, 96), k)
    assert bool(w[0, 1] >> 5 & 1) == bool(k[0, 37])


def test_restatement_vs_reference_first_step():
    z = R.load_fixture("step0")
    nu, ni = int(z["n_users"]), int(z["n_items"])
    A = R.dense_adj(z["adj_idx"], z["adj_val"], nu + ni)
    assert np.array_equal(A, A.T)
    p = z["pairs"].astype(np.int64)
    out, g = R.model_loss_grad(R.init_params(z), A, 2, p[0], p[1], 0.1, 2.0, 0.3, _keep(z))
    want = float(z["step0_loss"])
    print(f"loss {out[0]:.9f} vs reference {want:.9f}")
    assert abs(out[0] - want) <= 1e-6 * abs(want)
    assert np.all(np.abs(out[1:] - z["step0_terms"]) <= 1e-6 * np.maximum(np.abs(z["step0_terms"]), 1e-3))
    for n in R.NAMES:
        w = z["step0_grad." + n]
        err, scale = float(np.abs(g[n] - w).max()), float(np.abs(w).max())
        print(f"  {n}: err {err:.3e}, scale {scale:.3e}, err / scale {err / scale:.2e}")
        assert err <= 1e-5 * scale, n


def test_restatement_without_modalities_and_all_dropped_row():
    """T / V absent: their terms are 0 and gT / gV None; a target row with every element
    dropped gives cosine 0 (term contribution 1 / B), not NaN."""
    rng = np.random.default_rng(2)
    nu, ni, d, B = 5, 4, 32, 9
    E, H = rng.standard_normal((nu + ni, d)), rng.standard_normal((ni, d))
    P, pb = rng.standard_normal((d, d)), rng.standard_normal(d)
    u, i = rng.integers(0, nu, B), rng.integers(0, ni, B)
    keep = {"item": np.ones((ni, d), bool)}
    keep["item"][i[0]] = False
    r = R.loss_grad(E, H, None, None, P, pb, u, i, nu, 0.1, 2.0, 0.5, keep)
    assert np.all(np.isfinite(r["out"])) and r["gT"] is None and r["gV"] is None
    assert np.all(r["out"][3:7] == 0)
    full = R.loss_grad(E, H, None, None, P, pb, u, i, nu, 0.1, 2.0, 0.5, None)
    assert r["out"][1] != full["out"][1]
    # finite differences of the total in E (the targets carry no gradient: hold them fixed)
    eps = 1e-6
    for (row, col) in ((u[1], 3), (nu + i[2], 7)):
        Ep, Em = E.copy(), E.copy()
        Ep[row, col] += eps
        Em[row, col] -= eps

        # the stop-gradient makes a plain finite difference see the targets move too; compare
        # the analytic gradient with the difference of a loss whose targets are frozen
        def frozen(Ex):
            XI = Ex[nu:] + H
            xu, xi = Ex[:nu][u], XI[i]
            tu = (E[:nu] * 1.0)[u] / 0.5
            ti = ((E[nu:] + H) * keep["item"])[i] / 0.5
            cu, _ = R._cos(xu @ P.T + pb, ti)
            ci, _ = R._cos(xi @ P.T + pb, tu)
            reg = (np.sqrt((Ex[:nu] ** 2).sum()) + np.sqrt((XI ** 2).sum())) / ni
            return (1 - cu.mean()) + (1 - ci.mean()) + 0.1 * reg

        fd = (frozen(Ep) - frozen(Em)) / (2 * eps)
        assert abs(fd - r["gE"][row, col]) <= 1e-6 * max(1.0, abs(fd)), (row, col, fd, r["gE"][row, col])


def test_initial_parameters_bit_equal():
    from rsx.bm3 import bm3_init
    from rsx.utils import init_seed

    z = R.load_fixture("step0")
    init_seed(999)
    got = bm3_init(int(z["n_users"]), int(z["n_items"]), 64, z["v_feat"].shape[1], z["t_feat"].shape[1])
    assert list(got) == [n for n in R.NAMES if "embedding.weight" not in n or n.startswith(("user", "item"))]
    for n, t in got.items():
        assert np.array_equal(t.numpy().view(np.int32), z["init." + n].view(np.int32)), n
    z2 = R.load_fixture("small")
    for n, t in got.items():
        assert np.array_equal(t.numpy().view(np.int32), z2["init." + n].view(np.int32)), n


def test_model_resolves_and_config_loads():
    from rsx.config import Config
    from rsx.utils import MODELS, get_model

    cls = get_model("BM3")
    assert cls.__name__ == "BM3" and cls.supports_graph_step and not cls.supports_fused_step
    c = Config("BM3", "baby", {"use_gpu": False})
    assert c["use_neg_sampling"] is False and c["cl_weight"] == 2.0 and c["embedding_size"] == 64
    assert c["n_layers"] == [1, 2] and c["dropout"] == [0.3, 0.5] and c["reg_weight"] == [0.1, 0.01]
    assert set(c["hyper_parameters"]) >= {"n_layers", "reg_weight", "dropout"}
    with pytest.raises(ValueError, match="BM3"):  # the message lists the models, the new one included
        get_model("NoSuchModel")
    assert "bm3" in MODELS


def test_cpu_configuration_is_refused():
    from rsx.config import Config
    from rsx.utils import get_model

    c = Config("BM3", "baby", {"use_gpu": False})
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):
        get_model("BM3")(c, None)


def test_unsupported_width_and_world_size_are_refused(monkeypatch):
    import torch.distributed as dist

    from rsx.bm3 import BM3

    cfg = {"use_gpu": True, "device": torch.device("cuda", 0), "embedding_size": 48}
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED.*embedding_size 48"):
        BM3.check_config(cfg)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    cfg["embedding_size"] = 64
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED.*world size 2"):
        BM3.check_config(cfg)


def _loader(tmp_path, model, extra, drop_key=None):
    from rsx.config import Config
    from rsx.data import RecDataset, TrainDataLoader
    from rsx.utils import init_seed

    d = tmp_path / "data" / "baby"
    d.mkdir(parents=True, exist_ok=True)
    shutil.copy(os.path.join(GOLD, "gold_small.inter"), d / "baby.inter")
    cfg = dict(data_path=str(tmp_path / "data") + "/", train_batch_size=512, use_gpu=False, rsx_sampler="host")
    cfg.update(extra)
    c = Config(model, "baby", cfg)
    if drop_key:
        c.final_config_dict.pop(drop_key)
    tr, _, _ = RecDataset(c).split()
    train = TrainDataLoader(c, tr, batch_size=512, shuffle=True)
    init_seed(999)
    train.pretrain_setup()
    return train


def test_host_pair_loader_yields_the_reference_stream(tmp_path):
    z = R.load_fixture("small")
    train = _loader(tmp_path, "BM3", {})
    assert train.use_neg_sampling is False
    for e in range(2):
        got = list(train)
        want = R.epoch_pairs(z, e)
        assert len(got) == len(want) == int(z[f"epoch{e}_nbatch"]) == 6
        assert got[-1].shape == (2, 462)  # 3,022 = 5 * 512 + 462
        for g, w in zip(got, want):
            assert g.dtype == torch.int64 and np.array_equal(g.numpy(), w)


@pytest.mark.parametrize("extra", [{}, {"use_neg_sampling": True}])
def test_triplet_batches_unchanged(tmp_path, extra, golden):
    """With the key absent or True the loader yields what it did: the reference's triplet
    stream the LightGCN fixture records, bit for bit."""
    z = golden("lightgcn_small")
    train = _loader(tmp_path, "LightGCN", extra, drop_key=None if extra else "use_neg_sampling")
    assert ("use_neg_sampling" in train.config) == bool(extra)
    assert train.use_neg_sampling is True
    got = torch.cat(list(train), dim=1).numpy()
    assert got.shape[0] == 3 and np.array_equal(got, z["epoch0_triplets"].astype(np.int64))


def test_bm3_struct_layout_symbols_and_refusals(tmp_path):
    from rsx import _lib as L

    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    inc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
    src = tmp_path / "sz.c"
    src.write_text('#include "rsx.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu %zu",'
                   ' sizeof(rsx_bm3_args), offsetof(rsx_bm3_args, E), offsetof(rsx_bm3_args, batch),'
                   ' offsetof(rsx_bm3_args, seed), offsetof(rsx_bm3_args, ws)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run([cc, "-I", inc, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    A = L.Bm3Args
    assert got == [C.sizeof(A), A.E.offset, A.batch.offset, A.seed.offset, A.ws.offset]
    lib = L.lib()
    for sym in ("rsx_bm3_ws_bytes", "rsx_bm3_loss_fwd", "rsx_bm3_loss_bwd"):
        assert sym in L.EXPORTED and hasattr(lib, sym)
    # refused before any launch (no GPU needed)
    assert lib.rsx_bm3_ws_bytes(512, 48) == 0 and lib.rsx_bm3_ws_bytes(0, 64) == 0
    a = A()
    a.n_users, a.n_items, a.d, a.batch = 4, 4, 48, 8
    assert lib.rsx_bm3_loss_fwd(C.byref(a), None, None) == L.RSX_ERR_UNSUPPORTED
    a.d = 256
    assert lib.rsx_bm3_loss_bwd(C.byref(a), None, None, None, None, None, None, None) == L.RSX_ERR_UNSUPPORTED
    a.d = 64
    assert lib.rsx_bm3_loss_fwd(C.byref(a), None, None) == 1001  # null tables: RSX_ERR_ARG


@pytest.mark.parametrize("d", [32, 64, 128])
def test_workspace_serves_every_shorter_batch(d):
    from rsx import _lib as L

    lib = L.lib()
    ws = np.array([lib.rsx_bm3_ws_bytes(b, d) for b in range(1, 2049)], dtype=np.int64)
    assert np.all(ws > 0) and np.all(np.diff(ws) >= 0)
    # the four [4 B, d] row buffers and the weight gradient's own workspace fit
    wg = np.array([lib.rsx_linear_rows_wgrad_ws_bytes(4 * b, d, d) for b in range(1, 2049)], dtype=np.int64)
    assert np.all(ws >= 4 * 4 * np.arange(1, 2049) * d * 4 + wg)


def test_graph_is_the_lightgcn_laplacian():
    """bm3.py:58-84 builds lightgcn.py's D^-1/2 A D^-1/2: the host builder that
    rsx_adj_build(ADJ_LIGHTGCN) equals bit for bit reproduces the captured norm_adj."""
    from helpers import coo_sorted, csr_to_sorted
    from rsx import graph

    z = R.load_fixture("step0")
    nu, ni = int(z["n_users"]), int(z["n_items"])
    rp, col, val = graph.lightgcn_norm_adj(z["train_u"], z["train_i"], nu, ni)
    r0, c0, v0 = csr_to_sorted(rp, col, val)
    r1, c1, v1 = coo_sorted(z["adj_idx"].astype(np.int64), z["adj_val"])
    assert np.array_equal(r0, r1) and np.array_equal(c0, c1)
    assert np.array_equal(v0.view(np.int32), v1.view(np.int32))
