"""SELFCFED_LGN without a GPU: the float64 restatement (tests/selfcf_ref.py) against the reference's
own first step (tests/golden/selfcfed_lgn_step0_small.npz, tools/capture_golden.py --only selfcf),
the initial draws, the graph, the registry entry, every refusal at construction, the reverse-slot
permutation on the host, the ctypes struct and the host-side refusals of the entry points.

Bounds.  The reference ran in float32; the restatement is float64, so the difference is the
reference's own rounding: loss and terms 1e-6 relative, gradients 1e-5 of the tensor's largest
magnitude (tests/test_bm3_cpu.py's bounds for the same kind of quantities)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import selfcf_ref as R


def _step0():
    z = R.load_fixture("step0")
    nu, ni = int(z["n_users"]), int(z["n_items"])
    keep = np.stack([R.unpack_keep(z["keep_user"], 64), R.unpack_keep(z["keep_item"], 64)])
    return z, nu, ni, keep


def test_bit_packing_round_trips():
    rng = np.random.default_rng(0)
    for n in (1, 31, 32, 33, 6044):
        k = rng.random(n) < 0.6
        w = R.pack_bits(k)
        assert w.shape == ((n + 31) // 32,) and w.dtype == np.uint32
        assert np.array_equal(R.unpack_bits(w, n), k)
    k = rng.random((2, 5, 128)) < 0.7
    assert np.array_equal(R.unpack_keep(R.pack_keep(k), 128), k)
    assert bool(R.pack_keep(k)[1, 2, 1] >> 5 & 1) == bool(k[1, 2, 37])


def test_fixture_draws_are_consistent():
    """The recorded edge draw: Â's values are val * scale (an f32 product) on the kept entries and 0
    elsewhere, the scale is float32(1 / (1 - rate)), and the two directions of an interaction were
    drawn independently (the dropped graph is not symmetric)."""
    z, nu, ni, _ = _step0()
    keep = R.unpack_bits(z["edge_keep"], z["adj_val"].size)
    assert z["scale"] == np.float32(1.0 / (1.0 - float(z["rate"])))
    assert np.array_equal(R.dropped(z["adj_val"], keep, z["scale"]).view(np.int32), z["drop_val"].view(np.int32))
    A = R.dense_adj(z["adj_idx"], z["drop_val"], nu + ni)
    assert not np.array_equal(A, A.T)
    assert list(z["param_names"]) == list(R.NAMES)


def test_restatement_vs_reference_first_step():
    z, nu, ni, keep = _step0()
    A = R.dense_adj(z["adj_idx"], z["drop_val"].astype(np.float64), nu + ni)
    p = z["pairs"].astype(np.int64)
    out, g = R.model_loss_grad(R.init_params(z), A, 2, p[0], p[1], 0.1, 0.3, keep, scale=float(np.float32(1 / 0.7)))
    want = float(z["step0_loss"])
    print(f"loss {out[0]:.9f} vs reference {want:.9f}")
    assert abs(out[0] - want) <= 1e-6 * abs(want)
    assert np.all(np.abs(out[1:] - z["step0_terms"]) <= 1e-6 * np.maximum(np.abs(z["step0_terms"]), 1e-3))
    for n in R.NAMES:
        w = z["step0_grad." + n]
        err, scale = float(np.abs(g[n] - w).max()), float(np.abs(w).max())
        print(f"  {n}: err {err:.3e}, scale {scale:.3e}, stored reference-vs-restatement {float(z['refdiff.grad.' + n]):.3e}")
        assert err <= 1e-5 * scale, n


def test_restatement_all_dropped_row_and_frozen_targets():
    """A target row with every element dropped gives cosine 0, not NaN; the analytic gradient
    equals the finite difference of the loss with its targets held fixed (the stop-gradient)."""
    rng = np.random.default_rng(2)
    nu, ni, d, B = 5, 4, 32, 9
    E = rng.standard_normal((nu + ni, d))
    P, pb = rng.standard_normal((d, d)), rng.standard_normal(d)
    u, i = rng.integers(0, nu, B), rng.integers(0, ni, B)
    keep = np.ones((2, B, d), bool)
    keep[1, 0] = False
    r = R.loss_grad(E, P, pb, u, i, nu, 0.1, 0.5, keep)
    assert np.all(np.isfinite(r["out"])) and np.all(np.isfinite(r["gE"]))
    one = R.loss_grad(E, P, pb, u[:1], i[:1], nu, 0.1, 0.5, keep[:, :1])
    assert one["out"][1] == 0.0
    tg = r["tg"]

    def frozen(Ex):
        xu, xi = Ex[u], Ex[nu + i]
        cu, _ = R._cos(xu @ P.T + pb, tg[B:])
        ci, _ = R._cos(xi @ P.T + pb, tg[:B])
        return -cu.mean() / 2 - ci.mean() / 2 + 0.1 * 0.5 * ((xu ** 2).sum() + (xi ** 2).sum())

    eps = 1e-6
    for (row, col) in ((u[1], 3), (nu + i[2], 7)):
        Ep, Em = E.copy(), E.copy()
        Ep[row, col] += eps
        Em[row, col] -= eps
        fd = (frozen(Ep) - frozen(Em)) / (2 * eps)
        assert abs(fd - r["gE"][row, col]) <= 1e-6 * max(1.0, abs(fd)), (row, col, fd, r["gE"][row, col])
    off = np.setdiff1d(np.arange(nu + ni), np.concatenate([u, nu + i]))
    assert np.all(r["gE"][off] == 0)


def test_initial_parameters_bit_equal():
    from rsx.selfcf import selfcf_init
    from rsx.utils import init_seed

    init_seed(999)
    got = selfcf_init(400, 200, 64)
    assert set(got) == set(R.NAMES)
    for which in ("step0", "small"):
        z = R.load_fixture(which)
        for n, t in got.items():
            assert np.array_equal(t.numpy().view(np.int32), z["init." + n].view(np.int32)), (which, n)


def test_graph_is_the_lightgcn_laplacian():
    """encoders.py:39-78 builds lightgcn.py's D^-1/2 A D^-1/2: the host builder that
    rsx_adj_build(ADJ_LIGHTGCN) equals bit for bit reproduces the captured sparse_norm_adj."""
    from helpers import coo_sorted, csr_to_sorted
    from rsx import graph

    z = R.load_fixture("step0")
    rp, col, val = graph.lightgcn_norm_adj(z["train_u"], z["train_i"], int(z["n_users"]), int(z["n_items"]))
    r0, c0, v0 = csr_to_sorted(rp, col, val)
    r1, c1, v1 = coo_sorted(z["adj_idx"].astype(np.int64), z["adj_val"])
    assert val.size == 6044 and np.array_equal(r0, r1) and np.array_equal(c0, c1)
    assert np.array_equal(v0.view(np.int32), v1.view(np.int32))


def test_model_resolves_and_config_loads():
    from rsx.config import Config
    from rsx.utils import MODELS, get_model

    assert MODELS["selfcfed_lgn"] == ("rsx.selfcf", "SELFCFED_LGN")
    cls = get_model("SELFCFED_LGN")
    assert cls.__name__ == "SELFCFED_LGN" and cls.supports_graph_step and cls.graph_step_persistent
    assert not cls.supports_fused_step
    c = Config("SELFCFED_LGN", "baby", {"use_gpu": False})
    assert c["use_neg_sampling"] is False and c["embedding_size"] == 64 and c["is_multimodal_model"] is False
    assert c["n_layers"] == [1, 2] and c["dropout"] == [0.1, 0.2, 0.5]
    assert c["reg_weight"] == [0.1, 0.01, 0.001, 0.0001, 0.00001, 0.0]
    assert set(c["hyper_parameters"]) >= {"n_layers", "dropout", "reg_weight"}
    with pytest.raises(ValueError, match="SELFCFED_LGN"):  # the message lists the models, the new one included
        get_model("NoSuchModel")


def test_cpu_configuration_is_refused():
    from rsx.config import Config
    from rsx.utils import get_model

    c = Config("SELFCFED_LGN", "baby", {"use_gpu": False})
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):
        get_model("SELFCFED_LGN")(c, None)


def test_every_construction_refusal(monkeypatch):
    import torch.distributed as dist

    from rsx.selfcf import SELFCFED_LGN

    ok = {"use_gpu": True, "device": torch.device("cuda", 0), "embedding_size": 64, "dropout": 0.3, "n_layers": None}
    SELFCFED_LGN.check_config(ok)  # n_layers None is the reference's 3
    for key, value, what in (("embedding_size", 32, "embedding_size 32"), ("embedding_size", 256, "embedding_size 256"),
                             ("dropout", 1.0, "dropout 1.0"), ("dropout", -0.1, "dropout -0.1"),
                             ("n_layers", -1, "n_layers -1"), ("use_gpu", False, "use_gpu"),
                             ("device", torch.device("cpu"), "no ROCm GPU")):
        with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED.*" + what):
            SELFCFED_LGN.check_config({**ok, key: value})
    for n_layers in (0, 1, 4, 7):
        SELFCFED_LGN.check_config({**ok, "n_layers": n_layers})
    SELFCFED_LGN.check_edges(2 ** 30 - 1)
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED.*directed entries"):
        SELFCFED_LGN.check_edges(2 ** 30)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED.*world size 2"):
        SELFCFED_LGN.check_config(ok)


def _csr(n, pairs):
    """CSR (rowptr, col) of the symmetric structure with the given (row, col) entries, both
    directions, repeats kept, sorted by row then column."""
    r = np.array([p[0] for p in pairs] + [p[1] for p in pairs])
    c = np.array([p[1] for p in pairs] + [p[0] for p in pairs])
    order = np.lexsort((c, r))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=rowptr[1:])
    return torch.from_numpy(rowptr), torch.from_numpy(c[order].astype(np.int32)), r[order]


def test_reverse_slots_on_the_host():
    """A graph with an empty row (node 2) and a repeated interaction (0 - 4 twice): rev is an
    involution without fixed points, pairs the k-th copy with the k-th copy and points at the
    transposed entry."""
    from rsx.selfcf import reverse_slots

    rowptr, col, row = _csr(6, [(0, 3), (0, 4), (0, 4), (1, 3), (1, 5)])
    assert rowptr[2] == rowptr[3]  # the empty row
    rev = reverse_slots(rowptr, col).numpy().astype(np.int64)
    nnz = col.numel()
    assert rev.dtype == np.int64 and sorted(rev) == list(range(nnz))
    assert np.array_equal(rev[rev], np.arange(nnz)) and np.all(rev != np.arange(nnz))
    assert np.array_equal(col.numpy()[rev], row) and np.array_equal(row[rev], col.numpy())
    copies = np.flatnonzero((row == 0) & (col.numpy() == 4))
    assert copies.size == 2 and rev[copies[0]] < rev[copies[1]]
    # the fixture's graph
    z = R.load_fixture("step0")
    idx = z["adj_idx"].astype(np.int64)
    n = int(z["n_users"] + z["n_items"])
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(idx[0], minlength=n), out=rp[1:])
    rev = reverse_slots(torch.from_numpy(rp), torch.from_numpy(idx[1].astype(np.int32))).numpy()
    assert np.array_equal(rev[rev], np.arange(6044)) and np.array_equal(idx[1][rev], idx[0])
    # a structure that is not symmetric is refused
    with pytest.raises(RuntimeError, match="not symmetric"):
        reverse_slots(torch.tensor([0, 1, 1]), torch.tensor([1], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="not sorted"):
        reverse_slots(torch.tensor([0, 2, 3, 4]), torch.tensor([2, 1, 0, 0], dtype=torch.int32))


def test_struct_layout_symbols_and_host_refusals(tmp_path):
    from rsx import _lib as L

    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    inc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
    src = tmp_path / "sz.c"
    src.write_text('#include "rsx.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu %zu %zu",'
                   ' sizeof(rsx_selfcf_args), offsetof(rsx_selfcf_args, E), offsetof(rsx_selfcf_args, users),'
                   ' offsetof(rsx_selfcf_args, p_drop), offsetof(rsx_selfcf_args, mask), offsetof(rsx_selfcf_args, ws_bytes));'
                   ' return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run([cc, "-I", inc, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    A = L.SelfcfArgs
    assert got == [C.sizeof(A), A.E.offset, A.users.offset, A.p_drop.offset, A.mask.offset, A.ws_bytes.offset]
    lib = L.lib()
    for sym in ("rsx_selfcf_edge_drop", "rsx_selfcf_ws_bytes", "rsx_selfcf_loss_fwd", "rsx_selfcf_loss_bwd",
                "rsx_selfcf_targets", "rsx_selfcf_eval_tables"):
        assert sym in L.EXPORTED and hasattr(lib, sym)
    # refused before any launch (no GPU needed)
    assert [lib.rsx_selfcf_ws_bytes(512, 32), lib.rsx_selfcf_ws_bytes(0, 64), lib.rsx_selfcf_ws_bytes(65537, 64)] == [0, 0, 0]
    assert lib.rsx_selfcf_ws_bytes(65536, 128) > 0
    a = A()
    a.n_users, a.n_items, a.d, a.batch = 4, 4, 32, 8
    assert lib.rsx_selfcf_loss_fwd(C.byref(a), None, None) == L.RSX_ERR_UNSUPPORTED
    a.d = 256
    assert lib.rsx_selfcf_loss_bwd(C.byref(a), None, None, None, None, None) == L.RSX_ERR_UNSUPPORTED
    a.d = 64
    assert lib.rsx_selfcf_loss_fwd(C.byref(a), None, None) == 1001  # null tables: RSX_ERR_ARG
    assert lib.rsx_selfcf_eval_tables(None, None, None, 4, 4, 32, None, None, None) == L.RSX_ERR_UNSUPPORTED
    assert lib.rsx_selfcf_eval_tables(None, None, None, 4, 4, 64, None, None, None) == 1001
    assert lib.rsx_selfcf_edge_drop(None, None, 4, None, None, None, None, None, None, None) == 1001


@pytest.mark.parametrize("d", [64, 128])
def test_workspace_serves_every_shorter_batch(d):
    from rsx import _lib as L

    lib = L.lib()
    b = np.arange(1, 2049)
    ws = np.array([lib.rsx_selfcf_ws_bytes(int(x), d) for x in b], dtype=np.int64)
    assert np.all(ws > 0) and np.all(np.diff(ws) >= 0)
    # the three [2 B, d] row buffers, the row list, the keys and the weight gradient's workspace fit
    wg = np.array([lib.rsx_linear_rows_wgrad_ws_bytes(2 * int(x), d, d) for x in b], dtype=np.int64)
    assert np.all(ws >= 3 * 2 * b * d * 4 + 2 * b * 8 + 3 * b * 4 + wg)
