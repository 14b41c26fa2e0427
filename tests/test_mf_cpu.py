"""BPR / VBPR without a GPU: model resolution and refusal, the ctypes struct, and the CPU
restatement (tests/mf_ref.py) against the reference's own outputs in
tests/golden/{bpr,vbpr}_small.npz (tools/capture_golden.py --only mf).

Tolerances are those tests/test_oracle_golden.py applies to the same LightGCN quantities
(first-step loss 1e-6 relative, gradients rtol 1e-5 / atol 1e-9) and tests/test_gpu_e2e.py's
training bounds (parameters atol 5e-5, metrics 1e-4): the last test shows that an f32 torch
run of the same steps stays inside the bounds the GPU tests then rely on."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mf_ref as R
import rsx_oracle as O
from helpers import eval_lists, metric_dict, train_mask_pairs

MODELS = ("BPR", "VBPR")
REG = 2.0  # the first value of the reg_weight list (the fixture's hparams)


def test_models_resolve_and_configs_load():
    from rsx.config import Config
    from rsx.utils import get_model

    for name in MODELS:
        cls = get_model(name)
        assert cls.__name__ == name and cls.supports_fused_step
        c = Config(name, "baby", {"use_gpu": False})
        assert c["embedding_size"] == 64 and c["reg_weight"][0] == REG and "reg_weight" in c["hyper_parameters"]
    assert Config("VBPR", "baby", {})["is_multimodal_model"] is True
    assert Config("BPR", "baby", {})["is_multimodal_model"] is False


@pytest.mark.parametrize("name", MODELS)
def test_cpu_configuration_is_refused(name):
    from rsx.config import Config
    from rsx.utils import get_model

    c = Config(name, "baby", {"use_gpu": False})
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):
        get_model(name)(c, None)


def test_unsupported_width_is_refused():
    from rsx.mf import MFRecommenderMixin

    cfg = {"use_gpu": True, "device": torch.device("cuda", 0), "embedding_size": 48}
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED.*embedding_size 48"):
        MFRecommenderMixin.check_config(cfg)


def test_more_than_one_rank_is_refused(monkeypatch):
    import torch.distributed as dist

    from rsx.mf import MFRecommenderMixin

    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    cfg = {"use_gpu": True, "device": torch.device("cuda", 0), "embedding_size": 64}
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED.*world size 2"):
        MFRecommenderMixin.check_config(cfg)


@pytest.mark.parametrize("d,F,B", [(64, 384, 2048), (32, 384, 2048), (64, 72, 2048), (128, 384, 2048),
                                   (64, 4480, 2048), (64, 72, 512), (64, 0, 2048)])
def test_workspace_serves_every_shorter_batch(d, F, B):
    """An engine sizes its workspace once for the configured batch; a shorter batch (the
    last of an epoch) must never need more.  The split-reduction plan's slot count is not
    monotonic in the row count, so the size queries return a bound that is."""
    from rsx import _lib as L

    lib = L.lib()
    mf = np.array([lib.rsx_mf_ws_bytes(b, d, F) for b in range(1, B + 1)], dtype=np.int64)
    assert np.all(mf > 0) and np.all(np.diff(mf) >= 0)
    if F:
        wg = np.array([lib.rsx_linear_rows_wgrad_ws_bytes(2 * b, d, F) for b in range(1, B + 1)], dtype=np.int64)
        exact = np.array([lib.rsx_linear_wgrad_ws_bytes(2 * b, d, F) for b in range(1, B + 1)], dtype=np.int64)
        assert np.all(np.diff(wg) >= 0)
        assert np.all(wg >= exact + 64 * d * 4)  # the plan's partial slots and the bias partials fit


def test_mf_step_struct_layout_matches_header(tmp_path):
    from rsx import _lib as L

    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    inc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
    src = tmp_path / "sz.c"
    src.write_text('#include "rsx.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu",'
                   ' sizeof(rsx_mf_step_args), offsetof(rsx_mf_step_args, X), offsetof(rsx_mf_step_args, adam),'
                   ' offsetof(rsx_mf_step_args, tag)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run([cc, "-I", inc, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(L.MfStep), L.MfStep.X.offset, L.MfStep.adam.offset, L.MfStep.tag.offset]
    for sym in ("rsx_linear_rows_fwd", "rsx_linear_rows_wgrad", "rsx_linear_rows_wgrad_ws_bytes", "rsx_mf_step",
                "rsx_mf_loss_grad", "rsx_mf_ws_bytes"):
        assert sym in L.EXPORTED and hasattr(L.lib(), sym)
    # shapes the kernels are not compiled for are refused before any launch (no GPU needed)
    assert L.lib().rsx_mf_ws_bytes(512, 48, 0) == 0 and L.lib().rsx_mf_ws_bytes(512, 64, 70) == 0
    assert L.lib().rsx_linear_rows_fwd(None, None, None, None, 8, 16, 48, None, 48, None) == L.RSX_ERR_UNSUPPORTED
    assert L.lib().rsx_linear_rows_fwd(None, None, None, None, 8, 18, 64, None, 64, None) == L.RSX_ERR_UNSUPPORTED


@pytest.mark.parametrize("name", MODELS)
def test_initial_parameters_bit_equal(name):
    from rsx.mf import bpr_init, vbpr_init
    from rsx.utils import init_seed

    z = R.load_fixture(name)
    nu, ni = int(z["n_users"]), int(z["n_items"])
    init_seed(999)
    X = R.features(z)
    got = bpr_init(nu, ni, 64) if name == "BPR" else vbpr_init(nu, ni, 64, X.shape[1])
    for g, n in zip(got, R.NAMES[name]):
        assert np.array_equal(g.numpy().view(np.int32), z["init." + n].view(np.int32)), n


@pytest.mark.parametrize("name", MODELS)
def test_first_step_vs_reference(name):
    z = R.load_fixture(name)
    ref = R.MFRef(R.fixture_params(z, name, "init."), REG, R.features(z))
    trip = R.epoch_batches(z, 0)[0]
    loss, grads = ref.loss_grad(trip)
    assert abs(loss - float(z["step0_loss"])) <= 1e-6 * abs(float(z["step0_loss"]))
    for g, n in zip(grads, R.NAMES[name]):
        np.testing.assert_allclose(g.numpy(), z["step0_grad." + n], rtol=1e-5, atol=1e-9, err_msg=n)
    ref.step(trip)
    for p, n in zip(ref.numpy(), R.NAMES[name]):
        np.testing.assert_allclose(p, z["step0_param." + n], rtol=0, atol=1e-6, err_msg=n)


@pytest.mark.parametrize("name", MODELS)
def test_training_bound_headroom(name):
    """The fixture's epochs on the fixture's triplets in f32 torch: parameters within atol
    5e-5 of the reference's, metric dicts within 1e-4, top-50 equal outside flagged ties."""
    z = R.load_fixture(name)
    epochs = R.FIXTURE[name][1]
    ref = R.MFRef(R.fixture_params(z, name, "init."), REG, R.features(z))
    for e in range(epochs):
        for trip in R.epoch_batches(z, e):
            ref.step(trip)
    last = epochs - 1
    worst = 0.0
    for p, n in zip(ref.numpy(), R.NAMES[name]):
        worst = max(worst, float(np.abs(p - z[f"epoch{last}_param." + n]).max()))
        np.testing.assert_allclose(p, z[f"epoch{last}_param." + n], rtol=0, atol=5e-5, err_msg=n)
    print(f"{name}: max |param - reference| after {epochs} epochs = {worst:.3e} (bound 5e-5)")
    for split in ("valid", "test"):
        tag = f"epoch{last}_{split}"
        users = z[tag + "_users"]
        scores = ref.scores(users)
        r, c = train_mask_pairs(z, users)
        scores[r, c] = -1e10
        _, idx = O.canonical_topk(scores, 50)
        want = z[tag + "_topk_idx"].astype(np.int64)
        ties = z[tag + "_inner_tie"] | z[tag + "_boundary_tie"]
        assert np.all(np.all(idx == want, axis=1) | ties)
        got = O.metrics_reference(idx, eval_lists(z, split))
        for k, v in metric_dict(z, tag).items():
            assert abs(got[k] - v) <= 1e-4 + 1e-12, (k, got[k], v)
