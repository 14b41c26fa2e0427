"""The shared checks of the per-model GPU tests (tests/helpers.py) cannot pass vacuously: each
passes on what it should accept and raises on what it should refuse, the bound taken from the
check's own formula on inputs made here."""
import os

import numpy as np
import pytest
import torch

from helpers import (LOSS_BATCHES, assert_same_run, check_params, check_vs_f32, loss_triplets, take_first,
                     write_dataset)


def _ref():
    return np.random.default_rng(0).standard_normal((7, 5))  # float64


@pytest.mark.parametrize("torch_err", [0.0, 1e-3])  # the bound's first term decides, then its second
def test_check_vs_f32_bound(torch_err):
    ref = _ref()
    scale = float(np.abs(ref).max())
    tor = ref.copy()
    tor[2, 3] += torch_err * scale
    bound = max(1e-4 * scale, 4 * float(np.abs(tor - ref).max()))
    assert bound == pytest.approx((4e-3 if torch_err else 1e-4) * scale)
    check_vs_f32("equal", ref.copy(), ref, tor)
    got = ref.copy()
    got[6, 4] -= 0.99 * bound
    check_vs_f32("just under", got, ref, tor)
    check_vs_f32("float32, another shape", got.astype(np.float32).reshape(-1), ref, tor.reshape(-1))
    got[6, 4] = ref[6, 4] - 1.01 * bound
    with pytest.raises(AssertionError, match="just over"):
        check_vs_f32("just over", got, ref, tor)


def test_check_vs_f32_refuses_nan():
    ref = _ref()
    got = ref.copy()
    got[0, 0] = np.nan
    with pytest.raises(AssertionError, match="nan"):
        check_vs_f32("nan", got, ref, ref)
    with pytest.raises(AssertionError, match="nan"):  # also where the float32 error is no number either
        check_vs_f32("nan", got, ref, got)


class _Two(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(1)
        self.a = torch.nn.Parameter(torch.randn(4, 3, generator=g))
        self.b = torch.nn.Linear(3, 2)


def test_check_params():
    m, rel = _Two(), 5e-5
    z = {"p." + n: p.detach().numpy().copy() for n, p in m.named_parameters()}
    assert sorted(z) == ["p.a", "p.b.bias", "p.b.weight"]
    check_params(m, z, "p.", rel)
    scale = float(np.abs(z["p.b.weight"]).max())
    z["p.b.weight"][1, 2] += 0.9 * rel * scale  # the fixture's own scale moves by less than rel of itself
    check_params(m, z, "p.", rel)
    z["p.b.weight"][1, 2] += 1.1 * rel * scale  # 2 rel scale off
    with pytest.raises(AssertionError, match="b.weight"):
        check_params(m, z, "p.", rel)
    with pytest.raises(KeyError):  # a parameter the fixture does not hold is no pass
        check_params(m, {k: v for k, v in z.items() if k != "p.a"}, "p.", rel)


def test_assert_same_run():
    a, b = _Two(), _Two()
    b.load_state_dict(a.state_dict())
    assert_same_run(a, b, [0.5, 0.25], [0.5, 0.25])
    with pytest.raises(AssertionError):
        assert_same_run(a, b, [0.5, 0.25], [0.5, 0.25 + 2.0 ** -30])
    with torch.no_grad():
        b.b.weight.view(torch.int32)[1, 0] ^= 1  # one bit of one parameter
    assert torch.allclose(a.b.weight, b.b.weight, rtol=1e-6)
    with pytest.raises(AssertionError, match="b.weight"):
        assert_same_run(a, b, [0.5], [0.5])


@pytest.mark.parametrize("which", ["both", "text", "none"])
def test_write_dataset_writes_the_files_it_was_given(tmp_path, which):
    v = np.arange(12, dtype=np.float32).reshape(4, 3) if which == "both" else None
    t = np.arange(8, dtype=np.float32).reshape(4, 2) if which != "none" else None
    path = write_dataset(tmp_path, v, t)
    assert path == str(tmp_path / "data") + "/" and os.listdir(path) == ["baby"]
    want = {"baby.inter": None, "image_feat_raw.npy": v, "text_feat_raw.npy": t}
    want = {k: a for k, a in want.items() if k == "baby.inter" or a is not None}
    assert sorted(os.listdir(os.path.join(path, "baby"))) == sorted(want)
    for k, a in want.items():
        if a is not None:
            assert np.array_equal(np.load(os.path.join(path, "baby", k)), a)
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gold_small.inter")
    with open(os.path.join(path, "baby", "baby.inter"), "rb") as f, open(gold, "rb") as g:
        assert f.read() == g.read()


def test_loss_triplets_plant_what_the_loss_tests_rely_on():
    """The batches of the MMGCN and GRCN loss tests, at their table sizes: B = 192 is the batch the
    tests always had; B = 300 has a user and an item first met past the first 256 keys of their
    lists, and still leaves a table row that no triplet touches."""
    nu, ni = 70, 50
    assert LOSS_BATCHES == (1, 192, 300)
    for B in LOSS_BATCHES:
        trip = loss_triplets(np.random.default_rng(3), nu, ni, B)
        assert trip.shape == (3, B) and trip.dtype == np.int64
        assert trip[0].min() >= 0 and trip[0].max() < nu and trip[1:].min() >= 0 and trip[1:].max() < ni
        rows = np.unique(np.concatenate([trip[0], nu + trip[1], nu + trip[2]]))
        assert rows.size < nu + ni
    rng = np.random.default_rng(3)  # B = 192, as the tests drew it before the batch became a parameter
    old = np.stack([rng.integers(0, nu, 192), rng.integers(0, ni, 192), rng.integers(0, ni, 192)]).astype(np.int64)
    old[0, rng.permutation(192)[:40]] = 11
    old[1, rng.permutation(192)[:40]] = 7
    old[2, rng.permutation(192)[:25]] = 7
    old[:, 5] = (0, 49, 0)
    assert np.array_equal(loss_triplets(np.random.default_rng(3), nu, ni, 192), old)
    assert np.flatnonzero(trip[0] == 13).min() >= 256 and np.flatnonzero(np.concatenate([trip[1], trip[2]]) == 9).min() >= 256


def test_take_first():
    c = {"hyper_parameters": ["lr", "reg", "layers"], "lr": [0.1, 0.01], "reg": 0.5, "layers": [2], "other": [7, 8]}
    assert take_first(c) is c
    assert c == {"hyper_parameters": ["lr", "reg", "layers"], "lr": 0.1, "reg": 0.5, "layers": 2, "other": [7, 8]}
