"""GRCN without a GPU: the float64 restatement (tests/grcn_ref.py) against the reference's own
run (tests/golden/grcn_step0_small.npz, grcn_small.npz)."""
import os

import numpy as np
import torch

import grcn_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("model_specific_conf", "id_gcn.id_embedding", "v_gcn.preference", "v_gcn.MLP.weight", "v_gcn.MLP.bias",
         "t_gcn.preference", "t_gcn.MLP.weight", "t_gcn.MLP.bias")
WHOLE = ("MLP.", "model_specific_conf")  # stored whole; the tables at a row stride


def load(name):
    return np.load(os.path.join(GOLD, name))


def hparams(z):
    return dict(s.split("=", 1) for s in z["hparams"])


def strides(z):
    return {k: int(v) for k, v in (s.split("=", 1) for s in z["row_strides"])}


def rows(a, name, k):
    return a if any(s in name for s in WHOLE) else a[::k]


def close(got, want, tol=1e-5):
    """Within `tol` of the tensor's scale (its largest magnitude)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = np.abs(want).max()
    err = np.abs(got - want).max() if want.size else 0.0
    assert err <= tol * scale, (err, scale)


def setup(dtype=torch.float64):
    z0, z = load("grcn_step0_small.npz"), load("grcn_small.npz")
    nu = int(z["n_users"])
    P = R.cast({n: torch.from_numpy(z["init." + n]) for n in NAMES}, dtype)
    feats = {"v": torch.from_numpy(z["v_feat"]).to(dtype), "t": torch.from_numpy(z["t_feat"]).to(dtype)}
    ei = R.edge_index(z["train_u"].astype(np.int64), z["train_i"].astype(np.int64), nu)
    return z0, z, nu, P, feats, ei


def test_fixture_sizes_and_hparams():
    for f in ("grcn_small.npz", "grcn_step0_small.npz"):
        assert os.path.getsize(os.path.join(GOLD, f)) < (1 << 20), f
    z0, z = load("grcn_step0_small.npz"), load("grcn_small.npz")
    hp = hparams(z0)
    assert float(hp["learning_rate"]) == 0.001 and float(hp["reg_weight"]) == 0.001 and int(hp["seed"]) == 999
    assert (int(hp["embedding_size"]), int(hp["latent_embedding"]), int(hp["n_layers"])) == (64, 64, 3)
    assert int(z["n_users"]) + int(z["n_items"]) == z["init.id_gcn.id_embedding"].shape[0]
    assert z0["step0_alpha_v"].shape == (2 * z["train_u"].size,)
    # the capture's own condition: no argmax within 1e-5 relative on either step
    assert float(z0["step0_min_gap"]) > 1e-5 and float(z0["step1_min_gap"]) > 1e-5


def test_routing_leaves_the_user_rows_of_the_aggregate_exactly_zero():
    """The routing loop runs on the directed user -> item edges: its aggregate lands on item
    rows only, so it only re-normalises the preferences (what the HIP path skips)."""
    _, _, nu, P, feats, ei = setup()
    keep = {}
    with torch.no_grad():
        rep, _ = R.cgcn(feats["v"], P["v_gcn.preference"], P["v_gcn.MLP.weight"], P["v_gcn.MLP.bias"], ei, nu, 3, keep)
        once, _ = R.cgcn(feats["v"], P["v_gcn.preference"], P["v_gcn.MLP.weight"], P["v_gcn.MLP.bias"], ei, nu, 0)
    assert len(keep["routing_user_rows"]) == 3
    for h in keep["routing_user_rows"]:
        assert h.shape[0] == nu and torch.count_nonzero(h) == 0
    assert (rep - once).abs().max() <= 1e-14  # float64 rounding of a re-normalised unit row


def test_restatement_two_steps_vs_fixture():
    """alpha, weights, representation, loss terms and every gradient of the first two steps in
    float64, each within 1e-5 of the tensor's scale, and the restatement's own parameters after
    its own Adam update: within 1e-5 of the tensor's scale plus, per element, what Adam's update
    turns the difference between the restatement's gradient and the reference's float32 one into
    (grcn_ref.adam_tolerance: it vanishes where |g| is far above Adam's eps and reaches a fraction
    of lr where |g| is near it; without that term id_embedding after the first step is 2.6e-6
    off against 2.1e-6, on elements with |g| below 1e-7)."""
    z0, z, nu, P, feats, ei = setup()
    hp, S = hparams(z0), strides(z0)
    lr = float(hp["learning_rate"])
    adam = R.Adam(P, lr)
    dgs, grefs = {n: [] for n in NAMES}, {n: [] for n in NAMES}
    k = S["param"] // S["grad"]
    for step in range(2):
        pre = f"step{step}_"
        trip = torch.from_numpy(z0[pre + "triplets"].astype(np.int64))
        fw, terms, grads = R.step(P, feats, ei, trip, nu, int(hp["n_layers"]), float(hp["reg_weight"]))
        close(fw["alphas"][0].detach(), z0[pre + "alpha_v"])
        close(fw["alphas"][1].detach(), z0[pre + "alpha_t"])
        close(fw["weight"].detach(), z0[pre + "weight"])
        close(fw["representation"].detach()[::S["rep"]], z0[pre + "representation"])
        for j, name in enumerate(("loss", "bpr", "reg")):
            want = float(z0[pre + name])
            assert abs(float(terms[j]) - want) <= 1e-5 * abs(want), (name, float(terms[j]), want)
        for n in NAMES:
            close(rows(grads[n].numpy(), n, S["grad"]), z0[pre + "grad." + n])
        adam.step(grads)
        for n in NAMES:
            gref = rows(z0[pre + "grad." + n].astype(np.float64), n, k)
            grefs[n].append(gref)
            dgs[n].append(rows(grads[n].numpy(), n, S["param"]) - gref)
            want = z0[pre + "param." + n].astype(np.float64)
            err = np.abs(rows(P[n].detach().numpy(), n, S["param"]) - want)
            extra = R.adam_tolerance(dgs[n], grefs[n], lr)
            tol = 1e-5 * np.abs(want).max() + extra
            share = float((extra > 1e-5 * np.abs(want).max()).mean())
            print(f"  step {step} param {n}: err {err.max():.3e}, scale {np.abs(want).max():.3e}, "
                  f"elements with an Adam term above 1e-5 of scale: {share:.4f}")
            assert (err <= tol).all(), (step, n, float((err - tol).max()))
            # the allowance is for the few elements with |g| near Adam's eps: it must not grow
            # to cover the table
            assert share < 1e-3, (step, n, share)
