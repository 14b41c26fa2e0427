"""Shared test helpers: fixture decoding, comparisons, the multi-process rendezvous, and the
scaffolding of the per-model GPU tests (dataset directory, loaders, model, epoch loop, the
checks against a reference run).  Plain functions: a model's test file passes in what is its own."""
from __future__ import annotations

import atexit
import os
import shutil
import tempfile

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def store_path() -> str:
    """A fresh rendezvous file for `init_pg` (one per spawned job).

    Spawned tests rendezvous through a torch FileStore, not a TCP port: a port picked by
    binding port 0 and closing the socket can be taken again before rank 0 listens on it
    (GPUTEST_r05: EADDRINUSE), and a rank retrying connect to a not-yet-listening
    ephemeral port can connect to itself. A file cannot race that way."""
    d = tempfile.mkdtemp(prefix="rsx_pg_")
    atexit.register(shutil.rmtree, d, True)
    return os.path.join(d, "store")


def init_pg(backend: str, rank: int, world: int, store: str, **kw):
    """torch.distributed.init_process_group over the FileStore at `store`; RANK and
    WORLD_SIZE are exported too, as a torchrun launch would (rsx reads WORLD_SIZE)."""
    import torch.distributed as dist

    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world))
    for k in ("MASTER_ADDR", "MASTER_PORT"):
        os.environ.pop(k, None)
    dist.init_process_group(backend, init_method="file://" + store, rank=rank, world_size=world, **kw)


def coo_from(z, prefix, n):
    idx = torch.from_numpy(z[prefix + "_idx"].astype(np.int64))
    val = torch.from_numpy(z[prefix + "_val"])
    return torch.sparse_coo_tensor(idx, val, (n, n)).coalesce()


def coo_sorted(idx: np.ndarray, val: np.ndarray):
    """(row, col, val) sorted by (row, col)."""
    order = np.lexsort((idx[1], idx[0]))
    return idx[0][order], idx[1][order], val[order]


def csr_to_sorted(rowptr, col, val):
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    return rows.astype(np.int64), col.astype(np.int64), val


def params(z, prefix, model):
    if model == "LightGCN":
        return z[prefix + "embedding_dict.user_emb"], z[prefix + "embedding_dict.item_emb"]
    if model == "LayerGCN":
        return z[prefix + "user_embeddings"], z[prefix + "item_embeddings"]
    return z[prefix + "user_embedding.weight"], z[prefix + "item_id_embedding.weight"]


def metric_dict(z, tag):
    return {str(k): float(v) for k, v in zip(z[tag + "_metric_keys"], z[tag + "_metric_vals"])}


def eval_lists(z, tag):
    lens = z[tag + "_eval_len"]
    items = z[tag + "_eval_items"]
    out = []
    o = 0
    for n in lens:
        out.append(items[o:o + n])
        o += n
    return out


def train_mask_pairs(z, users: np.ndarray):
    """(batch_row, item) of the users' training items (EvalDataLoader mask, dataloader.py:370-391)."""
    tu, ti = z["train_u"], z["train_i"]
    pos = {int(u): k for k, u in enumerate(users)}
    sel = np.isin(tu, users)
    rows = np.array([pos[int(u)] for u in tu[sel]], dtype=np.int64)
    return rows, ti[sel].astype(np.int64)


def topk_equal_modulo_ties(idx_a, idx_b, scores, rtol=1e-5):
    """Rows match exactly, or differ only among items whose scores tie within rtol."""
    bad = 0
    for r in range(idx_a.shape[0]):
        if np.array_equal(idx_a[r], idx_b[r]):
            continue
        sa = scores[r, idx_a[r]]
        sb = scores[r, idx_b[r]]
        scale = max(1e-6, float(np.abs(scores[r]).max()))
        if not np.allclose(sa, sb, rtol=0, atol=rtol * scale):
            bad += 1
    return bad


def canonical_topk_fast(scores: np.ndarray, k: int):
    """oracle.canonical_topk (score desc, index asc) for wide rows: the k-th largest value
    per row by partition, then an exact (score, index) sort of the items at or above it."""
    n_rows, n = scores.shape
    kth = -np.partition(-scores, k - 1, axis=1)[:, k - 1]
    idx = np.empty((n_rows, k), dtype=np.int64)
    val = np.empty((n_rows, k), dtype=scores.dtype)
    for r in range(n_rows):
        cand = np.nonzero(scores[r] >= kth[r])[0]
        sv = scores[r, cand]
        order = np.lexsort((cand, -sv))[:k]
        idx[r] = cand[order]
        val[r] = sv[order]
    return val, idx


# ------------------------------------------------- the per-model tests' scaffolding
def dev(a, device, grad=False):
    """A numpy array on `device` (None stays None), as a leaf that requires grad if asked."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return t.requires_grad_(True) if grad else t


def check_vs_f32(name, got, ref, tor):
    """|got - ref| within max(1e-4 scale, 4 |torch f32 - ref|)."""
    ref = np.asarray(ref)
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    tor = np.asarray(tor, dtype=np.float64).reshape(ref.shape)
    scale = float(np.abs(ref).max())
    terr = float(np.abs(tor - ref).max())
    bound = max(1e-4 * scale, 4 * terr)
    err = float(np.abs(got - ref).max())
    print(f"  {name}: err {err:.3e}, scale {scale:.3e}, torch f32 err {terr:.3e}, bound {bound:.3e}")
    assert np.all(np.isfinite(got)), name
    assert err <= bound, name


def unflagged(pres, n):
    """[n, 1] float64 mask of the rows no pre-activation of `pres` comes near zero on (a float32
    rounding can move an element across leaky_relu's kink there); at most 5 % flagged."""
    from mmgcn_ref import near_zero_rows

    flag = near_zero_rows(pres)
    share = float(flag.float().mean())
    print(f"  flagged rows: {int(flag.sum())} of {n} ({share:.3%})")
    assert share <= 0.05
    return (~flag).double()[:, None]


LOSS_BATCHES = (1, 192, 300)


def loss_triplets(rng, nu, ni, B):
    """[3, B] triplets for a triplet loss's kernel test (nu > 13, ni > 9).  B = 1: the one drawn
    triplet (one lane group of the block works; key lists of 1 and 2 entries).  Otherwise 40
    repeats of user 11, 40 + 25 of item 7 as a positive and as a negative, and a triplet with the
    last item.  B > 256 also has user 13 and item 9 only at indices >= 256 of their key lists
    (users [B]; items [positives; negatives], 2 B): the wave that leads either sum scans a whole
    256-key chunk without a match, and its walk starts at the second chunk."""
    trip = np.stack([rng.integers(0, nu, B), rng.integers(0, ni, B), rng.integers(0, ni, B)]).astype(np.int64)
    if B == 1:
        return trip
    trip[0, rng.permutation(B)[:40]] = 11  # 40 repeats of one user
    trip[1, rng.permutation(B)[:40]] = 7  # and of one hot item, among the positives
    trip[2, rng.permutation(B)[:25]] = 7  # and among the negatives
    trip[:, 5] = (0, ni - 1, 0)
    assert (trip[0] == 11).sum() >= 40 and (trip[1] == 7).sum() >= 40
    if B > 256:
        trip[0][trip[0] == 13] = 11
        trip[1:][trip[1:] == 9] = 7
        three = [258, B - 20, B - 1]  # triplets past the first chunk
        trip[0, three] = 13
        trip[1, [three[0], three[2]]] = 9  # item keys 258 and B - 1 ...
        trip[2, three[1]] = 9  # ... and 2 B - 20
        items = np.concatenate([trip[1], trip[2]])
        assert np.flatnonzero(trip[0] == 13).tolist() == three
        assert np.flatnonzero(items == 9).tolist() == [258, B - 1, 2 * B - 20]
    return trip


def take_first(c):
    """The first value of every hyper-parameter a Config lists several of; returns `c`."""
    for k in c["hyper_parameters"]:
        if isinstance(c[k], list):
            c[k] = c[k][0]
    return c


def write_dataset(tmp_path, v_feat, t_feat):
    """tmp_path/data/baby with the small interaction file and the feature tables given (None: no
    file); returns the `data_path` of a Config."""
    d = tmp_path / "data" / "baby"
    d.mkdir(parents=True, exist_ok=True)
    shutil.copy(os.path.join(GOLD, "gold_small.inter"), d / "baby.inter")
    if v_feat is not None:
        np.save(d / "image_feat_raw.npy", v_feat)
    if t_feat is not None:
        np.save(d / "text_feat_raw.npy", t_feat)
    return str(tmp_path / "data") + "/"


def loaders(model_name, tmp_path, cfg):
    """(config, train, valid, test loaders) on write_dataset's directory: batches of 512, evaluation
    batches of 256, the host sampler; `cfg` holds the model's own keys and overrides these."""
    from rsx.config import Config
    from rsx.data import EvalDataLoader, RecDataset, TrainDataLoader

    common = dict(data_path=str(tmp_path / "data") + "/", train_batch_size=512, eval_batch_size=256, rsx_sampler="host")
    c = take_first(Config(model_name, "baby", {**common, **cfg}))
    ds = RecDataset(c)
    tr, va, te = ds.split()
    for s in (ds, tr, va, te):
        str(s)
    train = TrainDataLoader(c, tr, batch_size=512, shuffle=True)
    valid = EvalDataLoader(c, va, additional_dataset=tr, batch_size=256)
    test = EvalDataLoader(c, te, additional_dataset=tr, batch_size=256)
    return c, train, valid, test


def make_model(name, c, train):
    from rsx.utils import get_model, init_seed

    init_seed(c["seed"])
    train.pretrain_setup()
    return get_model(name)(c, train)


def record_batches(train):
    """Wraps the loader's batch source; returns the list every batch it hands out is appended to."""
    rec, orig = [], train._next_batch_data

    def wrapped():
        b = orig()
        rec.append(b.cpu().clone())
        return b

    train._next_batch_data = wrapped
    return rec


def train_epochs(t, m, train, epochs, after_pre_epoch=None, after_epoch=None):
    """The Trainer's epochs as quick_start drives them, each loss a finite float; the hooks take
    the epoch's number.  Returns the losses, the device idle."""
    losses = []
    for epoch in range(epochs):
        m.cur_epoch = epoch
        m.pre_epoch_processing()
        if after_pre_epoch is not None:
            after_pre_epoch(epoch)
        loss, _ = t._train_epoch(train, epoch)
        assert not torch.is_tensor(loss) and np.isfinite(loss)
        losses.append(loss)
        if after_epoch is not None:
            after_epoch(epoch)
        t.lr_scheduler.step()
        t._epoch_for_lr += 1
    torch.cuda.synchronize()
    return losses


def check_params(m, z, prefix, rel):
    """Every parameter within rel of its scale of the fixture's z[prefix + name]."""
    for n, p in m.named_parameters():
        w = z[prefix + n]
        scale = float(np.abs(w).max())
        err = float(np.abs(p.detach().cpu().numpy() - w).max())
        print(f"  {n}: err / scale {err / scale:.2e} (bound {rel:g})")
        assert err <= rel * scale, n


def check_eval(t, m, z, loaders, tag_prefix="epoch1_"):
    """Per (split, loader): the metrics within 1e-4 of the fixture's, the evaluated users its own,
    the top-50 equal modulo ties."""
    for split, loader in loaders:
        tag = tag_prefix + split
        res = t.evaluate(loader)
        ref = metric_dict(z, tag)
        assert res.keys() == ref.keys()
        for k in ref:
            assert abs(res[k] - ref[k]) <= 1e-4, (k, res[k], ref[k])
        assert np.array_equal(loader.eval_u.cpu().numpy(), z[tag + "_users"])
        _, idx = m.full_sort_topk([loader.eval_u, None], 50, loader)
        scores = m.full_sort_predict([loader.eval_u, None]).cpu().numpy()
        assert topk_equal_modulo_ties(idx.cpu().numpy(), z[tag + "_topk_idx"].astype(np.int64), scores) == 0


def assert_same_run(a, b, la, lb):
    """Two runs bit for bit: equal losses, torch.equal parameters."""
    assert la == lb
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), n


def quick_start_case(model, tmp_path, v_feat, t_feat, overrides):
    """`main.py -m <model> -d baby` from tmp_path on write_dataset's directory; quick_start's result."""
    from rsx.quick_start import quick_start

    cfg = {"data_path": write_dataset(tmp_path, v_feat, t_feat), "train_batch_size": 512, **overrides}
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        return quick_start(model, "baby", cfg, log=False)
    finally:
        os.chdir(cwd)
