"""What the per-model step-time tools (tools/*_step_time.py) share: the import paths, the common
arguments, the synthetic model at a dataset's shape, the window timer and the Trainer's step,
eager and captured.  Plain functions; a tool keeps what it measures."""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (os.path.join(REPO, "recommendar-systems_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from helpers import take_first  # noqa: E402


def parser(steps: int, warmup: int) -> argparse.ArgumentParser:
    """The arguments every tool takes, with the tool's own defaults."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=steps, help="iterations per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per variant (median, min, max reported)")
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graph (a rehearsal)")
    return ap


def require_gpu(tool: str, args=None):
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool}: needs a GPU (step times are device measurements)")
    if args is not None and args.repeats < 5:
        raise SystemExit(f"{tool}: at least 5 windows")


def synth_model(model_name, dataset, args, cfg, feats, negatives=True):
    """(model, config, four batches of 2048, training edges): the model on rsx.synth data at
    `dataset`'s shape times --scale, its feature files `feats` = ((file name, width, seed), ...),
    seed 999.  The batches are training interactions, with a drawn negative row if asked."""
    from scipy.sparse import coo_matrix

    from rsx import synth
    from rsx.config import Config
    from rsx.utils import get_model, init_seed

    df = synth.shaped(dataset, seed=0, scale=args.scale)
    df = df[df.x_label == 0]
    nu, ni = int(df.userID.max()) + 1, int(df.itemID.max()) + 1
    ds = types.SimpleNamespace(get_user_num=lambda: nu, get_item_num=lambda: ni)
    loader = types.SimpleNamespace(dataset=ds, inter_matrix=lambda form="coo": coo_matrix(
        (np.ones(len(df)), (df.userID.values, df.itemID.values)), shape=(nu, ni)))
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, dataset))
        for name, width, seed in feats:
            np.save(os.path.join(root, dataset, name), synth.features(ni, width, seed=seed))
        c = take_first(Config(model_name, dataset, dict(data_path=root + "/", train_batch_size=2048, seed=999, **cfg)))
        init_seed(999)
        m = get_model(model_name)(c, loader)
    rng = np.random.default_rng(1)
    sel = rng.permutation(len(df))[: 4 * 2048].reshape(4, 2048)

    def batch(s):
        rows = [df.userID.values[s], df.itemID.values[s]] + ([rng.integers(0, ni, 2048)] if negatives else [])
        return torch.from_numpy(np.stack(rows).astype(np.int64)).cuda()

    return m, c, [batch(s) for s in sel], len(df)


def alternated(args, runs: dict, steps=None) -> dict:
    """ms per iteration of each run in `runs`, their windows alternated: name -> [median, min, max]
    of --repeats windows of `steps` (--steps) iterations between two device events, after a
    warm-up of every run on the timed shape."""
    steps = steps or args.steps
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for run in runs.values():
        for _ in range(min(args.warmup, steps)):
            run()
    torch.cuda.synchronize()
    out = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, run in runs.items():
            e0.record()
            for _ in range(steps):
                run()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) / steps)
    return {k: [round(sorted(v)[len(v) // 2], 4), round(min(v), 4), round(max(v), 4)] for k, v in out.items()}


def captured(run):
    """`run` captured in a graph after one eager call; returns the replay."""
    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    return g.replay


def not_measured(e: Exception, width: int = 160) -> str:
    return "not measured: " + str(e).splitlines()[0][:width]


def trainer_step(c, m, batches, graph: bool, select=None):
    """(trainer, step): a Trainer of `m` with rsx_graph_step = graph, and the call that takes its
    next step over `batches` in turn (`select`, if given, is called first: it sets the variant)."""
    from rsx.trainer import Trainer

    c["rsx_graph_step"] = graph
    t = Trainer(c, m)
    k = [0]

    def step():
        if select is not None:
            select()
        t.train_step(batches[k[0] % len(batches)], k[0])
        k[0] += 1

    return t, step


def trainer_runs(args, c, m, batches, variants=None, order=(False, True)) -> dict:
    """The step through the Trainer, eager then captured (the captures last: a failed capture
    leaves the stream unusable): step[_<variant>]_eager and _graph -> [median, min, max] ms, the
    variants of `variants` = {name: select} alternated window by window."""
    res = {}
    for graph in order:
        tag = "graph" if graph else "eager"
        runs = {f"step_{name}_{tag}" if name else f"step_{tag}": trainer_step(c, m, batches, graph, select)[1]
                for name, select in (variants or {"": None}).items()}
        try:
            res.update(alternated(args, runs))
        except RuntimeError as e:
            if not graph:
                raise
            res["step_graph"] = not_measured(e)
    return res


def stage_times(args, names, ev, one_step):
    """--warmup then --steps calls of one_step(it), which records ev[0] .. ev[len(names)] around
    its stages: (stage -> ms per step, and their "sum"; the summed ms per stage; the last loss)."""
    acc = np.zeros(len(names))
    for it in range(args.warmup + args.steps):
        loss = one_step(it)
        torch.cuda.synchronize()
        if it >= args.warmup:
            acc += [ev[k].elapsed_time(ev[k + 1]) for k in range(len(names))]
    split = {n: round(float(v) / args.steps, 4) for n, v in zip(names, acc)}
    split["sum"] = round(float(acc.sum()) / args.steps, 4)
    return split, acc, loss
