#!/usr/bin/env python3
"""ms/step and interactions/s of the BPR / VBPR training step (rsx_mf_step) on rsx.synth data.

Cases: the sports shape (35,598 users, 18,357 items), d = 64, B = 2048: BPR, and VBPR with
raw features F = 4480 and F = 1536.  Each case: warm-up steps on the timed shape, then
`--repeats` windows of `--steps` steps, each between two device events (device-sampled epoch
batches, so no host work between launches): the median window is the figure, the minimum
and maximum its spread; the same again replayed from one captured graph; and the f32 torch
restatement (tests/mf_ref.py, which projects every item as the reference does) timed on 16
CPU threads in the same run.  Prints one JSON line per case with the step's algorithmic
bytes (what the algorithm must move, from the shapes) and `algorithmic_bytes_per_s_over_8TBps`:
those bytes over the median time over the 8 TB/s HBM peak.  That is an algorithmic rate, not
measured HBM traffic: the BPR working set (tables, moments, scratch: about 55 MB) and most
of VBPR's stay resident in the 256 MB Infinity Cache between steps.  Needs a GPU: there is no
CPU fallback for the measured path.

Usage:  python tools/mf_step_time.py [--steps 4000] [--repeats 5] [--warmup 200] [--scale 1.0] [--cpu-steps 3]
                                     [--case NAME] [--no-graph]
"""
from __future__ import annotations

import json
import time

import numpy as np
import torch

from _step_time import parser, require_gpu

HBM_PEAK = 8.0e12


def step_bytes(nu: int, ni: int, d: int, F: int, B: int) -> dict:
    """Bytes one step must move, per phase (f32).  Adam: p, m, v, g read and p, m, v
    written for every parameter (dense, as torch.optim.Adam).  Loss: the 3 B batch rows
    read by the forward and again by the backward, and their gradient rows added
    (read + write).  Projection: the 2 B gathered feature rows, W and the output rows.
    Weight gradient: the feature rows again, the gradient rows, dW."""
    du = 2 * d if F else d
    n_param = nu * du + ni * d + (d * F + d if F else 0)
    out = {"adam": 28 * n_param, "loss": 2 * 4 * B * 3 * du + 8 * B * 3 * du}
    if F:
        out["proj"] = 4 * (2 * B * F + d * F + 2 * B * d)
        out["wgrad"] = 4 * (2 * B * F + 2 * B * d + d * F)
    out["total"] = sum(out.values())
    return out


def run_case(name: str, F: int, args, df) -> dict:
    from rsx import synth
    from rsx.mf import MFEngine, bpr_init, vbpr_init

    import mf_ref as R

    dev = torch.device("cuda:0")
    d, B = 64, 2048
    nu, ni = int(df.userID.max()) + 1, int(df.itemID.max()) + 1
    tu, ti = df.userID.values.astype(np.int64), df.itemID.values.astype(np.int64)
    torch.manual_seed(0)
    X = None
    if F:
        X = synth.features(ni, F, seed=5)
        init = [t.numpy() for t in vbpr_init(nu, ni, d, F)]
        kw = dict(W=init[2], b=init[3], features=X)
    else:
        init = [t.numpy() for t in bpr_init(nu, ni, d)]
        kw = {}
    eng = MFEngine(tu, ti, nu, ni, d, 1e-2, 1e-3, dev, init[0], init[1], batch=B, seed=1, **kw)
    nb = eng.n_inter // B  # full batches only: one shape in the timed window

    def steps(k, first=0):
        for j in range(first, first + k):
            eng.step(epoch=j // nb, start=(j % nb) * B)

    def windows(run):
        """ms/step of `--repeats` timed windows of `--steps` steps: (median, min, max)."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = []
        for w in range(args.repeats):
            e0.record()
            run(w)
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / args.steps)
        out.sort()
        return out[len(out) // 2], out[0], out[-1]

    steps(args.warmup)
    torch.cuda.synchronize()
    # (the one sampling launch per epoch is part of training and stays inside the window)
    ms, ms_min, ms_max = windows(lambda w: steps(args.steps, args.warmup + w * args.steps))
    # the same step replayed from a captured graph (fixed batch): launch overhead removed
    trip = eng.sampler.sample(0, 0, B)
    ms_graph = g_min = g_max = float("nan")
    if not args.no_graph:
        eng.step(triplets=trip)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.step(triplets=trip)
        for _ in range(20):
            g.replay()
        torch.cuda.synchronize()

        def replays(_):
            for _ in range(args.steps):
                g.replay()

        ms_graph, g_min, g_max = windows(replays)
    assert bool(torch.isfinite(eng.loss_out).all()) and int(eng.halt[0]) == 0
    # the f32 restatement on the CPU (16 threads), same shapes, same batch
    cpu_ms = float("nan")
    if args.cpu_steps > 0:
        torch.set_num_threads(16)
        ref = R.MFRef(init, 1e-2, X)
        t_cpu = trip.cpu()
        ref.step(t_cpu)
        t0 = time.perf_counter()
        for _ in range(args.cpu_steps):
            ref.step(t_cpu)
        cpu_ms = (time.perf_counter() - t0) / args.cpu_steps * 1e3
    by = step_bytes(nu, ni, d, F, B)
    return {"case": name, "n_users": nu, "n_items": ni, "d": d, "F": F, "batch": B,
            "launches_per_step": 7 if F else 3,
            "steps_per_window": args.steps, "windows": args.repeats,
            "ms_per_step": round(ms, 4), "ms_per_step_min_max": [round(ms_min, 4), round(ms_max, 4)],
            "interactions_per_s": round(B / ms * 1e3),
            "ms_per_step_graph": round(ms_graph, 4), "ms_per_step_graph_min_max": [round(g_min, 4), round(g_max, 4)],
            "cpu_f32_16thr_ms_per_step": round(cpu_ms, 2),
            "bytes": by, "algorithmic_bytes_per_s_over_8TBps": round(by["total"] / (ms * 1e-3) / HBM_PEAK, 4)}


def main():
    ap = parser(steps=4000, warmup=200)
    ap.add_argument("--cpu-steps", type=int, default=3, help="0: skip the CPU restatement")
    ap.add_argument("--case", default=None, help="one of BPR, VBPR_F4480, VBPR_F1536 (default: all)")
    ap.add_argument("--no-graph", action="store_true", help="skip the captured-graph timing (profiler runs)")
    args = ap.parse_args()
    require_gpu("mf_step_time")
    from rsx import synth

    df = synth.shaped("sports", seed=0, scale=args.scale)
    for name, F in (("BPR", 0), ("VBPR_F4480", 4480), ("VBPR_F1536", 1536)):
        if args.case in (None, name):
            print(json.dumps(run_case(name, F, args, df)), flush=True)


if __name__ == "__main__":
    main()
