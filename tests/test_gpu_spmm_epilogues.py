"""Every epilogue kind, width and row class of rsx_spmm / rsx_rowwise / rsx_spmm_batch
against tests/spmm_ref.py: the float64 restatement of include/rsx.h with a derived
bound per element (see that module's docstring; tests/test_spmm_ref_cpu.py shows a
correct f32 evaluation meets every bound and that the comparator reports mutants).

Every launch here is made twice from the same inputs and must give the same bits;
after every launch the slab's arrival counters must be zero; x always has more rows
than the graph has columns.  alpha = 0.7 and beta = 1/3 throughout.

Graphs (spmm_ref.edge_graph / many_long_graph / walk_graph / rebound):
  edge       640 x 700, duplicates, built at chunk 32 and 64: short rows of degree 0, 1, 7,
             8, 9, 15, 16, 17, 24, 31, 32; just-long rows 33, 63, 64, 65, 96, 97, chunk + 1;
             hubs of 2, 3, GPB, 3 GPB, 3 GPB + 1, 4 GPB, 4 GPB + 1 chunks for GPB = 32, 16, 8,
             4 (either side of the fixup's four-accumulator loop at every width); one hub of
             291 chunks, the last partial; every 7th row empty; one all-zero e0 row.
  many-long  > 1,024 split rows: the fixups run as a launch of their own.
  walk       > 65,536 work items: every group walks several items at every width, and the
             d = 64 next-item (col, val) prefetch runs.
"""
import json
import os

import numpy as np
import pytest
import torch

import spmm_ref as R
from rsx import _lib as L
from rsx import ops

pytestmark = pytest.mark.gpu

ALPHA, BETA = R.ALPHA, R.BETA
PTRS = ("y", "s_in", "s_out", "f", "zero0", "zero1", "r_add", "p", "m", "v", "g_out", "e0", "aux", "aux_w",
        "row_tag", "reg_cnt", "reg_k", "x_tag")
TAG, NOT_TAG = 7, 3
RATIOS = {}  # (kind name, d) -> largest error / bound seen in this run


@pytest.fixture(scope="module", autouse=True)
def _ratio_table():
    """Prints the largest error / bound per kind and width when the module is done (and
    writes it as JSON to $RSX_SPMM_RATIOS when that names a file)."""
    yield
    rows = [f"{'kind':14s}" + "".join(f"{d:>8d}" for d in R.WIDTHS)]
    for name in R.KIND_NAMES:
        rows.append(f"{name:14s}" + "".join(f"{RATIOS.get((name, d), float('nan')):8.3f}" for d in R.WIDTHS))
    print("\nlargest error / bound per kind and width\n" + "\n".join(rows))
    path = os.environ.get("RSX_SPMM_RATIOS")
    if path:
        with open(path, "w") as fh:
            json.dump({f"{k}/{d}": v for (k, d), v in RATIOS.items()}, fh, indent=1)


_graphs, _csrs = {}, {}


def graph(name, chunk=32):
    if (name, chunk) not in _graphs:
        make = {"edge": R.edge_graph, "many": R.many_long_graph, "walk": R.walk_graph}[name]
        _graphs[name, chunk] = make(chunk)
    return _graphs[name, chunk]


def csr(cuda, name, chunk, kind):
    """The DeviceCSR of a graph with the values the kind takes (|val| for the LayerGCN kinds)."""
    g = graph(name, chunk)
    pos = kind in (R.LAYERGCN, R.LAYERGCN_BWD)
    if (name, chunk, pos) not in _csrs:
        A = ops.DeviceCSR(g.rowptr, g.col, R.graph_vals(g, kind), g.n_cols, cuda, chunk=chunk)
        assert (A.n_work, A.n_long, A.n_slots) == R.schedule_counts(g.rowptr, chunk)
        _csrs[name, chunk, pos] = A
    return g, _csrs[name, chunk, pos]


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _counters_zero(A, d):
    slab = A.slab(d) if A is not None else None
    if slab is not None:
        cnt = slab[A.n_slots * d:].view(torch.int32)
        assert cnt.numel() == A.n_long and not cnt.any().item(), "arrival counters left non-zero"


def launch(cuda, A, kind, d, x, o, alias=None, dev_tag=False, dev_step=False, n_rows=None):
    """One rsx_spmm (A None: rsx_rowwise) from fresh device copies of the operands `o`;
    returns the outputs as numpy arrays.  alias {output: input} passes the input's buffer as
    the output too."""
    t = {k: _dev(v, cuda) for k, v in o.items() if isinstance(v, np.ndarray)}
    for out_name, in_name in (alias or {}).items():
        t[out_name] = t[in_name]
    adam = None
    if "adam" in o:
        hp = o["adam"]
        if dev_step:
            t["step_dev"] = torch.tensor([hp["step"]], dtype=torch.int64, device=cuda)
        adam = ops.adam_struct(hp["lr"], -5 if dev_step else hp["step"], hp["beta1"], hp["beta2"], hp["eps"],
                               hp["weight_decay"], t.get("step_dev"))
    ptrs = {k: t[k] for k in PTRS if k in t}
    if "halt" in o:
        ptrs["halt"] = t["halt"] = torch.tensor([o["halt"]], dtype=torch.int32, device=cuda)
    e = ops.epi(kind, ALPHA, BETA, adam, **ptrs)
    if "row_tag" in o:
        e.tag_flags = int(o["tag_flags"])
        e.tag = int(o["tag"])
        if dev_tag:  # the device value must win over the host field
            t["tag_dev"] = torch.tensor([o["tag"]], dtype=torch.int32, device=cuda)
            e.tag_dev = t["tag_dev"].data_ptr()
            e.tag = NOT_TAG
    if A is None:
        ops.rowwise(n_rows, d, e)
    else:
        assert x.shape[0] > A.n_cols
        A.spmm_epi(_dev(x, cuda), e, d)
    torch.cuda.synchronize()
    _counters_zero(A, d)
    names = [w for w in R.WRITES[kind] if w in t] + [z for z in ("zero0", "zero1", "reg_cnt") if z in t]
    return {k: t[k].cpu().numpy() for k in names}


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(R.bits(a[k]), R.bits(b[k])), f"{k}: bits differ"


def run(cuda, A, g, kind, d, x, o, val=None, alias=None, n_rows=None, what="", **kw):
    """Launch twice (same bits), compare every output with the reference, record the ratios."""
    got = launch(cuda, A, kind, d, x, o, alias=alias, n_rows=n_rows, **kw)
    same_bits(got, launch(cuda, A, kind, d, x, o, alias=alias, n_rows=n_rows, **kw))
    if g is None:
        ref = R.reference(None, None, None, None, kind, ALPHA, BETA, n_rows=n_rows, d=d, **o)
    else:
        ref = R.reference(g.rowptr, g.col, R.graph_vals(g, kind) if val is None else val, x, kind, ALPHA, BETA, **o)
    old = dict(o)
    for out_name, in_name in (alias or {}).items():
        old[out_name] = o[in_name]
    ratios = R.assert_within(ref, got, old, f"{R.KIND_NAMES[kind]} d={d} {what}")
    key = (R.KIND_NAMES[kind], d)
    RATIOS[key] = max(RATIOS.get(key, 0.0), max(ratios.values()))
    return got


def tags(g, x, o, kind, flags, x_tagged=None, seed=21):
    """Tag about 40 % of the rows (every other hub), poison what the flags promise is never
    read, and add the tag fields to the operands."""
    n_tags = max(x.shape[0] if x is not None else 0, next(iter(o.values())).shape[0])
    tagged = R.tag_rows(g, n_tags, seed) if g is not None else np.random.default_rng(seed).random(n_tags) < 0.4
    if x is not None:
        R.poison_untagged(o, x, tagged, flags, kind, x_tagged)
    o.update(row_tag=np.where(tagged, TAG, NOT_TAG).astype(np.int32), tag=TAG, tag_flags=flags)
    if x_tagged is not None:
        o["x_tag"] = np.where(x_tagged, TAG, NOT_TAG).astype(np.int32)
    return tagged


# ---------------------------------------------------------------------------
# the edge graph: every kind, width and chunk size, and the operand variants
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [32, 64])
@pytest.mark.parametrize("d", R.WIDTHS)
@pytest.mark.parametrize("kind", range(8), ids=R.KIND_NAMES)
def test_edge_graph_every_kind(cuda, kind, d, chunk):
    g, A = csr(cuda, "edge", chunk, kind)
    assert 0 < A.n_long <= 1024
    x, o = R.make_case(g, kind, d)
    run(cuda, A, g, kind, d, x, o, what=f"chunk={chunk}")


@pytest.mark.parametrize("chunk", [32, 64])
@pytest.mark.parametrize("d", R.WIDTHS)
def test_edge_graph_null_operands(cuda, d, chunk):
    for kind, drop in ((R.LAYERGCN, ("s_in",)), (R.LAYERSUM, ("y",)), (R.FINAL, ("aux", "e0")),
                       (R.FINAL, ("s_in", "r_add", "aux", "e0")), (R.FINAL, ("s_in", "aux")), (R.ADD, ("s_in", "r_add")),
                       (R.ADD, ("r_add",)), (R.ADAM, ("g_out", "r_add", "zero0", "zero1")),
                       (R.LAYERGCN_BWD, ("s_in", "r_add")), (R.LAYERSUM, ("s_in",)), (R.AXPBY, ("s_in",))):
        g, A = csr(cuda, "edge", chunk, kind)
        x, o = R.make_case(g, kind, d, seed=1)
        for name in drop:
            del o[name]
        run(cuda, A, g, kind, d, x, o, what=f"without {drop}")


@pytest.mark.parametrize("chunk", [32, 64])
@pytest.mark.parametrize("d", R.WIDTHS)
def test_edge_graph_aliased_outputs(cuda, d, chunk):
    for kind, out_name in ((R.LAYERSUM, "s_out"), (R.LAYERGCN, "s_out"), (R.LAYERGCN_BWD, "s_out"), (R.ADD, "y")):
        g, A = csr(cuda, "edge", chunk, kind)
        x, o = R.make_case(g, kind, d, seed=2)
        del o[out_name]
        run(cuda, A, g, kind, d, x, o, alias={out_name: "s_in"}, what=f"{out_name} = s_in")


@pytest.mark.parametrize("chunk", [32, 64])
@pytest.mark.parametrize("d", R.WIDTHS)
def test_edge_graph_adam_step_dev_and_halt(cuda, d, chunk):
    g, A = csr(cuda, "edge", chunk, R.ADAM)
    x, o = R.make_case(g, R.ADAM, d, seed=3)
    host = run(cuda, A, g, R.ADAM, d, x, o)
    same_bits(host, launch(cuda, A, R.ADAM, d, x, o, dev_step=True))  # step_dev: bit for bit the host step
    # halted: p, m, v keep their bits; g_out is still written, zero0 / zero1 still cleared
    halted = run(cuda, A, g, R.ADAM, d, x, dict(o, halt=1), what="halt")
    for k in ("p", "m", "v"):
        assert np.array_equal(R.bits(halted[k]), R.bits(o[k]))
    assert np.array_equal(R.bits(halted["g_out"]), R.bits(host["g_out"]))
    assert not halted["zero0"].any() and not halted["zero1"].any()
    same_bits(host, run(cuda, A, g, R.ADAM, d, x, dict(o, halt=0), what="halt = 0"))


@pytest.mark.parametrize("chunk", [32, 64])
@pytest.mark.parametrize("d", R.WIDTHS)
def test_edge_graph_reg_counts(cuda, d, chunk):
    """The regulariser as occurrence counts: ADAM reads them and leaves them (no ZERO flag),
    ADD reads them and clears every row's."""
    for kind in (R.ADAM, R.ADD):
        g, A = csr(cuda, "edge", chunk, kind)
        x, o = R.make_case(g, kind, d, seed=4)
        del o["r_add"]
        o.update(reg_cnt=R.reg_counts(g.n_rows, np.random.default_rng(d)), reg_k=R.REG_K)
        if kind == R.ADD:
            o["p"] = np.random.default_rng(d + 1).standard_normal((g.n_rows, d)).astype(np.float32)
        got = run(cuda, A, g, kind, d, x, o, what="reg_cnt")
        cleared = not got["reg_cnt"][:3 * g.n_rows].any()
        assert cleared == (kind == R.ADD)


# ---------------------------------------------------------------------------
# fixups in a launch of their own; groups that walk several items
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", R.WIDTHS)
@pytest.mark.parametrize("kind", [R.FINAL, R.ADAM, R.LAYERGCN_BWD], ids=lambda k: R.KIND_NAMES[k])
def test_many_long_rows_fixup_launch(cuda, kind, d):
    g, A = csr(cuda, "many", 32, kind)
    assert A.n_long > 1024
    x, o = R.make_case(g, kind, d)
    run(cuda, A, g, kind, d, x, o, what="many-long")


@pytest.mark.parametrize("d", R.WIDTHS)
@pytest.mark.parametrize("kind", [R.STORE, R.LAYERGCN_BWD, R.ADAM, R.ADD], ids=lambda k: R.KIND_NAMES[k])
def test_walk_graph_several_items_per_group(cuda, kind, d):
    g, A = csr(cuda, "walk", 32, kind)
    assert A.n_work > 65536 and g.n_rows >= 66000
    x, o = R.make_case(g, kind, d)
    if kind == R.ADD:  # an untagged item must not leave a prefetch behind for the next
        tags(g, x, o, kind, R.TAG_ROWS | R.TAG_SPARSE_X)
    run(cuda, A, g, kind, d, x, o, what="walk")


# ---------------------------------------------------------------------------
# tag flags, each as a property of the kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", R.WIDTHS)
@pytest.mark.parametrize("kind", [R.FINAL, R.STORE], ids=lambda k: R.KIND_NAMES[k])
def test_tag_rows_leaves_untagged_rows_alone(cuda, kind, d):
    g, A = csr(cuda, "edge", 32, kind)
    x, o = R.make_case(g, kind, d, seed=5)
    tagged = tags(g, x, o, kind, R.TAG_ROWS)[:g.n_rows]
    got = run(cuda, A, g, kind, d, x, o, what="ROWS")
    for k, v in got.items():  # (the comparator has checked this; said once more in the open)
        assert np.array_equal(R.bits(v[~tagged]), R.bits(o[k][~tagged])), k
    assert not got["zero0"][tagged].any()
    same_bits(got, launch(cuda, A, kind, d, x, o, dev_tag=True))


@pytest.mark.parametrize("d", R.WIDTHS)
def test_tag_sparse_x(cuda, d):
    g, A = csr(cuda, "edge", 32, R.ADD)
    x, o = R.make_case(g, R.ADD, d, seed=6)
    tags(g, x, o, R.ADD, R.TAG_SPARSE_X)
    assert np.isnan(x).any()
    got = run(cuda, A, g, R.ADD, d, x, o, what="SPARSE_X, row_tag for both sides")
    assert np.isfinite(got["y"]).all()
    same_bits(got, launch(cuda, A, R.ADD, d, x, o, dev_tag=True))
    # X's rows numbered apart from the output rows
    x, o = R.make_case(g, R.ADD, d, seed=6)
    x_tagged = np.random.default_rng(77).random(x.shape[0]) < 0.4
    tags(g, x, o, R.ADD, R.TAG_SPARSE_X, x_tagged=x_tagged)
    o["row_tag"] = o["row_tag"][:g.n_rows].copy()  # only x_tag may be indexed by column
    got = run(cuda, A, g, R.ADD, d, x, o, what="SPARSE_X, x_tag")
    assert np.isfinite(got["y"]).all()


@pytest.mark.parametrize("d", R.WIDTHS)
@pytest.mark.parametrize("kind", [R.ADD, R.ADAM], ids=lambda k: R.KIND_NAMES[k])
def test_tag_sparse_s_and_r(cuda, kind, d):
    g, A = csr(cuda, "edge", 32, kind)
    for flags in (R.TAG_SPARSE_S, R.TAG_SPARSE_R, R.TAG_SPARSE_S | R.TAG_SPARSE_R):
        x, o = R.make_case(g, kind, d, seed=7)
        tagged = tags(g, x, o, kind, flags)
        got = run(cuda, A, g, kind, d, x, o, what=f"flags {flags}")
        assert all(np.isfinite(v).all() for v in got.values())
        same_bits(got, launch(cuda, A, kind, d, x, o, dev_tag=True))
    # ADAM's counts under SPARSE_R: the untagged rows hold large counts nothing may read
    if kind == R.ADAM:
        x, o = R.make_case(g, kind, d, seed=7)
        del o["r_add"]
        tagged = tags(g, x, o, kind, R.TAG_SPARSE_S | R.TAG_SPARSE_R)
        o.update(reg_cnt=R.reg_counts(g.n_rows, np.random.default_rng(d), tagged[:g.n_rows], True), reg_k=R.REG_K)
        got = run(cuda, A, g, kind, d, x, o, what="SPARSE_R counts")
        assert np.array_equal(got["reg_cnt"], o["reg_cnt"])  # no ZERO flag: left as they are


@pytest.mark.parametrize("d", R.WIDTHS)
def test_tag_zero_clears_tagged_rows_only(cuda, d):
    g, A = csr(cuda, "edge", 32, R.ADAM)
    x, o = R.make_case(g, R.ADAM, d, seed=8)
    del o["r_add"]
    tagged = tags(g, x, o, R.ADAM, R.TAG_ZERO)[:g.n_rows]
    o.update(reg_cnt=R.reg_counts(g.n_rows, np.random.default_rng(d)) + 1, reg_k=R.REG_K)
    got = run(cuda, A, g, R.ADAM, d, x, o, what="ZERO")
    cnt = got["reg_cnt"][:3 * g.n_rows].reshape(-1, 3)
    for k in ("zero0", "zero1"):
        assert not got[k][tagged].any()
        assert np.array_equal(R.bits(got[k][~tagged]), R.bits(o[k][~tagged]))
    assert not cnt[tagged].any() and cnt[~tagged].all()
    same_bits(got, launch(cuda, A, R.ADAM, d, x, o, dev_tag=True))


@pytest.mark.parametrize("d", R.WIDTHS)
def test_tag_flag_combinations_the_steps_use(cuda, d):
    S, Rr, X, Z = R.TAG_SPARSE_S, R.TAG_SPARSE_R, R.TAG_SPARSE_X, R.TAG_ZERO
    for kind, flags, counts in ((R.LAYERSUM, S | X, False), (R.ADD, S | X, False), (R.ADAM, S | Rr | Z, True),
                                (R.ADAM, S | Rr | Z, False), (R.ADAM, Rr | Z, False), (R.ADD, X | Rr, False),
                                (R.AXPBY, S | X, False), (R.FINAL, S | Rr, False)):
        g, A = csr(cuda, "edge", 32, kind)
        x, o = R.make_case(g, kind, d, seed=9)
        tagged = tags(g, x, o, kind, flags)
        if counts:
            del o["r_add"]
            o.update(reg_cnt=R.reg_counts(g.n_rows, np.random.default_rng(d), tagged[:g.n_rows], True),
                     reg_k=R.REG_K)
        got = run(cuda, A, g, kind, d, x, o, what=f"flags {flags}")
        same_bits(got, launch(cuda, A, kind, d, x, o, dev_tag=True))


# ---------------------------------------------------------------------------
# a graph rebound onto the edge graph's schedule
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", R.WIDTHS)
@pytest.mark.parametrize("kind", [R.LAYERGCN, R.ADD], ids=lambda k: R.KIND_NAMES[k])
def test_rebound_graph(cuda, kind, d):
    g, A = csr(cuda, "edge", 32, kind)
    rb = R.rebound(g)
    deg, deg0 = np.diff(rb.rowptr), np.diff(g.rowptr)
    assert deg[g.marks["hub291"]] == 0 and ((deg == 0) & (deg0 > 0) & (deg0 <= 32)).any()
    B = ops.DeviceCSR.rebind(A, _dev(rb.rowptr, cuda), _dev(rb.col, cuda), _dev(R.graph_vals(rb, kind), cuda))
    x, o = R.make_case(g, kind, d, seed=10)
    run(cuda, B, rb, kind, d, x, o, what="rebound")
    # and the template still computes its own product afterwards (shared slab, counters re-armed)
    run(cuda, A, g, kind, d, x, o, what="template after rebind")


# ---------------------------------------------------------------------------
# rsx_rowwise: acc = 0
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", R.WIDTHS)
@pytest.mark.parametrize("kind", range(8), ids=R.KIND_NAMES)
def test_rowwise_every_kind(cuda, kind, d):
    n = 300
    x, o = R.make_case(None, kind, d, n_rows=n)
    run(cuda, None, None, kind, d, None, o, n_rows=n, what="rowwise")
    x, o = R.make_case(None, kind, d, n_rows=n, seed=1)
    tagged = tags(None, None, o, kind, R.TAG_ROWS)[:n]
    got = run(cuda, None, None, kind, d, None, o, n_rows=n, what="rowwise ROWS")
    for k, v in got.items():
        assert np.array_equal(R.bits(v[~tagged]), R.bits(o[k][~tagged])), k


# ---------------------------------------------------------------------------
# rsx_spmm_batch
# ---------------------------------------------------------------------------
EMPTY = R.Graph(np.zeros(18, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), 17, 5, 32, {})


def _batch_problem(cuda, kind, d, fourth="edge64"):
    """Four products: the edge graph, an empty matrix in the middle, the edge graph again
    (its second slab), and the chunk-64 edge graph (fixups ride in the one launch) or the
    many-long graph (more than 1,024 fixups in all: they get the second launch)."""
    ge, Ae = csr(cuda, "edge", 32, kind)
    g4, A4 = csr(cuda, "edge", 64, kind) if fourth == "edge64" else csr(cuda, "many", 32, kind)
    empty = ops.DeviceCSR(EMPTY.rowptr, EMPTY.col, EMPTY.val, EMPTY.n_cols, cuda)
    cases = []
    for i, (g, A) in enumerate(zip([ge, EMPTY, ge, g4], [Ae, empty, Ae, A4])):
        rng = np.random.default_rng(100 * d + i)
        x = rng.standard_normal((A.n_cols + 5, d)).astype(np.float32)
        o = {"y": R.sentinel((A.n_rows, d))}
        if kind != R.STORE:
            o["s_in"] = rng.standard_normal((A.n_rows, d)).astype(np.float32)
        if kind == R.ADD:
            o["r_add"] = rng.standard_normal((A.n_rows, d)).astype(np.float32)
        cases.append((g, A, x, o))
    return cases


@pytest.mark.parametrize("fourth", ["edge64", "many"])
@pytest.mark.parametrize("d", R.WIDTHS)
@pytest.mark.parametrize("kind", [R.STORE, R.ADD, R.AXPBY], ids=lambda k: R.KIND_NAMES[k])
def test_batch_equals_its_single_products(cuda, kind, d, fourth):
    cases = _batch_problem(cuda, kind, d, fourth)
    assert (sum(A.n_long for _, A, _, _ in cases) > 1024) == (fourth == "many")
    singles = [run(cuda, A, g, kind, d, x, o, what="batch member alone") for g, A, x, o in cases]
    for _ in range(2):  # twice: same bits
        ts = [{k: _dev(v, cuda) for k, v in o.items()} for _, _, _, o in cases]
        xs = [_dev(x, cuda) for _, _, x, _ in cases]
        epis = [ops.epi(kind, ALPHA, BETA, **t) for t in ts]
        ops.spmm_batch([A for _, A, _, _ in cases], xs, epis, d)
        torch.cuda.synchronize()
        for i, ((g, A, _, _), t, one) in enumerate(zip(cases, ts, singles)):
            assert np.array_equal(R.bits(t["y"].cpu().numpy()), R.bits(one["y"])), f"product {i}"
            _counters_zero(A, d)
        twice = cases[0][1]  # the graph used twice: its second slab's counters too
        assert not twice.slab(d, 1)[twice.n_slots * d:].view(torch.int32).any().item()


def test_batch_argument_errors(cuda):
    d = 64
    cases = _batch_problem(cuda, R.STORE, d)
    As = [A for _, A, _, _ in cases]
    xs = [_dev(x, cuda) for _, _, x, _ in cases]
    ys = [torch.full((A.n_rows, d), 5.0, device=cuda) for A in As]

    def epis(kinds):
        return [ops.epi(k, ALPHA, BETA, y=y, s_in=y, s_out=y) for k, y in zip(kinds, ys)]

    with pytest.raises(RuntimeError, match="RSX_ERR_ARG"):  # count = 5
        ops.spmm_batch(As + As[:1], xs + xs[:1], epis([R.STORE] * 4) + epis([R.STORE])[:1], d)
    with pytest.raises(RuntimeError, match="RSX_ERR_ARG"):  # mixed kinds
        ops.spmm_batch(As, xs, epis([R.STORE, R.STORE, R.ADD, R.STORE]), d)
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):  # a kind the batch does not take
        ops.spmm_batch(As, xs, epis([R.LAYERSUM] * 4), d)
    x48 = [torch.zeros(A.n_cols + 5, 48, device=cuda) for A in As]
    with pytest.raises(RuntimeError, match="RSX_ERR_UNSUPPORTED"):  # d = 48
        ops.spmm_batch(As, x48, epis([R.STORE] * 4), 48)
    # a NULL slab for a graph with split rows
    import ctypes as C

    A = As[0]
    assert A.n_long > 0
    arr_a = (C.c_void_p * 1)(C.addressof(A.struct))
    arr_x = (C.c_void_p * 1)(xs[0].data_ptr())
    arr_e = (L.Epilogue * 1)(*epis([R.STORE])[:1])
    arr_s = (C.c_void_p * 1)(None)
    rc = L.lib().rsx_spmm_batch(1, arr_a, arr_x, d, arr_e, arr_s, ops._stream())
    assert rc == 1003  # RSX_ERR_WORKSPACE
    torch.cuda.synchronize()
    for y in ys:  # every error returned before any launch: nothing was written
        assert (y == 5.0).all().item()
