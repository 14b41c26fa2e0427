"""tests/spmm_ref.py checked on the CPU before anything touches a GPU: the float64
restatement of rsx_spmm's contract against torch in float64, a float32 evaluation
in the documented summation order against every bound (so the bounds the GPU tests
use are attainable by a correct f32 evaluation, nothing excluded), and the
comparator against ten single mutations, each of which it must report."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spmm_ref as R

A_, B_ = R.ALPHA, R.BETA
af, bf = float(np.float32(A_)), float(np.float32(B_))


@pytest.fixture(scope="module")
def edge():
    return {c: R.edge_graph(c) for c in (32, 64)}


def _dense(g, val):
    import scipy.sparse as sp

    return np.asarray(sp.csr_matrix((val.astype(np.float64), g.col.astype(np.int64), g.rowptr),
                                    shape=(g.n_rows, g.n_cols + 5)).todense())


def _ref(g, kind, x, o, alpha=A_, beta=B_, val=None):
    return R.reference(g.rowptr, g.col, R.graph_vals(g, kind) if val is None else val, x, kind, alpha, beta, **o)


def _values(ref):
    return {k: r.v for k, r in ref.items()}


# ---------------------------------------------------------------------------
# the reference against torch in float64
# ---------------------------------------------------------------------------
def test_edge_graph_has_the_row_classes(edge):
    for chunk, g in edge.items():
        deg = np.diff(g.rowptr)
        for k in (0, 1, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 63, 64, 65, 96, 97, chunk + 1):
            assert (deg == k).any(), k
        nch = (deg + chunk - 1) // chunk
        assert set(R.hub_chunk_counts()) <= set(nch.tolist())
        h = g.marks["hub291"]
        assert nch[h] == 291 and deg[h] % chunk != 0
        assert (deg[::7] == 0).all()
        n_work, n_long, n_slots = R.schedule_counts(g.rowptr, chunk)
        assert 0 < n_long <= 1024
        # duplicates within a row are present (they add)
        r = g.marks["hub291"]
        cols = g.col[g.rowptr[r]:g.rowptr[r + 1]]
        assert np.unique(cols).size < cols.size


def test_other_graphs_reach_their_paths():
    g = R.many_long_graph()
    assert R.schedule_counts(g.rowptr, 32)[1] > 1024
    w = R.walk_graph()
    assert R.schedule_counts(w.rowptr, 32)[0] > 65536
    assert abs((np.diff(w.rowptr) == 0).mean() - 0.3) < 0.02
    e = R.edge_graph(32)
    rb = R.rebound(e)
    assert (np.diff(rb.rowptr) <= np.diff(e.rowptr)).all()
    assert np.diff(rb.rowptr)[e.marks["hub291"]] == 0


def test_layergcn_rows_equal_autograd(edge):
    g, d = edge[32], 32
    val = R.graph_vals(g, R.LAYERGCN)
    x, o = R.make_case(g, R.LAYERGCN, d)
    fwd = _ref(g, R.LAYERGCN, x, o)
    Ad = torch.from_numpy(_dense(g, val))
    Z = (af * (Ad @ torch.from_numpy(x.astype(np.float64)))).requires_grad_(True)  # z = alpha acc
    e = torch.from_numpy(o["e0"].astype(np.float64)).requires_grad_(True)
    c = F.cosine_similarity(Z, e, dim=-1)
    out = c[:, None] * Z
    ok = (np.diff(g.rowptr) > 0) & (np.abs(o["e0"]).sum(1) > 0)  # the non-degenerate rows
    assert ok.sum() > 500
    np.testing.assert_allclose(fwd["aux_w"].v[ok], c.detach().numpy()[ok], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(fwd["y"].v[ok], out.detach().numpy()[ok], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(fwd["s_out"].v[ok], (o["s_in"] + out.detach().numpy())[ok], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(fwd["aux"].v, Z.detach().numpy(), rtol=1e-12, atol=1e-13)
    # degenerate rows, exactly: an empty row has acc = 0, c = 0, y = 0; a zero e0 row c = 0, y = 0
    for rows in (np.diff(g.rowptr) == 0, np.arange(g.n_rows) == g.marks["zero_e0"]):
        assert not fwd["aux_w"].v[rows].any() and not fwd["aux_w"].bound[rows].any()
        assert not fwd["y"].v[rows].any() and not fwd["y"].bound[rows].any()
    assert not fwd["aux"].v[np.diff(g.rowptr) == 0].any()

    # backward: z, c from the forward, dE = alpha A xb + r_add
    xb, ob = R.make_case(g, R.LAYERGCN_BWD, d)
    ob["aux"] = fwd["aux"].v.astype(np.float32)
    z64 = torch.from_numpy(ob["aux"].astype(np.float64)).requires_grad_(True)
    e2 = torch.from_numpy(ob["e0"].astype(np.float64)).requires_grad_(True)
    c2 = F.cosine_similarity(z64, e2, dim=-1)
    ob["aux_w"] = c2.detach().numpy().astype(np.float32)
    bwd = _ref(g, R.LAYERGCN_BWD, xb, ob)
    dE = af * (Ad @ torch.from_numpy(xb.astype(np.float64))) + torch.from_numpy(ob["r_add"].astype(np.float64))
    (c2[:, None] * z64).backward(dE)
    ok = (np.abs(ob["aux"]).sum(1) > 0) & (np.abs(ob["e0"]).sum(1) > 0)
    # c was rounded to f32 on its way into aux_w: compare to that precision
    np.testing.assert_allclose(bwd["y"].v[ok], z64.grad.numpy()[ok], rtol=3e-6, atol=1e-6)
    np.testing.assert_allclose(bwd["s_out"].v[ok], (ob["s_in"] + e2.grad.numpy())[ok], rtol=3e-6, atol=1e-6)
    # a zero z row: y = c dE with one rounding, s_out = s_in exactly
    zr = np.abs(ob["aux"]).sum(1) == 0
    assert zr.any()
    np.testing.assert_array_equal(bwd["s_out"].v[zr], ob["s_in"][zr].astype(np.float64))
    assert not bwd["s_out"].bound[zr].any()
    cd = ob["aux_w"][zr].astype(np.float64)[:, None] * dE.numpy()[zr]
    np.testing.assert_allclose(bwd["y"].v[zr], cd, rtol=1e-13, atol=0)


def test_adam_equals_torch_optim_three_steps():
    n, d = 40, 32
    rng = np.random.default_rng(5)
    p = rng.standard_normal((n, d)).astype(np.float32)
    hp = dict(R.ADAM_HP)
    f32 = lambda k: float(np.float32(hp[k]))  # noqa: E731
    tp = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    opt = torch.optim.Adam([tp], lr=f32("lr"), betas=(f32("beta1"), f32("beta2")), eps=f32("eps"),
                           weight_decay=f32("weight_decay"))
    m, v = np.zeros_like(p, dtype=np.float64), np.zeros_like(p, dtype=np.float64)
    p64 = p.astype(np.float64)
    for step in (1, 2, 3):
        g = rng.standard_normal((n, d)).astype(np.float32)
        tp.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
        hp["step"] = step
        # float64 operands straight through (the reference promotes, it does not round)
        out = R.reference(None, None, None, None, R.ADAM, 1.0, 1.0, n_rows=n, d=d, s_in=g, p=p64, m=m, v=v, adam=hp)
        p64, m, v = out["p"].v, out["m"].v, out["v"].v
        np.testing.assert_allclose(p64, tp.detach().numpy(), rtol=1e-12, atol=1e-14)
        st = opt.state[tp]
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-15)


def test_final_with_four_stored_layers_is_the_plain_sum(edge):
    g, d = edge[64], 64
    x, o = R.make_case(g, R.FINAL, d)
    ref = _ref(g, R.FINAL, x, o)
    want = (sum(o[k].astype(np.float64) for k in ("s_in", "r_add", "aux", "e0"))
            + af * (_dense(g, g.val) @ x.astype(np.float64))) * bf
    np.testing.assert_allclose(ref["f"].v, want, rtol=1e-12, atol=1e-12)
    assert not ref["zero0"].v.any() and not ref["zero1"].v.any()


# ---------------------------------------------------------------------------
# a float32 evaluation stays inside every bound
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [32, 64])
@pytest.mark.parametrize("d", R.WIDTHS)
@pytest.mark.parametrize("kind", range(8), ids=R.KIND_NAMES)
def test_emulate_f32_is_within_every_bound(edge, kind, d, chunk):
    g = edge[chunk]
    x, o = R.make_case(g, kind, d)
    val = R.graph_vals(g, kind)
    ref = R.reference(g.rowptr, g.col, val, x, kind, A_, B_, **o)
    got = R.emulate_f32(g.rowptr, g.col, val, x, kind, A_, B_, chunk=chunk, **o)
    assert set(got) == set(ref)  # every output, every element
    ratios = R.assert_within(ref, got, o, f"{R.KIND_NAMES[kind]} d={d} chunk={chunk}")
    assert all(np.isfinite(r) for r in ratios.values())


@pytest.mark.parametrize("kind,flags", [(R.ADD, R.TAG_ROWS | R.TAG_SPARSE_X), (R.FINAL, R.TAG_ROWS),
                                        (R.ADAM, R.TAG_SPARSE_S | R.TAG_SPARSE_R | R.TAG_ZERO),
                                        (R.LAYERSUM, R.TAG_SPARSE_S | R.TAG_SPARSE_X)],
                         ids=["ADD-rows-x", "FINAL-rows", "ADAM-s-r-zero", "LAYERSUM-s-x"])
def test_emulate_f32_is_within_every_bound_under_tags(edge, kind, flags):
    g, d = edge[32], 32
    x, o = R.make_case(g, kind, d)
    tagged = R.tag_rows(g, x.shape[0])
    R.poison_untagged(o, x, tagged, flags, kind)
    o.update(row_tag=np.where(tagged, 7, 3).astype(np.int32), tag=7, tag_flags=flags)
    if kind == R.ADAM:
        o.update(reg_cnt=R.reg_counts(g.n_rows, np.random.default_rng(1), tagged[:g.n_rows], True), reg_k=R.REG_K)
        del o["r_add"]
    ref = R.reference(g.rowptr, g.col, g.val, x, kind, A_, B_, **o)
    got = R.emulate_f32(g.rowptr, g.col, g.val, x, kind, A_, B_, chunk=32, **o)
    assert set(got) == set(ref)
    R.assert_within(ref, got, o, R.KIND_NAMES[kind])


# ---------------------------------------------------------------------------
# the comparator reports every mutant
# ---------------------------------------------------------------------------
def _detected(ref, mutant, old):
    """The float64 result itself passes with ratio 0; the mutant is out of bound somewhere."""
    clean = R.compare(ref, {k: _values(ref)[k] for k in mutant}, old)
    assert all(v == 0.0 for v in clean.values()), clean
    return any(not v <= 1.0 for v in R.compare(ref, mutant, old).values())


@pytest.mark.parametrize("mark", ["deg9", "deg17"])
def test_mutant_dropped_last_nonzero(edge, mark):
    g, d = edge[32], 64
    x, o = R.make_case(g, R.STORE, d)
    ref = _ref(g, R.STORE, x, o)
    val = g.val.copy()
    val[g.rowptr[g.marks[mark] + 1] - 1] = 0
    mut = _values(_ref(g, R.STORE, x, o, val=val))
    assert _detected(ref, mut, o)
    # and it is that row the comparator objects to
    row = np.zeros(g.n_rows, dtype=bool)
    row[g.marks[mark]] = True
    assert (np.abs(mut["y"] - ref["y"].v) > ref["y"].bound)[row].any()


@pytest.mark.parametrize("chunk", [32, 64])
def test_mutant_dropped_hub_chunk(edge, chunk):
    g, d = edge[chunk], 32
    x, o = R.make_case(g, R.LAYERSUM, d)
    ref = _ref(g, R.LAYERSUM, x, o)
    val = g.val.copy()
    b = g.rowptr[g.marks["hub291"]] + 100 * chunk
    val[b:b + chunk] = 0
    assert _detected(ref, _values(_ref(g, R.LAYERSUM, x, o, val=val)), o)


@pytest.mark.parametrize("kind", [R.FINAL, R.ADD, R.ADAM, R.LAYERGCN_BWD], ids=lambda k: R.KIND_NAMES[k])
def test_mutant_omitted_r_add(edge, kind):
    g, d = edge[32], 32
    x, o = R.make_case(g, kind, d)
    ref = _ref(g, kind, x, o)
    assert _detected(ref, _values(_ref(g, kind, x, {k: v for k, v in o.items() if k != "r_add"})), o)


def test_mutant_beta_before_the_sum_in_final(edge):
    g, d = edge[32], 32
    x, o = R.make_case(g, R.FINAL, d)
    ref = _ref(g, R.FINAL, x, o)
    acc = _ref(g, R.STORE, x, {}, alpha=1.0)["y"].v
    f = bf * o["s_in"].astype(np.float64) + o["r_add"] + o["aux"] + o["e0"] + af * acc
    assert _detected(ref, {"f": f}, o)


@pytest.mark.parametrize("kind", range(8), ids=R.KIND_NAMES)
def test_mutant_omitted_alpha(edge, kind):
    g, d = edge[32], 32
    x, o = R.make_case(g, kind, d)
    ref = _ref(g, kind, x, o)
    assert _detected(ref, _values(_ref(g, kind, x, o, alpha=1.0)), o)


def test_mutant_zero1_left_uncleared(edge):
    g, d = edge[32], 32
    x, o = R.make_case(g, R.ADAM, d)
    ref = _ref(g, R.ADAM, x, o)
    assert _detected(ref, {"zero1": o["zero1"].astype(np.float64)}, o)


def test_mutant_neighbouring_rows_c_in_layergcn(edge):
    g, d = edge[32], 64
    x, o = R.make_case(g, R.LAYERGCN, d)
    ref = _ref(g, R.LAYERGCN, x, o)
    c = np.roll(ref["aux_w"].v, 1)
    y = c[:, None] * ref["aux"].v
    for mut in ({"y": y}, {"s_out": o["s_in"] + y}, {"aux_w": c}):
        assert _detected(ref, mut, o)


def test_mutant_backward_without_the_c_z_term(edge):
    g, d = edge[32], 64
    x, o = R.make_case(g, R.LAYERGCN_BWD, d)
    ref = _ref(g, R.LAYERGCN_BWD, x, o)
    z, e, c = (o[k].astype(np.float64) for k in ("aux", "e0", "aux_w"))
    dE = af * _ref(g, R.STORE, x, {}, alpha=1.0, val=np.abs(g.val))["y"].v + o["r_add"]
    nz = np.maximum(np.sqrt((z * z).sum(1)), R.EPS)
    ne = np.maximum(np.sqrt((e * e).sum(1)), R.EPS)
    gz = (dE * z).sum(1)
    y = c[:, None] * dE + (gz / (nz * ne))[:, None] * e
    assert _detected(ref, {"y": y}, o)
    # the full formula, assembled the same way, is not reported
    kz = np.where(nz > R.EPS, c / (nz * nz), 0.0)
    assert R.compare(ref, {"y": y - (gz * kz)[:, None] * z}, o)["y"] <= 1e-6


def test_mutant_reads_untagged_s_in_under_sparse_s(edge):
    g, d = edge[32], 32
    for kind in (R.ADD, R.ADAM, R.LAYERSUM, R.AXPBY, R.FINAL):
        x, o = R.make_case(g, kind, d)
        tagged = R.tag_rows(g, x.shape[0])
        o.update(row_tag=np.where(tagged, 7, 3).astype(np.int32), tag=7, tag_flags=R.TAG_SPARSE_S)
        ref = _ref(g, kind, x, o)
        mut = _values(_ref(g, kind, x, dict(o, tag_flags=0)))  # s_in read on every row
        assert _detected(ref, mut, o), R.KIND_NAMES[kind]
