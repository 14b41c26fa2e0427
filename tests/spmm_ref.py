"""The contract of rsx_spmm / rsx_rowwise (include/rsx.h) restated in numpy float64.

reference() evaluates one call as the header's comment block states it and returns,
for every output the kind writes, the float64 value, the bound a correct f32
evaluation must meet, and the rows that are written at all (the others keep their
old contents).  emulate_f32() evaluates the same call in numpy float32 in the
summation order the header documents; the CPU tests require it to stay inside every
bound, which shows the bounds are attainable without looking at the kernel.
compare() is the comparator both the CPU and the GPU tests call.

Where the bounds come from (u = 2^-24, the f32 unit roundoff; nothing is fitted):

  accumulator   dacc = 1e-5 |acc| + 2e-7 (|A||x|) sqrt(max(deg, 1)), the bound
                test_gpu_kernels.py uses for the plain product.
  linear kinds  every quantity is carried as (value, error).  One f32 multiply a*b adds
                u |a b| to |a| eb + |b| ea; one f32 add adds u (|a| + |b|) to ea + eb,
                except that adding an exact zero is exact.  STORE, LAYERSUM, FINAL,
                AXPBY, ADD, ADAM's g, m and v (first order in g) all go through this
                arithmetic, so |scale| dacc and one roundoff per epilogue operation
                fall out of it, and a row whose result is exact gets the bound 0.
  p of ADAM     max |P(g + dg) - P(g)|, |P(g - dg) - P(g)| with P the float64 update
                as a function of the gradient, plus the update's own rounding (the same
                error arithmetic run with an exact g; the f32-rounded constants
                1 - beta1, 1 - beta2, lr / bc1, sqrt(bc2) carry u each).
  LAYERGCN      z = alpha acc, c = <z / nz, e / ne> with nz = max(|z|, eps), ne = max(|e|, eps).
                The computed z is z + dz, |dz| <= |alpha| dacc + u |z|.  For unit vectors,
                | (z + dz)/|z + dz| - z/|z| | <= 2 |dz|_2 / |z|_2, and |e / ne| =
                |e|_2 / ne <= 1, so the accumulator moves c by at most
                2 |dz|_2 / |z|_2 * (|e|_2 / ne).  Rounding: a d-term f32 dot product in
                any order is off by at most gamma_d sum |x_i y_i|, gamma_d = d u / (1 - d u).
                <z, e> therefore adds gamma_d sum |z_i e_i| / (nz ne) to c; <z, z> and
                <e, e> (positive terms) are relatively gamma_d accurate, their square
                roots gamma_d / 2 + u each; the product nz * ne and the division add u
                each: |c| (gamma_d + 4 u).  Together
                  dc = 2 |dz|_2 / |z|_2 (|e|_2 / ne) + gamma_d sum|z_i e_i| / (nz ne)
                       + |c| (gamma_d + 4 u).
                y = c z: dy = |c| dz + |z| dc + dc dz + u |c z|; s_out = s_in + y adds one
                add; aux = z carries dz; aux_w = c carries dc.  A zero z row has dz = 0 and
                c = 0 exactly; a zero e0 row has <z, e> = 0 exactly, so dc = 0 and y = 0.
  LAYERGCN_BWD  z, c, e are inputs (exact).  dE = alpha acc + r_add carries ddE from the
                linear arithmetic.  gz = <dE, z>: dgz = sum |z_i| ddE_i + gamma_d sum |dE_i z_i|.
                inv = 1 / (nz ne) is relatively gamma_d + 4 u accurate (two norms, one
                multiply, one divide), and so are kz = c / nz^2 and ke = c / ne^2.  The
                coefficients A = gz inv, Bz = gz kz, Be = gz ke carry
                  dA = inv dgz + |A| (gamma_d + 5 u),  dB = |k| dgz + |B| (gamma_d + 5 u),
                and y = c dE + A e - Bz z, s_out = s_in + (A z - Be e) are assembled with
                the linear arithmetic (an fma counted as two roundings).  A zero z row
                has gz = 0 exactly: y = c dE with one rounding, s_out = s_in.

emulate_f32 rounds every product and every add (two roundings where the kernel may
use one fma), sums the nonzeros of a work item of `chunk` nonzeros in order and a
split row's partials in chunk order.  (The header documents that order for a row of up
to 256 / (d / 4) chunks and another fixed order beyond; the bounds hold for any order.)
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import scipy.sparse as sp

STORE, LAYERSUM, FINAL, ADAM, LAYERGCN, AXPBY, LAYERGCN_BWD, ADD = range(8)
KIND_NAMES = ["STORE", "LAYERSUM", "FINAL", "ADAM", "LAYERGCN", "AXPBY", "LAYERGCN_BWD", "ADD"]
TAG_ROWS, TAG_SPARSE_X, TAG_SPARSE_S, TAG_SPARSE_R, TAG_ZERO = 1, 2, 4, 8, 16
WIDTHS = (32, 64, 128, 256)

U = 2.0 ** -24
EPS = float(np.float32(1e-8))  # the clamp of F.cosine_similarity, as the f32 constant the header names
F64, F32 = np.float64, np.float32

# value, bound: [n_rows, ...] float64; rows: bool [n_rows], the rows the call writes
Out = namedtuple("Out", "v bound rows")


# ---------------------------------------------------------------------------
# (value, error) arithmetic and its float32 twin
# ---------------------------------------------------------------------------
class E:
    """A float64 value with a bound on the error of its f32 evaluation."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=F64)
        self.e = np.broadcast_to(np.asarray(e, dtype=F64), self.v.shape) if np.ndim(e) <= self.v.ndim \
            else np.asarray(e, dtype=F64)

    def exact_zero(self):
        return (self.v == 0) & (self.e == 0)


class Bound64:
    """float64 values carrying first-order f32 rounding bounds."""

    def lift(self, a):
        return E(np.asarray(a, dtype=F64))

    def const(self, c, rounded=False):
        c = float(c)
        return E(c, U * abs(c) if rounded else 0.0)

    def add(self, a, b):
        r = U * (np.abs(a.v) + np.abs(b.v))
        r = np.where(a.exact_zero() | b.exact_zero(), 0.0, r)
        return E(a.v + b.v, a.e + b.e + r)

    def sub(self, a, b):
        return self.add(a, E(-b.v, b.e))

    def mul(self, a, b):
        v = a.v * b.v
        return E(v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e + U * np.abs(v))

    def div(self, a, b):
        v = a.v / b.v
        return E(v, (a.e + np.abs(v) * b.e) / np.abs(b.v) + U * np.abs(v))

    def sqrt(self, a):
        v = np.sqrt(a.v)
        return E(v, a.e / (2.0 * np.where(v > 0, v, 1.0)) + U * v)

    def col(self, a):  # a per-row quantity against [n, d] rows
        return E(a.v[:, None], a.e[:, None])


class Float32:
    """numpy float32: every operation rounds once."""

    def lift(self, a):
        return np.asarray(a, dtype=F32)

    def const(self, c, rounded=False):
        return F32(c)

    def add(self, a, b):
        return (a + b).astype(F32)

    def sub(self, a, b):
        return (a - b).astype(F32)

    def mul(self, a, b):
        return (a * b).astype(F32)

    def div(self, a, b):
        return (a / b).astype(F32)

    def sqrt(self, a):
        return np.sqrt(a).astype(F32)

    def col(self, a):
        return a[:, None]


# ---------------------------------------------------------------------------
# the product
# ---------------------------------------------------------------------------
def _masked(x, mask, dtype):
    x = np.asarray(x, dtype=dtype)
    return x if mask is None else np.where(mask[:, None], x, dtype(0))


def product64(rowptr, col, val, x, xmask=None):
    """acc = A x in float64 (duplicate columns add) with the accumulator bound; rows of x
    off `xmask` count as zero whatever they hold."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = rowptr.size - 1
    X = _masked(x, xmask, F64)
    val, col = np.asarray(val, dtype=F64), np.asarray(col, dtype=np.int64)
    acc = np.asarray(sp.csr_matrix((val, col, rowptr), shape=(n, X.shape[0])) @ X)
    # |A| from |val| entry by entry (abs() of a scipy matrix would add duplicates first)
    mag = np.asarray(sp.csr_matrix((np.abs(val), col, rowptr), shape=(n, X.shape[0])) @ np.abs(X))
    deg = np.diff(rowptr).astype(F64)[:, None]
    return E(acc, 1e-5 * np.abs(acc) + 2e-7 * mag * np.sqrt(np.maximum(deg, 1.0)))


def product32(rowptr, col, val, x, chunk, xmask=None):
    """acc = A x in float32: a work item's nonzeros (at most `chunk`) in nonzero order from
    zero, a split row's partials then added in chunk order."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = rowptr.size - 1
    X = _masked(x, xmask, F32)
    val = np.asarray(val, dtype=F32)
    col = np.asarray(col, dtype=np.int64)
    deg = np.diff(rowptr)
    nch = np.maximum((deg + chunk - 1) // chunk, 1)  # an empty row is one empty item
    first = np.concatenate([[0], np.cumsum(nch)])
    row_of = np.repeat(np.arange(n), nch)
    k_of = np.arange(first[-1]) - first[row_of]
    beg = rowptr[row_of] + k_of * chunk
    end = np.minimum(beg + chunk, rowptr[row_of + 1])
    part = np.zeros((first[-1], X.shape[1]), dtype=F32)
    for t in range(chunk):
        live = np.nonzero(beg + t < end)[0]
        if live.size == 0:
            break
        j = beg[live] + t
        part[live] = (part[live] + (val[j][:, None] * X[col[j]]).astype(F32)).astype(F32)
    acc = part[first[:-1]].copy()
    for k in range(1, int(nch.max())):
        rows = np.nonzero(nch > k)[0]
        acc[rows] = (acc[rows] + part[first[rows] + k]).astype(F32)
    return acc


# ---------------------------------------------------------------------------
# LayerGCN rows: float64 with bounds, and float32
# ---------------------------------------------------------------------------
def _norms64(z, e):
    rz, re = np.sqrt((z * z).sum(1)), np.sqrt((e * e).sum(1))
    return rz, re, np.maximum(rz, EPS), np.maximum(re, EPS)


def _lgcn_fwd64(ar, acc, e0, s_in):
    z, dz = acc.v, acc.e
    e = np.asarray(e0, dtype=F64)
    d = z.shape[1]
    gam = d * U / (1.0 - d * U)
    rz, re, nz, ne = _norms64(z, e)
    c = (z * e).sum(1) / (nz * ne)
    ndz = np.sqrt((dz * dz).sum(1))
    dc = np.where(rz > 0, 2.0 * ndz / np.where(rz > 0, rz, 1.0), 0.0) * (re / ne) \
        + gam * (np.abs(z) * np.abs(e)).sum(1) / (nz * ne) + np.abs(c) * (gam + 4.0 * U)
    cz = c[:, None] * z
    y = E(cz, np.abs(c)[:, None] * dz + np.abs(z) * dc[:, None] + dc[:, None] * dz + U * np.abs(cz))
    s = ar.add(ar.lift(s_in), y) if s_in is not None else y
    return {"y": y, "s_out": s, "aux": acc, "aux_w": E(c, dc)}


def _lgcn_fwd32(ar, acc, e0, s_in):
    z, e = acc, np.asarray(e0, dtype=F32)
    dot = lambda a, b: (a * b).astype(F32).sum(1, dtype=F32)  # noqa: E731
    nz = np.maximum(np.sqrt(dot(z, z)), F32(1e-8))
    ne = np.maximum(np.sqrt(dot(e, e)), F32(1e-8))
    c = (dot(z, e) / (nz * ne).astype(F32)).astype(F32)
    y = (c[:, None] * z).astype(F32)
    s = (np.asarray(s_in, dtype=F32) + y).astype(F32) if s_in is not None else y
    return {"y": y, "s_out": s, "aux": z, "aux_w": c}


def _lgcn_bwd64(ar, dE, z, c, e, s_in):
    z, c, e = (np.asarray(t, dtype=F64) for t in (z, c, e))
    d = z.shape[1]
    gam = d * U / (1.0 - d * U)
    rz, re, nz, ne = _norms64(z, e)
    gz = (dE.v * z).sum(1)
    dgz = (np.abs(z) * dE.e).sum(1) + gam * np.abs(dE.v * z).sum(1)
    inv = 1.0 / (nz * ne)
    kz = np.where(rz > EPS, c / (nz * nz), 0.0)  # the clamped norm is a constant: no second term
    ke = np.where(re > EPS, c / (ne * ne), 0.0)
    rel = gam + 5.0 * U

    def coef(k):
        v = gz * k
        return v, np.abs(k) * dgz + np.abs(v) * rel

    def term(cf, w):  # coefficient (value, error) times an exact row, one multiply
        v = cf[0][:, None] * w
        return E(v, np.abs(w) * cf[1][:, None] + U * np.abs(v))

    A, Bz, Be = coef(inv), coef(kz), coef(ke)
    neg = lambda cf: (-cf[0], cf[1])  # noqa: E731
    y = ar.add(ar.add(ar.mul(E(c[:, None]), dE), term(A, e)), term(neg(Bz), z))
    de = ar.add(term(A, z), term(neg(Be), e))
    s = ar.add(ar.lift(s_in), de) if s_in is not None else de
    return {"y": y, "s_out": s}


def _lgcn_bwd32(ar, dE, z, c, e, s_in):
    z, c, e = (np.asarray(t, dtype=F32) for t in (z, c, e))
    dot = lambda a, b: (a * b).astype(F32).sum(1, dtype=F32)  # noqa: E731
    rz, re = np.sqrt(dot(z, z)), np.sqrt(dot(e, e))
    nz, ne = np.maximum(rz, F32(1e-8)), np.maximum(re, F32(1e-8))
    gz = dot(dE, z)
    inv = (F32(1) / (nz * ne).astype(F32)).astype(F32)
    kz = np.where(rz > F32(1e-8), (c / (nz * nz).astype(F32)).astype(F32), F32(0))
    ke = np.where(re > F32(1e-8), (c / (ne * ne).astype(F32)).astype(F32), F32(0))
    A, Bz, Be = (gz * inv).astype(F32), (gz * kz).astype(F32), (gz * ke).astype(F32)
    y = (c[:, None] * dE).astype(F32)
    y = (y + (A[:, None] * e).astype(F32)).astype(F32)
    y = (y - (Bz[:, None] * z).astype(F32)).astype(F32)
    de = ((A[:, None] * z).astype(F32) - (Be[:, None] * e).astype(F32)).astype(F32)
    s = (np.asarray(s_in, dtype=F32) + de).astype(F32) if s_in is not None else de
    return {"y": y, "s_out": s}


# ---------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------
def adam_consts(adam):
    """torch.optim.Adam's scalars from the f32 hyper-parameters of rsx_adam (float64)."""
    lr, b1, b2, eps, wd = (float(F32(adam[k])) for k in ("lr", "beta1", "beta2", "eps", "weight_decay"))
    step = int(adam["step"])
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return dict(lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, omb1=1.0 - b1, omb2=1.0 - b2, step_size=lr / bc1,
                bc2_sqrt=np.sqrt(bc2))


def _adam(ar, p, m, v, g, k):
    """One torch.optim.Adam update in the arithmetic `ar`; returns p, m, v and the gradient
    the moments saw (weight decay included)."""
    if k["wd"] != 0.0:
        g = ar.add(g, ar.mul(ar.const(k["wd"]), p))
    m2 = ar.add(m, ar.mul(ar.const(k["omb1"], True), ar.sub(g, m)))
    v2 = ar.add(ar.mul(v, ar.const(k["b2"])), ar.mul(ar.mul(ar.const(k["omb2"], True), g), g))
    denom = ar.add(ar.div(ar.sqrt(v2), ar.const(k["bc2_sqrt"], True)), ar.const(k["eps"]))
    p2 = ar.add(p, ar.div(ar.mul(ar.const(-k["step_size"], True), m2), denom))
    return p2, m2, v2, g


def _adam_p64(p, m, v, g, k):
    if k["wd"] != 0.0:
        g = g + k["wd"] * p
    m2 = m + k["omb1"] * (g - m)
    v2 = v * k["b2"] + k["omb2"] * g * g
    return p - k["step_size"] * m2 / (np.sqrt(v2) / k["bc2_sqrt"] + k["eps"])


# ---------------------------------------------------------------------------
# one call
# ---------------------------------------------------------------------------
def _call(ar, is64, rowptr, col, val, x, kind, alpha, beta, chunk, n_rows, d, o):
    """The call in arithmetic `ar`: {output: (value, rows written)} and the cleared counts."""
    n = int(n_rows) if rowptr is None else len(rowptr) - 1
    row_tag = o.get("row_tag")
    flags = int(o.get("tag_flags", 0)) if row_tag is not None else 0
    tag = int(o.get("tag", 0))
    every = np.ones(n, dtype=bool)
    tagged = (np.asarray(row_tag)[:n] == tag) if flags else every
    live = tagged if flags & TAG_ROWS else every  # untagged output rows are skipped entirely
    if rowptr is None:
        acc = ar.lift(np.zeros((n, d)))
    else:
        xmask = None
        if flags & TAG_SPARSE_X:  # x rows not tagged are zero, whatever the memory holds
            xt = np.asarray(o["x_tag"] if o.get("x_tag") is not None else row_tag)
            xmask = np.zeros(np.asarray(x).shape[0], dtype=bool)
            k = min(xt.size, xmask.size)
            xmask[:k] = xt[:k] == tag
        acc = product64(rowptr, col, val, x, xmask) if is64 else product32(rowptr, col, val, x, chunk, xmask)

    def opnd(name, flag=0):  # a row operand, zero off the tagged rows under its flag; None = NULL
        t = o.get(name)
        if t is None:
            return None
        return ar.lift(_masked(t, tagged if flags & flag else None, F64 if is64 else F32))

    a_, b_ = ar.const(F32(alpha)), ar.const(F32(beta))
    sacc = ar.mul(a_, acc)
    out = {}

    def regc(honour_sparse_r):  # (cnt[3r] k0 + cnt[3r+1] k1) + cnt[3r+2] k2 per row, in f32
        cnt = np.asarray(o["reg_cnt"]).reshape(-1)[:3 * n].reshape(n, 3)
        rk = np.asarray(o["reg_k"], dtype=F32)
        if honour_sparse_r and flags & TAG_SPARSE_R:
            cnt = np.where(tagged[:, None], cnt, 0)
        t = [ar.mul(ar.lift(cnt[:, i]), ar.const(rk[i])) for i in range(3)]
        return ar.col(ar.add(ar.add(t[0], t[1]), t[2]))

    if kind == STORE:
        out["y"] = sacc
    elif kind == LAYERSUM:
        s = opnd("s_in", TAG_SPARSE_S)
        out["y"] = sacc
        out["s_out"] = ar.add(s, sacc) if s is not None else sacc
    elif kind == FINAL:
        t = None
        for term in (opnd("s_in", TAG_SPARSE_S), opnd("r_add", TAG_SPARSE_R), opnd("aux"), opnd("e0")):
            if term is not None:
                t = term if t is None else ar.add(t, term)
        out["f"] = ar.mul(b_, ar.add(t, sacc) if t is not None else sacc)
    elif kind == AXPBY:
        s = opnd("s_in", TAG_SPARSE_S)
        out["y"] = ar.add(sacc, ar.mul(b_, s)) if s is not None else sacc
    elif kind == ADD:
        t = sacc
        s, r = opnd("s_in", TAG_SPARSE_S), opnd("r_add", TAG_SPARSE_R)
        if s is not None:
            t = ar.add(t, s)
        if o.get("reg_cnt") is not None:  # every written row's counts are read and cleared
            t = ar.add(t, ar.mul(regc(False), opnd("p")))
            out["reg_cnt"] = live
        elif r is not None:
            t = ar.add(t, r)
        out["y"] = ar.mul(b_, t)
    elif kind == ADAM:
        s, r = opnd("s_in", TAG_SPARSE_S), opnd("r_add", TAG_SPARSE_R)
        p, m, v = opnd("p"), opnd("m"), opnd("v")
        g = ar.mul(b_, ar.add(s, sacc) if s is not None else sacc)
        if o.get("reg_cnt") is not None:
            g = ar.add(g, ar.mul(regc(True), p))
            out["reg_cnt"] = live & tagged if flags & TAG_ZERO else np.zeros(n, dtype=bool)  # else left
        elif r is not None:
            g = ar.add(g, r)
        k = adam_consts(o["adam"])
        p2, m2, v2, gw = _adam(ar, p, m, v, g, k)
        if is64:
            # p: the float64 update at g +- dg, plus the update's own rounding (exact g)
            p0 = _adam_p64(p.v, m.v, v.v, g.v, k)
            move = np.maximum(np.abs(_adam_p64(p.v, m.v, v.v, g.v + g.e, k) - p0),
                              np.abs(_adam_p64(p.v, m.v, v.v, g.v - g.e, k) - p0))
            p2 = E(p0, move + _adam(ar, p, m, v, E(g.v), k)[0].e)
        wr = live if not int(o.get("halt", 0)) else np.zeros(n, dtype=bool)  # halted: p, m, v stay
        out["p"], out["m"], out["v"] = (p2, wr), (m2, wr), (v2, wr)
        out["g_out"] = gw
    elif kind == LAYERGCN:
        f = _lgcn_fwd64 if is64 else _lgcn_fwd32
        out.update(f(ar, sacc, o["e0"], o.get("s_in")))  # z = alpha acc; s_in is loaded under any flag
    elif kind == LAYERGCN_BWD:
        r = opnd("r_add")
        dE = ar.add(sacc, r) if r is not None else sacc
        f = _lgcn_bwd64 if is64 else _lgcn_bwd32
        out.update(f(ar, dE, o["aux"], o["aux_w"], o["e0"], o.get("s_in")))
    else:
        raise ValueError(f"kind {kind}")
    res = {name: (t if isinstance(t, tuple) else (t, live)) for name, t in out.items() if name != "reg_cnt"}
    cleared = {"reg_cnt": out["reg_cnt"]} if "reg_cnt" in out else {}
    zrows = live & tagged if flags & TAG_ZERO else live
    for name in ("zero0", "zero1"):
        if o.get(name) is not None:
            cleared[name] = zrows
    return n, res, cleared


def _dims(rowptr, x, n_rows, d):
    if rowptr is None:
        return int(n_rows), int(d)
    return len(rowptr) - 1, int(np.asarray(x).shape[1])


def reference(rowptr, col, val, x, kind, alpha, beta, n_rows=None, d=None, **o):
    """{output: Out(value, bound, rows)} of rsx_spmm (rowptr None: rsx_rowwise over n_rows rows
    of width d, acc = 0).  Operands are passed by their rsx_epilogue names; a missing one is
    NULL.  `adam` is a dict (lr, beta1, beta2, eps, weight_decay, step: the host step or the
    value step_dev holds).  zero0 / zero1 / reg_cnt are given with their old contents and come
    back cleared on the documented rows."""
    n, d = _dims(rowptr, x, n_rows, d)
    if n > _BLOCK:
        return _reference_by_blocks(rowptr, col, val, x, kind, alpha, beta, n, d, o)
    _, res, cleared = _call(Bound64(), True, rowptr, col, val, x, kind, alpha, beta, None, n, d, o)
    outs = {name: Out(t.v, t.e, rows) for name, (t, rows) in res.items()}
    for name, rows in cleared.items():
        old = np.asarray(o[name])
        if name == "reg_cnt":
            new = old.copy().reshape(-1)
            new[:3 * n] = np.where(np.repeat(rows, 3), 0, new[:3 * n])
            outs[name] = Out(new.astype(F64), np.zeros(new.shape), np.ones(new.size, dtype=bool))
        else:
            outs[name] = Out(np.zeros(old.shape), np.zeros(old.shape), rows)
    return outs


_BLOCK = 4096
_ROW_OPERANDS = ("y", "s_in", "s_out", "f", "zero0", "zero1", "r_add", "p", "m", "v", "g_out", "e0", "aux", "aux_w")


def _reference_by_blocks(rowptr, col, val, x, kind, alpha, beta, n, d, o):
    """reference() over blocks of rows (rows are independent): a block's arrays stay in the
    cache, and the blocks run on a few threads.  Same values as one call over all rows."""
    import os
    from concurrent.futures import ThreadPoolExecutor

    def block(r0):
        r1 = min(r0 + _BLOCK, n)
        ob = {}
        for k, v in o.items():
            if k in _ROW_OPERANDS and v is not None:
                ob[k] = v[r0:r1]
            elif k == "reg_cnt" and v is not None:
                ob[k] = np.asarray(v).reshape(-1)[3 * r0:3 * r1]
            elif k == "row_tag" and v is not None:
                ob[k] = v[r0:r1]
                if o.get("x_tag") is None:
                    ob["x_tag"] = v  # X's rows keep their own numbering
            elif k != "x_tag" or v is not None:
                ob[k] = v
        if rowptr is None:
            return reference(None, None, None, None, kind, alpha, beta, n_rows=r1 - r0, d=d, **ob)
        b, e = int(rowptr[r0]), int(rowptr[r1])
        return reference(np.asarray(rowptr[r0:r1 + 1]) - b, col[b:e], val[b:e], x, kind, alpha, beta, **ob)

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        parts = list(pool.map(block, range(0, n, _BLOCK)))
    outs = {}
    for name in parts[0]:
        v, bound, rows = (np.concatenate([getattr(p[name], f) for p in parts]) for f in Out._fields)
        if name == "reg_cnt":  # whatever follows the 3 n counts (the scales) is not the call's
            tail = np.asarray(o[name]).reshape(-1)[3 * n:].astype(F64)
            v, bound, rows = np.concatenate([v, tail]), np.zeros(v.size + tail.size), np.ones(v.size + tail.size, bool)
        outs[name] = Out(v, bound, rows)
    return outs


def emulate_f32(rowptr, col, val, x, kind, alpha, beta, chunk=32, n_rows=None, d=None, **o):
    """The same call evaluated in numpy float32: {output: array}, the rows the call does not
    write holding the old contents passed under the output's name (zero if none)."""
    n, d = _dims(rowptr, x, n_rows, d)
    _, res, cleared = _call(Float32(), False, rowptr, col, val, x, kind, alpha, beta, chunk, n, d, o)
    got = {}
    for name, (t, rows) in res.items():
        t = np.asarray(t, dtype=F32)
        old = np.asarray(o[name], dtype=F32) if o.get(name) is not None else np.zeros_like(t)
        got[name] = np.where(rows.reshape((-1,) + (1,) * (t.ndim - 1)), t, old)
    for name, rows in cleared.items():
        old = np.asarray(o[name])
        if name == "reg_cnt":
            new = old.copy().reshape(-1)
            new[:3 * n] = np.where(np.repeat(rows, 3), 0, new[:3 * n])
            got[name] = new
        else:
            got[name] = np.where(rows[:, None], F32(0), old.astype(F32))
    return got


# ---------------------------------------------------------------------------
# the comparator
# ---------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def compare(ref, got, old=None):
    """{output: largest error / bound} over every element of every array in `got` (each must
    be an output of `ref`).  An element with bound 0 must match exactly (ratio 0, else inf); a
    non-finite value where the reference is finite is inf; a row the call does not write must
    hold the bits of old[output] (else inf)."""
    ratios = {}
    for name, g in got.items():
        r = ref[name]
        g = np.asarray(g)
        if g.shape != r.v.shape:
            raise AssertionError(f"{name}: shape {g.shape}, reference {r.v.shape}")
        rows = r.rows.reshape((-1,) + (1,) * (g.ndim - 1))
        err = np.abs(g.astype(F64) - r.v)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err <= r.bound, np.where(r.bound > 0, err / r.bound, 0.0), np.inf)
        q = np.where(np.isfinite(g), q, np.inf)
        worst = float(np.max(np.where(rows, q, 0.0), initial=0.0))
        if not r.rows.all():
            if old is None or old.get(name) is None:
                raise AssertionError(f"{name}: rows are left unwritten and no old contents were given")
            same = bits(g) == bits(np.asarray(old[name]).astype(g.dtype, copy=False))
            if not np.all(np.where(rows, True, same)):
                worst = np.inf
        ratios[name] = worst
    return ratios


def assert_within(ref, got, old=None, what=""):
    ratios = compare(ref, got, old)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{what}: error / bound {bad}"
    return ratios


# ---------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------
Graph = namedtuple("Graph", "rowptr col val n_rows n_cols chunk marks")


def schedule_counts(rowptr, chunk):
    """(n_work, n_long, n_slots) of rsx_csr_schedule_host."""
    deg = np.diff(np.asarray(rowptr))
    long_ = deg > chunk
    slots = int(((deg[long_] + chunk - 1) // chunk).sum())
    return int(slots + (~long_).sum()), int(long_.sum()), slots


def _from_degrees(deg, n_cols, rng, chunk, marks=None):
    deg = np.asarray(deg, dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    col = rng.integers(0, n_cols, size=int(rowptr[-1])).astype(np.int32)  # duplicates allowed
    val = rng.standard_normal(col.size).astype(F32)
    return Graph(rowptr, col, val, deg.size, n_cols, chunk, marks or {})


def hub_chunk_counts():
    """Chunk counts that put a hub's fixup on either side of the four-accumulator loop for
    every groups-per-block value (GPB = 256 / (d / 4) = 32, 16, 8, 4)."""
    s = {2, 3}
    for gpb in (32, 16, 8, 4):
        s |= {gpb, 3 * gpb, 3 * gpb + 1, 4 * gpb, 4 * gpb + 1}
    return sorted(s)


def edge_graph(chunk, seed=11):
    """640 x 700 with explicit short, just-long and hub degrees (see the GPU test's module
    docstring); marks: 'hubs' (rows), 'deg9', 'deg17', 'hub291', 'zero_e0' (a short non-empty row)."""
    rng = np.random.default_rng(seed + chunk)
    n_rows, n_cols = 640, 700
    deg = rng.geometric(0.15, size=n_rows)
    deg[::7] = 0
    explicit = [0, 1, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 63, 64, 65, 96, 97, chunk + 1]
    hubs = [(k - 1) * chunk + int(rng.integers(1, chunk + 1)) for k in hub_chunk_counts()]
    hubs.append(290 * chunk + chunk // 2 - 3)  # 291 chunks, the last one partial
    # spread over the rows that are not forced empty, hubs at both ends of the row range
    free = [r for r in range(n_rows) if r % 7]
    slots = free[3:3 + len(explicit)] + free[40:40 + len(hubs) - 4] + free[-4:]
    for r, k in zip(slots, explicit + hubs):
        deg[r] = k
    marks = {"deg9": slots[explicit.index(9)], "deg17": slots[explicit.index(17)],
             "hubs": np.asarray(slots[len(explicit):]), "hub291": slots[-1], "zero_e0": free[30]}
    assert deg[marks["zero_e0"]] > 0
    return _from_degrees(deg, n_cols, rng, chunk, marks)


def many_long_graph(chunk=32, seed=12):
    """1,100 rows of degree 33..100 plus 200 short ones: more than 1,024 split rows, so the
    fixups run as a launch of their own."""
    rng = np.random.default_rng(seed)
    deg = np.concatenate([rng.integers(33, 101, size=1100), rng.integers(0, 20, size=200)])
    return _from_degrees(rng.permutation(deg), 700, rng, chunk)


def walk_graph(chunk=32, seed=13, n_rows=66400):
    """Rows of degree 0..40, 30 % empty, 700 columns: more work items than 2,048 blocks hold
    groups at any width, so every group walks several items."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(1, 41, size=n_rows)
    deg[rng.random(n_rows) < 0.3] = 0
    return _from_degrees(deg, 700, rng, chunk)


def rebound(g, seed=14):
    """A graph keeping about half of each row's nonzeros of `g` (every row's degree <= the
    template's); the 291-chunk hub and some short rows become empty."""
    rng = np.random.default_rng(seed)
    keep = rng.random(g.col.size) < 0.5
    rows = np.repeat(np.arange(g.n_rows), np.diff(g.rowptr))
    empty = np.zeros(g.n_rows, dtype=bool)
    empty[g.marks["hub291"]] = True
    empty[rng.choice(g.n_rows, size=25, replace=False)] = True
    empty[g.marks["hubs"][:-1]] = False
    keep &= ~empty[rows]
    deg = np.bincount(rows[keep], minlength=g.n_rows)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    return Graph(rowptr, g.col[keep], g.val[keep], g.n_rows, g.n_cols, g.chunk, g.marks)


# ---------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------
ALPHA, BETA = 0.7, 1.0 / 3.0
ADAM_HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, step=3)
# per kind: the row operands it reads, and the outputs it writes
READS = {STORE: (), LAYERSUM: ("s_in",), FINAL: ("s_in", "r_add", "aux", "e0"), ADAM: ("s_in", "r_add"),
         LAYERGCN: ("e0", "s_in"), AXPBY: ("s_in",), LAYERGCN_BWD: ("r_add", "aux", "e0", "s_in"),
         ADD: ("s_in", "r_add")}
WRITES = {STORE: ("y",), LAYERSUM: ("y", "s_out"), FINAL: ("f",), ADAM: ("p", "m", "v", "g_out"),
          LAYERGCN: ("y", "s_out", "aux", "aux_w"), AXPBY: ("y",), LAYERGCN_BWD: ("y", "s_out"), ADD: ("y",)}


def make_case(g, kind, d, seed=0, n_rows=None):
    """Seeded operands for one call on graph `g` (None: rowwise over n_rows): (x, operands).
    Signed values for the linear kinds; the LayerGCN kinds take |val| on the graph side (see
    graph_vals).  Outputs are pre-filled with a NaN-payload sentinel, zero0 / zero1 with
    non-zero values, ADAM's m and v with non-zero moments."""
    rng = np.random.default_rng(1000 * kind + d + seed)
    n = g.n_rows if g is not None else n_rows
    x = rng.standard_normal((g.n_cols + 5, d)).astype(F32) if g is not None else None
    rnd = lambda: rng.standard_normal((n, d)).astype(F32)  # noqa: E731
    o = {name: rnd() for name in READS[kind]}
    for name in WRITES[kind]:
        if name not in o:
            o[name] = sentinel((n,) if name == "aux_w" else (n, d))
    o["zero0"], o["zero1"] = rnd() + F32(3), rnd() - F32(3)
    if kind == ADAM:
        o["p"] = rnd()
        o["m"] = (0.1 * rng.standard_normal((n, d))).astype(F32)
        o["v"] = (0.01 + 0.1 * rng.random((n, d))).astype(F32)
        o["adam"] = dict(ADAM_HP)
    if kind in (LAYERGCN, LAYERGCN_BWD):
        zr = g.marks.get("zero_e0") if g is not None else 5
        if zr is not None:
            o["e0"][zr] = 0
    if kind == LAYERGCN_BWD:
        o["aux_w"] = rng.uniform(-1, 1, size=n).astype(F32)
        deg = np.diff(g.rowptr) if g is not None else np.arange(n) % 3
        o["aux"][deg == 0] = 0  # the rows the forward leaves with a zero pre-scale row
        if zr is not None:
            o["aux_w"][zr] = 0  # what the forward saves for a zero ego row
    return x, o


def sentinel(shape):
    """float32 NaNs with a payload: a row the kernel must not touch keeps these exact bits."""
    return np.full(shape, 0x7FC0BEEF, dtype=np.uint32).view(F32)


def graph_vals(g, kind):
    """The graph's values for a kind: |val| for the LayerGCN kinds (a normalised adjacency,
    which keeps |z| away from cancellation), signed otherwise."""
    return np.abs(g.val) if kind in (LAYERGCN, LAYERGCN_BWD) else g.val


def reg_counts(n, rng, tagged=None, big_off_tag=False):
    """Occurrence counts [3 n + 4] int32 with the three scales behind them, as the fused BPR
    leaves them; with big_off_tag the untagged rows hold large counts nothing may read."""
    cnt = rng.integers(0, 4, size=(n, 3)).astype(np.int32)
    if tagged is not None:
        cnt[~tagged] = 1_000_000 if big_off_tag else 0
    return np.concatenate([cnt.reshape(-1), np.zeros(4, dtype=np.int32)])


REG_K = np.asarray([1e-3, 2e-3, -1.5e-3], dtype=F32)


def tag_rows(g, n_tags, seed=21, share=0.4):
    """About 40 % of `n_tags` rows tagged (bool); every other hub of `g` tagged, the rest not."""
    rng = np.random.default_rng(seed)
    tagged = rng.random(n_tags) < share
    hubs = g.marks.get("hubs")
    if hubs is not None:
        tagged[hubs[0::2]] = True
        tagged[hubs[1::2]] = False
    return tagged


def poison_untagged(o, x, tagged, flags, kind, x_tagged=None):
    """NaN in every row a tag flag promises is never loaded: x rows under SPARSE_X (numbered
    by x_tagged when given), s_in rows under SPARSE_S, r_add rows under SPARSE_R."""
    n = next(v.shape[0] for k, v in o.items() if k in ("y", "f", "p"))
    if flags & TAG_SPARSE_X:
        xt = tagged if x_tagged is None else x_tagged
        x[~xt[:x.shape[0]]] = np.nan
    for name, flag in (("s_in", TAG_SPARSE_S), ("r_add", TAG_SPARSE_R)):
        if flags & flag and o.get(name) is not None and kind not in (LAYERGCN, LAYERGCN_BWD):
            o[name][~tagged[:n]] = np.nan
