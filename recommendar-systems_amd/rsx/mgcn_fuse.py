"""MGCN's per-row blocks on the fused HIP kernels (csrc/mgcn.hip), with autograd.

* `purify`    — item * sigmoid(gate_x(feats_x)), x = image, text (mgcn.py:152-154)
* `fuse`      — the behaviour-aware fuser over every [users; items] row (mgcn.py:187-201)
* `fuse_rows` — the same block on the batch rows only: compact (all, side, content) rows
                out, whole-table gradients back (repeated rows summed in a fixed order)

One forward and one backward launch each; the Linear weight gradients come from
rsx_smore_wgrad on the pre-activation gradient rows (one launch pair a block), the
[1, d] second query weight's from the backward's own ordered reduction.  f32 throughout.
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import ops
from .dense import _wgrad
from .smore_fuse import _c, supported  # noqa: F401 - `supported` is this module's too

_p, _arr = ops._p, ops._arr


class _Purify(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fv, ft, item, Wv, bv, Wt, bt):
        feat = [_c(fv), _c(ft)]
        W, b = [_c(Wv), _c(Wt)], [_c(bv), _c(bt)]
        item = _c(item)
        n, d = item.shape
        outs = [torch.empty_like(item) for _ in range(2)]
        L.check(L.lib().rsx_mgcn_purify(0, _arr(feat), _p(item), _arr(W), _arr(b), n, d, _arr(outs), None, None, None,
                                        None, ops._stream()), "rsx_mgcn_purify")
        ctx.save_for_backward(*feat, item, *W, *b)
        return tuple(outs)

    @staticmethod
    def backward(ctx, gv, gt):
        fv, ft, item, Wv, Wt, bv, bt = ctx.saved_tensors
        n, d = item.shape
        gi = torch.empty_like(item)
        gf = [torch.empty_like(item) for _ in range(2)]
        dz = [torch.empty_like(item) for _ in range(2)]
        gouts = [None if g is None else _c(g) for g in (gv, gt)]
        L.check(L.lib().rsx_mgcn_purify(1, _arr([fv, ft]), _p(item), _arr([Wv, Wt]), _arr([bv, bt]), n, d, None,
                                        _arr(gouts), _p(gi), _arr(gf), _arr(dz), ops._stream()), "rsx_mgcn_purify")
        (gWv, gbv), (gWt, gbt) = _wgrad([(dz[0], fv, True), (dz[1], ft, True)], d, item.device)
        return gf[0], gf[1], gi, gWv, gbv, gWt, gbt


def purify(image_feats, text_feats, item, gate_v, gate_t):
    """(image_item_embeds, text_item_embeds) = item * sigmoid(gate_x(feats_x)); gate_x are
    the reference's nn.Sequential(Linear, Sigmoid) modules."""
    lv, lt = gate_v[0], gate_t[0]
    return _Purify.apply(image_feats, text_feats, item, lv.weight, lv.bias, lt.weight, lt.bias)


def _fuse_call(backward, W, b, C_, I_, T_, rows, n, outs, gins, gouts, dz, dif, dw2, ws):
    d = C_.shape[1]
    L.check(L.lib().rsx_mgcn_fuse(backward, _arr(W), _arr(b), _p(C_), _p(I_), _p(T_), _p(rows), n, C_.shape[0], d,
                                  *[_p(t) for t in outs], *[_p(t) for t in gins], *[_p(t) for t in gouts],
                                  _arr(dz) if dz is not None else None, _p(dif), _p(dw2), _p(ws),
                                  ws.numel() if ws is not None else 0, ops._stream()), "rsx_mgcn_fuse")


class _Fuse(torch.autograd.Function):
    """rows = None: the full form (outputs [N, d], g_content_in unused); else the rows form
    (compact outputs, the third one the gathered content rows)."""

    @staticmethod
    def forward(ctx, C_, I_, T_, rows, W1, b1, w2, Wip, bip, Wtp, btp):
        C_, I_, T_ = _c(C_), _c(I_), _c(T_)
        W = [_c(W1), _c(w2), _c(Wip), _c(Wtp)]
        b = [_c(b1), None, _c(bip), _c(btp)]
        d = C_.shape[1]
        if rows is None:
            n = C_.shape[0]
            all_, side = torch.empty_like(C_), torch.empty_like(C_)
            c_rows, t_rows = C_, T_
            _fuse_call(0, W, b, C_, I_, T_, None, n, (all_, side, None, None), (None,) * 3, (None,) * 3, None, None,
                       None, None)
        else:
            rows = _c(rows)
            n = rows.numel()
            out = torch.empty(4, n, d, dtype=torch.float32, device=C_.device)
            all_, side, c_rows, t_rows = out.unbind(0)
            _fuse_call(0, W, b, C_, I_, T_, rows, n, (all_, side, c_rows, t_rows), (None,) * 3, (None,) * 3, None, None,
                       None, None)
        ctx.has_rows = rows is not None
        ctx.save_for_backward(C_, I_, T_, rows if rows is not None else torch.empty(0), c_rows, t_rows, *W,
                              b[0], b[2], b[3])
        if rows is None:
            return all_, side
        return all_, side, c_rows

    @staticmethod
    def backward(ctx, g_all, g_side, g_crows=None):
        C_, I_, T_, rows, c_rows, t_rows, W1, w2, Wip, Wtp, b1, bip, btp = ctx.saved_tensors
        rows = rows if ctx.has_rows else None
        n = rows.numel() if rows is not None else C_.shape[0]
        d = C_.shape[1]
        dev = C_.device
        if g_all is None:
            g_all = torch.zeros(n, d, dtype=torch.float32, device=dev)
        g_all = _c(g_all)
        g_side = None if g_side is None else _c(g_side)
        g_crows = None if g_crows is None else _c(g_crows)
        gtab = torch.empty(3, *C_.shape, dtype=torch.float32, device=dev)
        *dz, dif = torch.empty(5, n, d, dtype=torch.float32, device=dev).unbind(0)
        dw2 = torch.empty_like(w2)
        ws = torch.empty(max(int(L.lib().rsx_mgcn_fuse_ws_bytes(n, C_.shape[0], d, int(rows is not None))), 4), dtype=torch.uint8,
                         device=dev)
        _fuse_call(1, [W1, w2, Wip, Wtp], [b1, None, bip, btp], C_, I_, T_, rows, n, (None,) * 4,
                   (g_all, g_side, g_crows), tuple(gtab.unbind(0)), dz, dif, dw2, ws)
        # query_common.0 runs on the image and on the text rows; their two row sets nearly
        # cancel where the views agree, so the kernel writes them as dz1I on I - T and
        # dz1I + dz1T on T (rsx.h): dW1 is the two products' sum, db1 the second's column sum
        (gWa, _), (gWb, gb1), (gWip, gbip), (gWtp, gbtp) = _wgrad(
            [(dz[0], dif, False), (dz[1], t_rows, True), (dz[2], c_rows, True), (dz[3], c_rows, True)], d, dev)
        return gtab[0], gtab[1], gtab[2], None, gWa + gWb, gb1, dw2, gWip, gbip, gWtp, gbtp


def _weights(m):
    q0, q2 = m.query_common[0], m.query_common[2]
    ip, tp = m.gate_image_prefer[0], m.gate_text_prefer[0]
    return q0.weight, q0.bias, q2.weight, ip.weight, ip.bias, tp.weight, tp.bias


def fuse(model, content, image_embeds, text_embeds):
    """(all_embeds, side_embeds) of the reference's fuser over every row."""
    return _Fuse.apply(content, image_embeds, text_embeds, None, *_weights(model))


def fuse_rows(model, content, image_embeds, text_embeds, rows):
    """(all, side, content) rows of the fuser at table rows `rows` (int64 [n], may repeat)."""
    return _Fuse.apply(content, image_embeds, text_embeds, rows, *_weights(model))
