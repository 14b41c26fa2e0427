"""Device-resident engine of the matrix-factorisation models (BPR, VBPR): every tensor in
HBM, one C-ABI call per batch (`rsx_mf_step`, csrc/mf.hip).

Holds the user table U [n_users, du], the item table I [n_items, d] and, with raw item
features X [n_items, F] (VBPR, reference src/models/vbpr.py:31-40), the projection
W [d, F], b [d]; each with its Adam moments, plus the gradient scratch, the triplet
buffer, a DeviceSampler, the f64 epoch-loss accumulator, the NaN halt flag and the
step count.  du = d without features (BPR, src/models/bpr.py:32-33) and 2 d with them.
Same surface as rsx.engine.LightGCNEngine: `step`, `set_lr`, `invalidate`, `loss_out`.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import ops

SUPPORTED_D = (32, 64, 128)


def unsupported(what: str) -> RuntimeError:
    return RuntimeError(f"RSX_ERR_UNSUPPORTED: {what} (the matrix-factorisation models run on the HIP path only)")


def bpr_init(n_users: int, n_items: int, d: int):
    """BPR's initial (user, item) tables: the reference's torch calls in its order on the
    CPU generator (bpr.py:32-38): the two nn.Embedding constructors' own normal_ draws,
    then xavier_normal_ on each weight (init.py:19-20, Module.apply visits them in order)."""
    ue = torch.nn.Embedding(n_users, d)
    ie = torch.nn.Embedding(n_items, d)
    torch.nn.init.xavier_normal_(ue.weight.data)
    torch.nn.init.xavier_normal_(ie.weight.data)
    return ue.weight.data, ie.weight.data


def vbpr_init(n_users: int, n_items: int, d: int, F: int):
    """VBPR's initial (u_embedding, i_embedding, item_linear.weight, item_linear.bias)
    (vbpr.py:31-45): two xavier_uniform_ tables, nn.Linear's own kaiming / bias draws,
    then xavier_normal_ on the Linear's weight and a zero bias (init.py:21-24; the bare
    Parameters are no modules, so they keep their xavier_uniform_ draws)."""
    u0 = torch.nn.init.xavier_uniform_(torch.empty(n_users, d * 2))
    i0 = torch.nn.init.xavier_uniform_(torch.empty(n_items, d))
    lin = torch.nn.Linear(F, d)
    torch.nn.init.xavier_normal_(lin.weight.data)
    torch.nn.init.constant_(lin.bias.data, 0)
    return u0, i0, lin.weight.data, lin.bias.data


class MFEngine:
    def __init__(self, train_u: np.ndarray, train_i: np.ndarray, n_users: int, n_items: int, dim: int, reg: float,
                 lr: float, device, user_emb: np.ndarray, item_emb: np.ndarray, W: np.ndarray | None = None,
                 b: np.ndarray | None = None, features: torch.Tensor | np.ndarray | None = None, seed: int = 0,
                 batch: int = 2048, weight_decay: float = 0.0):
        self.device = dev = ops.require_device(device)
        self.n_users, self.n_items, self.d = int(n_users), int(n_items), int(dim)
        self.reg, self.lr, self.wd = float(reg), float(lr), float(weight_decay)
        if self.d not in SUPPORTED_D:
            raise unsupported(f"embedding_size {self.d} not in {SUPPORTED_D}")
        self.F = 0 if features is None else int(features.shape[1])
        if self.F % 4:
            raise unsupported(f"feature width {self.F} is not a multiple of 4")
        self.du = 2 * self.d if self.F else self.d
        f32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).contiguous().to(dev)  # noqa: E731
        self.U, self.I = f32(user_emb), f32(item_emb)
        if tuple(self.U.shape) != (self.n_users, self.du) or tuple(self.I.shape) != (self.n_items, self.d):
            raise ValueError("user / item table shapes do not match (n_users, du) / (n_items, d)")
        self.X = self.W = self.b = None
        if self.F:
            self.X = (features if torch.is_tensor(features) else torch.from_numpy(np.asarray(features)))
            self.X = self.X.to(device=dev, dtype=torch.float32).contiguous()
            self.W, self.b = f32(W), f32(b)
        self.params = [t for t in (self.U, self.I, self.W, self.b) if t is not None]
        self.m = [torch.zeros_like(t) for t in self.params]
        self.v = [torch.zeros_like(t) for t in self.params]
        self.g = [torch.zeros_like(t) for t in self.params]  # gU, gI: zero between steps
        self.loss_out = torch.zeros(1, dtype=torch.float32, device=dev)
        self.loss_acc = torch.zeros(1, dtype=torch.float64, device=dev)
        self.halt = torch.zeros(2, dtype=torch.int32, device=dev)
        self.step_count = 0
        # the step count on the device: rsx_mf_step advances it and its Adam reads it, so a
        # step captured into a graph advances on every replay (step_count is the host's
        # mirror: the halt tag; `sync_step_count` after replays)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self.batch = int(batch)
        self.ws = torch.empty(L.lib().rsx_mf_ws_bytes(max(self.batch, 1), self.d, self.F), dtype=torch.uint8,
                              device=dev)
        self.sampler = ops.DeviceSampler(np.asarray(train_u), np.asarray(train_i), self.n_users, dev, seed=seed)
        self.n_inter = self.sampler.n_inter
        self.epoch_trip = torch.zeros(3 * self.n_inter, dtype=torch.int64, device=dev)
        self._epoch_sampled = None
        self._trip = None  # step_draw's triplet buffer
        self._table = None if not self.F else torch.zeros(self.n_items, self.du, dtype=torch.float32, device=dev)
        self._table_valid = False
        self._table_versions = None
        self._st = self._struct(self.g, self.loss_acc, self.halt, self.loss_out)
        # the autograd path: its own loss word, no epoch accumulator, no halt (rsx_mf_loss_grad)
        self.grad_loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self._sg = self._struct(self.g, None, None, self.grad_loss)

    def _struct(self, g, loss_acc, halt, loss_out) -> "L.MfStep":
        st = L.MfStep()
        st.n_users, st.n_items, st.d, st.F, st.reg = self.n_users, self.n_items, self.d, self.F, self.reg
        names = ("U", "I", "W", "b")
        for k, t in enumerate(self.params):
            n = names[k]
            setattr(st, n, t.data_ptr())
            setattr(st, "m" + n, self.m[k].data_ptr())
            setattr(st, "v" + n, self.v[k].data_ptr())
            setattr(st, "g" + n, g[k].data_ptr())
        st.X = self.X.data_ptr() if self.F else None
        st.loss_out = loss_out.data_ptr()
        st.loss_acc = loss_acc.data_ptr() if loss_acc is not None else None
        st.halt = halt.data_ptr() if halt is not None else None
        st.ws, st.ws_bytes = self.ws.data_ptr(), self.ws.numel()
        st.sample = None
        st.step_dev = self.step_dev.data_ptr() if halt is not None else None
        return st

    def sync_step_count(self) -> int:
        """Adopt the device step counter (after graph replays of a captured step)."""
        self.step_count = int(self.step_dev.item())
        return self.step_count

    def set_lr(self, lr: float):
        self.lr = float(lr)

    def invalidate(self):
        self._table_valid = False

    def _bind(self, st, triplets: torch.Tensor):
        t = triplets[:3]
        if t.dtype != torch.int64 or not t.is_cuda:
            raise RuntimeError("triplets must be an int64 [3, B] tensor on the GPU")
        t = t.contiguous()
        if t.shape[1] > self.batch:
            raise RuntimeError("batch larger than the engine's batch size")
        self._keep = t
        st.triplets, st.batch = t.data_ptr(), t.shape[1]

    def step(self, triplets: torch.Tensor | None = None, epoch: int = 0, start: int = 0) -> None:
        """One batch: given `triplets` (int64 [3, B] on the device), or the device sampler's
        batch at position `start` of `epoch` (one sampling launch per epoch)."""
        st = self._st
        if triplets is None:
            if self._epoch_sampled != epoch:
                self.sampler.sample_epoch(epoch, self.batch, out=self.epoch_trip)
                self._epoch_sampled = epoch
            if start % self.batch:
                raise RuntimeError("start must be a multiple of the batch size")
            triplets = ops.DeviceSampler.batch_view(self.epoch_trip, self.n_inter, self.batch, start // self.batch)
        self._bind(st, triplets)
        st.sample = None
        self._launch(st)

    def step_draw(self, epoch: int, start: int) -> torch.Tensor:
        """One batch whose triplets rsx_mf_step draws itself (`sample` of its arguments: the
        per-batch form of the device sampler, no epoch buffer): epoch positions [start,
        start + batch), fewer at the end of the epoch.  Returns the [3, count] triplets."""
        st = self._st
        if self._trip is None:
            self._trip = torch.zeros(3 * self.batch, dtype=torch.int64, device=self.device)
        self._sa = self.sampler.args(epoch, start)
        st.sample = C.pointer(self._sa)
        st.triplets, st.batch = self._trip.data_ptr(), self.batch
        self._launch(st)
        st.sample = None
        count = min(self.batch, self.n_inter - start)
        return self._trip[: 3 * count].view(3, count)

    def _launch(self, st):
        self.step_count += 1
        st.adam = ops.adam_struct(self.lr, self.step_count, weight_decay=self.wd)
        st.tag = self.step_count
        L.check(L.lib().rsx_mf_step(C.byref(st), ops._stream()), "rsx_mf_step")
        self._table_valid = False

    def loss_grad(self, triplets: torch.Tensor):
        """(loss [1], [gU, gI(, gW, gb)]) of one batch, fresh tensors (rsx_mf_loss_grad)."""
        st = self._sg
        self._bind(st, triplets)
        g = [torch.empty_like(t) for t in self.params]
        p = [ops._p(t) for t in g] + [None] * (4 - len(g))
        L.check(L.lib().rsx_mf_loss_grad(C.byref(st), *p, ops._stream()), "rsx_mf_loss_grad")
        return self.grad_loss.clone(), g

    def item_table(self) -> torch.Tensor:
        """[n_items, du] item rows for evaluation: I, and with features [I , X W^T + b]
        (reference vbpr.py:70-71), the right half by one dense rsx_linear_rows_fwd;
        recomputed only after the parameters changed: after a step of this engine, an
        `invalidate()`, or an in-place torch update of I, W or b (an optimiser on the
        autograd path), which the tensors' version counters show."""
        if not self.F:
            return self.I
        versions = tuple(t._version for t in (self.I, self.W, self.b))
        if not self._table_valid or versions != self._table_versions:
            self._table_versions = versions
            self._table[:, : self.d].copy_(self.I)
            right = self._table[:, self.d:]
            L.check(L.lib().rsx_linear_rows_fwd(ops._p(self.X), ops._p(self.W), ops._p(self.b), None, self.n_items,
                                                self.F, self.d, C.c_void_p(right.data_ptr()), self.du,
                                                ops._stream()), "rsx_linear_rows_fwd")
            self._table_valid = True
        return self._table


class MFLoss(torch.autograd.Function):
    """BPR / VBPR batch loss; the kernel produces the gradients with the loss."""

    @staticmethod
    def forward(ctx, engine, triplets, *params):
        loss, g = engine.loss_grad(triplets)
        ctx.save_for_backward(*g)
        return loss[0]

    @staticmethod
    def backward(ctx, go):
        return (None, None, *(go * g for g in ctx.saved_tensors))


class MFRecommenderMixin:
    """What BPR and VBPR share above the engine (reference src/models/bpr.py:67-95,
    vbpr.py:77-106): the autograd loss, the fused step, scoring and top-k."""

    supports_fused_step = True

    @staticmethod
    def check_config(config):
        ops.require_single_gpu(config, unsupported)
        if config["embedding_size"] not in SUPPORTED_D:
            raise unsupported(f"embedding_size {config['embedding_size']} not in {SUPPORTED_D}")

    def _engine_params(self):
        raise NotImplementedError

    def train(self, mode: bool = True):
        self.engine.invalidate()
        return super().train(mode)

    def calculate_loss(self, interaction):
        self.engine.invalidate()
        return MFLoss.apply(self.engine, interaction[:3], *self._engine_params())

    def fused_step(self, interaction, lr: float):
        self.engine.set_lr(lr)
        self.engine.step(triplets=interaction)

    def full_sort_predict(self, interaction):
        with torch.no_grad():
            return ops.score_dense(self.engine.U, interaction[0].contiguous(), self.engine.item_table())

    def full_sort_topk(self, interaction, k: int, eval_data):
        with torch.no_grad():
            return ops.fullsort_topk(self.engine.U, interaction[0].contiguous(), self.engine.item_table(),
                                     eval_data.mask_rowptr, eval_data.mask_col, k)

    @property
    def device_loss_acc(self):
        return self.engine.loss_acc

    @property
    def device_halt(self):
        """(halt flag [2] int32 on the device, engine step count): {1, step} once a batch
        loss was NaN; the parameters stay those of the last finite step."""
        return self.engine.halt, self.engine.step_count
