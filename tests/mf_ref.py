"""CPU restatement of the two matrix-factorisation models, BPR and VBPR, with torch ops and
torch.optim.Adam (what the reference's models compute: bpr.py:67-87, vbpr.py:69-98,
loss.py:33-51, trainer.py:133,238), runnable in f32 and f64.  The GPU tests compare the HIP
path with it; tests/test_mf_cpu.py compares it with the reference's own outputs in
tests/golden/{bpr,vbpr}_small.npz."""
from __future__ import annotations

import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = {"BPR": ("user_embedding.weight", "item_embedding.weight"),
         "VBPR": ("u_embedding", "i_embedding", "item_linear.weight", "item_linear.bias")}
FIXTURE = {"BPR": ("bpr_small", 3), "VBPR": ("vbpr_small", 2)}  # (file, epochs)
_CACHE = {}


def load_fixture(model: str) -> dict:
    """The model's fixture, with `step0_param.*` rebuilt from its stored XOR against `init.*`
    (tools/capture_golden.py capture_mf keeps the file under 1 MiB that way; bit-exact)."""
    if model not in _CACHE:
        z = dict(np.load(os.path.join(GOLDEN, FIXTURE[model][0] + ".npz")))
        for k in [k for k in z if k.startswith("step0_param_xor.")]:
            name = k[len("step0_param_xor."):]
            z["step0_param." + name] = (z.pop(k) ^ z["init." + name].view(np.int32)).view(np.float32)
        _CACHE[model] = z
    return _CACHE[model]


def features(z) -> np.ndarray | None:
    """cat(t_feat, v_feat) as reference vbpr.py:33-34, or None (BPR)."""
    if "v_feat" not in z:
        return None
    return np.concatenate([z["t_feat"], z["v_feat"]], axis=1)


def fixture_params(z, model: str, prefix: str):
    return [z[prefix + n] for n in NAMES[model]]


def epoch_batches(z, epoch: int, batch: int = 512):
    t = z[f"epoch{epoch}_triplets"].astype(np.int64)
    return [torch.from_numpy(np.ascontiguousarray(t[:, a: a + batch])) for a in range(0, t.shape[1], batch)]


class MFRef:
    """params: [U, I] (BPR) or [U, I, W, b] with the fixed features X (VBPR)."""

    def __init__(self, params, reg: float, X=None, lr: float = 1e-3, dtype=torch.float32, weight_decay: float = 0.0):
        self.p = [torch.tensor(np.asarray(a), dtype=dtype).requires_grad_(True) for a in params]
        self.X = None if X is None else torch.tensor(np.asarray(X), dtype=dtype)
        self.reg = reg
        self.opt = torch.optim.Adam(self.p, lr=lr, weight_decay=weight_decay)

    def item_table(self):
        if self.X is None:
            return self.p[1]
        return torch.cat((self.p[1], torch.nn.functional.linear(self.X, self.p[2], self.p[3])), -1)

    def loss(self, trip):
        trip = torch.as_tensor(trip)
        items = self.item_table()
        u, p, n = self.p[0][trip[0]], items[trip[1]], items[trip[2]]
        ps, ns = torch.mul(u, p).sum(dim=1), torch.mul(u, n).sum(dim=1)
        mf = -torch.log(1e-10 + torch.sigmoid(ps - ns)).mean()
        emb = (torch.norm(u, p=2) + torch.norm(p, p=2) + torch.norm(n, p=2)) / u.shape[0]
        return mf + self.reg * emb

    def loss_grad(self, trip):
        for t in self.p:
            t.grad = None
        loss = self.loss(trip)
        loss.backward()
        return loss.item(), [t.grad.detach().clone() if t.grad is not None else torch.zeros_like(t) for t in self.p]

    def step(self, trip, lr: float | None = None) -> float:
        if lr is not None:
            for g in self.opt.param_groups:
                g["lr"] = lr
        self.opt.zero_grad()
        loss = self.loss(trip)
        loss.backward()
        self.opt.step()
        return loss.item()

    def numpy(self):
        return [t.detach().numpy() for t in self.p]

    def scores(self, users):
        with torch.no_grad():
            return (self.p[0][torch.as_tensor(users)] @ self.item_table().t()).numpy()
