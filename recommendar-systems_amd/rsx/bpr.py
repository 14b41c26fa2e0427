"""BPR on the rsx HIP path — drop-in for the reference's models/bpr.py.

Same class name, constructor `(config, dataloader)`, YAML keys (embedding_size,
reg_weight), parameter names (user_embedding.weight, item_embedding.weight),
initialisation and loss (reference src/models/bpr.py:20-95).  The two parameters are
views of the tables an rsx.mf.MFEngine owns, so the autograd path (`calculate_loss`
with any torch optimiser) and the fused path (`fused_step`: one `rsx_mf_step` call per
batch) update the same storage.  There is no torch fallback: a configuration the HIP
path does not cover is refused at construction with RSX_ERR_UNSUPPORTED.
"""
from __future__ import annotations

import numpy as np
import torch.nn as nn

from .mf import MFEngine, MFRecommenderMixin, bpr_init
from .recommender import GeneralRecommender


class BPR(MFRecommenderMixin, GeneralRecommender):
    def __init__(self, config, dataloader):
        self.check_config(config)
        super().__init__(config, dataloader)
        self.embedding_size = config["embedding_size"]
        self.reg_weight = config["reg_weight"]
        u0, i0 = bpr_init(self.n_users, self.n_items, self.embedding_size)  # the reference's draws
        im = dataloader.inter_matrix(form="coo")
        self.engine = MFEngine(im.row.astype(np.int64), im.col.astype(np.int64), self.n_users, self.n_items,
                               self.embedding_size, self.reg_weight, lr=config["learning_rate"] or 1e-3,
                               device=self.device, user_emb=u0.numpy(), item_emb=i0.numpy(),
                               seed=int(config["seed"] or 0), batch=int(config["train_batch_size"]),
                               weight_decay=float(config["weight_decay"] or 0.0))
        self.user_embedding = nn.Embedding(self.n_users, self.embedding_size, _weight=self.engine.U)
        self.item_embedding = nn.Embedding(self.n_items, self.embedding_size, _weight=self.engine.I)

    def _engine_params(self):
        return self.user_embedding.weight, self.item_embedding.weight

    def get_user_embedding(self, user):
        return self.user_embedding.weight[user]

    def get_item_embedding(self, item):
        return self.item_embedding.weight[item]

    def forward(self):
        return self.user_embedding.weight, self.item_embedding.weight
