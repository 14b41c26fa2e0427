"""VBPR on the rsx HIP path — drop-in for the reference's models/vbpr.py.

Same class name, constructor `(config, dataloader)`, YAML keys (embedding_size,
reg_weight), parameter names (u_embedding, i_embedding, item_linear.weight,
item_linear.bias), initialisation and loss (reference src/models/vbpr.py:20-106).  The
raw item features are cat(t_feat, v_feat), or the one set that exists (:33-38).  The
reference projects every item's features on every step (:70); here a training batch
projects its own 2 B item rows (`rsx_linear_rows_fwd`) and evaluation projects the whole
table once per parameter change (rsx.mf.MFEngine.item_table).  All parameters are views
of the engine's buffers; no torch fallback (RSX_ERR_UNSUPPORTED at construction).
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn

from .mf import MFEngine, MFRecommenderMixin, unsupported, vbpr_init
from .recommender import GeneralRecommender


class VBPR(MFRecommenderMixin, GeneralRecommender):
    def __init__(self, config, dataloader):
        self.check_config(config)
        # the feature files GeneralRecommender is about to load (recommender.py: same paths)
        root = os.path.abspath((config["data_path"] or "") + config["dataset"])
        files = [os.path.join(root, config[k] or "") for k in ("vision_feature_file", "text_feature_file")]
        if config["end2end"] or not config["is_multimodal_model"] or not any(os.path.isfile(f) for f in files):
            raise unsupported("VBPR needs a vision or text feature file (is_multimodal_model: True, "
                              f"one of {files})")
        super().__init__(config, dataloader)
        self.u_embedding_size = self.i_embedding_size = d = config["embedding_size"]
        self.reg_weight = config["reg_weight"]
        if self.v_feat is not None and self.t_feat is not None:
            self.item_raw_features = torch.cat((self.t_feat, self.v_feat), -1)
        else:
            self.item_raw_features = self.v_feat if self.v_feat is not None else self.t_feat
        F = int(self.item_raw_features.shape[1])
        if F % 4:
            raise unsupported(f"feature width {F} is not a multiple of 4")
        u0, i0, w0, b0 = vbpr_init(self.n_users, self.n_items, d, F)  # the reference's draws
        im = dataloader.inter_matrix(form="coo")
        self.engine = MFEngine(im.row.astype(np.int64), im.col.astype(np.int64), self.n_users, self.n_items, d,
                               self.reg_weight, lr=config["learning_rate"] or 1e-3, device=self.device,
                               user_emb=u0.numpy(), item_emb=i0.numpy(), W=w0.numpy(),
                               b=b0.numpy(), features=self.item_raw_features,
                               seed=int(config["seed"] or 0), batch=int(config["train_batch_size"]),
                               weight_decay=float(config["weight_decay"] or 0.0))
        self.u_embedding = nn.Parameter(self.engine.U)
        self.i_embedding = nn.Parameter(self.engine.I)
        self.item_linear = nn.Module()  # the parameter names of the reference's nn.Linear
        self.item_linear.weight = nn.Parameter(self.engine.W)
        self.item_linear.bias = nn.Parameter(self.engine.b)

    def _engine_params(self):
        return self.u_embedding, self.i_embedding, self.item_linear.weight, self.item_linear.bias

    def get_user_embedding(self, user):
        return self.u_embedding[user, :]

    def forward(self):
        """(user table, [i_embedding , item_linear(features)]) as reference vbpr.py:69-75."""
        with torch.no_grad():
            self.engine.invalidate()
            return self.u_embedding, self.engine.item_table()
