"""The plugin API models implement — same surface as the reference's
AbstractRecommender / GeneralRecommender (src/common/abstract_recommender.py:10-103).

A model is constructed as `Cls(config, dataloader)`; the trainer calls
`parameters()`, `train()/eval()`, `pre_epoch_processing()`,
`post_epoch_processing()`, `calculate_loss(interaction)` and
`full_sort_predict([users, mask])`.  rsx models add two optional fast paths the
rsx Trainer uses when present:

* `fused_step(interaction, lr)` — the whole batch (forward, loss, backward,
  Adam) on the device, loss accumulated on the device (no host sync);
* `full_sort_topk(batch, k, eval_data)` — scores, train-item mask and top-k
  fused in one kernel, never materialising the score matrix.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn

from . import ops


class AbstractRecommender(nn.Module):
    supports_fused_step = False

    def pre_epoch_processing(self):
        pass

    def post_epoch_processing(self):
        pass

    def calculate_loss(self, interaction):
        raise NotImplementedError

    def predict(self, interaction):
        raise NotImplementedError

    def full_sort_predict(self, interaction):
        raise NotImplementedError

    def __str__(self):
        n = sum(int(np.prod(p.size())) for p in self.parameters())
        return super().__str__() + f"\nTrainable parameters: {n}"


class GeneralRecommender(AbstractRecommender):
    def __init__(self, config, dataloader):
        super().__init__()
        self.USER_ID = config["USER_ID_FIELD"]
        self.ITEM_ID = config["ITEM_ID_FIELD"]
        self.NEG_ITEM_ID = (config["NEG_PREFIX"] or "neg__") + str(self.ITEM_ID)
        self.n_users = dataloader.dataset.get_user_num()
        self.n_items = dataloader.dataset.get_item_num()
        self.batch_size = config["train_batch_size"]
        self.device = config["device"]
        self.v_feat, self.t_feat = None, None
        if not config["end2end"] and config["is_multimodal_model"]:
            root = os.path.abspath((config["data_path"] or "") + config["dataset"])
            vf = os.path.join(root, config["vision_feature_file"] or "")
            tf = os.path.join(root, config["text_feature_file"] or "")
            if os.path.isfile(vf):
                self.v_feat = torch.from_numpy(np.load(vf)).type(torch.FloatTensor).to(self.device)
            if os.path.isfile(tf):
                self.t_feat = torch.from_numpy(np.load(tf)).type(torch.FloatTensor).to(self.device)
            assert self.v_feat is not None or self.t_feat is not None, "Features all NONE"

    def require_features(self, unsupported, need: int = 1, vision: str = "image") -> None:
        """The feature-table checks of the multimodal HIP models, refused with the model's own
        `unsupported(what)`: fewer tables than the `need` (0, 1 or 2) its forward takes, or a
        width that is no multiple of 4 (the projection kernels read float4 rows)."""
        if need == 1 and self.v_feat is None and self.t_feat is None:
            raise unsupported("no feature file at all")
        for name, f in ((vision, self.v_feat), ("text", self.t_feat)):
            if f is None and need == 2:
                raise unsupported(f"no {name} feature file: {type(self).__name__}'s forward needs both modalities")
            if f is not None and f.shape[1] % 4:
                raise unsupported(f"{name} feature width {f.shape[1]} is not a multiple of 4")


class EvalTables:
    """Full-sort evaluation on the eval-mode (user table, item table), computed once per
    eval() session and kept in `_eval_cache` until train() (a mixin in front of
    GeneralRecommender)."""
    _eval_cache = None

    def _eval_tables(self):
        with torch.no_grad():
            u, i = self.forward(self.norm_adj_csr)
        return u.contiguous(), i.contiguous()

    def _cached_eval_tables(self):
        if self._eval_cache is None:
            self._eval_cache = self._eval_tables()
        return self._eval_cache

    def full_sort_predict(self, interaction):
        u, i = self._cached_eval_tables()
        return ops.score_dense(u, interaction[0].contiguous(), i)

    def full_sort_topk(self, interaction, k, eval_data):
        u, i = self._cached_eval_tables()
        return ops.fullsort_topk(u, interaction[0].contiguous(), i, eval_data.mask_rowptr, eval_data.mask_col, k)

    def train(self, mode: bool = True):
        self._eval_cache = None
        return super().train(mode)
