"""MGCN on the rsx HIP path — drop-in for the reference's models/mgcn.py (ACM MM'23), the
model SMORE was derived from: SMORE without the spectral block and the fusion view.

Same class name, constructor `(config, dataloader)`, YAML keys, module names and creation
order (reference src/models/mgcn.py:22-104, so `init_seed` gives the reference's initial
weights), forward, loss and scoring (:146-263):

* the SMORE-normalised user-item graph (rsx_adj_build, ADJ_SMORE), its user block R and
  the two kNN item graphs (one knn_k; rsx.blocks' builders and caches);
* the feature projections over the whole tables: rsx_linear_rows_fwd / rsx_linear_bwd;
* the behaviour-guided purifier and the behaviour-aware fuser: rsx.mgcn_fuse
  (csrc/mgcn.hip);
* the UI backbone (`rsx.blocks.ui_backbone`) and the item views (`SF.view_prop`);
* BPR + InfoNCE on the batch rows: `SF.smore_loss_rows` with the temperature 0.2 of
  mgcn.py:250 (`self.tau` is unused there and here);
* evaluation: the fused full-sort on the cached eval-mode tables.

One GPU, sparse item graphs, both modalities, embedding_size 64 / 128; anything else raises
RSX_ERR_UNSUPPORTED at construction (no torch fallback).
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import mgcn_fuse as MF
from . import ops
from . import smore_fuse as SF
from .blocks import _BatchIndex, _DevGraph, _ego, _join_tables, _RowsOff, cached_knn, ui_backbone
from .dense import _Project
from .lightgcn import _BprLoss
from .nn import RsxLinear
from .recommender import EvalTables, GeneralRecommender

CL_TEMPERATURE = 0.2  # mgcn.py:250-251


def unsupported(what: str) -> RuntimeError:
    return RuntimeError(f"RSX_ERR_UNSUPPORTED: {what} (MGCN runs on the HIP path only)")


class MGCN(EvalTables, GeneralRecommender):
    # a training batch has no host syncs; no per-epoch buffer rebuilds: the Trainer may
    # capture it in a HIP graph and keep the captured steps across epochs
    supports_graph_step = True
    graph_step_persistent = True

    @staticmethod
    def check_config(config):
        ops.require_single_gpu(config, unsupported)
        if not MF.supported(config["embedding_size"]):
            raise unsupported(f"embedding_size {config['embedding_size']} not in (64, 128)")
        if int(config["knn_k"]) > 32:
            raise unsupported(f"knn_k {config['knn_k']} > 32")

    def __init__(self, config, dataset):
        self.check_config(config)
        super().__init__(config, dataset)
        ops.require_device(self.device)
        self.require_features(unsupported, need=2)
        self.sparse = True
        self.cl_loss = config["cl_loss"]
        self.n_ui_layers = config["n_ui_layers"]
        self.embedding_dim = d = config["embedding_size"]
        self.knn_k = config["knn_k"]
        self.n_layers = config["n_layers"]
        self.reg_weight = config["reg_weight"]
        chunk = int(config["rsx_chunk"] or 32)
        kchunk = int(config["rsx_knn_chunk"] or 64)
        self.interaction_matrix = im = dataset.inter_matrix(form="coo").astype(np.float32)
        nu, ni = self.n_users, self.n_items
        # parameters in the reference's creation order (identical init under init_seed), drawn
        # on the CPU generator as the reference does
        self.user_embedding = nn.Embedding(nu, d)
        self.item_id_embedding = nn.Embedding(ni, d)
        nn.init.xavier_uniform_(self.user_embedding.weight)
        nn.init.xavier_uniform_(self.item_id_embedding.weight)
        _join_tables(self.user_embedding, self.item_id_embedding, self.device)
        # norm_adj and R (mgcn.py:45-47,109-136: SMORE's normalisation)
        drp, dcol, dval = ops.adj_build(im.row.astype(np.int64), im.col.astype(np.int64), nu, ni, ops.ADJ_SMORE,
                                        self.device)
        self.norm_adj_csr = ops.DeviceCSR.from_device(drp, dcol, dval, nu + ni, chunk)
        rp, col, val = self.norm_adj_csr.rowptr_host, dcol.cpu().numpy(), dval.cpu().numpy()
        e = int(rp[nu])
        rows = np.repeat(np.arange(nu), np.diff(rp[: nu + 1]))
        self.R = _DevGraph(rows, col[:e].astype(np.int64) - nu, val[:e], nu, ni, self.device, kchunk)
        # the kNN item graphs (mgcn.py:50-69), built and cached as SMORE's
        root = os.path.abspath((config["data_path"] or "") + (config["dataset"] or ""))
        self.knn_mode = config["rsx_knn"] or config["rsx_sampler"] or "device"
        if self.knn_mode not in ("device", "host"):
            raise ValueError(f"rsx_knn must be 'device' or 'host', got {self.knn_mode!r}")
        self.image_embedding = nn.Embedding.from_pretrained(self.v_feat.clone(), freeze=False)
        self.image_graph = _DevGraph(*cached_knn(root, "image", self.v_feat, self.knn_k, self.sparse, self.knn_mode,
                                                 self.device), ni, ni, self.device, kchunk)
        self.text_embedding = nn.Embedding.from_pretrained(self.t_feat.clone(), freeze=False)
        self.text_graph = _DevGraph(*cached_knn(root, "text", self.t_feat, self.knn_k, self.sparse, self.knn_mode,
                                                self.device), ni, ni, self.device, kchunk)
        self.image_trs = nn.Linear(self.v_feat.shape[1], d)
        self.text_trs = nn.Linear(self.t_feat.shape[1], d)
        self.softmax = nn.Softmax(dim=-1)
        self.query_common = nn.Sequential(RsxLinear(d, d), nn.Tanh(), RsxLinear(d, 1, bias=False))
        self.gate_v = nn.Sequential(RsxLinear(d, d), nn.Sigmoid())
        self.gate_t = nn.Sequential(RsxLinear(d, d), nn.Sigmoid())
        self.gate_image_prefer = nn.Sequential(RsxLinear(d, d), nn.Sigmoid())
        self.gate_text_prefer = nn.Sequential(RsxLinear(d, d), nn.Sigmoid())
        self.tau = 0.5  # as the reference: set, never read
        # training loss on the batch rows only (rsx_mgcn_batch_rows: False = full tables)
        flag = config.get("rsx_mgcn_batch_rows", True)
        self.batch_rows = bool(flag if flag is not None else True)
        self._bidx = _BatchIndex(self.device)
        self._rows_off = _RowsOff(self.n_users, self.device)
        self._tags = None
        self.to(self.device)

    # --------------------------------------------------------------- forward
    def _views(self, rows=None):
        """Everything before the fuser: (content, image_embeds, text_embeds) tables.  With
        `rows` (the batch rows) content is exact on those rows only."""
        item_id = self.item_id_embedding.weight
        image_feats = _Project.apply(self.image_embedding.weight, self.image_trs.weight, self.image_trs.bias)
        text_feats = _Project.apply(self.text_embedding.weight, self.text_trs.weight, self.text_trs.bias)
        img_i, txt_i = MF.purify(image_feats, text_feats, item_id, self.gate_v, self.gate_t)
        content = ui_backbone(self, _ego(self.user_embedding.weight, item_id), self.norm_adj_csr, self.n_ui_layers,
                              rows)
        image_embeds = SF.view_prop(img_i, self.image_graph, self.R, self.n_layers, self.n_users)
        text_embeds = SF.view_prop(txt_i, self.text_graph, self.R, self.n_layers, self.n_users)
        return content, image_embeds, text_embeds

    def _forward_all(self):
        content, image_embeds, text_embeds = self._views()
        all_embeds, side = MF.fuse(self, content, image_embeds, text_embeds)
        return all_embeds, side, content

    def forward(self, adj=None, train=False):
        """Reference signature: (users, items) or, with train=True, (users, items, side, content)."""
        all_embeds, side, content = self._forward_all()
        users, items = torch.split(all_embeds, [self.n_users, self.n_items], dim=0)
        if train:
            return users, items, side, content
        return users, items

    # ------------------------------------------------------------------ loss
    def calculate_loss(self, interaction):
        B = interaction.shape[1]
        if self.batch_rows:
            # the fuser is row-local and the loss reads all / side / content at the batch's
            # users, positives and negatives alone: its other rows are never computed
            ar, trip = self._bidx[B]
            rows = self._rows_off.rows(interaction[:3])
            content, image_embeds, text_embeds = self._views(rows)
            all_c, side_c, content_c = MF.fuse_rows(self, content, image_embeds, text_embeds, rows)
            total, _ = SF.smore_loss_rows(all_c, side_c, content_c, trip, ar, B, self.reg_weight, self.batch_size,
                                          self.cl_loss, CL_TEMPERATURE)
            return total
        users, pos = interaction[0], interaction[1]
        all_embeds, side, content = self._forward_all()
        bpr = _BprLoss.apply(all_embeds, None, None, interaction[:3].contiguous(), L.RSX_BPR_SMORE,
                             float(self.reg_weight), float(self.batch_size), self.n_users, self.n_items)
        cl_items, cl_users = SF.infonce2(side, content, users, pos, self.n_users, CL_TEMPERATURE)
        return bpr + self.cl_loss * (cl_items + cl_users)

    # ------------------------------------------------------------ evaluation
    def full_sort_predict(self, interaction):
        u, i = self._eval_tables()  # not the cached tables: a forward per call
        return ops.score_dense(u, interaction[0].contiguous(), i)
