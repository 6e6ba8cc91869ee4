"""DCCF on the HIP path; interface of the reference's models/general_cf/dccf.py (:14-156): constructor argument, forward() and its
6-tuple, cal_loss(batch), full_predict(batch) and the loss dictionary keys.  Underneath,

  reference                                             here
  torch_sparse.spmm with D^-1/2 A D^-1/2 (:57-63, :74)   ops.spmm over data_handler.torch_adj (same pattern, same normalization)
  split + 2 x (GEMM, softmax, GEMM) + concat (:77-80)    ops.intent_aggregate_stacked: one launch, no [N, K] tensor (csrc/intent.hip)
  4 index_selects + AdaptiveMask + spmm (:83-90)         AdaptiveMask on the node table (SDDMM) + ops.spmm_valued, no [nnz, d] tensor
  cal_infonce_loss x 6 per layer (:125-130)              the fused InfoNCE kernels on the gathered unique rows

No torch_sparse.  The model draws nothing, so model.device_rng has no effect on it."""
import numpy as np
import scipy.sparse as sp
import torch as t
from torch import nn

from ... import ops
from ...config.configurator import configs
from ..aug_utils import AdaptiveMask
from ..loss_utils import cal_bpr_loss_stacked, cal_infonce_loss, reg_params
from ._graph_cf import GraphCF

init = nn.init.xavier_uniform_


class DCCF(GraphCF):
    def __init__(self, data_handler):
        # The reference draws, in this order (:42-45, :53-55): N(0,1) for the two nn.Embedding tables, xavier for user_intent and
        # item_intent, then xavier over the two tables again.  GraphCF initialises its one-buffer pair first; its draws are taken
        # back and the reference's sequence is replayed, so one seed gives the reference's parameters bit for bit.
        rng_state = t.get_rng_state()
        super().__init__(data_handler)
        t.set_rng_state(rng_state)

        # adjacency pattern in the reference's entry order (:19-25): both directions stacked, .tocsr().tocoo()
        trn = data_handler.trn_mat.tocoo()
        rows, cols = trn.row, trn.col
        n = self.user_num + self.item_num
        new_rows = np.concatenate([rows, cols + self.user_num], axis=0)
        new_cols = np.concatenate([cols + self.user_num, rows], axis=0)
        plain_adj = sp.coo_matrix((np.ones(len(new_rows)), (new_rows, new_cols)), shape=[n, n]).tocsr().tocoo()
        self.A_in_shape = plain_adj.shape
        self.all_h_list = t.from_numpy(plain_adj.row.astype(np.int64))
        self.all_t_list = t.from_numpy(plain_adj.col.astype(np.int64))
        self.adaptive_masker = AdaptiveMask(head_list=self.all_h_list, tail_list=self.all_t_list, matrix_shape=self.A_in_shape,
                                            device=configs['device'])

        # hyper parameters
        model_cfg = configs['model']
        self.intent_num = model_cfg['intent_num']
        self.cl_weight = model_cfg['cl_weight']
        self.temperature = model_cfg['temperature']

        # model parameters, in the reference's draw order
        t.empty(self.user_num, self.embedding_size).normal_()          # nn.Embedding(user_num, d)
        t.empty(self.item_num, self.embedding_size).normal_()          # nn.Embedding(item_num, d)
        self.user_intent = nn.Parameter(init(t.empty(self.embedding_size, self.intent_num)), requires_grad=True)
        self.item_intent = nn.Parameter(init(t.empty(self.embedding_size, self.intent_num)), requires_grad=True)
        self._init_weight()

    def _init_weight(self):
        init(self.user_embeds.data)
        init(self.item_embeds.data)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # a checkpoint of the reference names the tables after its nn.Embedding modules
        for name in ('user_embeds', 'item_embeds'):
            old = prefix + name + '.weight'
            if old in state_dict and prefix + name not in state_dict:
                state_dict[prefix + name] = state_dict.pop(old)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self):
        if not self.is_training and self.final_embeds is not None:
            return self.final_embeds[:self.user_num], self.final_embeds[self.user_num:], None, None, None, None

        masker = self.adaptive_masker
        all_embeds = [self._stacked_tables(alias_ok=True)]
        gnn_embeds, int_embeds, gaa_embeds, iaa_embeds = [], [], [], []
        total = all_embeds[0]
        for i in range(self.layer_num):
            cur = all_embeds[i]
            gnn_layer_embeds = ops.spmm(self.adj, cur)                                                       # :74
            int_layer_embeds = ops.intent_aggregate_stacked(cur, self.user_num, self.user_intent, self.item_intent)      # :77-80
            gaa_layer_embeds = masker.propagate(masker(gnn_layer_embeds)[1], cur)                            # :83-84, :87, :89
            iaa_layer_embeds = masker.propagate(masker(int_layer_embeds)[1], cur)                            # :85-86, :88, :90
            gnn_embeds.append(gnn_layer_embeds)
            int_embeds.append(int_layer_embeds)
            gaa_embeds.append(gaa_layer_embeds)
            iaa_embeds.append(iaa_layer_embeds)
            all_embeds.append(gnn_layer_embeds + int_layer_embeds + gaa_layer_embeds + iaa_layer_embeds + cur)
            total = total + all_embeds[-1]
        self.final_embeds = total
        return total[:self.user_num], total[self.user_num:], gnn_embeds, int_embeds, gaa_embeds, iaa_embeds

    def _cal_cl_loss(self, users, positems, negitems, gnn_emb, int_emb, gaa_emb, iaa_emb):
        users = t.unique(users)
        items = t.unique(t.concat([positems, negitems])) + self.user_num      # rows of the stacked tables
        n_unique_users = users.shape[0]
        cl_loss = 0.0
        for i in range(len(gnn_emb)):
            for idx in (users, items):
                anchor = gnn_emb[i][idx]
                for other in (int_emb[i], gaa_emb[i], iaa_emb[i]):
                    view = other[idx]
                    # every term, the item terms too, over the number of unique USERS: the reference's own expression (:125-130)
                    cl_loss = cl_loss + cal_infonce_loss(anchor, view, view, self.temperature, self.infonce_precision) / n_unique_users
        return cl_loss

    def cal_loss(self, batch_data):
        self.is_training = True
        self._begin_step()
        _, _, gnn_embeds, int_embeds, gaa_embeds, iaa_embeds = self.forward()
        ancs, poss, negs = batch_data
        bpr_loss = cal_bpr_loss_stacked(self.final_embeds, self.user_num, ancs, poss, negs, divisor=ancs.shape[0])
        reg_loss = self.reg_weight * reg_params(self)
        cl_loss = self.cl_weight * self._cal_cl_loss(ancs, poss, negs, gnn_embeds, int_embeds, gaa_embeds, iaa_embeds)
        loss = bpr_loss + reg_loss + cl_loss
        losses = {'bpr_loss': bpr_loss, 'reg_loss': reg_loss, 'cl_loss': cl_loss}
        return loss, losses

    def _embeddings_for_eval(self):
        self._stacked_e0 = None          # (evaluation never reuses a training step's concatenated tables)
        with t.no_grad():
            user_embeds, item_embeds = self.forward()[:2]
        self.is_training = False
        return user_embeds, item_embeds

    def full_predict(self, batch_data):
        users, items = self._embeddings_for_eval()
        return self._score_all_items(users, items, batch_data)
