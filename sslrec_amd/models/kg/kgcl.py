"""KGCL on the HIP path; interface of the reference's models/kg/kgcl.py (:87-371): KGCL(data_handler), get_aug_views() (once per epoch,
trainer/trainer.py:517), cal_loss(batch) with the four views at batch[3:7] -> (loss, {'rec_loss', 'cl_loss'}), generate() -> (user table,
item table), rating, full_predict(batch), cal_kg_loss, and predict_topk for the device top-k evaluation.  The parameters are all_embed
[node_num, d] and relation_embed [relation_num, d] (normal, std 0.1), rgat.W [d, d] and rgat.a [2 d, 1] (xavier, gain 1.414) and rgat.fc =
Linear(2 d, d), drawn in that order (:119-126, :48-52), so one seed gives the reference's initial values and its `state_dict` loads.
rgat.W and rgat.a are never used in the forward, here as upstream: their gradient stays None.  Underneath,

  reference                                                        here
  fc(cat(x[head], x[tail])) . relation_emb[edge_type], LeakyReLU,   ops.rgat_aggregate on the model's own RelGraph: two [N, d] matmuls
  scatter_softmax, scatter_sum (:60-72; needs torch_scatter)        for the node tables P and Q, then one CSR walk (online softmax), no
                                                                    [E, d] tensor, forward and backward (csrc/rgat.hip)
  edge_index[:, random_indices] (:18-24)                            the same np.random.choice draw as a keep mask over the edges
  _sparse_dropout rebuilds the COO (:27-40), torch.sparse.mm        ops.spmm over the DroppedView of the plan of norm_adj
  F.normalize (:80)                                                 ops.normalize_add(zeros, .)
  _get_norm_adj_mat of the masked matrix, twice per epoch           new entry VALUES over the plan of norm_adj, formed on the device from
  (:226-228 -> :140-185: dok_matrix, dict, scipy, a new COO)        integer degree counts (ui_view_values); no new plan per epoch
  _infonce_overall (:351-371)                                       ops.infonce_loss_gathered(v1, v2, idx, 0.2, variant=0): the same sum,
                                                                    -cos(z1, z2) / tau + log sum over ALL rows of exp(cos(z1, .) / tau)

Where the code disagrees with its yml or the paper, the code is followed:
  * tau = 0.2, cl_weight = 0.1 and mu = 0.95 are hard-coded (:96-98); the yml's `tau`, `cl_weight` and `mu` are not read.
  * RGAT.forward returns the LAST hop's normalised table, not the residual sum it also computes (:84).
  * relation_embed has relation_num rows indexed by edge_type itself; the RelGraph is built with rel = edge_type - 1 and
    n_rel = relation_num - 1, so the op gets relation_embed[1:] (row 0, the interact relation, takes no gradient, as upstream).
  * The message dropout applies only when `mess_dropout & self.training` (:290-291): generate() in eval mode applies none.
The InfoNCE kernel normalises with 1 / sqrt(1e-8 + |x|^2) where upstream clamps the norm at 1e-8 (cosine_similarity, F.normalize); for
the rows of this model (|x| ~ 0.1 .. 1) that moves a cosine by less than 1e-6 relative, which tests/test_kgcl.py measures.

The model's own graph: `_samp_edge_from_dict(kg_dict, 15)` (:187-198) runs once at construction with Python's random.sample per head in
kg_dict order, and the RelGraph is built from that sample once; the handler's rel_graph is not used.

Random draws per step, in the reference's order (:254-257): torch.rand(nnz) for `_sparse_dropout` of norm_adj, literally -- the keep flag
is floor(rate + rand), the scale 1 / (1 - rate) --, then np.random.choice(E, int(E * (1 - rate)), replace=False) on the host, then the
message dropout (nn.Dropout on the tables' device) in each of the three forwards.  With model.device_rng both masks are drawn on the
device (the edge mask as E independent flags: the kept count is binomial, not exactly int(E * (1 - rate))).  train.hip_graph is refused:
the edge sample is drawn on the host in every step.  `train_trans` (the TransR step, cal_kg_loss over the handler's triplet batches) is
refused by the handler; cal_kg_loss itself is here as composed torch."""
import random

import numpy as np
import torch as t
import torch.nn.functional as F
from torch import nn

from ... import ops
from ...config.configurator import configs
from ...graph import DroppedView, PropGraph, RelGraph, RevaluedView, graph_of
from ..aug_utils import _pinned
from ..base_model import BaseModel

TRIPLET_NUM = 15


def samp_edge_from_dict(kg_dict, triplet_num=TRIPLET_NUM):
    """`_samp_edge_from_dict` (:187-198): at most triplet_num (relation, tail) pairs per head, random.sample in kg_dict order; int64
    [E, 3] rows (head, tail, relation)"""
    edges = []
    for h in kg_dict:
        t_list = kg_dict[h]
        picked = random.sample(t_list, triplet_num) if len(t_list) > triplet_num else t_list
        edges.extend([h, tail, r] for r, tail in picked)
    return np.asarray(edges, dtype=np.int64).reshape(-1, 3)


def norm_adj_pattern(ui_mat, n_users, n_items):
    """The pattern of `_get_norm_adj_mat` (:140-185) in its entry order, row-major with ascending columns: (rows, cols) int64 [2 m] of the
    [U + I, U + I] matrix, whose first m entries are the distinct (u, U + i) sorted by (u, i) and whose last m the (U + i, u) sorted by
    (i, u); `inter_entry` [nnz of ui_mat] the first-half entry of every interaction (a repeated pair shares one), and `mirror` [m]: entry
    m + k is the transpose of entry mirror[k]."""
    u, i = np.asarray(ui_mat.row, dtype=np.int64), np.asarray(ui_mat.col, dtype=np.int64)
    key, inter_entry = np.unique(u * n_items + i, return_inverse=True)
    eu, ei = key // n_items, key % n_items
    mirror = np.lexsort((eu, ei))                          # by item, then user
    rows = np.concatenate([eu, n_users + ei[mirror]])
    cols = np.concatenate([n_users + ei, eu[mirror]])
    return rows, cols, inter_entry.reshape(-1), mirror


def ui_aug_weights(stability, mu):
    """the keep probabilities per item of `_get_ui_aug_views` (:201-210) from the cosine of the two kg views"""
    kg_stability = t.exp(stability)
    kg_weights = (kg_stability - kg_stability.min()) / (kg_stability.max() - kg_stability.min())
    kg_weights = kg_weights.where(kg_weights > 0.3, t.ones_like(kg_weights) * 0.3)
    weights = mu / t.mean(kg_weights) * kg_weights
    return weights.where(weights < 0.95, t.ones_like(weights) * 0.95)


def ui_view_values(inter_mask, inter_entry, entry_user, entry_item, mirror, n_users, n_items):
    """`_get_norm_adj_mat` of the masked interaction matrix (:226-228 -> :140-185) as VALUES over the full pattern of norm_adj, in its
    entry order: float32((deg_u + 1e-7)^-0.5 (deg_i + 1e-7)^-0.5) computed in float64 with the INTEGER degrees of the masked graph, on
    both halves; 0 for a dropped entry.  All index tensors int64 on one device; runs there (no scipy, no dict).  Returns (values [2 m],
    kept [m] bool)."""
    m = entry_user.numel()
    kept = t.zeros(m, dtype=t.int64, device=inter_mask.device).index_add_(0, inter_entry, inter_mask.to(t.int64)) > 0
    deg_u = t.bincount(entry_user[kept], minlength=n_users)
    deg_i = t.bincount(entry_item[kept], minlength=n_items)
    du = (deg_u.double() + 1e-7).pow(-0.5)
    di = (deg_i.double() + 1e-7).pow(-0.5)
    half = t.where(kept, du[entry_user] * di[entry_item], t.zeros((), dtype=t.float64, device=kept.device)).float()
    return t.cat([half, half[mirror]]), kept


class RGAT(nn.Module):
    """holds the reference RGAT's parameters under its names and in its order (:48-52) and its message dropout"""

    def __init__(self, channel, n_hops, mess_dropout_rate=0.4):
        super().__init__()
        self.mess_dropout_rate = mess_dropout_rate
        self.W = nn.Parameter(t.empty(size=(channel, channel)))
        nn.init.xavier_uniform_(self.W.data, gain=1.414)
        self.a = nn.Parameter(t.empty(size=(2 * channel, 1)))
        nn.init.xavier_uniform_(self.a.data, gain=1.414)
        self.fc = nn.Linear(2 * channel, channel)
        self.n_hops = n_hops
        self.slope = 0.2
        self.dropout = nn.Dropout(p=mess_dropout_rate)

    def forward(self, graph, entity_emb, relation_emb, keep=None, mess_dropout=True):
        """:74-84: the last hop's normalised table"""
        for _ in range(self.n_hops):
            entity_emb = ops.rgat_aggregate(graph, entity_emb, self.fc.weight, self.fc.bias, relation_emb, keep, self.slope)
            if mess_dropout:
                entity_emb = self.dropout(entity_emb)
            entity_emb = ops.normalize_add(t.zeros_like(entity_emb), entity_emb)
        return entity_emb


class KGCL(BaseModel):
    def __init__(self, data_handler):
        if configs['train'].get('hip_graph'):
            raise NotImplementedError('train.hip_graph is not supported by KGCL: every step draws its edge sample with np.random.choice on '
                                      'the host, which a captured step cannot do')
        super().__init__(data_handler)
        self.data_handler = data_handler
        data_cfg, model_cfg = configs['data'], configs['model']
        self.n_users, self.n_items = data_cfg['user_num'], data_cfg['item_num']
        self.n_relations, self.n_entities, self.n_nodes = data_cfg['relation_num'], data_cfg['entity_num'], data_cfg['node_num']
        self.tau, self.cl_weight, self.mu = 0.2, 0.1, 0.95                     # hard-coded upstream (:96-98)
        self.decay = model_cfg['decay_weight']
        self.emb_size = model_cfg['embedding_size']
        self.context_hops = model_cfg['layer_num_kg']
        self.layer_num = model_cfg['layer_num']
        self.node_dropout = model_cfg['node_dropout']
        self.node_dropout_rate = model_cfg['node_dropout_rate']
        self.mess_dropout = model_cfg['mess_dropout']
        self.mess_dropout_rate = model_cfg['mess_dropout_rate']
        self.device_rng = bool(model_cfg.get('device_rng'))
        device = t.device(configs['device'])

        # norm_adj (:111) and what the per-epoch views need, once
        rows, cols, inter_entry, mirror = norm_adj_pattern(data_handler.ui_mat, self.n_users, self.n_items)
        m = mirror.size
        n = self.n_users + self.n_items
        deg = np.bincount(rows, minlength=n).astype(np.float64) + 1e-7
        vals = np.power(deg, -0.5)[rows] * np.power(deg, -0.5)[cols]
        self.norm_adj = t.sparse_coo_tensor(t.from_numpy(np.vstack([rows, cols])), t.from_numpy(vals).float(), (n, n),
                                            check_invariants=False).to(device)
        if self.norm_adj.is_cuda:
            graph_of(self.norm_adj)
        self._inter_entry = t.from_numpy(inter_entry).to(device)
        self._entry_user = t.from_numpy(rows[:m].copy()).to(device)
        self._entry_item = t.from_numpy(cols[:m] - self.n_users).to(device)
        self._mirror = t.from_numpy(mirror).to(device)
        self._inter_item = t.from_numpy(np.asarray(data_handler.ui_mat.col, dtype=np.int64)).to(device)

        # the model's own typed graph (:116-117): sampled once
        self.kg_dict = data_handler.kg_dict
        self.kg_sample = samp_edge_from_dict(self.kg_dict, TRIPLET_NUM)
        self.rel_graph = RelGraph(self.kg_sample[:, 0], self.kg_sample[:, 1], self.kg_sample[:, 2] - 1, self.n_entities, self.n_relations - 1,
                                  device=device if device.type == 'cuda' else 'cpu')

        self.all_embed = nn.Parameter(nn.init.normal_(t.empty(self.n_nodes, self.emb_size), std=0.1))
        self.relation_embed = nn.Parameter(nn.init.normal_(t.empty(self.n_relations, self.emb_size), std=0.1))
        self.rgat = RGAT(self.emb_size, self.context_hops, self.mess_dropout_rate)
        self.is_training = True
        self._eval_tables = None                                          # (user table, item table) of the current evaluation
        self.last_keep = self.last_ui_keep = None                         # the step's two masks (tests, diagnostics)

    # -- graphs and views --------------------------------------------------------------------------------------------------------------
    def _rel_graph(self, device):
        g = self.rel_graph
        if g.device != device:                               # built for configs['device']: follow the tables
            g = self.rel_graph = RelGraph(g.head, g.tail, g.rel, g.n, g.n_rel, device=device)
        return g

    def _adj(self, device):
        if self.norm_adj.device != device:
            self.norm_adj = self.norm_adj.to(device)
            for name in ('_inter_entry', '_entry_user', '_entry_item', '_mirror', '_inter_item'):
                setattr(self, name, getattr(self, name).to(device))
        return self.norm_adj

    def _edge_keep(self, n_edges, rate, device):
        """`_edge_sampling` (:18-24) as a mask: uint8 [E] on `device` with int(E * rate) kept edges"""
        if self.device_rng and device.type == 'cuda':
            return (t.rand(n_edges, device=device) < rate).to(t.uint8)
        picked = np.random.choice(n_edges, size=int(n_edges * rate), replace=False)
        keep = np.zeros(n_edges, dtype=np.uint8)
        keep[picked] = 1
        return t.from_numpy(keep).to(device)

    def _ui_keep(self, nnz, device):
        """the keep flags of `_sparse_dropout` (:27-32), literally: floor(rate + rand) per stored entry, bool [nnz] on `device`"""
        rate = self.node_dropout_rate
        draw = t.rand(nnz, device=device) if self.device_rng and device.type == 'cuda' else _pinned.rand_to((nnz,), device)
        return (draw + rate).floor().type(t.bool)

    def _view(self, vals):
        """norm_adj with new entry values (None: its own) as what `_spread` multiplies by: a view over the one plan on a HIP device, a
        torch sparse tensor on the host"""
        adj = self._adj(self.all_embed.device)
        if adj.is_cuda:
            return graph_of(adj) if vals is None else RevaluedView(graph_of(adj), vals)
        if vals is None:
            return adj
        return t.sparse_coo_tensor(adj._indices(), vals, adj.shape, check_invariants=False)

    def _dropped(self, ui_keep):
        """norm_adj after `_sparse_dropout`"""
        adj = self._adj(self.all_embed.device)
        scale = 1. / (1 - self.node_dropout_rate)
        if adj.is_cuda:
            return DroppedView(graph_of(adj), ui_keep, scale)
        return t.sparse_coo_tensor(adj._indices()[:, ui_keep], adj._values()[ui_keep] * scale, adj.shape, check_invariants=False)

    @staticmethod
    def _spread(view, table):
        if isinstance(view, (PropGraph, DroppedView, RevaluedView)):
            return ops.spmm(view, table)
        return t.sparse.mm(view.to(table.dtype), table)

    @t.no_grad()
    def get_aug_views(self):
        """:230-247: (kg keep mask 1, kg keep mask 2, ui view 1, ui view 2).  The kg views are keep masks over the model's RelGraph; a ui
        view is norm_adj's pattern with the re-normalised values of the masked interaction matrix (ui_view_values)."""
        device = self.all_embed.device
        graph = self._rel_graph(device)
        self._adj(device)
        entity_emb, relation_emb = self.all_embed[self.n_users:, :], self.relation_embed[1:]
        kg_view_1 = self._edge_keep(graph.n_edges, 0.5, device)
        kg_view_2 = self._edge_keep(graph.n_edges, 0.5, device)
        kg_v1_ro = self.rgat(graph, entity_emb, relation_emb, kg_view_1, False)[:self.n_items, :]
        kg_v2_ro = self.rgat(graph, entity_emb, relation_emb, kg_view_2, False)[:self.n_items, :]
        stability = F.cosine_similarity(kg_v1_ro, kg_v2_ro, dim=-1)
        self.last_aug_weights = ui_aug_weights(stability, self.mu)
        views, self.last_aug_masks = [], []                              # the per-interaction draws (tests, diagnostics)
        for _ in range(2):
            edge_mask = t.bernoulli(self.last_aug_weights[self._inter_item]).bool()
            vals, _ = ui_view_values(edge_mask, self._inter_entry, self._entry_user, self._entry_item, self._mirror, self.n_users, self.n_items)
            views.append(self._view(vals.to(self.all_embed.dtype)))
            self.last_aug_masks.append(edge_mask)
        return kg_view_1, kg_view_2, views[0], views[1]

    # -- forward -----------------------------------------------------------------------------------------------------------------------
    def forward(self, kg_keep, ui_view):
        """:286-301: RGAT over the (masked) typed graph, then LightGCN's mean over the layers of the (user, item) table"""
        user_emb, entity_emb = self.all_embed[:self.n_users, :], self.all_embed[self.n_users:, :]
        graph = self._rel_graph(self.all_embed.device)
        entity_emb = self.rgat(graph, entity_emb, self.relation_embed[1:], kg_keep, bool(self.mess_dropout) & self.training)
        all_emb = t.cat([user_emb, entity_emb[:self.n_items, :]], dim=0)
        total = all_emb
        for _ in range(self.layer_num):
            all_emb = self._spread(ui_view, all_emb)
            total = total + all_emb
        total = total / (self.layer_num + 1)
        return total[:self.n_users], total[self.n_users:]

    def _bpr_loss(self, users_emb, pos_emb, neg_emb):
        """:316-321 with loss_utils.cal_bpr_loss: sum softplus(neg - pos)"""
        reg_loss = (1 / 2) * (users_emb.norm(2).pow(2) + pos_emb.norm(2).pow(2) + neg_emb.norm(2).pow(2)) / float(users_emb.shape[0])
        if users_emb.is_cuda and users_emb.dtype == t.float32:
            return ops.bpr_loss(users_emb, pos_emb, neg_emb), reg_loss
        return F.softplus((users_emb * neg_emb).sum(-1) - (users_emb * pos_emb).sum(-1)).sum(), reg_loss

    def _infonce_overall(self, table1, table2, idx):
        """`_infonce_overall(z1[idx], z2[idx], z2)` (:351-371)"""
        if table1.is_cuda and table1.dtype == t.float32:
            return ops.infonce_loss_gathered(table1, table2, idx, temp=self.tau, variant=0)
        z1, z2 = table1[idx], table2[idx]
        between = F.cosine_similarity(z1, z2) / self.tau
        everyone = F.normalize(z1) @ F.normalize(table2).t() / self.tau
        return (t.logsumexp(everyone, dim=1) - between).sum()

    def cal_loss(self, batch_data):
        self.is_training = True
        self._eval_tables = None
        user, pos_item, neg_item = batch_data[:3]
        kg_view_1, kg_view_2, ui_view_1, ui_view_2 = batch_data[3:7]
        device = self.all_embed.device
        adj = self._adj(device)
        keep = ui_keep = None
        if self.node_dropout:
            ui_keep = self._ui_keep(adj._nnz(), device)
            keep = self._edge_keep(self._rel_graph(device).n_edges, 1 - self.node_dropout_rate, device)
        self.last_keep, self.last_ui_keep = keep, ui_keep
        user_emb, item_emb = self.forward(keep, self._view(None) if ui_keep is None else self._dropped(ui_keep))
        rec_loss, reg_loss = self._bpr_loss(user_emb[user], item_emb[pos_item], item_emb[neg_item])
        users_v1, items_v1 = self.forward(kg_view_1, ui_view_1)
        users_v2, items_v2 = self.forward(kg_view_2, ui_view_2)
        cl_loss = self.cl_weight * (self._infonce_overall(users_v1, users_v2, user) + self._infonce_overall(items_v1, items_v2, pos_item))
        loss = rec_loss + self.decay * reg_loss + cl_loss
        return loss, {'rec_loss': rec_loss.detach(), 'cl_loss': cl_loss.detach()}

    def generate(self):
        """(user table, item table) over the full graphs (:303-305)"""
        return self.forward(None, self._view(None))

    def rating(self, u_emb, i_emb):
        return u_emb @ i_emb.t()

    def cal_kg_loss(self, batch_data):
        """:323-349 (TransE-style scores and an L2 term), [B, d]-sized composed torch"""
        h, r, pos_t, neg_t = batch_data
        entity_emb = self.all_embed[self.n_users:, :]
        r_embed, h_embed, pos_t_embed, neg_t_embed = self.relation_embed[r], entity_emb[h], entity_emb[pos_t], entity_emb[neg_t]
        pos_score = t.sum(t.pow(h_embed + r_embed - pos_t_embed, 2), dim=1)
        neg_score = t.sum(t.pow(h_embed + r_embed - neg_t_embed, 2), dim=1)
        kg_loss = t.mean((-1.0) * F.logsigmoid(neg_score - pos_score))
        l2 = lambda x: t.mean(t.sum(t.pow(x, 2), dim=1, keepdim=False) / 2.)
        return kg_loss + 1e-3 * (l2(h_embed) + l2(r_embed) + l2(pos_t_embed) + l2(neg_t_embed))

    # -- evaluation --------------------------------------------------------------------------------------------------------------------
    def _embeddings_for_eval(self):
        """the two tables for scoring: the first evaluation after a training step propagates anew (one forward per evaluation, the
        reference's eval_at_one_forward), the later batches reuse it"""
        if self.is_training or self._eval_tables is None:
            with t.no_grad():
                user_emb, item_emb = self.generate()
            self._eval_tables = (user_emb.contiguous(), item_emb.contiguous())
            self.is_training = False
        return self._eval_tables

    def train(self, mode=True):
        if mode:                         # back to training: the evaluation cache is stale
            self.is_training = True
            self._eval_tables = None
        return super().train(mode)

    def full_predict(self, batch_data):
        user_emb, item_emb = self._embeddings_for_eval()
        pck_users, train_mask = batch_data
        if user_emb.is_cuda and user_emb.shape[1] <= ops.INFONCE_DIMS[-1]:
            return ops.full_predict(user_emb, item_emb, pck_users.long(), train_mask)
        return self._mask_predict(user_emb[pck_users.long()] @ item_emb.T, train_mask)

    def predict_topk(self, users, k, trn_csr_device):
        """top-k unseen items without the dense train mask (GraphCF.predict_topk)"""
        user_emb, item_emb = self._embeddings_for_eval()
        if int(k) > ops.EVAL_KMAX:
            raise ValueError('predict_topk: k = %d exceeds the kernel\'s %d' % (int(k), ops.EVAL_KMAX))
        return ops.eval_topk(user_emb, item_emb, users.long(), k, trn_csr_device)
