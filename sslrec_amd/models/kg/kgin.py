"""KGIN on the HIP path; interface of the reference's models/kg/kgin.py (:189-335): KGIN(data_handler), cal_loss(batch) -> (loss,
{'loss', 'rec_loss', 'reg_loss', 'cor'}), generate() -> (user table, item table), rating, full_predict(batch), and predict_topk for the
device top-k evaluation.  The parameters are all_embed [node_num, d], latent_emb [F, d], gcn.weight [relation_num - 1, d] and
gcn.disen_weight_att [F, relation_num - 1], drawn in that order (:233-236, :71-76), so one seed gives the reference's initial values and
its `state_dict` loads.  Underneath,

  reference                                                        here
  weight[edge_type - 1], entity_emb[tail] * ., scatter_mean         ops.rel_aggregate on the handler's RelGraph: one CSR walk, no [E, d]
  (:33-36; needs torch_scatter)                                     tensor, forward and backward (csrc/kgin.hip)
  edge_index[:, random_indices] (:83-88)                            the same np.random.choice draw as a keep mask over the edges; one
                                                                    mask serves all hops, nothing is rebuilt
  _sparse_dropout rebuilds the COO (:90-103), torch.sparse.mm       ops.spmm over the DroppedView of the handler's plan
  mm, softmax, expand to [U, F, d], product, sum (:38-46)           ops.factor_modulate: one launch, D = softmax(att) @ weight once
  F.normalize + torch.add (:180-185)                                ops.normalize_add
  _cul_cor, create_loss (:105-158, :321-335)                        the same composed torch: [F, R]- and [B, d]-sized

One deliberate deviation.  The reference's `nn.Parameter(x).to(device)` (:219-220) leaves a plain tensor on a CUDA device, so its two
embedding tables are never trained there; its CPU run registers and trains them.  Here both are parameters on every device.

Random draws per step, in the reference's order: np.random.choice(E, int(E * rate), replace=False) on the host (the kept edge SET is the
reference's; the order of the kept edges, which upstream only changes the order of the sums, is the graph's), then torch.rand(nnz) for
`_sparse_dropout`, followed literally: the keep flag is floor(rate + rand), the scale 1 / (1 - rate).  The message dropout is F.dropout on
the tables' device.  The node dropout is applied in generate() too, as upstream.  With model.device_rng the edge mask is drawn on the
device as E independent flags: the kept count is then binomial around E * rate, not exactly int(E * rate).  train.hip_graph is refused:
the edge sample is drawn on the host in every step."""
import numpy as np
import torch as t
import torch.nn.functional as F
from torch import nn

from ... import ops
from ...config.configurator import configs
from ...graph import DroppedView, graph_of
from ..aug_utils import _pinned
from ..base_model import BaseModel

init = nn.init.xavier_uniform_


def distance_correlation(a, b):
    """distance correlation of two vectors [n] (:111-130): doubly centred distance matrices, every square root taken of max(., 0) + 1e-8"""
    def centred(x):
        x = x.unsqueeze(-1)
        sq = x ** 2
        dist = t.sqrt(t.clamp(sq - 2 * (x @ x.t()) + sq.t(), min=0) + 1e-8)
        return dist - dist.mean(dim=0, keepdim=True) - dist.mean(dim=1, keepdim=True) + dist.mean()
    n = a.shape[0]
    A, B = centred(a), centred(b)

    def dcov(P, Q):
        return t.sqrt(t.clamp((P * Q).sum() / n ** 2, min=0) + 1e-8)
    return dcov(A, B) / t.sqrt(dcov(A, A) * dcov(B, B) + 1e-8)


def cosine_similarity_sq(a, b):
    """squared cosine of two vectors (:106-110); no clamp of the norms, as upstream"""
    return ((a / a.norm(dim=0, keepdim=True)) * (b / b.norm(dim=0, keepdim=True))).sum(dim=0) ** 2


def mutual_information(att, temperature):
    """:131-145 on disen_weight_att [F, R]"""
    att_t = att.t()
    normed = att_t / att_t.norm(dim=1, keepdim=True)
    pos = t.exp((normed * normed).sum(dim=1) / temperature)
    ttl = t.exp((att_t @ att).sum(dim=1) / temperature)
    return -t.log(pos / ttl).sum()


def factor_correlation(att, ind, temperature=0.2):
    """`_cul_cor` (:105-158): the independence term of the F rows of disen_weight_att"""
    if ind == 'mi':
        return mutual_information(att, temperature)
    pair = distance_correlation if ind == 'distance' else cosine_similarity_sq
    cor = 0
    for i in range(att.shape[0]):
        for j in range(i + 1, att.shape[0]):
            cor = cor + pair(att[i], att[j])
    return cor


class GraphConv(nn.Module):
    """holds the reference GraphConv's parameters under its names (gcn.weight, gcn.disen_weight_att) and its message dropout"""

    def __init__(self, channel, n_factors, n_relations, mess_dropout_rate):
        super().__init__()
        self.weight = nn.Parameter(init(t.empty(n_relations - 1, channel)))
        self.disen_weight_att = nn.Parameter(init(t.empty(n_factors, n_relations - 1)))
        self.dropout = nn.Dropout(p=mess_dropout_rate)
        self.temperature = 0.2


class KGIN(BaseModel):
    def __init__(self, data_handler):
        if configs['train'].get('hip_graph'):
            raise NotImplementedError('train.hip_graph is not supported by KGIN: every step draws its edge sample with np.random.choice on '
                                      'the host, which a captured step cannot do')
        super().__init__(data_handler)
        self.data_handler = data_handler
        data_cfg, model_cfg = configs['data'], configs['model']
        self.n_users, self.n_items = data_cfg['user_num'], data_cfg['item_num']
        self.n_relations, self.n_entities, self.n_nodes = data_cfg['relation_num'], data_cfg['entity_num'], data_cfg['node_num']
        self.decay = model_cfg['decay_weight']
        self.emb_size = model_cfg['embedding_size']
        self.context_hops = model_cfg['layer_num']
        self.node_dropout = model_cfg['node_dropout']
        self.node_dropout_rate = model_cfg['node_dropout_rate']
        self.mess_dropout = model_cfg['mess_dropout']
        self.mess_dropout_rate = model_cfg['mess_dropout_rate']
        self.n_factors = model_cfg['n_factors']
        self.ind = model_cfg['ind']
        self.sim_decay = model_cfg['sim_regularity']
        self.device_rng = bool(model_cfg.get('device_rng'))

        self.all_embed = nn.Parameter(init(t.empty(self.n_nodes, self.emb_size)))
        self.latent_emb = nn.Parameter(init(t.empty(self.n_factors, self.emb_size)))
        self.gcn = GraphConv(self.emb_size, self.n_factors, self.n_relations, self.mess_dropout_rate)
        self.is_training = True
        self.final_user_embeds = self.final_entity_embeds = None          # the last training step's propagated tables
        self._eval_tables = None                                          # (user table, item table) of the current evaluation
        self.last_keep = self.last_ui_keep = None          # the step's two masks (tests, diagnostics)

    # -- the two graphs ----------------------------------------------------------------------------------------------------------------
    def _rel_graph(self, device):
        g = self.data_handler.rel_graph
        if g.device != device:                               # the handler built it for configs['device']: follow the tables
            from ...graph import RelGraph
            g = self.data_handler.rel_graph = RelGraph(g.head, g.tail, g.rel, g.n, g.n_rel, device=device)
        return g

    def _edge_keep(self, n_edges, device):
        """`_edge_sampling` (:83-88) as a mask: uint8 [E] on `device`, or None without node dropout"""
        rate = self.node_dropout_rate
        if self.device_rng and device.type == 'cuda':
            return (t.rand(n_edges, device=device) < rate).to(t.uint8)
        picked = np.random.choice(n_edges, size=int(n_edges * rate), replace=False)
        keep = np.zeros(n_edges, dtype=np.uint8)
        keep[picked] = 1
        return t.from_numpy(keep).to(device)

    def _ui_keep(self, nnz, device):
        """the keep flags of `_sparse_dropout` (:90-95), literally: floor(rate + rand) per stored entry, bool [nnz] on `device`"""
        rate = self.node_dropout_rate
        draw = t.rand(nnz, device=device) if self.device_rng and device.type == 'cuda' else _pinned.rand_to((nnz,), device)
        return (draw + rate).floor().type(t.bool)

    def _interact(self, x, ui_keep):
        """interact_mat (after `_sparse_dropout` when a mask is given) as a function table -> product"""
        adj = self.data_handler.interact_mat
        scale = 1. / (1 - self.node_dropout_rate) if ui_keep is not None else 1.0
        if x.is_cuda:
            graph = graph_of(adj)
            view = graph if ui_keep is None else DroppedView(graph, ui_keep, scale)
            return lambda table: ops.spmm(view, table)
        # host tensors: the reference's statements (the tests' float64 runs use them)
        adj = adj.to(x.device)
        idx, val = adj._indices(), adj._values()
        if ui_keep is not None:
            idx, val = idx[:, ui_keep], val[ui_keep]
        dense_adj = t.sparse_coo_tensor(idx, val.to(x.dtype) * scale, adj.shape)
        return lambda table: t.sparse.mm(dense_adj, table)

    # -- forward -----------------------------------------------------------------------------------------------------------------------
    def _propagate(self, mess_dropout, node_dropout):
        """GraphConv.forward (:160-187): (entity_res_emb, user_res_emb, cor)"""
        user_emb, entity_emb = self.all_embed[:self.n_users, :], self.all_embed[self.n_users:, :]
        device = self.all_embed.device
        graph = self._rel_graph(device)
        keep = ui_keep = None
        if node_dropout:
            keep = self._edge_keep(graph.n_edges, device)
            ui_keep = self._ui_keep(self.data_handler.interact_mat._nnz(), device)
        self.last_keep, self.last_ui_keep = keep, ui_keep
        interact = self._interact(entity_emb, ui_keep)
        weight, att = self.gcn.weight, self.gcn.disen_weight_att
        cor = factor_correlation(att, self.ind, self.gcn.temperature)
        disen_weight = t.softmax(att, dim=-1) @ weight                              # [F, d], once per forward
        entity_res, user_res = entity_emb, user_emb
        for hop in range(self.context_hops):
            entity_agg = ops.rel_aggregate(graph, entity_emb, weight, keep)
            user_agg = ops.factor_modulate(interact(entity_emb), user_emb, self.latent_emb, disen_weight)
            if mess_dropout:
                entity_agg = self.gcn.dropout(entity_agg)
                user_agg = self.gcn.dropout(user_agg)
            if hop + 1 < self.context_hops:                                         # the normalised tables feed the next hop
                entity_emb = ops.normalize_add(t.zeros_like(entity_agg), entity_agg)
                user_emb = ops.normalize_add(t.zeros_like(user_agg), user_agg)
                entity_res, user_res = entity_res + entity_emb, user_res + user_emb
            else:                                                                   # the last hop's are only added
                entity_res, user_res = ops.normalize_add(entity_res, entity_agg), ops.normalize_add(user_res, user_agg)
        return entity_res, user_res, cor

    def create_loss(self, users, pos_items, neg_items, cor):
        """:321-335"""
        batch_size = users.shape[0]
        pos_scores = (users * pos_items).sum(dim=1)
        neg_scores = (users * neg_items).sum(dim=1)
        mf_loss = -F.logsigmoid(pos_scores - neg_scores).mean()
        regularizer = (users.norm() ** 2 + pos_items.norm() ** 2 + neg_items.norm() ** 2) / 2
        emb_loss = self.decay * regularizer / batch_size
        cor_loss = self.sim_decay * cor
        return mf_loss + emb_loss + cor_loss, mf_loss, emb_loss, cor

    def cal_loss(self, batch_data):
        self.is_training = True
        self._eval_tables = None
        user, pos_item, neg_item = batch_data[:3]
        entity_gcn_emb, user_gcn_emb, cor = self._propagate(self.mess_dropout, self.node_dropout)
        self.final_user_embeds, self.final_entity_embeds = user_gcn_emb, entity_gcn_emb
        loss, rec_loss, reg_loss, cor = self.create_loss(user_gcn_emb[user], entity_gcn_emb[pos_item], entity_gcn_emb[neg_item], cor)
        return loss, {'loss': loss.detach(), 'rec_loss': rec_loss.detach(), 'reg_loss': reg_loss.detach(), 'cor': cor.detach()}

    def generate(self):
        """(user table, item table) for scoring (:299-310): the message dropout follows the module's train / eval mode, the node dropout
        is drawn here too"""
        entity_gcn_emb, user_gcn_emb, _ = self._propagate(self.mess_dropout, self.node_dropout)
        return user_gcn_emb, entity_gcn_emb[:self.n_items]

    def rating(self, u_emb, i_emb):
        return u_emb @ i_emb.t()

    # -- evaluation --------------------------------------------------------------------------------------------------------------------
    def _embeddings_for_eval(self):
        """the two tables for scoring: the first evaluation after a training step propagates anew (one forward per evaluation, the
        reference's eval_at_one_forward), the later batches reuse it"""
        if self.is_training or self._eval_tables is None:
            with t.no_grad():
                user_emb, item_emb = self.generate()
            from ...rng import flush_host_replay
            flush_host_replay()                              # evaluation drew from the replayed CPU generator: hand it back
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
