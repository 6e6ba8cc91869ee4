"""KGRec on the HIP path; interface of the reference's models/kg/kgrec.py (:319-575): KGRec(data_handler), cal_loss(batch) -> (loss,
{'rec_loss', 'mae_loss', 'cl_loss'}), generate() -> (user table, item table), rating, full_predict(batch),
generate_global_attn_score(), and predict_topk for the device top-k evaluation.  The parameters are all_embed [node_num, d],
gcn.relation_emb [relation_num - 1, d], gcn.W_Q [d, d] (xavier uniform) and the two MLPs contrast_fn.mlp1 / contrast_fn.mlp2
(Linear, ReLU, Linear), drawn in that order (:367-369, :33-42, :196-205), so one seed gives the reference's initial values and its
`state_dict` loads.  Underneath,

  reference                                                        here
  (entity_emb[head] @ W_Q) . (entity_emb[tail] @ W_Q) .            ops.attn_hgcn_aggregate on the handler's RelGraph: one [N, d] matmul for
  relation_emb[edge_type - 1] per head / sqrt(d_k), softmax over    the node table T = X W_Q, then one CSR walk with an online softmax per
  the head entity's edges (torch_geometric), the weighted sum of    attention head; no [E, d] tensor, forward and backward (csrc/rmha.hip)
  entity_emb[tail] * relation_emb (torch_scatter) (:63-82)
  norm_attn_computer (:165-188) and the two scatter_mean of        ops.rel_rationale: one walk by head, one by tail, [E]- and [N]-sized
  cal_loss (:414-417)                                               outputs
  kg_agg / forward_kg (:136-163)                                   ops.rel_aggregate (csrc/kgin.hip)
  edge_index[:, random_indices], edge_index[:, ~mask],              uint8 keep masks over the ONE RelGraph, read through the edge ids: the
  edge_index[:, cl_kg_mask] (:232-302)                              sample S, enc = S minus the masked edges, cl = S minus the least scored
  _sparse_dropout rebuilds the COO (:305-316), scatter_sum          ops.spmm over a DroppedView of the handler's plan of D^-1 A, in both
  over inter_edge (:84-87, :149-155)                                directions; the contrastive view is a second mask, scale 1 / (keep keep')
  F.normalize + torch.add (:112-117)                                ops.normalize_add

cal_loss follows :398-472 step by step, and the reference's quirks stay:
  * `_relation_aware_edge_sampling` loops i = 0 .. relation_num - 2 over edge types that run 1 .. relation_num - 1: type 0 selects
    nothing (np.random.choice(0, 0, replace=False) returns an empty array and leaves numpy's state alone) and the LAST type is never
    sampled, so its edges are absent from every training step.
  * forward_ui and forward_kg are called without `mess_dropout`, so the two contrastive views drop messages whatever the yml says;
    `model.mess_dropout` governs only the recommendation task's forward.
  * `_adaptive_kg_drop_cl` ranks by the NOISY score (the Gumbel draw of the MAE mask is added in place before it).
  * `std` (:420) is computed and never used, and `epoch_start` (:400) only switches a log line: neither is here.
`item_attn` (never passed by the reference's own calls) and `generate_kg_drop` (it reads `kg_drop_test_keep_rate`, which nothing sets)
are left out.

Random draws per step, in the reference's order: np.random.choice per edge type on the host; torch.rand_like on the device (Gumbel);
np.random.choice(|S|, mae_msize) on the host; torch.rand(nnz) of `_sparse_dropout`, literally (floor(rate + rand)); the message dropout
of the first forward; torch.rand_like and torch.multinomial (`samp_func: torch`) or numpy's weighted choice (`np`) for the interaction
view; the message dropout of forward_ui and forward_kg; torch.randperm(item_num) on the host for the negatives of Contrast (the CPU generator, whose
draws a trainer may replay on the device, is handed back to the host just before).  With
model.device_rng the sample S (exactly int(n_r rate) edges per type, by a sort of uniform keys), the random mask, the interaction
dropout and the permutation are drawn on the device and neither host generator moves.  What a step selected is kept on the model
(last_sample_ids, last_enc_keep, last_cl_keep, last_masked_ids, last_ui_keep, last_cl_ui_ids, last_rand_item, last_mess_masks) for tests
and diagnostics.  train.hip_graph is refused: the sizes of the masked sets change from step to step."""
import numpy as np
import torch as t
import torch.nn.functional as F
from torch import nn

from ... import ops
from ...config.configurator import configs
from ...graph import DroppedView, RelGraph, graph_of
from ..aug_utils import _pinned
from ..base_model import BaseModel


class AttnHGCN(nn.Module):
    """holds the reference AttnHGCN's parameters under its names and in its order (:33-42) and its message dropout"""

    def __init__(self, channel, n_hops, n_users, n_relations, node_dropout_rate=0.5, mess_dropout_rate=0.1):
        super().__init__()
        self.n_relations, self.n_users = n_relations, n_users
        self.node_dropout_rate, self.mess_dropout_rate = node_dropout_rate, mess_dropout_rate
        self.relation_emb = nn.Parameter(nn.init.xavier_uniform_(t.empty(n_relations - 1, channel)))
        self.W_Q = nn.Parameter(t.empty(channel, channel))
        self.n_heads = 2
        self.d_k = channel // self.n_heads
        nn.init.xavier_uniform_(self.W_Q)
        self.n_hops = n_hops
        self.dropout = nn.Dropout(p=mess_dropout_rate)
        self.last_masks = []

    def _drop(self, x):
        """nn.Dropout as a product with its own mask (0 or 1 / (1 - p)), which is kept: the same draw, the same bits"""
        if not self.training or self.mess_dropout_rate == 0:
            self.last_masks.append(None)
            return x
        mask = self.dropout(t.ones_like(x))
        self.last_masks.append(mask)
        return x * mask

    def forward(self, graph, user_emb, entity_emb, keep, interact, mess_dropout=True):
        """:92-119 (item_attn None); interact: table [n_entities, d] -> [n_users, d], the product with inter_edge_w"""
        entity_res_emb, user_res_emb = entity_emb, user_emb
        for _ in range(self.n_hops):
            entity_emb, user_emb = ops.attn_hgcn_aggregate(graph, entity_emb, self.W_Q, self.relation_emb, keep), interact(entity_emb)
            if mess_dropout:
                entity_emb, user_emb = self._drop(entity_emb), self._drop(user_emb)
            entity_emb = ops.normalize_add(t.zeros_like(entity_emb), entity_emb)
            user_emb = ops.normalize_add(t.zeros_like(user_emb), user_emb)
            entity_res_emb, user_res_emb = entity_res_emb + entity_emb, user_res_emb + user_emb
        return entity_res_emb, user_res_emb

    def forward_ui(self, user_emb, item_emb, to_users, to_items, mess_dropout=True):
        """:121-134; to_users: item table -> user_agg, to_items: user table -> item_agg (ui_agg :149-155)"""
        item_res_emb = item_emb
        for _ in range(self.n_hops):
            user_emb, item_emb = to_users(item_emb), to_items(user_emb)
            if mess_dropout:
                item_emb, user_emb = self._drop(item_emb), self._drop(user_emb)
            item_emb = ops.normalize_add(t.zeros_like(item_emb), item_emb)
            user_emb = ops.normalize_add(t.zeros_like(user_emb), user_emb)
            item_res_emb = item_res_emb + item_emb
        return item_res_emb

    def forward_kg(self, graph, entity_emb, keep, mess_dropout=True):
        """:136-147 with kg_agg (:157-163)"""
        entity_res_emb = entity_emb
        for _ in range(self.n_hops):
            entity_emb = ops.rel_aggregate(graph, entity_emb, self.relation_emb, keep)
            if mess_dropout:
                entity_emb = self._drop(entity_emb)
            entity_emb = ops.normalize_add(t.zeros_like(entity_emb), entity_emb)
            entity_res_emb = entity_res_emb + entity_emb
        return entity_res_emb

    @t.no_grad()
    def norm_attn_computer(self, graph, entity_emb, keep=None, return_logits=False):
        """:165-188 over a keep mask: the scores (and logits) by edge id of the graph, 0 off the mask"""
        score, logits, _, _ = ops.rel_rationale(graph, entity_emb @ self.W_Q, self.relation_emb, keep)
        return (score, logits) if return_logits else score


class Contrast(nn.Module):
    """:191-229"""

    def __init__(self, num_hidden, tau=0.7):
        super().__init__()
        self.tau = tau
        self.mlp1 = nn.Sequential(nn.Linear(num_hidden, num_hidden, bias=True), nn.ReLU(), nn.Linear(num_hidden, num_hidden, bias=True))
        self.mlp2 = nn.Sequential(nn.Linear(num_hidden, num_hidden, bias=True), nn.ReLU(), nn.Linear(num_hidden, num_hidden, bias=True))
        self.device_rng = False
        self.last_rand_item = None

    def sim(self, z1, z2):
        return t.mm(F.normalize(z1), F.normalize(z2).t())

    def self_sim(self, z1, z2):
        return (F.normalize(z1) * F.normalize(z2)).sum(1)

    def loss(self, z1, z2):
        f = lambda x: t.exp(x / self.tau)
        between_sim = f(self.self_sim(z1, z2))
        if self.device_rng and z1.is_cuda:
            rand_item = t.randperm(z1.shape[0], device=z1.device)
        else:
            from ...rng import flush_host_replay
            flush_host_replay()                              # `_sparse_dropout` drew from the replayed CPU generator: hand it back first
            rand_item = t.randperm(z1.shape[0]).to(z1.device)
        self.last_rand_item = rand_item
        neg_sim = f(self.self_sim(z1, z2[rand_item])) + f(self.self_sim(z2, z1[rand_item]))
        return -t.log(between_sim / (between_sim + between_sim + neg_sim))

    def forward(self, z1, z2):
        return self.loss(self.mlp1(z1), self.mlp2(z2)).mean()


def gumbel_like(x):
    """-log(-log(U)) with U = torch.rand_like(x) (:244, :421)"""
    return -t.log(-t.log(t.rand_like(x)))


class KGRec(BaseModel):
    def __init__(self, data_handler):
        if configs['train'].get('hip_graph'):
            raise NotImplementedError('train.hip_graph is not supported by KGRec: every step draws its edge sample on the host and the '
                                      'sizes of its masked edge sets change, which a captured step cannot follow')
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
        self.mae_coef = model_cfg['mae_coef']
        self.mae_msize = model_cfg['mae_msize']
        self.cl_coef = model_cfg['cl_coef']
        self.tau = model_cfg['tau']
        self.cl_drop = model_cfg['cl_drop_ratio']
        self.samp_func = model_cfg['samp_func']
        self.device_rng = bool(model_cfg.get('device_rng'))

        # the edge ids of every type, once: what `edge_type == i` selects in _relation_aware_edge_sampling (:260-262)
        edge_type = np.asarray(data_handler.kg_edges)[:, 2].astype(np.int64)
        self._type_ids = [np.nonzero(edge_type == i)[0] for i in range(self.n_relations - 1)]

        self.all_embed = nn.Parameter(nn.init.xavier_uniform_(t.empty(self.n_nodes, self.emb_size)))
        self.gcn = AttnHGCN(channel=self.emb_size, n_hops=self.context_hops, n_users=self.n_users, n_relations=self.n_relations,
                            node_dropout_rate=self.node_dropout_rate, mess_dropout_rate=self.mess_dropout_rate)
        self.contrast_fn = Contrast(self.emb_size, tau=self.tau)
        self.contrast_fn.device_rng = self.device_rng
        self.is_training = True
        self._eval_tables = None                                          # (user table, item table) of the current evaluation
        self.last_sample_ids = self.last_enc_keep = self.last_cl_keep = self.last_masked_ids = None
        self.last_ui_keep = self.last_cl_ui_ids = self.last_rand_item = self.last_mess_masks = None

    # -- the two graphs ----------------------------------------------------------------------------------------------------------------
    def _rel_graph(self, device):
        g = self.data_handler.rel_graph
        if g.device != device:                               # the handler built it for configs['device']: follow the tables
            g = self.data_handler.rel_graph = RelGraph(g.head, g.tail, g.rel, g.n, g.n_rel, device=device)
        return g

    def _interact_mat(self, device):
        adj = self.data_handler.interact_mat
        if adj.device != device:
            adj = self.data_handler.interact_mat = adj.to(device)
        return adj

    def _ui_products(self, table, keep, scale):
        """(to_users, to_items) of inter_edge_w restricted to the entries `keep` (None: all) and scaled: the [U, n_entities] matrix
        D^-1 A times an entity table, and its transpose times a user table"""
        adj = self._interact_mat(table.device)
        if table.is_cuda:
            graph = graph_of(adj)
            fwd = graph if keep is None else DroppedView(graph, keep, scale)
            bwd = graph.transposed() if keep is None else DroppedView(graph.transposed(), keep, scale)
            return (lambda x: ops.spmm(fwd, x)), (lambda x: ops.spmm(bwd, x))
        # host tensors: the reference's statements (the tests' float64 runs use them)
        idx, val = adj._indices(), adj._values()
        if keep is not None:
            idx, val = idx[:, keep], val[keep]
        mat = t.sparse_coo_tensor(idx, val.to(table.dtype) * scale, adj.shape)
        mat_t = mat.t().coalesce()
        return (lambda x: t.sparse.mm(mat, x)), (lambda x: t.sparse.mm(mat_t, x))

    # -- the draws ---------------------------------------------------------------------------------------------------------------------
    def _sample_ids(self, rate, device):
        """`_relation_aware_edge_sampling` (:258-271): the ORIGINAL edge ids in the reference's concatenation order, int64 on `device`"""
        if self.device_rng and device.type == 'cuda':
            graph = self._rel_graph(device)
            sizes = t.tensor([int(ids.size * rate) if 0 < i else 0 for i, ids in enumerate(self._type_ids)] + [0], device=device)
            typ = graph.rel + 1                                                    # the stored type of every edge
            order = t.argsort(typ.double() + t.rand(graph.n_edges, device=device, dtype=t.float64))       # by type, random inside one
            starts = t.cumsum(t.bincount(typ, minlength=self.n_relations), 0) - t.bincount(typ, minlength=self.n_relations)
            typ_sorted = typ[order]
            rank = t.arange(graph.n_edges, device=device) - starts[typ_sorted]
            return order[rank < sizes[typ_sorted]]
        ids = []
        for of_type in self._type_ids:
            n_edges = of_type.size
            random_indices = np.random.choice(n_edges, size=int(n_edges * rate), replace=False)
            ids.append(of_type[random_indices])
        return t.from_numpy(np.concatenate(ids)).to(device)

    def _random_positions(self, n, size, device):
        """the second group of `_mae_edge_mask_adapt_mixed` (:282-283)"""
        if self.device_rng and device.type == 'cuda':
            return t.randperm(n, device=device)[:size]
        return t.from_numpy(np.random.choice(n, size=size, replace=False)).to(device)

    def _ui_keep(self, nnz, device):
        """the keep flags of `_sparse_dropout` (:305-311), literally: floor(keep_rate + rand) per stored entry, bool [nnz] on `device`"""
        keep_rate = 1 - self.node_dropout_rate
        draw = t.rand(nnz, device=device) if self.device_rng and device.type == 'cuda' else _pinned.rand_to((nnz,), device)
        return (draw + keep_rate).floor().type(t.bool)

    def _adaptive_ui_drop_cl(self, item_attn_mean, ui_keep, keep_rate):
        """:241-255: the entry ids (of the full interaction matrix) of the contrastive view, drawn among the kept entries"""
        adj = self._interact_mat(item_attn_mean.device)
        kept_ids = t.nonzero(ui_keep).reshape(-1)
        inter_attn_prob = item_attn_mean[adj._indices()[1][kept_ids]]
        inter_attn_prob = inter_attn_prob + gumbel_like(inter_attn_prob)
        inter_attn_prob = F.softmax(inter_attn_prob, dim=0)
        size = int(keep_rate * kept_ids.numel())
        if self.samp_func == 'np':
            picked = np.random.choice(np.arange(kept_ids.numel()), size=size, replace=False, p=inter_attn_prob.cpu().numpy())
            picked = t.from_numpy(picked).to(kept_ids.device)
        else:
            picked = t.multinomial(inter_attn_prob, size, replacement=False)
        return kept_ids[picked]

    # -- the step ----------------------------------------------------------------------------------------------------------------------
    def cal_loss(self, batch_data):
        self.is_training = True
        self._eval_tables = None
        user, pos_item, neg_item = batch_data[:3]
        device = self.all_embed.device
        graph = self._rel_graph(device)
        E = graph.n_edges
        user_emb, item_emb = self.all_embed[:self.n_users, :], self.all_embed[self.n_users:, :]
        self.gcn.last_masks = []
        keep_rate = 1 - self.node_dropout_rate

        # 1. graph sparsification: S as a mask, its edges in the reference's order as ids
        sample_ids = self._sample_ids(keep_rate, device)
        n_s = sample_ids.numel()
        s_keep = t.zeros(E, dtype=t.uint8, device=device)
        s_keep[sample_ids] = 1
        # 2. rationale scores, and their means per entity for the interaction view (:411-418)
        score, _, mean_1, mean_2 = ops.rel_rationale(graph, item_emb.detach() @ self.gcn.W_Q.detach(), self.gcn.relation_emb.detach(), s_keep)
        one = t.ones((), dtype=mean_1.dtype, device=device)
        item_attn_mean = (0.5 * t.where(mean_1 == 0., one, mean_1) + 0.5 * t.where(mean_2 == 0., one, mean_2))[:self.n_items]
        # the masked set of the MAE task: the top scores under Gumbel noise and as many random positions (:420-427)
        edge_attn_score = score[sample_ids]
        edge_attn_score = edge_attn_score + gumbel_like(edge_attn_score)
        topk_pos = t.topk(edge_attn_score, self.mae_msize, sorted=False)[1]
        rand_pos = self._random_positions(n_s, self.mae_msize, device)
        mask_bool = t.zeros(n_s, dtype=t.bool, device=device)
        mask_bool[topk_pos] = True
        mask_bool[rand_pos] = True
        masked_ids = sample_ids[mask_bool]
        enc_keep = s_keep.clone()
        enc_keep[masked_ids] = 0

        nnz = self._interact_mat(device)._nnz()
        ui_keep = self._ui_keep(nnz, device)
        to_users, _ = self._ui_products(item_emb, ui_keep, 1. / keep_rate)

        # rec task
        entity_gcn_emb, user_gcn_emb = self.gcn(graph, user_emb, item_emb, enc_keep, to_users, mess_dropout=self.mess_dropout)
        loss, rec_loss, reg_loss = self.create_bpr_loss(user_gcn_emb[user], entity_gcn_emb[pos_item], entity_gcn_emb[neg_item])

        # MAE task with dot-product decoder: the masked edges by plain gathers
        node_pair_emb = t.stack([entity_gcn_emb[graph.head[masked_ids]], entity_gcn_emb[graph.tail[masked_ids]]], dim=1)
        masked_edge_emb = self.gcn.relation_emb[graph.rel[masked_ids]]
        mae_loss = self.mae_coef * self.create_mae_loss(node_pair_emb, masked_edge_emb)

        # CL task: S minus the least scored (by the noisy score), the interaction view by its scores (:456-465)
        cl_rate = 1 - self.cl_drop
        least = t.topk(-edge_attn_score, int((1 - cl_rate) * n_s), sorted=False)[1]
        cl_keep = s_keep.clone()
        cl_keep[sample_ids[least]] = 0
        cl_ui_ids = self._adaptive_ui_drop_cl(item_attn_mean, ui_keep, cl_rate)
        cl_ui_keep = t.zeros(nnz, dtype=t.bool, device=device)
        cl_ui_keep[cl_ui_ids] = True
        cl_to_users, cl_to_items = self._ui_products(item_emb, cl_ui_keep, 1. / keep_rate / cl_rate)
        pad = t.zeros(self.n_entities - self.n_items, self.emb_size, dtype=item_emb.dtype, device=device)
        item_agg_ui = self.gcn.forward_ui(user_emb, item_emb[:self.n_items],
                                          lambda items: cl_to_users(t.cat([items, pad], dim=0)), lambda users: cl_to_items(users)[:self.n_items])
        item_agg_kg = self.gcn.forward_kg(graph, item_emb, cl_keep)[:self.n_items]
        cl_loss = self.cl_coef * self.contrast_fn(item_agg_ui, item_agg_kg)

        self.last_sample_ids, self.last_enc_keep, self.last_cl_keep, self.last_masked_ids = sample_ids, enc_keep, cl_keep, masked_ids
        self.last_ui_keep, self.last_cl_ui_ids, self.last_rand_item = ui_keep, cl_ui_ids, self.contrast_fn.last_rand_item
        self.last_mess_masks = self.gcn.last_masks
        return loss + mae_loss + cl_loss, {'rec_loss': loss.detach(), 'mae_loss': mae_loss.detach(), 'cl_loss': cl_loss.detach()}

    def create_bpr_loss(self, users, pos_items, neg_items):
        """:507-523"""
        batch_size = users.shape[0]
        pos_scores = t.sum(t.mul(users, pos_items), dim=1)
        neg_scores = t.sum(t.mul(users, neg_items), dim=1)
        mf_loss = -1 * t.mean(F.logsigmoid(pos_scores - neg_scores))
        regularizer = (t.norm(users) ** 2 + t.norm(pos_items) ** 2 + t.norm(neg_items) ** 2) / 2
        emb_loss = self.decay * regularizer / batch_size
        return mf_loss + emb_loss, mf_loss, emb_loss

    def create_mae_loss(self, node_pair_emb, masked_edge_emb=None):
        """:525-534"""
        head_embs, tail_embs = node_pair_emb[:, 0, :], node_pair_emb[:, 1, :]
        pos1 = tail_embs * masked_edge_emb if masked_edge_emb is not None else tail_embs
        return -t.log(t.sigmoid(t.mul(pos1, head_embs).sum(1))).mean()

    def generate(self):
        """(user table, item table) over the full graphs without message dropout (:485-495)"""
        user_emb, item_emb = self.all_embed[:self.n_users, :], self.all_embed[self.n_users:, :]
        to_users, _ = self._ui_products(item_emb, None, 1.0)
        entity_emb, user_emb = self.gcn(self._rel_graph(item_emb.device), user_emb, item_emb, None, to_users, mess_dropout=False)
        return user_emb, entity_emb[:self.n_items]

    def rating(self, u_emb, i_emb):
        return t.matmul(u_emb, i_emb.t())

    def generate_global_attn_score(self):
        """:567-574: (scores by edge id, edge_index [2, E], edge_type [E]) over the whole graph"""
        item_emb = self.all_embed[self.n_users:, :]
        graph = self._rel_graph(item_emb.device)
        return self.gcn.norm_attn_computer(graph, item_emb), t.stack([graph.head, graph.tail]), graph.rel + 1

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
