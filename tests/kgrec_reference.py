"""CPU restatement of the reference's KGRec (models/kg/kgrec.py: AttnHGCN.shared_layer_agg :63-88, non_attn_agg / kg_agg :48-61 :157-163,
ui_agg :149-155, forward :92-119, forward_ui :121-134, forward_kg :136-147, norm_attn_computer :165-188, Contrast :191-229, cal_loss
:398-472, create_bpr_loss :507-523, create_mae_loss :525-534), shared by test_kgrec_host.py, test_kgrec.py and test_kgrec_walk_edges.py
(test infrastructure, no tests of its own).  Every torch function takes any dtype: the float64 run is the yardstick, the float32 run
measures what fp32 arithmetic costs (tests/mhcn_reference.py's convention: max|x - ref64| / max|ref64| per tensor, the kernels at most
4 x the fp32 restatement's error, floor 8 * 2^-23).

Written from the formulas: the reference itself needs torch_scatter and torch_geometric.  scatter_softmax is exp(e - max of the head)
over an index_add_ of the same, scatter_sum is index_add_, scatter_mean an index_add_ over the clamped count; the edge samples, the
sparse-dropout flags, the message-dropout masks and Contrast's permutation are handed in instead of drawn.  Edges are (head, tail, rel)
int64 with rel = edge_type - 1, so relation_emb is indexed by rel itself."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from kgcl_reference import _kept, head_max, scatter_softmax, scatter_sum  # noqa: F401
from mhcn_reference import FLOOR, both_precisions, check, leaf, randn, rel_err  # noqa: F401  (the shared helper conventions)

N_HEADS = 2


def scatter_mean(src, index, dim_size):
    """torch_scatter.scatter_mean: the sum over the clamped count; src [E] or [E, d]"""
    out = torch.zeros((dim_size,) + tuple(src.shape[1:]), dtype=src.dtype).index_add_(0, index, src)
    cnt = torch.zeros(dim_size, dtype=src.dtype).index_add_(0, index, torch.ones(index.numel(), dtype=src.dtype)).clamp(min=1)
    return out / (cnt if src.dim() == 1 else cnt.unsqueeze(1))


def scatter_softmax_heads(e, index, dim_size):
    """torch_geometric.utils.softmax of e [E, heads] over `index`, column by column"""
    return torch.stack([scatter_softmax(e[:, a], index, dim_size) for a in range(e.shape[1])], dim=1)


# ---- AttnHGCN ------------------------------------------------------------------------------------------------------
def shared_layer_agg_kg(entity_emb, w_q, relation_emb, edges, keep=None):
    """:63-82, literally: the [E, d] gathers through `@ W_Q`"""
    head, tail, rel = _kept(edges, keep)
    n_entities, d = entity_emb.shape
    d_k = d // N_HEADS
    query = (entity_emb[head] @ w_q).view(-1, N_HEADS, d_k)
    key = (entity_emb[tail] @ w_q).view(-1, N_HEADS, d_k)
    key = key * relation_emb[rel].view(-1, N_HEADS, d_k)
    edge_attn_score = (query * key).sum(dim=-1) / math.sqrt(d_k)
    neigh_relation_emb = entity_emb[tail] * relation_emb[rel]
    value = neigh_relation_emb.view(-1, N_HEADS, d_k)
    edge_attn_score = scatter_softmax_heads(edge_attn_score, head, n_entities)
    entity_agg = (value * edge_attn_score.view(-1, N_HEADS, 1)).view(-1, N_HEADS * d_k)
    return scatter_sum(entity_agg, head, n_entities)


def rel_mh_attention(x, t, r, edges, keep=None):
    """the contract of ops.rel_mh_attention: the same lines with the node table t in place of `entity_emb[.] @ W_Q`"""
    head, tail, rel = _kept(edges, keep)
    n, d = x.shape
    d_k = d // N_HEADS
    key = t[tail].view(-1, N_HEADS, d_k) * r[rel].view(-1, N_HEADS, d_k)
    score = (t[head].view(-1, N_HEADS, d_k) * key).sum(dim=-1) / math.sqrt(d_k)
    score = scatter_softmax_heads(score, head, n)
    value = (x[tail] * r[rel]).view(-1, N_HEADS, d_k)
    return scatter_sum((value * score.view(-1, N_HEADS, 1)).view(-1, d), head, n)


def mh_logits(t, r, edges, keep=None):
    """[E', 2]: the two logits of every kept edge"""
    head, tail, rel = _kept(edges, keep)
    d_k = t.shape[1] // N_HEADS
    key = t[tail].view(-1, N_HEADS, d_k) * r[rel].view(-1, N_HEADS, d_k)
    return (t[head].view(-1, N_HEADS, d_k) * key).sum(dim=-1) / math.sqrt(d_k)


def norm_attn_computer(entity_emb, w_q, relation_emb, edges, keep=None):
    """:165-188 over the kept edges: (edge_attn_score, edge_attn_logits), both [E']"""
    head, tail, rel = _kept(edges, keep)
    d_k = entity_emb.shape[1] // N_HEADS
    query = (entity_emb[head] @ w_q).view(-1, N_HEADS, d_k)
    key = (entity_emb[tail] @ w_q).view(-1, N_HEADS, d_k)
    key = key * relation_emb[rel].view(-1, N_HEADS, d_k)
    edge_attn = (query * key).sum(dim=-1) / math.sqrt(d_k)
    edge_attn_logits = edge_attn.mean(-1).detach()
    edge_attn_score = scatter_softmax(edge_attn_logits, head, entity_emb.shape[0])
    norm = torch.zeros(entity_emb.shape[0], dtype=torch.int64).index_add_(0, head, torch.ones_like(head))
    return edge_attn_score * norm[head], edge_attn_logits


def rel_rationale(t, r, edges, keep=None):
    """the contract of ops.rel_rationale: (score [E], logits [E], mean_head [N], mean_tail [N]), 0 off the mask"""
    head, tail, rel = _kept(edges, keep)
    n, E = t.shape[0], edges[0].numel()
    lbar = mh_logits(t, r, edges, keep).mean(-1)
    cnt = torch.zeros(n, dtype=torch.int64).index_add_(0, head, torch.ones_like(head))
    sc = scatter_softmax(lbar, head, n) * cnt[head]
    sel = torch.ones(E, dtype=torch.bool) if keep is None else keep.bool()
    score, logits = torch.zeros(E, dtype=t.dtype), torch.zeros(E, dtype=t.dtype)
    score[sel], logits[sel] = sc, lbar
    return score, logits, scatter_mean(sc, head, n), scatter_mean(sc, tail, n)


def kg_agg(entity_emb, relation_emb, edges, keep=None):
    """:157-163 (and the entity side of non_attn_agg :48-56)"""
    head, tail, rel = _kept(edges, keep)
    return scatter_mean(entity_emb[tail] * relation_emb[rel], head, entity_emb.shape[0])


def ui_agg(user_emb, item_emb, a):
    """:149-155 with the [U, I] matrix `a` of the edge weights: (user_agg, item_agg)"""
    return a @ item_emb, a.t() @ user_emb


def _drop(x, mask):
    return x if mask is None else x * mask


def gcn_forward(user_emb, entity_emb, w_q, relation_emb, edges, keep, a, n_hops, masks=None):
    """:92-119 (item_attn None); a: the [U, n_entities] matrix of inter_edge_w; masks: per hop (entity mask, user mask) already scaled by
    1 / (1 - p), or None"""
    entity_res_emb, user_res_emb = entity_emb, user_emb
    for hop in range(n_hops):
        entity_emb, user_emb = shared_layer_agg_kg(entity_emb, w_q, relation_emb, edges, keep), a @ entity_emb
        if masks is not None:
            entity_emb, user_emb = _drop(entity_emb, masks[hop][0]), _drop(user_emb, masks[hop][1])
        entity_emb, user_emb = F.normalize(entity_emb), F.normalize(user_emb)
        entity_res_emb, user_res_emb = torch.add(entity_res_emb, entity_emb), torch.add(user_res_emb, user_emb)
    return entity_res_emb, user_res_emb


def forward_ui(user_emb, item_emb, a, n_hops, masks=None):
    """:121-134; masks: per hop (item mask, user mask)"""
    item_res_emb = item_emb
    for hop in range(n_hops):
        user_emb, item_emb = ui_agg(user_emb, item_emb, a)
        if masks is not None:
            item_emb, user_emb = _drop(item_emb, masks[hop][0]), _drop(user_emb, masks[hop][1])
        item_emb, user_emb = F.normalize(item_emb), F.normalize(user_emb)
        item_res_emb = torch.add(item_res_emb, item_emb)
    return item_res_emb


def forward_kg(entity_emb, relation_emb, edges, keep, n_hops, masks=None):
    """:136-147; masks: per hop an entity mask"""
    entity_res_emb = entity_emb
    for hop in range(n_hops):
        entity_emb = kg_agg(entity_emb, relation_emb, edges, keep)
        if masks is not None:
            entity_emb = _drop(entity_emb, masks[hop])
        entity_emb = F.normalize(entity_emb)
        entity_res_emb = torch.add(entity_res_emb, entity_emb)
    return entity_res_emb


# ---- Contrast and the losses -----------------------------------------------------------------------------------------
def _mlp(p, prefix, z):
    return F.linear(F.relu(F.linear(z, p[prefix + '.0.weight'], p[prefix + '.0.bias'])), p[prefix + '.2.weight'], p[prefix + '.2.bias'])


def contrast(p, z1, z2, rand_item, tau):
    """:207-229 with the permutation handed in"""
    h1, h2 = _mlp(p, 'contrast_fn.mlp1', z1), _mlp(p, 'contrast_fn.mlp2', z2)

    def self_sim(a, b):
        return (F.normalize(a) * F.normalize(b)).sum(1)

    def f(x):
        return torch.exp(x / tau)
    between_sim = f(self_sim(h1, h2))
    neg_sim = f(self_sim(h1, h2[rand_item])) + f(self_sim(h2, h1[rand_item]))
    return (-torch.log(between_sim / (between_sim + between_sim + neg_sim))).mean()


def bpr_loss(users, pos_items, neg_items, decay):
    """:507-523: (loss, mf_loss, emb_loss)"""
    batch_size = users.shape[0]
    pos_scores = torch.sum(torch.mul(users, pos_items), axis=1)
    neg_scores = torch.sum(torch.mul(users, neg_items), axis=1)
    mf_loss = -1 * torch.mean(F.logsigmoid(pos_scores - neg_scores))
    regularizer = (torch.norm(users) ** 2 + torch.norm(pos_items) ** 2 + torch.norm(neg_items) ** 2) / 2
    emb_loss = decay * regularizer / batch_size
    return mf_loss + emb_loss, mf_loss, emb_loss


def mae_loss(head_embs, tail_embs, masked_edge_emb):
    """:525-534"""
    return -torch.log(torch.sigmoid(torch.mul(tail_embs * masked_edge_emb, head_embs).sum(1))).mean()


def model_loss(p, sizes, edges, sel, mats, batch, hp, masks=None):
    """:398-472 over handed-in selections.  p: name -> tensor; sizes = (n_users, n_items); edges = (head, tail, rel) of the whole graph;
    sel = {'enc_keep', 'cl_keep' bool [E], 'masked_ids' int64 (edge ids sent to the MAE loss), 'rand_item' int64 [n_items]};
    mats = (the [U, n_entities] matrix after `_sparse_dropout`, the [U, n_items] matrix of the contrastive view);
    hp = {'layer_num', 'decay', 'mae_coef', 'cl_coef', 'tau'}; masks = None or {'gcn': ..., 'ui': ..., 'kg': ...} per hop"""
    n_users, n_items = sizes
    user, pos_item, neg_item = batch
    head, tail, rel = edges
    masks = masks or {}
    user_emb, item_emb = p['all_embed'][:n_users], p['all_embed'][n_users:]
    w_q, relation_emb = p['gcn.W_Q'], p['gcn.relation_emb']
    entity_gcn_emb, user_gcn_emb = gcn_forward(user_emb, item_emb, w_q, relation_emb, edges, sel['enc_keep'], mats[0], hp['layer_num'],
                                               masks.get('gcn'))
    loss, rec_loss, reg_loss = bpr_loss(user_gcn_emb[user], entity_gcn_emb[pos_item], entity_gcn_emb[neg_item], hp['decay'])
    m = sel['masked_ids']
    mae = hp['mae_coef'] * mae_loss(entity_gcn_emb[head[m]], entity_gcn_emb[tail[m]], relation_emb[rel[m]])
    item_agg_ui = forward_ui(user_emb, item_emb[:n_items], mats[1], hp['layer_num'], masks.get('ui'))
    item_agg_kg = forward_kg(item_emb, relation_emb, edges, sel['cl_keep'], hp['layer_num'], masks.get('kg'))[:n_items]
    cl = hp['cl_coef'] * contrast(p, item_agg_ui, item_agg_kg, sel['rand_item'], hp['tau'])
    return {'loss': loss + mae + cl, 'rec_loss': loss, 'mae_loss': mae, 'cl_loss': cl}


# ---- the draws -----------------------------------------------------------------------------------------------------------
def relation_aware_edge_sampling(edge_type, n_relations, samp_rate):
    """`_relation_aware_edge_sampling` (:258-271) with `_edge_sampling` (:296-302): the ORIGINAL edge ids in the reference's
    concatenation order.  edge_type int64 numpy [E], the types as stored (1 .. n_relations - 1); the loop runs i = 0 .. n_relations - 2."""
    ids = []
    for i in range(n_relations - 1):
        of_type = np.nonzero(edge_type == i)[0]
        n_edges = of_type.size
        random_indices = np.random.choice(n_edges, size=int(n_edges * samp_rate), replace=False)
        ids.append(of_type[random_indices])
    return np.concatenate(ids) if ids else np.zeros(0, dtype=np.int64)


PARAM_NAMES = ['all_embed', 'gcn.relation_emb', 'gcn.W_Q'] + ['contrast_fn.%s.%d.%s' % (m, i, w) for m in ('mlp1', 'mlp2') for i in (0, 2)
                                                               for w in ('weight', 'bias')]


def draw_params(n_nodes, n_relations, d, seed):
    """the parameters in the reference constructors' order (:367-369, :33-42, :196-205) after torch.manual_seed(seed)"""
    torch.manual_seed(seed)
    init = torch.nn.init.xavier_uniform_
    p = {'all_embed': init(torch.empty(n_nodes, d)), 'gcn.relation_emb': init(torch.empty(n_relations - 1, d)),
         'gcn.W_Q': init(torch.empty(d, d))}
    for m in ('mlp1', 'mlp2'):
        for i in (0, 2):
            lin = torch.nn.Linear(d, d, bias=True)
            p['contrast_fn.%s.%d.weight' % (m, i)], p['contrast_fn.%s.%d.bias' % (m, i)] = lin.weight.detach(), lin.bias.detach()
    return p
