"""CPU restatement of the reference's KGIN (models/kg/kgin.py: Aggregator :23-48, GraphConv.forward :160-187, _cul_cor :105-158,
create_loss :321-335), shared by test_kgin_host.py and test_kgin.py (test infrastructure, no tests of its own).  Every torch function
takes any dtype: the float64 run is the yardstick, the float32 run measures what fp32 arithmetic costs (tests/mhcn_reference.py's
convention: max|x - ref64| / max|ref64| per tensor, the kernels at most 4 x the fp32 restatement's error, floor 8 * 2^-23).

Written from the formulas: scatter_mean is index_add_ divided by the clamped count (there is no torch_scatter), the edge sample and the
sparse-dropout flags are handed in as masks instead of drawn, the [U, F, d] expansion of the reference is kept."""
import numpy as np
import torch
import torch.nn.functional as F

from mhcn_reference import FLOOR, both_precisions, check, leaf, randn, rel_err  # noqa: F401  (the shared helper conventions)


# ---- Aggregator ----------------------------------------------------------------------------------------------------
def scatter_mean(src, index, dim_size):
    """mean of the rows of src [E, d] per index value; 0 where no row carries the value"""
    total = torch.zeros(dim_size, src.shape[1], dtype=src.dtype).index_add_(0, index, src)
    count = torch.zeros(dim_size, dtype=src.dtype).index_add_(0, index, torch.ones(index.numel(), dtype=src.dtype))
    return total / count.clamp(min=1).unsqueeze(1)


def kg_aggregate(entity_emb, weight, head, tail, rel, keep=None):
    """:33-36 with rel = edge_type - 1 and the edge sample as a mask over the edges"""
    if keep is not None:
        sel = keep.bool()
        head, tail, rel = head[sel], tail[sel], rel[sel]
    neigh = entity_emb[tail] * weight[rel]
    return scatter_mean(neigh, head, entity_emb.shape[0])


def factor_modulate(user_agg, user_emb, latent_emb, disen_weight):
    """:38-46 from user_agg = interact_mat @ entity_emb and disen_weight = softmax(disen_weight_att) @ weight, expansion included"""
    n_users, channel = user_agg.shape
    n_factors = latent_emb.shape[0]
    score = torch.softmax(user_emb @ latent_emb.t(), dim=1).unsqueeze(-1)
    expanded = disen_weight.expand(n_users, n_factors, channel)
    return user_agg * (expanded * score).sum(dim=1) + user_agg


def aggregator(entity_emb, user_emb, latent_emb, edges, keep, interact, weight, disen_weight_att):
    head, tail, rel = edges
    entity_agg = kg_aggregate(entity_emb, weight, head, tail, rel, keep)
    disen_weight = torch.softmax(disen_weight_att, dim=-1) @ weight
    user_agg = factor_modulate(interact @ entity_emb, user_emb, latent_emb, disen_weight)
    return entity_agg, user_agg


# ---- _cul_cor ------------------------------------------------------------------------------------------------------
def _distance_correlation(t1, t2):
    channel = t1.shape[0]
    zeros = torch.zeros(channel, channel, dtype=t1.dtype)
    zero = torch.zeros(1, dtype=t1.dtype)
    t1, t2 = t1.unsqueeze(-1), t2.unsqueeze(-1)
    a_, b_ = (t1 @ t1.t()) * 2, (t2 @ t2.t()) * 2
    s1, s2 = t1 ** 2, t2 ** 2
    a = torch.sqrt(torch.max(s1 - a_ + s1.t(), zeros) + 1e-8)
    b = torch.sqrt(torch.max(s2 - b_ + s2.t(), zeros) + 1e-8)
    A = a - a.mean(dim=0, keepdim=True) - a.mean(dim=1, keepdim=True) + a.mean()
    B = b - b.mean(dim=0, keepdim=True) - b.mean(dim=1, keepdim=True) + b.mean()
    dcov_AB = torch.sqrt(torch.max((A * B).sum() / channel ** 2, zero) + 1e-8)
    dcov_AA = torch.sqrt(torch.max((A * A).sum() / channel ** 2, zero) + 1e-8)
    dcov_BB = torch.sqrt(torch.max((B * B).sum() / channel ** 2, zero) + 1e-8)
    return (dcov_AB / torch.sqrt(dcov_AA * dcov_BB + 1e-8)).reshape(())


def _cosine_sq(t1, t2):
    n1 = t1 / t1.norm(dim=0, keepdim=True)
    n2 = t2 / t2.norm(dim=0, keepdim=True)
    return (n1 * n2).sum(dim=0) ** 2


def _mutual_information(att, temperature=0.2):
    disen_T = att.t()
    normed = disen_T / disen_T.norm(dim=1, keepdim=True)
    pos = torch.exp(torch.sum(normed * normed, dim=1) / temperature)
    ttl = torch.exp(torch.sum(disen_T @ att, dim=1) / temperature)
    return -torch.sum(torch.log(pos / ttl))


def cul_cor(att, ind):
    if ind == 'mi':
        return _mutual_information(att)
    cor = 0
    n_factors = att.shape[0]
    for i in range(n_factors):
        for j in range(i + 1, n_factors):
            cor = cor + (_distance_correlation(att[i], att[j]) if ind == 'distance' else _cosine_sq(att[i], att[j]))
    return cor


# ---- GraphConv.forward, create_loss ---------------------------------------------------------------------------------
def graph_conv(p, n_users, edges, keep, interact, n_hops, ind, mess_masks=None):
    """p: name -> tensor (all_embed, latent_emb, gcn.weight, gcn.disen_weight_att); edges = (head, tail, rel) int64 with rel =
    edge_type - 1; keep: the edge sample as a mask or None; interact: the [U, N] matrix AFTER `_sparse_dropout` (dense or sparse, of
    p's dtype); mess_masks: per hop (entity mask, user mask) already scaled by 1 / (1 - p), or None for no message dropout"""
    user_emb, entity_emb = p['all_embed'][:n_users], p['all_embed'][n_users:]
    entity_res, user_res = entity_emb, user_emb
    cor = cul_cor(p['gcn.disen_weight_att'], ind)
    for hop in range(n_hops):
        entity_emb, user_emb = aggregator(entity_emb, user_emb, p['latent_emb'], edges, keep, interact, p['gcn.weight'], p['gcn.disen_weight_att'])
        if mess_masks is not None:
            entity_emb, user_emb = entity_emb * mess_masks[hop][0], user_emb * mess_masks[hop][1]
        entity_emb, user_emb = F.normalize(entity_emb), F.normalize(user_emb)
        entity_res, user_res = entity_res + entity_emb, user_res + user_emb
    return entity_res, user_res, cor


def create_loss(users, pos_items, neg_items, cor, decay, sim_decay):
    batch_size = users.shape[0]
    pos_scores = (users * pos_items).sum(dim=1)
    neg_scores = (users * neg_items).sum(dim=1)
    mf_loss = -1 * torch.mean(F.logsigmoid(pos_scores - neg_scores))
    regularizer = (torch.norm(users) ** 2 + torch.norm(pos_items) ** 2 + torch.norm(neg_items) ** 2) / 2
    emb_loss = decay * regularizer / batch_size
    return mf_loss + emb_loss + sim_decay * cor, mf_loss, emb_loss, cor


def model_loss(p, n_users, edges, keep, interact, n_hops, ind, batch, decay, sim_decay, mess_masks=None):
    entity_res, user_res, cor = graph_conv(p, n_users, edges, keep, interact, n_hops, ind, mess_masks)
    user, pos, neg = batch
    loss, mf, emb, cor = create_loss(user_res[user], entity_res[pos], entity_res[neg], cor, decay, sim_decay)
    return {'user': user_res, 'entity': entity_res, 'loss': loss, 'rec_loss': mf, 'reg_loss': emb, 'cor': cor}


def sparse_dropout_dense(interact_coo, ui_keep, rate, dt):
    """the dense [U, N] matrix `_sparse_dropout` (:90-103) leaves: the kept entries times 1 / (1 - rate); ui_keep None = no dropout"""
    idx, val = interact_coo._indices(), interact_coo._values().to(dt)
    if ui_keep is not None:
        idx, val = idx[:, ui_keep], val[ui_keep] * (1. / (1 - rate))
    return torch.sparse_coo_tensor(idx, val, interact_coo.shape).to_dense()


PARAM_NAMES = ['all_embed', 'latent_emb', 'gcn.weight', 'gcn.disen_weight_att']


def draw_params(n_nodes, d, n_factors, n_relations, seed):
    """the parameters in the reference constructors' order (:233-236, then :71-76) after torch.manual_seed(seed)"""
    torch.manual_seed(seed)
    init = torch.nn.init.xavier_uniform_
    return {'all_embed': init(torch.empty(n_nodes, d)), 'latent_emb': init(torch.empty(n_factors, d)),
            'gcn.weight': init(torch.empty(n_relations - 1, d)), 'gcn.disen_weight_att': init(torch.empty(n_factors, n_relations - 1))}


def edge_sample_mask(n_edges, rate):
    """`_edge_sampling`'s draw (:87) as a mask over the edges"""
    keep = np.zeros(n_edges, dtype=bool)
    keep[np.random.choice(n_edges, size=int(n_edges * rate), replace=False)] = True
    return keep


def sparse_dropout_flags(nnz, rate):
    """`_sparse_dropout`'s draw (:93-95)"""
    random_tensor = rate
    random_tensor += torch.rand(nnz)
    return torch.floor(random_tensor).type(torch.bool)
