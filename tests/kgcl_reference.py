"""CPU restatement of the reference's KGCL (models/kg/kgcl.py: RGAT.agg :60-72, RGAT.forward :74-84, KGCL.forward :286-301, _bpr_loss
:316-321 with loss_utils.cal_bpr_loss, _infonce_overall :351-371, _get_ui_aug_views :200-228, _get_norm_adj_mat :140-185), shared by
test_kgcl_host.py and test_kgcl.py (test infrastructure, no tests of its own).  Every torch function takes any dtype: the float64 run is
the yardstick, the float32 run measures what fp32 arithmetic costs (tests/mhcn_reference.py's convention: max|x - ref64| / max|ref64| per
tensor, the kernels at most 4 x the fp32 restatement's error, floor 8 * 2^-23).

Written from the formulas: scatter_softmax is exp(e - max of the head) over an index_add_ of the same, scatter_sum is index_add_ (there
is no torch_scatter); the edge samples, the sparse-dropout flags and the message-dropout masks are handed in instead of drawn."""
import random

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn.functional as F

from mhcn_reference import FLOOR, both_precisions, check, leaf, randn, rel_err  # noqa: F401  (the shared helper conventions)

SLOPE = 0.2
TAU, CL_WEIGHT, MU = 0.2, 0.1, 0.95


# ---- RGAT ----------------------------------------------------------------------------------------------------------
def head_max(e, index, dim_size):
    """per-head maximum of e (a constant of the softmax), vectorised: sort by (head, e) and take each head's last"""
    mx = torch.full((dim_size,), float('-inf'), dtype=e.dtype)
    if index.numel():
        order = np.lexsort((e.detach().numpy(), index.numpy()))
        idx_sorted = index.numpy()[order]
        last = np.nonzero(np.append(idx_sorted[1:] != idx_sorted[:-1], True))[0]
        mx[torch.from_numpy(idx_sorted[last])] = e.detach()[torch.from_numpy(order[last])]
    return mx


def scatter_softmax(e, index, dim_size):
    ex = torch.exp(e - head_max(e, index, dim_size)[index])
    total = torch.zeros(dim_size, dtype=e.dtype).index_add_(0, index, ex)
    return ex / total[index]


def scatter_sum(src, index, dim_size):
    return torch.zeros(dim_size, src.shape[1], dtype=src.dtype).index_add_(0, index, src)


def _kept(edges, keep):
    head, tail, rel = edges
    if keep is not None:
        sel = keep.bool()
        head, tail, rel = head[sel], tail[sel], rel[sel]
    return head, tail, rel


def rgat_agg(entity_emb, relation_emb, fc_weight, fc_bias, edges, keep=None):
    """:60-72, literally: the [E, 2 d] concatenation through fc; edges = (head, tail, rel) int64 with relation_emb indexed by rel"""
    head, tail, rel = _kept(edges, keep)
    a_input = torch.cat([entity_emb[head], entity_emb[tail]], dim=-1)
    e_input = torch.multiply(F.linear(a_input, fc_weight, fc_bias), relation_emb[rel]).sum(-1)
    e = F.leaky_relu(e_input, SLOPE)
    e = scatter_softmax(e, head, entity_emb.shape[0])
    return scatter_sum(entity_emb[tail] * e.view(-1, 1), head, entity_emb.shape[0])


def rel_attention(x, p, q, r, edges, keep=None, slope=SLOPE):
    """the contract of ops.rel_attention: the same lines with the node tables p and q in place of fc(cat(., .))"""
    head, tail, rel = _kept(edges, keep)
    e = F.leaky_relu(((p[head] + q[tail]) * r[rel]).sum(-1), slope)
    e = scatter_softmax(e, head, x.shape[0])
    return scatter_sum(x[tail] * e.view(-1, 1), head, x.shape[0])


def rgat_forward(entity_emb, relation_emb, fc_weight, fc_bias, edges, keep, n_hops, mess_masks=None):
    """:74-84: the last hop's normalised table; mess_masks: per hop a mask already scaled by 1 / (1 - p), or None"""
    for hop in range(n_hops):
        entity_emb = rgat_agg(entity_emb, relation_emb, fc_weight, fc_bias, edges, keep)
        if mess_masks is not None:
            entity_emb = entity_emb * mess_masks[hop]
        entity_emb = F.normalize(entity_emb)
    return entity_emb


# ---- KGCL ----------------------------------------------------------------------------------------------------------
def kgcl_forward(p, n_users, n_items, edges, keep, g, n_hops, layer_num, mess_masks=None):
    """:286-301; p: name -> tensor; edges carry rel = edge_type - 1, so relation_embed[1:] is indexed; g: the [U + I, U + I] matrix"""
    user_emb, entity_emb = p['all_embed'][:n_users], p['all_embed'][n_users:]
    entity_emb = rgat_forward(entity_emb, p['relation_embed'][1:], p['rgat.fc.weight'], p['rgat.fc.bias'], edges, keep, n_hops, mess_masks)
    all_emb = torch.cat([user_emb, entity_emb[:n_items]], dim=0)
    emb_list = [all_emb]
    for _ in range(layer_num):
        all_emb = g @ all_emb
        emb_list.append(all_emb)
    all_emb = torch.mean(torch.stack(emb_list, dim=1), dim=1)
    return torch.split(all_emb, [n_users, n_items])


def bpr_loss(users_emb, pos_emb, neg_emb):
    reg_loss = (1 / 2) * (users_emb.norm(2).pow(2) + pos_emb.norm(2).pow(2) + neg_emb.norm(2).pow(2)) / float(users_emb.shape[0])
    pos_preds = (users_emb * pos_emb).sum(-1)
    neg_preds = (users_emb * neg_emb).sum(-1)
    return torch.sum(F.softplus(neg_preds - pos_preds)), reg_loss


def infonce_overall(z1, z2, z_all, tau=TAU):
    """:351-371 (the batch never has as many rows as the table here, so sim(z1, z_all) is the matrix form)"""
    def f(x):
        return torch.exp(x / tau)
    between_sim = f(F.cosine_similarity(z1, z2))
    all_sim = f(torch.mm(F.normalize(z1), F.normalize(z_all).t()))
    return torch.sum(-torch.log(between_sim / torch.sum(all_sim, 1)))


def model_loss(p, n_users, n_items, edges, keeps, graphs, n_hops, layer_num, batch, decay):
    """:249-284; keeps = (step mask, view 1 mask, view 2 mask) over the edges, graphs = (dropped norm_adj, ui view 1, ui view 2)"""
    user, pos, neg = batch
    user_emb, item_emb = kgcl_forward(p, n_users, n_items, edges, keeps[0], graphs[0], n_hops, layer_num)
    rec_loss, reg_loss = bpr_loss(user_emb[user], item_emb[pos], item_emb[neg])
    u1, i1 = kgcl_forward(p, n_users, n_items, edges, keeps[1], graphs[1], n_hops, layer_num)
    u2, i2 = kgcl_forward(p, n_users, n_items, edges, keeps[2], graphs[2], n_hops, layer_num)
    cl_loss = CL_WEIGHT * (infonce_overall(u1[user], u2[user], u2) + infonce_overall(i1[pos], i2[pos], i2))
    return {'loss': rec_loss + decay * reg_loss + cl_loss, 'rec_loss': rec_loss, 'cl_loss': cl_loss}


PARAM_NAMES = ['all_embed', 'relation_embed', 'rgat.W', 'rgat.a', 'rgat.fc.weight', 'rgat.fc.bias']


def draw_params(n_nodes, n_relations, d, seed):
    """the parameters in the reference constructors' order (:119-126, then :48-52) after torch.manual_seed(seed)"""
    torch.manual_seed(seed)
    p = {'all_embed': torch.nn.init.normal_(torch.empty(n_nodes, d), std=0.1),
         'relation_embed': torch.nn.init.normal_(torch.empty(n_relations, d), std=0.1),
         'rgat.W': torch.nn.init.xavier_uniform_(torch.empty(d, d), gain=1.414),
         'rgat.a': torch.nn.init.xavier_uniform_(torch.empty(2 * d, 1), gain=1.414)}
    fc = torch.nn.Linear(2 * d, d)
    p['rgat.fc.weight'], p['rgat.fc.bias'] = fc.weight.detach(), fc.bias.detach()
    return p


def samp_edge_from_dict(kg_dict, triplet_num=15):
    """:187-198: rows [h, t, r]"""
    samp_edges = []
    for h in kg_dict:
        t_list = kg_dict[h]
        samp_edges_i = random.sample(t_list, triplet_num) if len(t_list) > triplet_num else t_list
        for r, t in samp_edges_i:
            samp_edges.append([h, t, r])
    return samp_edges


# ---- the per-epoch views --------------------------------------------------------------------------------------------
def norm_adj_mat(ui_mat, n_users, n_items):
    """:140-185 in scipy: (A > 0) row sums + 1e-7 to the power -0.5 on both sides of the symmetric 0/1 matrix; COO, row-major"""
    ui = sp.coo_matrix(ui_mat)
    A = sp.coo_matrix((np.ones(2 * ui.nnz, dtype=np.float32), (np.concatenate([ui.row, ui.col + n_users]), np.concatenate([ui.col + n_users, ui.row]))),
                      shape=(n_users + n_items, n_users + n_items)).tocsr()
    A.data[:] = 1                                          # the dict of the reference keeps one entry per pair
    sum_arr = (A > 0).sum(axis=1)
    diag = np.power(np.array(sum_arr.flatten())[0] + 1e-7, -0.5)
    D = sp.diags(diag)
    return sp.coo_matrix(D * A * D)


def aug_weights(stability, mu=MU):
    """:201-210"""
    kg_stability = torch.exp(stability)
    kg_weights = (kg_stability - kg_stability.min()) / (kg_stability.max() - kg_stability.min())
    kg_weights = kg_weights.where(kg_weights > 0.3, torch.ones_like(kg_weights) * 0.3)
    weights = mu / torch.mean(kg_weights) * (kg_weights)
    return weights.where(weights < 0.95, torch.ones_like(weights) * 0.95)


def masked_norm_adj(ui_mat, edge_mask, n_users, n_items):
    """:218-228 from the per-interaction mask"""
    ui = sp.coo_matrix(ui_mat)
    m = np.asarray(edge_mask, dtype=bool)
    return norm_adj_mat(sp.coo_matrix((ui.data[m], (ui.row[m], ui.col[m])), shape=(n_users, n_items)), n_users, n_items)


def dense(coo, dt):
    return torch.from_numpy(np.asarray(sp.coo_matrix(coo).astype(np.float32).todense())).to(dt)


def sparse_dropout_dense(adj_coo, ui_keep, rate, dt):
    """the dense matrix `_sparse_dropout` (:27-40) leaves of a torch sparse adjacency; ui_keep None = no dropout"""
    idx, val = adj_coo._indices(), adj_coo._values().to(dt)
    if ui_keep is not None:
        idx, val = idx[:, ui_keep], val[ui_keep] * (1. / (1 - rate))
    return torch.sparse_coo_tensor(idx, val, adj_coo.shape).to_dense()
