"""CPU restatement of the reference's MHCN (models/social/mhcn.py) and of the motif matrices of its data handler
(data_utils/data_handler_social.py:98-137), shared by test_mhcn_host.py and test_mhcn.py (test infrastructure, no tests of its own).
Every torch function takes any dtype: the float64 run is the yardstick, the float32 run measures what fp32 arithmetic costs
(tests/test_gformer.py's convention: max|x - ref64| / max|ref64| per tensor, the kernels at most 4 x the fp32 restatement's error, floor
8 * 2^-23).  The statements are the reference's own: `_channel_attention` with its stack / transposes, F.normalize, row_shuffle /
row_col_shuffle / score with the permutations handed in instead of drawn, and `sigmoid().log()`.  The motifs are dense U x U numpy."""
import numpy as np
import torch
import torch.nn.functional as F

FLOOR = 8 * 2.0 ** -23


def randn(shape, seed, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def leaf(x, dt):
    return x.detach().to(dt).clone().requires_grad_(True)


def rel_err(x, ref):
    ref = ref.double()
    return float((x.detach().cpu().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def check(name, got, ref64, ref32):
    e32, e = rel_err(ref32, ref64), rel_err(got, ref64)
    bound = max(4 * e32, FLOOR)
    print('%-40s kernel %.3e  fp32 torch %.3e  (%.2f / %.2f units of 2^-23 max|ref|)  bound %.3e' % (name, e, e32, e * 2 ** 23, e32 * 2 ** 23, bound))
    assert torch.isfinite(got).all(), name
    assert e <= bound, '%s: kernel error %.3e > bound %.3e (fp32 torch: %.3e)' % (name, e, bound, e32)


def both_precisions(fn):
    return fn(torch.float64), fn(torch.float32)


# ---- the model's expressions ----------------------------------------------------------------------------------------
def self_gating(em, weight, bias):
    """mhcn.py:34-43: em * sigmoid(Linear(em))"""
    gates = torch.sigmoid(F.linear(em, weight, bias))
    return em * gates


def channel_attention(attn, attn_mat, *channel_embeds):
    """mhcn.py:54-64, literally"""
    weights = []
    for embed in channel_embeds:
        weight = (attn * (embed @ attn_mat)).sum(1)
        weights.append(weight)
    weights = torch.stack(weights, 0)
    score = F.softmax(torch.t(weights), dim=-1)
    mixed_embeds = 0
    for i in range(len(weights)):
        mixed_embeds = mixed_embeds + torch.t(torch.multiply(torch.t(score)[i], torch.t(channel_embeds[i])))
    return mixed_embeds, score


def row_shuffle(embed, indices):
    return embed[indices]


def row_col_shuffle(embed, col_indices, row_indices):
    corrupted_embed = torch.t(torch.t(embed)[col_indices])
    return corrupted_embed[row_indices]


def score(x1, x2):
    return (x1 * x2).sum(1)


def log_sigmoid_reference(x):
    return x.sigmoid().log()


def log_sigmoid_stable(x):
    return torch.clamp(x, max=0) - torch.log1p(torch.exp(-x.abs()))


def hierarchical_self_supervision(user_embeds, edge_embeds, perms, log_sigmoid=log_sigmoid_reference):
    """mhcn.py:121-143 with edge_embeds = t.spmm(adj, user_embeds) formed by the caller and the five draws handed in"""
    row_u, col_1, row_1, col_2, row_2 = perms
    pos = score(user_embeds, edge_embeds)
    neg1 = score(row_shuffle(user_embeds, row_u), edge_embeds)
    neg2 = score(row_col_shuffle(edge_embeds, col_1, row_1), user_embeds)
    local_ssl = -(log_sigmoid(pos - neg1) + log_sigmoid(neg1 - neg2)).sum()
    graph = edge_embeds.mean(0)
    pos = score(edge_embeds, graph)
    neg1 = score(row_col_shuffle(edge_embeds, col_2, row_2), graph)
    global_ssl = -log_sigmoid(pos - neg1).sum()
    return local_ssl + global_ssl


PARAM_NAMES = ['user_embeds', 'item_embeds'] + ['%s.%s' % (g, p) for g in ('gating1', 'gating2', 'gating3', 'gating4', 'sgating1', 'sgating2',
                                                                            'sgating3') for p in ('weight', 'bias')] + ['attn', 'attn_mat']


def draw_params(U, I, d, seed):
    """the parameters in the reference constructor's order (:20-31) after torch.manual_seed(seed): name -> float32 tensor"""
    from torch import nn
    torch.manual_seed(seed)
    init = nn.init.xavier_uniform_
    p = {'user_embeds': init(torch.empty(U, d)), 'item_embeds': init(torch.empty(I, d))}
    for g in ('gating1', 'gating2', 'gating3', 'gating4', 'sgating1', 'sgating2', 'sgating3'):
        lin = nn.Linear(d, d)
        p[g + '.weight'], p[g + '.bias'] = lin.weight.detach(), lin.bias.detach()
    p['attn'] = init(torch.empty(1, d))
    p['attn_mat'] = init(torch.empty(d, d))
    return p


def model_forward(p, H, R, layer_num):
    """mhcn.py:66-118: p name -> tensor, H = (H_s, H_j, H_p) and R as dense or sparse matrices of p's dtype"""
    ue = p['user_embeds']
    c = [self_gating(ue, p['gating%d.weight' % k], p['gating%d.bias' % k]) for k in (1, 2, 3)]
    simp = self_gating(ue, p['gating4.weight'], p['gating4.bias'])
    all_c = [[c[0]], [c[1]], [c[2]]]
    all_simp, item_embeds = [simp], p['item_embeds']
    all_i = [item_embeds]
    for _ in range(layer_num):
        mixed = channel_attention(p['attn'], p['attn_mat'], *c)[0] + simp / 2
        for k in range(3):
            c[k] = H[k] @ c[k]
            all_c[k] += [F.normalize(c[k], p=2, dim=1)]
        new_item_embeds = R.t() @ mixed
        all_i += [F.normalize(new_item_embeds, p=2, dim=1)]
        simp = R @ item_embeds
        all_simp += [F.normalize(simp, p=2, dim=1)]
        item_embeds = new_item_embeds
    c = [sum(x) for x in all_c]
    simp = sum(all_simp)
    ret_user, attn_score = channel_attention(p['attn'], p['attn_mat'], *c)
    ret_user = ret_user + simp / 2
    return ret_user, sum(all_i), attn_score


def model_loss(p, H, R, layer_num, batch, perms, reg_weight, ss_rate, log_sigmoid=log_sigmoid_reference):
    """mhcn.py:145-161 with the 15 draws handed in (perms[channel] = the five of that channel): the final tables and the loss parts"""
    user_embeds, item_embeds, _ = model_forward(p, H, R, layer_num)
    ancs, poss, negs = batch
    anc, pos, neg = user_embeds[ancs], item_embeds[poss], item_embeds[negs]
    bpr = F.softplus((anc * neg).sum(-1) - (anc * pos).sum(-1)).sum()          # loss_utils.py:7-10
    reg = 0
    for name in PARAM_NAMES:
        reg = reg + p[name].norm(2).square()
    reg = reg_weight * reg
    ss = 0
    for k in range(3):
        em = self_gating(user_embeds, p['sgating%d.weight' % (k + 1)], p['sgating%d.bias' % (k + 1)])
        ss = ss + hierarchical_self_supervision(em, H[k] @ em, perms[k], log_sigmoid)
    ss = ss * ss_rate
    return {'user': user_embeds, 'item': item_embeds, 'bpr_loss': bpr, 'reg_loss': reg, 'ss_loss': ss, 'loss': bpr + reg + ss}


# ---- the handler's matrices, dense ----------------------------------------------------------------------------------
def dense_motifs(S, Y):
    """A1 .. A10 of data_handler_social.py:99-117 on dense float64 arrays (`.dot` = matrix product, `*` = entry-wise product)"""
    S, Y = np.asarray(S, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    B = S * S.T
    U = S - B
    C1 = (U.dot(U)) * U.T
    A1 = C1 + C1.T
    C2 = (B.dot(U)) * U.T + (U.dot(B)) * U.T + (U.dot(U)) * B
    A2 = C2 + C2.T
    C3 = (B.dot(B)) * U + (B.dot(U)) * B + (U.dot(B)) * B
    A3 = C3 + C3.T
    A4 = (B.dot(B)) * B
    C5 = (U.dot(U)) * U + (U.dot(U.T)) * U + (U.T.dot(U)) * U
    A5 = C5 + C5.T
    A6 = (U.dot(B)) * U + (B.dot(U.T)) * U.T + (U.T.dot(U)) * B
    A7 = (U.T.dot(B)) * U.T + (B.dot(U)) * U + (U.dot(U.T)) * B
    A8 = (Y.dot(Y.T)) * B
    A9 = (Y.dot(Y.T)) * U
    A9 = A9 + A9.T
    A10 = Y.dot(Y.T) - A8 - A9
    return [A1, A2, A3, A4, A5, A6, A7, A8, A9, A10]


def dense_row_normalized(H):
    s = H.sum(axis=1, keepdims=True)
    out = np.zeros_like(H)
    np.multiply(H, 1.0 / np.where(s == 0, 1.0, s), out=out, where=H != 0)
    return out


def dense_adjacencies(S, Y):
    """(H_s, H_j, H_p, R) dense float64: :119-126 and :128-137"""
    A = dense_motifs(S, Y)
    H_s = dense_row_normalized(sum(A[:7]))
    H_j = dense_row_normalized(A[7] + A[8])
    H_p = A[9] * (A[9] > 1)
    H_p = dense_row_normalized(H_p)
    Y = np.asarray(Y, dtype=np.float64)
    udeg, ideg = Y.sum(axis=1), Y.sum(axis=0)
    R = np.zeros_like(Y)
    r, c = np.nonzero(Y)
    R[r, c] = Y[r, c] / np.sqrt(udeg[r]) / np.sqrt(ideg[c])
    return H_s, H_j, H_p, R
