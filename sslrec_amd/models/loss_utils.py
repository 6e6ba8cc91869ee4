"""Loss library of the hot path, same names / signatures / return conventions as the
reference's models/loss_utils.py (cal_bpr_loss :7-10, reg_pick_embeds :13-17, reg_params
:20-24, cal_infonce_loss :30-39, cal_infonce_loss_spec_nodes :42-51, alignment :75-79, uniformity :82-86), backed by the fused HIP kernels of sslrec_amd.ops.

`cal_*_gathered` are the table-level forms the in-tree models use: they take the full
embedding tables plus the batch indices, so the [B, d] gathers of lightgcn.py:49-51 /
simgcl.py:32-37 are never materialized.  The other five functions of the upstream file
belong to models outside this path's scope and are not provided.
"""
from .. import ops


def cal_bpr_loss(anc_embeds, pos_embeds, neg_embeds, divisor=1.0):
    """sum_b softplus(<a,n> - <a,p>)  (the caller divides by the batch size -- or passes it as `divisor`, which folds
    the division and its backward into the kernels)."""
    return ops.bpr_loss(anc_embeds, pos_embeds, neg_embeds, variant=0, divisor=divisor)


def cal_bpr_loss_gathered(user_embeds, item_embeds, ancs, poss, negs, divisor=1.0):
    return ops.bpr_loss_gathered(user_embeds, item_embeds, ancs, poss, negs, variant=0, divisor=divisor)


def cal_bpr_loss_stacked(stacked_embeds, user_num, ancs, poss, negs, divisor=1.0, add=None):
    """same loss on the stacked [users; items] table that the propagation returns (no slicing).  add (a 0-d tensor, e.g. the
    regularizer term): returns (bpr + add, bpr) -- the sum comes out of the same launch"""
    return ops.bpr_loss_stacked(stacked_embeds, user_num, ancs, poss, negs, variant=0, divisor=divisor, add=add)


def cal_infonce_loss(embeds1, embeds2, all_embeds2, temp=1.0, precision=None):
    """sum_b [ -<e1^,e2^>/temp + log sum_j exp(<e1^, all^_j>/temp) ] with x^ = x/sqrt(1e-8+|x|^2).
    `precision` (not in the reference): arithmetic of the products, see ops.infonce_loss."""
    return ops.infonce_loss(embeds1, embeds2, all_embeds2, temp, variant=0, precision=precision)


def cal_infonce_loss_gathered(table1, table2, idx, temp=1.0, precision=None):
    """cal_infonce_loss(table1[idx], table2[idx], table2, temp) without the gathers."""
    return ops.infonce_loss_gathered(table1, table2, idx, temp, variant=0, precision=precision)


def cal_infonce_loss_two_sided(stacked1, stacked2, user_num, user_idx, item_idx, temp=1.0, precision=None):
    """cal_infonce_loss(U1[user_idx], U2[user_idx], U2, temp) + cal_infonce_loss(I1[item_idx], I2[item_idx], I2, temp) on the stacked
    [users; items] tables of two views: both terms of simgcl.py:49 / sgl.py:57-59 as one autograd node (no slicing of the tables)"""
    return ops.infonce_loss_two_sided(stacked1, stacked2, user_num, user_idx, item_idx, temp, variant=0, precision=precision)


def cal_infonce_loss_spec_nodes(embeds1, embeds2, nodes, temp, precision=None):
    """-log(nume / deno).mean() over `nodes` with x^ = F.normalize(x + 1e-8), nume = exp(<e1^[n], e2^[n]> / temp) and
    deno = sum_j exp(<e1^[n], e2^_j> / temp) + 1e-8 (loss_utils.py:42-51), on the fused gathered InfoNCE: no [B, M] tensor.

    The two tables are normalized the reference's way with element-wise torch ops over [N, d]; the kernel normalizes its rows once
    more, x / sqrt(1e-8 + |x|^2), which moves a unit row by a factor 1 - 5e-9 and a cosine by 1e-8, below fp32 resolution.
    The 1e-8 added to the denominator is NOT carried: it changes a node's term by log(1 + 1e-8 / deno) <= 1e-8 / deno, and the node's
    own positive is one of the M summands, so deno >= exp(c / temp) with c its cosine, and deno ~ M for unrelated rows.  For the
    term to reach the 8 * 2^-23 ~ 1e-6 relative floor the tests hold the loss to (a loss of order log M >= 1), deno would have to
    fall below 1e-2, i.e. EVERY cosine of the node below temp * ln(1e-2 / M) -- at temp 0.1 and M = 220 below -1, which no cosine
    is; at temp 1.0 the bound is 1e-8 * e / M.  `precision` (not in the reference): see ops.infonce_loss."""
    import torch.nn.functional as F
    from ..ops import _need_gpu
    _need_gpu(embeds1, embeds2, nodes)
    normed1 = F.normalize(embeds1 + 1e-8, p=2)
    normed2 = F.normalize(embeds2 + 1e-8, p=2)
    return ops.infonce_loss_gathered(normed1, normed2, nodes, temp, variant=0, precision=precision) / nodes.shape[0]


def alignment(x, y, alpha=2):
    """mean_b |x^_b - y^_b|^alpha with x^ = F.normalize(x) (loss_utils.py:75-79) for dense [B, d] rows: the fused kernels of
    csrc/au.hip with identity indices; alpha != 2 runs the reference's expression"""
    return ops.alignment(x, y, alpha)


def uniformity(x):
    """log mean over the B (B - 1) / 2 pairs of exp(-2 |x^_i - x^_j|^2) (loss_utils.py:82-86) without the pair vector"""
    return ops.uniformity(x)


def cal_align_uniform_loss_stacked(stacked_embeds, user_num, ancs, poss, gamma, scale=1.0):
    """(loss, align_loss, uniform_loss) of directau.py:43-47 on the stacked [users; items] table: gathers, both losses and their sum
    as one autograd node; `scale` multiplies the gathered rows (the mean over the layers when the table is their sum)"""
    return ops.align_uniform_loss_stacked(stacked_embeds, user_num, ancs, poss, gamma, scale)


def reg_pick_embeds(embeds_list):
    reg_loss = 0
    for embeds in embeds_list:
        reg_loss += embeds.square().sum()
    return reg_loss


def reg_params(model, weight=1.0):
    """weight * sum over parameters of ||W||_2^2: one fused sum-of-squares kernel per parameter (the reference
    runs `norm` + `square` and their autograd per parameter, then multiplies by reg_weight: lightgcn.py:53)"""
    reg_loss = 0
    for W in model.parameters():
        reg_loss += ops.sum_squares(W, weight)
    return reg_loss
