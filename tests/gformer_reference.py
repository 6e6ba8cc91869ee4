"""CPU restatement of the reference's GFormer (models/general_cf/gformer.py) shared by test_gformer_host.py and test_gformer.py (test
infrastructure, no tests of its own).  Every function takes any dtype; the float64 run is the yardstick, the float32 run measures what
fp32 arithmetic costs (tests/test_autocf.py's convention: max|x - ref64| / max|ref64| per tensor, the kernels at most 4 x the fp32
restatement's error, floor 8 * 2^-23).  The PNN layer is restated LITERALLY, with the reference's repeat / reshape and its [N, A, 2d]
tensor; the masker with its Python loops and scipy matrices."""
import numpy as np
import scipy.sparse as sp
import torch
import torch.nn.functional as F
from scipy.sparse.csgraph import shortest_path

FLOOR = 8 * 2.0 ** -23


def randn(shape, seed, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def lt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).long()


def leaf(x, dt):
    return x.detach().to(dt).clone().requires_grad_(True)


def rel_err(x, ref):
    ref = ref.double()
    return float((x.detach().cpu().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def check(name, got, ref64, ref32):
    e32, e = rel_err(ref32, ref64), rel_err(got, ref64)
    bound = max(4 * e32, FLOOR)
    print('%-34s kernel %.3e  fp32 torch %.3e  (%.2f / %.2f units of 2^-23 max|ref|)  bound %.3e' % (name, e, e32, e * 2 ** 23, e32 * 2 ** 23, bound))
    assert torch.isfinite(got).all(), name
    assert e <= bound, '%s: kernel error %.3e > bound %.3e (fp32 torch: %.3e)' % (name, e, bound, e32)


def both_precisions(fn):
    return fn(torch.float64), fn(torch.float32)


# ---- anchors --------------------------------------------------------------------------------------------------------
def ref_hops(rows, cols, n, anchors):
    """gformer.py:152-176 as hop counts [n, A] int16, -1 for an unreached node: scipy's unweighted shortest paths from the anchors"""
    mat = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    dist = shortest_path(mat, directed=False, unweighted=True, indices=np.asarray(anchors))
    return np.where(np.isinf(dist), -1, dist).astype(np.int16).T.copy()


def ref_dists(hops, dt):
    """t.tensor(handler.dists_array, dtype=t.float32) of gformer.py:205 from hop counts [N, A]: [A, N], float32-rounded, as `dt`"""
    h = torch.as_tensor(np.asarray(hops)).double()
    w = torch.where(h < 0, torch.zeros((), dtype=torch.float64), 1.0 / (h + 1.0))
    return w.float().to(dt).T


def ref_pnn(embeds, anchors, dists, weight=None, bias=None):
    """PNNLayer.forward, gformer.py:202-218, literally (without the .squeeze(), which only matters for A = 1).  dists: [A, N].  Without a
    weight the Linear is left out: the mean over the anchors of the [N, A, 2d] messages, i.e. the two feature halves"""
    d = embeds.shape[1]
    A = len(anchors)
    set_ids_emb = embeds[torch.as_tensor(anchors).long()]
    set_ids_reshape = set_ids_emb.repeat(dists.shape[1], 1).reshape(-1, A, d)
    messages = set_ids_reshape * dists.T.unsqueeze(2)
    self_feature = embeds.repeat(A, 1).reshape(-1, A, d)
    messages = torch.cat((messages, self_feature), dim=-1)
    if weight is not None:
        messages = F.linear(messages, weight, bias)
    return torch.mean(messages, dim=1)


# ---- layers ---------------------------------------------------------------------------------------------------------
def ref_gt_layer(rows, cols, embeds, wq, wk, wv, heads):
    """GTLayer.forward, gformer.py:235-255: (resEmbeds, att [E, H])"""
    n, d = embeds.shape
    row_e, col_e = embeds[rows], embeds[cols]
    qe, ke, ve = ((x @ w).view(-1, heads, d // heads) for x, w in ((row_e, wq), (col_e, wk), (col_e, wv)))
    att = torch.exp(torch.clamp(torch.einsum('ehd, ehd -> eh', qe, ke), -10.0, 10.0))
    norm = torch.zeros(n, heads, dtype=embeds.dtype).index_add_(0, rows, att)[rows]
    att = att / (norm + 1e-8)
    res = torch.einsum('eh, ehd -> ehd', att, ve).reshape(-1, d)
    return torch.zeros(n, d, dtype=embeds.dtype).index_add_(0, rows, res), att


def ref_scores(rows, cols, q, k, heads):
    """att.sum(-1) from projected node tables"""
    n, d = q.shape
    att = torch.exp(torch.clamp(torch.einsum('ehd, ehd -> eh', q[rows].view(-1, heads, d // heads), k[cols].view(-1, heads, d // heads)), -10.0, 10.0))
    norm = torch.zeros(n, heads, dtype=q.dtype).index_add_(0, rows, att)[rows]
    return (att / (norm + 1e-8)).sum(-1)


def ref_spmm(adj, x):
    rows, cols, vals = adj
    return torch.zeros(x.shape[0], x.shape[1], dtype=x.dtype).index_add_(0, rows, vals.to(x.dtype)[:, None] * x[cols])


def ref_forward(params, n_user, cfg, is_test, sub, cmp, enc, dec, anchors=None, dists=None):
    """GFormer.forward, gformer.py:49-75.  params: uEmbeds, iEmbeds, q, k, v, then (linear_out.w, .b, linear_hidden.w, .b) per PNN layer;
    matrices as (rows, cols, vals) int64 / float tensors, dec as (rows, cols)"""
    ue, ie, wq, wk, wv = params[:5]
    embeds = torch.cat([ue, ie], dim=0)
    lst = [embeds]
    emb, _ = ref_gt_layer(cmp[0], cmp[1], embeds, wq, wk, wv, cfg['head'])
    c_list = [embeds, cfg['gtw'] * emb]
    emb, _ = ref_gt_layer(sub[0], sub[1], embeds, wq, wk, wv, cfg['head'])
    sub_list = [embeds, cfg['gtw'] * emb]
    for _ in range(cfg['layer_num']):
        e1, e2, e3 = ref_spmm(enc, lst[-1]), ref_spmm(sub, lst[-1]), ref_spmm(cmp, lst[-1])
        sub_list.append(e2)
        lst.append(e1)
        c_list.append(e3)
    if not is_test:
        for i in range(cfg['pnn_layer']):
            lh_w, lh_b = params[5 + 4 * i + 2], params[5 + 4 * i + 3]
            lst.append(ref_pnn(lst[-1], anchors, dists, lh_w, lh_b))
    if dec is not None:
        emb, _ = ref_gt_layer(dec[0], dec[1], lst[-1], wq, wk, wv, cfg['head'])
        lst.append(emb)
    total = sum(lst)
    return total[:n_user], total[n_user:], sum(c_list), sum(sub_list)


def ref_contrast(nodes, all1, all2=None):
    """gformer.py:129-137"""
    if all2 is not None:
        return torch.log(torch.exp(all1[nodes] @ all2.T).sum(-1)).mean()
    return torch.log(torch.exp(all1[torch.unique(nodes)] @ all1.T).sum(-1)).mean()


def ref_step(params, n_user, cfg, batch_train, batch, sub, cmp, enc, dec, anchors, dists):
    """cal_loss, gformer.py:87-115: (loss, bpr_loss, reg_loss, cl_loss)"""
    ue, ie, c_list, sub_lst = ref_forward(params, n_user, cfg, False, sub, cmp, enc, dec, anchors, dists)
    ancs, poss, negs = batch
    anc, pos, neg = ue[ancs], ie[poss], ie[negs]
    anc2, pos2 = sub_lst[:n_user][ancs], sub_lst[n_user:][poss]
    bpr = (-torch.sum(anc * pos, dim=-1)).mean()
    diff = torch.sum(anc2 * pos2, dim=-1) - torch.sum(anc2 * neg, dim=-1)
    bpr2 = -diff.sigmoid().log().sum() / batch_train
    reg = sum(w.norm(2).square() for w in params) * cfg['reg_weight']
    nce = torch.log(torch.exp(sub_lst[ancs] * c_list[ancs]).sum(-1)).mean()
    cl = (ref_contrast(ancs, ue) + ref_contrast(poss, ie)) * cfg['ssl_reg'] + ref_contrast(ancs, ue, ie) + cfg['ctra'] * nce
    return bpr + reg + cl + cfg['b2'] * bpr2, bpr, reg, cl


# ---- LocalGraph and the masker on the host (numpy draws, scipy matrices, Python loops: gformer.py:330-503) --------------------------------
def _coalesce(mat):
    coo = mat.tocoo().astype(np.float32)
    ten = torch.sparse_coo_tensor(torch.from_numpy(np.asarray([coo.row, coo.col])).long(), torch.from_numpy(coo.data), coo.shape).coalesce()
    idx = ten._indices().numpy()
    return idx[0], idx[1], ten._values().numpy()


def ref_add_adj(rows, cols, n, add_rate):
    """LocalGraph.forward, :333-349: the entries of add_adj (coalesced)"""
    tmp_rows = np.random.choice(rows, size=[int(len(rows) * add_rate)])
    tmp_cols = np.random.choice(cols, size=[int(len(cols) * add_rate)])
    every = np.arange(n)
    new_rows = np.concatenate([tmp_rows, tmp_cols, every, rows])
    new_cols = np.concatenate([tmp_cols, tmp_rows, every, cols])
    mat = sp.csr_matrix((np.ones(len(new_rows), dtype=np.int64), (new_rows, new_cols)), shape=(n, n))
    r, c, _ = _coalesce(mat)
    return r, c


def _drop_flags(n_entries, keep_index):
    """the `while` loop of :394-407 / :444-457"""
    drop, i, j = [], 0, 0
    while i < n_entries:
        if j == len(keep_index):
            drop.append(True)
            i += 1
            continue
        if i == keep_index[j]:
            drop.append(False)
            j += 1
        else:
            drop.append(True)
        i += 1
    return np.array(drop, dtype=bool)


def _normalized(rows, cols, n):
    """:414-424 / :459-469: (rows, cols, vals, raw values before the normalisation)"""
    mat = sp.csr_matrix((np.ones(len(rows), dtype=np.int64), (rows, cols)), shape=(n, n))
    rowsum = np.array(mat.sum(1))
    d_inv = np.power(rowsum, -0.5).flatten()
    d_inv[np.isinf(d_inv)] = 0.
    d_mat = sp.diags(d_inv)
    r, c, v = _coalesce(d_mat.dot(mat).dot(d_mat))
    _, _, raw = _coalesce(mat)
    return r, c, v, raw


def ref_create_sub_adj(users_up, items_up, att_edge, flag, n, sub_rate):
    """:378-425; att_edge a CPU tensor, clamped in place when flag is False"""
    if flag:
        att = (att_edge.detach().cpu() + 0.001).numpy()
    else:
        att_f = att_edge
        att_f[att_f > 3] = 3
        att = 1.0 / (np.exp((att_f.detach().cpu() + 1E-8).numpy()))
    p = att / att.sum()
    keep_index = np.random.choice(np.arange(len(users_up)), int(len(users_up) * sub_rate), replace=False, p=p)
    keep_index.sort()
    _drop_flags(len(users_up), keep_index)
    rows = np.concatenate([np.arange(n), users_up[keep_index]])
    cols = np.concatenate([np.arange(n), items_up[keep_index]])
    return _normalized(rows, cols, n)


def ref_masker(users_up, items_up, att_edge, n, cfg):
    """RandomMaskSubgraphs.forward, :427-503: {'enc', 'sub', 'cmp': (rows, cols, vals, raw), 'dec': (rows, cols)}"""
    E = len(users_up)
    att_f = att_edge
    att_f[att_f > 3] = 3
    att_f = 1.0 / (np.exp((att_f.detach().cpu() + 1E-8).numpy()))
    p = att_f / att_f.sum()
    keep_index = np.random.choice(np.arange(E), int(E * cfg['keep_rate']), replace=False, p=p)
    keep_index.sort()
    rows = np.concatenate([np.arange(n), users_up[keep_index]])
    cols = np.concatenate([np.arange(n), items_up[keep_index]])
    drop = _drop_flags(E, keep_index)
    enc = _normalized(rows, cols, n)
    drop_rows, drop_cols = users_up[drop], items_up[drop]
    ext_rows = np.random.choice(rows, size=[int(len(drop_rows) * cfg['ext'])])
    ext_cols = np.random.choice(cols, size=[int(len(drop_cols) * cfg['ext'])])
    tmp_rows = np.concatenate([ext_rows, drop_rows])
    tmp_cols = np.concatenate([ext_cols, drop_cols])
    new_rows = np.random.choice(tmp_rows, size=[int(E * cfg['reRate'])])
    new_cols = np.random.choice(tmp_cols, size=[int(E * cfg['reRate'])])
    all_rows = np.concatenate([new_rows, new_cols, np.arange(n), rows])
    all_cols = np.concatenate([new_cols, new_rows, np.arange(n), cols])
    hash_val = np.unique(all_rows.astype(np.int64) * n + all_cols.astype(np.int64))
    dec_cols = hash_val % n
    dec_rows = (hash_val - dec_cols) // n
    sub = ref_create_sub_adj(users_up, items_up, att_edge, True, n, cfg['sub'])
    cmp = ref_create_sub_adj(users_up, items_up, att_edge, False, n, cfg['sub'])
    return {'enc': enc, 'sub': sub, 'cmp': cmp, 'dec': (dec_rows, dec_cols)}


def small_bipartite(n_user, n_item, n_inter, seed, isolated=()):
    """a random symmetric bipartite adjacency on n_user + n_item nodes as (rows, cols) int64, both directions; nodes in `isolated` have
    no entry"""
    rng = np.random.RandomState(seed)
    u, i = rng.randint(0, n_user, n_inter), rng.randint(0, n_item, n_inter) + n_user
    ok = ~np.isin(u, isolated) & ~np.isin(i, isolated)
    key = np.unique(u[ok].astype(np.int64) * (n_user + n_item) + i[ok])
    u, i = key // (n_user + n_item), key % (n_user + n_item)
    return np.concatenate([u, i]), np.concatenate([i, u])
