"""float64 references and invariant checks shared by test_ncl_host.py and test_ncl.py (test infrastructure, no tests of its own)."""
import math

import numpy as np
import torch

U24 = 2.0 ** -24


def xavier_like(N, d, K, seed):
    """the regime KMeansClustering really runs in: rows of a xavier-uniform table, centroids0 = t.rand -- most clusters go empty"""
    gen = torch.Generator().manual_seed(seed)
    bound = math.sqrt(6.0 / (N + d))
    x = (torch.rand(N, d, generator=gen) * 2 - 1) * bound
    return x, torch.rand(K, d, generator=gen)


def blobs(seed=7):
    """N = 1200, d = 32: 8 Gaussian blobs (sigma 0.01) around randn centres; centroids0 = one member of each blob + copies of the first
    four: 12 clusters, of which the 4 copies stay empty under the lowest-index tie rule.  Margins between blobs are of order 1."""
    gen = torch.Generator().manual_seed(seed)
    centres = torch.randn(8, 32, generator=gen)
    owner = torch.arange(1200) % 8
    x = centres[owner] + 0.01 * torch.randn(1200, 32, generator=gen)
    c0 = torch.cat([x[:8], x[:4]]).clone()
    return x, c0


def lowest_argmin(dist):
    """argmin over dim 1 with the LOWEST index among equal values, spelled out (no reliance on a library's tie behaviour)"""
    K = dist.shape[1]
    ks = torch.arange(K)
    return torch.where(dist == dist.min(dim=1, keepdim=True).values, ks, K).min(dim=1).values


def dist64(x, cent):
    x, cent = x.double().cpu(), cent.double().cpu()
    return (x[:, None, :] - cent[None, :, :]).square().sum(-1)


def lloyd64(x, c0, iters):
    """aug_utils.py:149-156 in float64; stops at a repeated assignment (from there on every iteration is the identity)"""
    x, cent = x.double(), c0.double()
    K = cent.shape[0]
    prev = None
    for it in range(iters):
        idx = lowest_argmin(dist64(x, cent))
        sums = torch.zeros_like(cent).index_add_(0, idx, x)
        counts = torch.bincount(idx, minlength=K).double()
        cent = sums / (counts[:, None] + 1e-6)
        if prev is not None and torch.equal(prev, idx):
            break
        prev = idx
    return cent, idx, counts


def check_assignment(x, cent_in, idx, what):
    """every row: its float64 distance to the chosen centroid <= min_k dist * (1 + rtol), rtol = 2 (d + 2) 2^-24 -- the rounding bound
    of the fp32 difference form, so no row is excluded"""
    d = x.shape[1]
    dist = dist64(x, cent_in)
    idx = idx.cpu()
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (x.shape[0],), what
    assert int(idx.min()) >= 0 and int(idx.max()) < cent_in.shape[0], what
    chosen = dist.gather(1, idx[:, None])[:, 0]
    lowest = dist.min(dim=1).values
    rtol = 2 * (d + 2) * U24
    worst = float(((chosen - lowest) / lowest.clamp_min(1e-300)).max())
    print('%s: worst relative excess of the chosen distance %.3e (bound %.3e)' % (what, worst, rtol))
    assert bool((chosen <= lowest * (1 + rtol)).all()), (what, worst, rtol)


def check_update(x, idx, cent_out, counts, what):
    """counts == bincount(idx) exactly; every centroid element within (count + 2) 2^-24 sum|x| (the bound of any fixed-order fp32
    sum) of the float64 sum / (count + 1e-6) over THESE idx; empty clusters exactly 0"""
    K = cent_out.shape[0]
    idx, x64 = idx.cpu(), x.double().cpu()
    cnt = torch.bincount(idx, minlength=K)
    assert tuple(counts.shape) == (K, 1) and counts.dtype == torch.float32, what
    assert torch.equal(counts.cpu()[:, 0].double(), cnt.double()), what
    sums = torch.zeros(K, x.shape[1], dtype=torch.float64).index_add_(0, idx, x64)
    mags = torch.zeros(K, x.shape[1], dtype=torch.float64).index_add_(0, idx, x64.abs())
    want = sums / (cnt.double()[:, None] + 1e-6)
    bound = (cnt.double()[:, None] + 2) * U24 * mags
    got = cent_out.double().cpu()
    err = (got - want).abs()
    ratio = float((err / bound.clamp_min(1e-300))[cnt > 0].max()) if bool((cnt > 0).any()) else 0.0
    print('%s: %d of %d clusters non-empty, worst centroid error / bound %.3e' % (what, int((cnt > 0).sum()), K, ratio))
    assert bool((err <= bound).all()), (what, ratio)
    assert bool((got[cnt == 0] == 0).all()), what


def check_step(x, cent_in, out, what):
    cent, idx, counts, _ = out
    check_assignment(x, cent_in, idx, what)
    check_update(x, idx, cent, counts, what)


# ---- the model ------------------------------------------------------------------------------------------------------
def ref_infonce(e1, e2, all2, temp):
    """loss_utils.py:30-39"""
    n1 = e1 / torch.sqrt(1e-8 + e1.square().sum(-1, keepdim=True))
    n2 = e2 / torch.sqrt(1e-8 + e2.square().sum(-1, keepdim=True))
    na = all2 / torch.sqrt(1e-8 + all2.square().sum(-1, keepdim=True))
    nume = -(n1 * n2 / temp).sum(-1)
    deno = torch.log(torch.sum(torch.exp(n1 @ na.T / temp), dim=-1))
    return (nume + deno).sum()


def ref_spmm(vals, heads, tails, x, n_rows):
    return torch.zeros(n_rows, x.shape[1], dtype=x.dtype).index_add(0, heads, vals[:, None] * torch.index_select(x, 0, tails))


def ref_ncl_forward(ue, ie, graph, layer_num, high_order):
    """ncl.py:34-41"""
    vals, heads, tails = graph
    lst = [torch.concat([ue, ie], dim=0)]
    for _ in range(max(layer_num, high_order * 2)):
        lst.append(ref_spmm(vals, heads, tails, lst[-1], lst[0].shape[0]))
    return sum(lst[:layer_num + 1]), lst


def ref_ncl_loss(ue, ie, graph, batch, clusters, cfg):
    """ncl.py:70-86 (with :51-68) given the clustering: clusters = (user_centroids, user2cluster, item_centroids, item2cluster)"""
    ancs, poss, negs = batch
    uc, u2c, ic, i2c = clusters
    U, B, temp = ue.shape[0], ancs.shape[0], cfg['temperature']
    embeds, lst = ref_ncl_forward(ue, ie, graph, cfg['layer_num'], cfg['high_order'])
    ego, context = lst[0], lst[cfg['high_order'] * 2]
    struct = (ref_infonce(context[:U][ancs], ego[:U][ancs], ego[:U], temp) + ref_infonce(context[U:][poss], ego[U:][poss], ego[U:], temp)) / B
    proto = (ref_infonce(ego[:U][ancs], uc[u2c[ancs]], uc, temp) + ref_infonce(ego[U:][poss], ic[i2c[poss]], ic, temp)) / B
    anc, pos, neg = embeds[:U][ancs], embeds[U:][poss], embeds[U:][negs]
    bpr = torch.nn.functional.softplus((anc * neg).sum(-1) - (anc * pos).sum(-1)).sum() / B
    reg = (ue.square().sum() + ie.square().sum()) * cfg['reg_weight']
    struct, proto = struct * cfg['struct_weight'], proto * cfg['proto_weight']
    return bpr + struct + proto + reg, {'bpr_loss': bpr, 'reg_loss': reg, 'struct_loss': struct, 'proto_loss': proto}


def fills(U, I, d):
    gen = torch.Generator().manual_seed(300)
    return (torch.randn(U, d, generator=gen) * 0.1).float(), (torch.randn(I, d, generator=gen) * 0.1).float()


def np_allclose(got, want, rtol, atol, what):
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), rtol=rtol, atol=atol, err_msg=what)
