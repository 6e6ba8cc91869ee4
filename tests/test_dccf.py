"""DCCF: the fused intent aggregation (sslrec_amd/csrc/intent.hip, ops.intent_aggregate / intent_aggregate_stacked) and the model
(sslrec_amd/models/general_cf/dccf.py).

Yardstick of the GPU tests, as in tests/test_adaptive_mask.py: a float64 torch restatement of the reference's expressions
(models/general_cf/dccf.py:65-146, models/aug_utils.py:73-79, models/loss_utils.py:7-39) written out below, gradients by torch autograd.
The same restatement runs in fp32 on the CPU; its error against float64 is measured per tensor as max|x - ref| / max|ref|, and the
kernels may be at most 4 x as far off, with a floor of 8 * 2^-23.  Both errors are printed per tensor.

The whole step with the DEFAULT InfoNCE arithmetic (two fp16 planes per operand) is held to the same bound where it holds;
a tensor on the cl path that exceeds it is held to DESIGN §2's whole-step bars instead (losses rtol 1e-5, gradients rtol 1e-4 / atol
1e-7, the bars of the four other models).  With model.infonce_precision = fp32 the 4 x bound applies to everything."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

N_USER, N_ITEM = 700, 500
N_NODE = N_USER + N_ITEM
FLOOR = 8 * 2.0 ** -23
DEV = 'cuda:0'


# ---------------------------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def square_lists():
    """the AdaptiveMask fixture graph: ~6,000 random interactions, a user of degree 499, an item of degree ~600, one user and one
    item without interactions; both directions stacked (dccf.py:21-23), entry list randomly permuted"""
    rng = np.random.RandomState(1234)
    u = rng.randint(0, N_USER - 1, 6000)
    i = rng.randint(0, N_ITEM - 1, 6000)
    u = np.concatenate([u, np.zeros(N_ITEM - 1, dtype=np.int64), rng.choice(N_USER - 1, 600, replace=False)])
    i = np.concatenate([i, np.arange(N_ITEM - 1), np.zeros(600, dtype=np.int64)])
    key = np.unique(u.astype(np.int64) * N_ITEM + i)
    u, i = key // N_ITEM, key % N_ITEM
    heads = np.concatenate([u, i + N_USER])
    tails = np.concatenate([i + N_USER, u])
    p = np.random.RandomState(99).permutation(heads.size)
    return heads[p].copy(), tails[p].copy()


def randn(shape, seed, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def lt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).long()


def leaf(x, dt):
    return x.detach().to(dt).clone().requires_grad_(True)


def gpu(x):
    return x.detach().float().to(DEV)


def rel_err(x, ref):
    ref = ref.double()
    return float((x.detach().cpu().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def check(name, got, ref64, ref32):
    e32, e = rel_err(ref32, ref64), rel_err(got, ref64)
    bound = max(4 * e32, FLOOR)
    print('%-22s kernel %.3e  fp32 torch %.3e  (%.2f / %.2f units of 2^-23 max|ref|)  bound %.3e' % (name, e, e32, e * 2 ** 23, e32 * 2 ** 23, bound))
    assert torch.isfinite(got).all(), name
    assert e <= bound, '%s: kernel error %.3e > bound %.3e (fp32 torch: %.3e)' % (name, e, bound, e32)


def both_precisions(fn):
    return fn(torch.float64), fn(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement (any dtype, CPU)
# ---------------------------------------------------------------------------------------------------------------------
def ref_intent(x, n_user, c_u, c_i):
    """dccf.py:77-80"""
    u, i = x[:n_user], x[n_user:]
    return torch.concat([torch.softmax(u @ c_u, dim=1) @ c_u.T, torch.softmax(i @ c_i, dim=1) @ c_i.T], dim=0)


def ref_spmm(vals, heads, tails, x, n_rows):
    return torch.zeros(n_rows, x.shape[1], dtype=x.dtype).index_add(0, heads, vals[:, None] * torch.index_select(x, 0, tails))


def ref_mask_values(emb, heads, tails, n_rows):
    """aug_utils.py:73-79 behind the gathers of dccf.py:83-86"""
    head_e = F.normalize(torch.index_select(emb, 0, heads))
    tail_e = F.normalize(torch.index_select(emb, 0, tails))
    alpha = (torch.sum(head_e * tail_e, dim=1).view(-1) + 1) / 2
    d_inv = torch.zeros(n_rows, dtype=alpha.dtype).index_add(0, heads, alpha).pow(-1).nan_to_num(0, 0, 0).view(-1)
    return d_inv[heads] * alpha


def ref_layer(e, n_user, c_u, c_i, g_vals, g_heads, g_tails, heads, tails):
    """dccf.py:74-97: (gnn, int, gaa, iaa, next)"""
    n = e.shape[0]
    gnn = ref_spmm(g_vals, g_heads, g_tails, e, n)
    inte = ref_intent(e, n_user, c_u, c_i)
    gaa = ref_spmm(ref_mask_values(gnn, heads, tails, n), heads, tails, e, n)
    iaa = ref_spmm(ref_mask_values(inte, heads, tails, n), heads, tails, e, n)
    return gnn, inte, gaa, iaa, gnn + inte + gaa + iaa + e


def ref_infonce(e1, e2, all2, temp):
    """loss_utils.py:30-39"""
    n1 = e1 / torch.sqrt(1e-8 + e1.square().sum(-1, keepdim=True))
    n2 = e2 / torch.sqrt(1e-8 + e2.square().sum(-1, keepdim=True))
    na = all2 / torch.sqrt(1e-8 + all2.square().sum(-1, keepdim=True))
    nume = -(n1 * n2 / temp).sum(-1)
    deno = torch.log(torch.sum(torch.exp(n1 @ na.T / temp), dim=-1))
    return (nume + deno).sum()


def ref_forward(params, n_user, L, g, heads, tails):
    ue, ie, c_u, c_i = params
    all_e = [torch.concat([ue, ie], dim=0)]
    parts = [[], [], [], []]
    for l in range(L):
        out = ref_layer(all_e[l], n_user, c_u, c_i, g[0], g[1], g[2], heads, tails)
        for lst, v in zip(parts, out[:4]):
            lst.append(v)
        all_e.append(out[4])
    return torch.stack(all_e, dim=1).sum(dim=1), parts


def ref_step(params, n_user, L, g, heads, tails, batch, temp, reg_w, cl_w):
    """dccf.py:105-146"""
    final, (gnn, inte, gaa, iaa) = ref_forward(params, n_user, L, g, heads, tails)
    ancs, poss, negs = batch
    ue, ie = final[:n_user], final[n_user:]
    a, p, n = ue[ancs], ie[poss], ie[negs]
    bpr = torch.sum(F.softplus((a * n).sum(-1) - (a * p).sum(-1))) / a.shape[0]
    reg = reg_w * sum(w.norm(2).square() for w in params)
    users = torch.unique(ancs)
    items = torch.unique(torch.concat([poss, negs]))
    cl = 0.0
    for l in range(L):
        ug, ig = gnn[l][:n_user][users], gnn[l][n_user:][items]
        for other in (inte[l], gaa[l], iaa[l]):
            uo = other[:n_user][users]
            cl = cl + ref_infonce(ug, uo, uo, temp) / ug.shape[0]
        for other in (inte[l], gaa[l], iaa[l]):
            io = other[n_user:][items]
            cl = cl + ref_infonce(ig, io, io, temp) / ug.shape[0]
    cl = cl_w * cl
    return bpr + reg + cl, bpr, reg, cl, final


# ---------------------------------------------------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------------------------------------------------
def test_intent_entry_points_reject_bad_arguments_without_a_gpu():
    from sslrec_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)       # a non-null HOST address: a call that got as far as a launch would fault, these return before
    bad = _lib.E_BADARG
    fwd, bwd, ws = lib.sslrec_intent_fwd_f32, lib.sslrec_intent_bwd_f32, lib.sslrec_intent_ws_bytes
    assert fwd(None, 4, 2, 32, p, p, 8, p, p, None) == bad                      # X is null
    assert fwd(p, 4, 2, 32, p, p, 8, None, p, None) == bad                      # Y is null
    assert fwd(p, 4, 2, 32, None, p, 8, p, p, None) == bad                      # C_u is null, its range is not empty
    assert fwd(p, 4, 2, 32, p, None, 8, p, p, None) == bad                      # C_i likewise
    assert bwd(p, p, p, 4, 2, 32, p, p, 8, None, p, p, p, None) == bad          # dX is null
    assert bwd(p, p, None, 4, 2, 32, p, p, 8, p, p, p, p, None) == bad          # lse is null
    assert bwd(p, None, p, 4, 2, 32, p, p, 8, p, p, p, p, None) == bad          # dY is null
    assert bwd(p, p, p, 4, 2, 32, p, p, 8, p, None, p, p, None) == bad          # dC_u is null, its range is not empty
    assert bwd(p, p, p, 4, 2, 32, p, p, 8, p, p, p, None, None) == bad          # the workspace is null
    for d in (0, 16, 48, 256):
        assert fwd(p, 4, 2, d, p, p, 8, p, p, None) == bad
        assert bwd(p, p, p, 4, 2, d, p, p, 8, p, p, p, p, None) == bad
        assert ws(4, 2, d, 8) == 0
    for k in (0, -1, 257):
        assert fwd(p, 4, 2, 32, p, p, k, p, p, None) == bad
        assert bwd(p, p, p, 4, 2, 32, p, p, k, p, p, p, p, None) == bad
        assert ws(4, 2, 32, k) == 0
    for n_split in (-1, 5):
        assert fwd(p, 4, n_split, 32, p, p, 8, p, p, None) == bad
        assert bwd(p, p, p, 4, n_split, 32, p, p, 8, p, p, p, p, None) == bad
        assert ws(4, n_split, 32, 8) == 0
    assert fwd(p, -1, 0, 32, p, p, 8, p, p, None) == bad
    assert fwd(p, 0, 0, 32, None, None, 8, p, None, None) == 0                  # N = 0: success without a launch
    assert bwd(p, p, p, 0, 0, 32, None, None, 8, p, None, None, None, None) == 0
    assert ws(1200, 700, 32, 128) > 0 and ws(1200, 700, 32, 128) % (32 * 128 * 4) == 0


def test_intent_aggregate_refuses_cpu_tensors():
    from sslrec_amd import ops
    with pytest.raises(RuntimeError, match='HIP device only'):
        ops.intent_aggregate(torch.zeros(8, 32), torch.zeros(32, 16))
    with pytest.raises(RuntimeError, match='HIP device only'):
        ops.intent_aggregate_stacked(torch.zeros(8, 32), 3, torch.zeros(32, 16), torch.zeros(32, 16))


def tiny_handler(device, over=None):
    from helpers import FixtureHandler
    from sslrec_amd.config.configurator import load_config
    from sslrec_amd.data_utils import synth
    overrides = {'data': {'synthetic': 'tiny'}}
    overrides.update(over or {})
    load_config('dccf', device=device, overrides=overrides)
    return FixtureHandler(synth.make_dataset('tiny', 2023)).load_adj_only()


def test_dccf_builds_from_its_config_with_the_reference_draw_order():
    from torch import nn
    from sslrec_amd.config.configurator import configs
    from sslrec_amd.models.bulid_model import build_model
    dh = tiny_handler('cpu')
    m = configs['model']
    assert (m['layer_num'], m['intent_num'], m['embedding_size']) == (2, 128, 32)
    assert (m['reg_weight'], m['cl_weight'], m['temperature']) == (1.0e-4, 1.0e-2, 0.2)
    torch.manual_seed(77)
    model = build_model(dh)
    assert type(model).__name__ == 'DCCF'
    assert {n: tuple(p.shape) for n, p in model.named_parameters()} == {
        'user_embeds': (300, 32), 'item_embeds': (220, 32), 'user_intent': (32, 128), 'item_intent': (32, 128)}
    # the reference's draws, dccf.py:42-45 then :53-55
    torch.manual_seed(77)
    init = nn.init.xavier_uniform_
    user_embeds, item_embeds = nn.Embedding(300, 32), nn.Embedding(220, 32)
    user_intent, item_intent = init(torch.empty(32, 128)), init(torch.empty(32, 128))
    init(user_embeds.weight)
    init(item_embeds.weight)
    assert torch.equal(model.user_embeds, user_embeds.weight) and torch.equal(model.item_embeds, item_embeds.weight)
    assert torch.equal(model.user_intent, user_intent) and torch.equal(model.item_intent, item_intent)
    # a checkpoint of the reference: the tables are nn.Embedding weights there
    sd = {'user_embeds.weight': torch.full((300, 32), 0.5), 'item_embeds.weight': torch.full((220, 32), -0.25),
          'user_intent': torch.ones(32, 128), 'item_intent': torch.zeros(32, 128)}
    model.load_state_dict(sd)
    assert torch.all(model.user_embeds == 0.5) and torch.all(model.item_embeds == -0.25) and torch.all(model.user_intent == 1)
    model.load_state_dict(model.state_dict())                                   # and this project's own names
    assert sorted(model.state_dict()) == ['item_embeds', 'item_intent', 'user_embeds', 'user_intent']
    # entry order of the adaptive graph: .tocsr().tocoo() of both directions stacked (dccf.py:19-25)
    h, t_ = model.all_h_list.numpy(), model.all_t_list.numpy()
    assert np.all(np.diff(h) >= 0) and h.size == 2 * dh.trn_mat.nnz and np.array_equal(np.sort(h), np.sort(t_))


# ---------------------------------------------------------------------------------------------------------------------
# GPU tests: the kernel
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_stacked(d, k, n=N_NODE, n_split=N_USER, x_scale=0.5, c_scale=0.3):
    x, c_u, c_i, r = randn((n, d), 1, x_scale), randn((d, k), 2, c_scale), randn((d, k), 3, c_scale), randn((n, d), 4)

    def fn(dt):
        xx, cu, ci = leaf(x, dt), leaf(c_u, dt), leaf(c_i, dt)
        y = ref_intent(xx, n_split, cu, ci)
        (y * r.to(dt)).sum().backward()
        return {'Y': y.detach(), 'dX': xx.grad, 'dC_u': cu.grad, 'dC_i': ci.grad}
    return (x, c_u, c_i, r) + both_precisions(fn)


def run_stacked(x, c_u, c_i, r, n_split):
    from sslrec_amd import ops
    xx, cu, ci = (gpu(v).requires_grad_(True) for v in (x, c_u, c_i))
    y = ops.intent_aggregate_stacked(xx, n_split, cu, ci)
    assert tuple(y.shape) == tuple(x.shape)
    (y * gpu(r)).sum().backward()
    return {'Y': y.detach(), 'dX': xx.grad, 'dC_u': cu.grad, 'dC_i': ci.grad}


@pytest.mark.gpu
@pytest.mark.parametrize('d,k', [(32, 128), (64, 128), (128, 128), (32, 100), (64, 4), (32, 256), (48, 128)])
def test_intent_stacked_forward_and_all_gradients(d, k):
    x, c_u, c_i, r, r64, r32 = ref_stacked(d, k)
    got = run_stacked(x, c_u, c_i, r, N_USER)
    for name in ('Y', 'dX', 'dC_u', 'dC_i'):
        check('%s d=%d K=%d' % (name, d, k), got[name], r64[name], r32[name])


@pytest.mark.gpu
def test_intent_single_table_and_edge_shapes():
    from sslrec_amd import ops
    d, k = 32, 128
    x, c, r = randn((N_NODE, d), 11, 0.5), randn((d, k), 12, 0.3), randn((N_NODE, d), 13)

    def fn(dt, rows=slice(None)):
        xx, cc = leaf(x[rows], dt), leaf(c, dt)
        y = torch.softmax(xx @ cc, dim=1) @ cc.T
        (y * r[rows].to(dt)).sum().backward()
        return {'Y': y.detach(), 'dX': xx.grad, 'dC': cc.grad}
    r64, r32 = both_precisions(fn)
    xx, cc = gpu(x).requires_grad_(True), gpu(c).requires_grad_(True)
    y = ops.intent_aggregate(xx, cc)                                           # n_split = N
    (y * gpu(r)).sum().backward()
    for name, got in (('Y', y), ('dX', xx.grad), ('dC', cc.grad)):
        check('single %s' % name, got, r64[name], r32[name])
    # n_split = 0: every row uses the item matrix; the user matrix gets a zero gradient
    xx, cu, ci = gpu(x).requires_grad_(True), gpu(2 * c).requires_grad_(True), gpu(c).requires_grad_(True)
    y = ops.intent_aggregate_stacked(xx, 0, cu, ci)
    (y * gpu(r)).sum().backward()
    for name, got in (('Y', y), ('dX', xx.grad), ('dC', ci.grad)):
        check('n_split=0 %s' % name, got, r64[name], r32[name])
    assert torch.all(cu.grad == 0)
    # N = 1
    one64, one32 = both_precisions(lambda dt: fn(dt, slice(0, 1)))
    xx, cc = gpu(x[:1]).requires_grad_(True), gpu(c).requires_grad_(True)
    y = ops.intent_aggregate(xx, cc)
    (y * gpu(r[:1])).sum().backward()
    for name, got in (('Y', y), ('dX', xx.grad), ('dC', cc.grad)):
        check('N=1 %s' % name, got, one64[name], one32[name])
    # N = 0
    xx, cc = torch.zeros(0, d, device=DEV, requires_grad=True), gpu(c).requires_grad_(True)
    y = ops.intent_aggregate(xx, cc)
    assert tuple(y.shape) == (0, d)
    y.sum().backward()
    assert tuple(xx.grad.shape) == (0, d) and torch.all(cc.grad == 0)


@pytest.mark.gpu
def test_intent_large_logits_need_the_max_subtraction():
    d, k = 32, 128
    x, c_u, c_i, r, r64, r32 = ref_stacked(d, k, x_scale=8.0, c_scale=4.0)
    z = torch.concat([x[:N_USER] @ c_u, x[N_USER:] @ c_i])
    assert float(z.max()) >= 100 and float(z.min()) <= -100, (float(z.min()), float(z.max()))      # exp(z) overflows fp32 beyond 88.7
    got = run_stacked(x, c_u, c_i, r, N_USER)
    for name in ('Y', 'dX', 'dC_u', 'dC_i'):
        check('large %s' % name, got[name], r64[name], r32[name])


@pytest.mark.gpu
def test_intent_two_runs_give_the_same_bits():
    x, c_u, c_i, r, _, _ = ref_stacked(64, 128)
    first, second = run_stacked(x, c_u, c_i, r, N_USER), run_stacked(x, c_u, c_i, r, N_USER)
    for name in first:
        assert torch.equal(first[name], second[name]), name


# ---------------------------------------------------------------------------------------------------------------------
# GPU tests: one layer, the whole step, evaluation and training
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_dccf_one_full_layer_all_four_branches():
    from sslrec_amd import ops
    from sslrec_amd.graph import PropGraph
    from sslrec_amd.models.aug_utils import AdaptiveMask
    d, k = 64, 128
    heads_np, tails_np = square_lists()
    heads, tails = lt(heads_np), lt(tails_np)
    deg = np.bincount(heads_np, minlength=N_NODE).astype(np.float64)
    a_hat = torch.from_numpy((deg[heads_np] ** -0.5) * (deg[tails_np] ** -0.5)).float()      # D^-1/2 A D^-1/2 (dccf.py:57-63), rounded once
    e, c_u, c_i, r = randn((N_NODE, d), 21, 0.1), randn((d, k), 22, 0.2), randn((d, k), 23, 0.2), randn((N_NODE, d), 24)

    def fn(dt):
        ee, cu, ci = leaf(e, dt), leaf(c_u, dt), leaf(c_i, dt)
        out = ref_layer(ee, N_USER, cu, ci, a_hat.to(dt), heads, tails, heads, tails)[4]
        (out * r.to(dt)).sum().backward()
        return {'out': out.detach(), 'dE': ee.grad, 'd user_intent': cu.grad, 'd item_intent': ci.grad}
    r64, r32 = both_precisions(fn)
    mask = AdaptiveMask(heads, tails, (N_NODE, N_NODE), device=DEV)
    g = PropGraph(heads_np, tails_np, a_hat.numpy(), (N_NODE, N_NODE), DEV)
    ee, cu, ci = gpu(e).requires_grad_(True), gpu(c_u).requires_grad_(True), gpu(c_i).requires_grad_(True)
    gnn = ops.spmm(g, ee)
    inte = ops.intent_aggregate_stacked(ee, N_USER, cu, ci)
    gaa = mask.propagate(mask(gnn)[1], ee)
    iaa = mask.propagate(mask(inte)[1], ee)
    out = gnn + inte + gaa + iaa + ee
    (out * gpu(r)).sum().backward()
    for name, got in (('out', out), ('dE', ee.grad), ('d user_intent', cu.grad), ('d item_intent', ci.grad)):
        check('layer ' + name, got, r64[name], r32[name])


def tiny_model(d, L, K, precision=None):
    from sslrec_amd.models.bulid_model import build_model
    model_over = {'embedding_size': d, 'layer_num': L, 'intent_num': K}
    if precision:
        model_over['infonce_precision'] = precision
    dh = tiny_handler(DEV, {'model': model_over})
    model = build_model(dh).to(DEV)
    with torch.no_grad():                                                       # seeded fill, the same for the restatement
        for i, (name, p) in enumerate(model.named_parameters()):
            scale = 0.3 if 'intent' in name else 0.1
            p.copy_(gpu(randn(tuple(p.shape), 300 + i, scale)))
    return dh, model


def tiny_batch():
    rng = np.random.RandomState(5)
    ancs = rng.randint(0, 120, 256)                                             # 256 triples over 120 users: repeated users, unique matters
    return lt(ancs), lt(rng.randint(0, 220, 256)), lt(rng.randint(0, 220, 256))


@functools.lru_cache(maxsize=None)
def ref_tiny_step(d, L, K):
    """float64 and fp32 restatement of one cal_loss + backward on `tiny` with the seeded fill of tiny_model"""
    dh = tiny_handler('cpu', {'model': {'embedding_size': d, 'layer_num': L, 'intent_num': K}})
    from sslrec_amd.config.configurator import configs
    n_user, n_item = 300, 220
    adj = dh.torch_adj.coalesce()
    g_heads, g_tails, g_vals = adj.indices()[0], adj.indices()[1], adj.values()
    trn = dh.trn_mat.tocoo()
    import scipy.sparse as sp
    rows = np.concatenate([trn.row, trn.col + n_user])
    cols = np.concatenate([trn.col + n_user, trn.row])
    plain = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=[n_user + n_item] * 2).tocsr().tocoo()
    heads, tails = lt(plain.row), lt(plain.col)
    shapes = [(n_user, d), (n_item, d), (d, K), (d, K)]
    fills = [randn(s, 300 + i, 0.3 if i >= 2 else 0.1).float().double() for i, s in enumerate(shapes)]
    batch = tiny_batch()
    m = configs['model']

    def fn(dt):
        params = [leaf(f, dt) for f in fills]
        loss, bpr, reg, cl, final = ref_step(params, n_user, L, (g_vals.to(dt), g_heads, g_tails), heads, tails, batch, m['temperature'],
                                             m['reg_weight'], m['cl_weight'])
        loss.backward()
        out = {'loss': loss.detach(), 'bpr_loss': bpr.detach(), 'reg_loss': reg.detach(), 'cl_loss': cl.detach(), 'final': final.detach()}
        out.update({'d ' + n: p.grad for n, p in zip(('user_embeds', 'item_embeds', 'user_intent', 'item_intent'), params)})
        return out
    return both_precisions(fn)


def run_tiny_step(d, L, K, precision):
    dh, model = tiny_model(d, L, K, precision)
    loss, parts = model.cal_loss([b.to(DEV) for b in tiny_batch()])
    loss.backward()
    got = {'loss': loss.detach()}
    got.update({k: v.detach() for k, v in parts.items()})
    got.update({'d ' + n: p.grad for n, p in model.named_parameters()})
    return dh, model, got


STEP_TENSORS = ('bpr_loss', 'reg_loss', 'cl_loss', 'loss', 'd user_embeds', 'd item_embeds', 'd user_intent', 'd item_intent')


@pytest.mark.gpu
@pytest.mark.parametrize('d,L,K', [(32, 2, 128), (64, 3, 16)])
def test_dccf_whole_step_fp32_infonce(d, L, K):
    r64, r32 = ref_tiny_step(d, L, K)
    _, _, got = run_tiny_step(d, L, K, 'fp32')
    assert sorted(k for k in got if k.endswith('_loss')) == ['bpr_loss', 'cl_loss', 'reg_loss']
    for name in STEP_TENSORS:
        check('%s d=%d L=%d' % (name, d, L), got[name], r64[name], r32[name])


@pytest.mark.gpu
@pytest.mark.parametrize('d,L,K', [(32, 2, 128), (64, 3, 16)])
def test_dccf_whole_step_default_infonce(d, L, K):
    r64, r32 = ref_tiny_step(d, L, K)
    _, _, got = run_tiny_step(d, L, K, None)
    for name in STEP_TENSORS:
        on_cl_path = name not in ('bpr_loss', 'reg_loss')
        try:
            check('%s d=%d L=%d' % (name, d, L), got[name], r64[name], r32[name])
        except AssertionError:
            if not on_cl_path:
                raise
            ref, x = r64[name], got[name].cpu().double()                        # DESIGN §2's whole-step bars
            rtol, atol = (1e-5, 0.0) if name.endswith('loss') else (1e-4, 1e-7)
            worst = float(((x - ref).abs() - rtol * ref.abs()).max())
            print('%-22s beyond 4 x fp32; whole-step bar rtol %g atol %g: worst excess %.3e' % (name, rtol, atol, worst))
            assert torch.allclose(x, ref, rtol=rtol, atol=atol), name


class _Log:
    def log(self, *a, **k):
        pass

    log_loss = log_eval = log


@pytest.mark.gpu
def test_dccf_evaluation_training_and_checkpoint(tmp_path, monkeypatch):
    from sslrec_amd.config.configurator import configs
    from sslrec_amd.trainer.trainer import Trainer
    d, L, K = 32, 2, 128
    r64, _ = ref_tiny_step(d, L, K)
    dh, model = tiny_model(d, L, K)
    final = r64['final']
    users = lt(np.array([0, 5, 17, 299, 150, 5]))
    trn = dh.trn_mat.tocsr()
    mask = torch.from_numpy(trn[users.numpy()].toarray()).double()
    scores = (final[:300][users] @ final[300:].T) * (1 - mask) - 1e8 * mask
    model.eval()
    got = model.full_predict((users.to(DEV), mask.float().to(DEV)))
    assert torch.allclose(got.cpu().double(), scores, rtol=1e-4, atol=1e-5)
    cached = model.final_embeds
    assert cached is not None and not model.is_training
    rowptr, col = lt(trn.indptr).to(DEV), lt(trn.indices).to(DEV)
    top = model.predict_topk(users.to(DEV), 10, (rowptr, col)).cpu()
    assert model.final_embeds is cached                                         # the second evaluation call reuses the tables
    want_vals = scores.topk(10).values
    assert torch.allclose(scores.gather(1, top), want_vals, rtol=1e-4, atol=1e-5)
    # three optimizer steps of the Trainer's Adam change all four parameters
    trainer = Trainer(dh, _Log())
    trainer.create_optimizer(model)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    model.train()
    batch = [b.to(DEV) for b in tiny_batch()]
    for _ in range(3):
        trainer.optimizer.zero_grad()
        loss, _ = model.cal_loss(batch)
        loss.backward()
        trainer.optimizer.step()
    assert torch.isfinite(loss)
    for n, p in model.named_parameters():
        assert not torch.equal(p.detach(), before[n]), n
    # save_model / load_model round trip
    _, fresh = tiny_model(d, L, K)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(configs['train'], 'save_model', True)
    trainer.save_model(model)
    saved = list((tmp_path / 'checkpoint' / 'dccf').glob('*.pth'))
    assert len(saved) == 1
    monkeypatch.setitem(configs['train'], 'pretrain_path', str(saved[0]))
    trainer.load_model(fresh)
    for (n, p), (_, q) in zip(model.named_parameters(), fresh.named_parameters()):
        assert torch.equal(p, q), n
