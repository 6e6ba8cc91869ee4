"""Learned edge weights: SDDMM, the row normalization of entry values, the value-differentiable SpMM and the AdaptiveMask
module (sslrec_amd/csrc/sddmm.hip, ops.sddmm / edge_cosine_weights / spmm_valued, models/aug_utils.py).

Yardstick of the GPU tests: a float64 torch restatement of the reference's AdaptiveMask (models/aug_utils.py:73-79: F.normalize of
the gathered rows, alpha = (cos + 1) / 2, row sums, .pow(-1).nan_to_num(0, 0, 0), D^-1[head] * alpha) and of the product DCCF
forms with it (models/general_cf/dccf.py:89), gradients by torch autograd.  The tolerance is not a constant: the same
restatement runs in fp32 on the CPU, its error against float64 is measured per tensor as max|x - ref| / max|ref|, and the
kernels may be at most 4 x as far off (they add the same fp32 terms in another order), with a floor of 8 * 2^-23 for tensors
the fp32 restatement happens to get exactly."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

N_USER, N_ITEM = 700, 500
N_NODE = N_USER + N_ITEM
FLOOR = 8 * 2.0 ** -23


# ---------------------------------------------------------------------------------------------------------------------
# fixture graph
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture_edges():
    """(users, items) of the de-duplicated interactions: ~6,000 random ones, user 0 linked to every item but the last (degree 499),
    item 0 linked to 600 random users, user 699 and item 499 without any interaction"""
    rng = np.random.RandomState(1234)
    u = rng.randint(0, N_USER - 1, 6000)
    i = rng.randint(0, N_ITEM - 1, 6000)
    u = np.concatenate([u, np.zeros(N_ITEM - 1, dtype=np.int64), rng.choice(N_USER - 1, 600, replace=False)])
    i = np.concatenate([i, np.arange(N_ITEM - 1), np.zeros(600, dtype=np.int64)])
    key = np.unique(u.astype(np.int64) * N_ITEM + i)
    return key // N_ITEM, key % N_ITEM


@functools.lru_cache(maxsize=None)
def square_lists():
    """both directions of every interaction stacked as in dccf.py:21-23, the entry list randomly permuted"""
    u, i = fixture_edges()
    heads = np.concatenate([u, i + N_USER])
    tails = np.concatenate([i + N_USER, u])
    p = np.random.RandomState(99).permutation(heads.size)
    return heads[p].copy(), tails[p].copy()


@functools.lru_cache(maxsize=None)
def rect_lists():
    """the user -> item half (700 x 500), randomly permuted"""
    u, i = fixture_edges()
    p = np.random.RandomState(7).permutation(u.size)
    return u[p].copy(), i[p].copy()


def table(rows, d, seed):
    return 0.1 * torch.randn(rows, d, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def rand_vec(n, seed, lo=0.0):
    return lo + torch.rand(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement (any dtype, CPU)
# ---------------------------------------------------------------------------------------------------------------------
def ref_weights(head_table, tail_table, heads, tails, n_rows):
    """aug_utils.py:73-79 behind the gathers of dccf.py:83-84"""
    head_e = F.normalize(torch.index_select(head_table, 0, heads))
    tail_e = F.normalize(torch.index_select(tail_table, 0, tails))
    alpha = (torch.sum(head_e * tail_e, dim=1).view(-1) + 1) / 2
    d_inv = torch.zeros(n_rows, dtype=alpha.dtype).index_add(0, heads, alpha).pow(-1).nan_to_num(0, 0, 0).view(-1)
    return d_inv[heads] * alpha


def ref_spmm(vals, heads, tails, x, n_rows):
    """torch_sparse.spmm(indices, values, m, n, x) (dccf.py:89)"""
    return torch.zeros(n_rows, x.shape[1], dtype=x.dtype).index_add(0, heads, vals[:, None] * torch.index_select(x, 0, tails))


def both_precisions(fn):
    """fn(dtype) -> dict of tensors; returns (float64 results, fp32-on-CPU results)"""
    return fn(torch.float64), fn(torch.float32)


def rel_err(x, ref):
    ref = ref.double()
    return float((x.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def check(name, got, ref64, ref32):
    e32, e = rel_err(ref32, ref64), rel_err(got, ref64)
    bound = max(4 * e32, FLOOR)
    print('%-14s kernel %.3e  fp32 torch %.3e  (%.2f / %.2f units of 2^-23 max|ref|)  bound %.3e' % (name, e, e32, e * 2 ** 23, e32 * 2 ** 23, bound))
    assert torch.isfinite(got).all(), name
    assert e <= bound, '%s: kernel error %.3e > bound %.3e (fp32 torch: %.3e)' % (name, e, bound, e32)


def leaf(x, dt):
    """a fresh leaf of dtype dt (never the shared float64 input itself)"""
    return x.detach().to(dt).clone().requires_grad_(True)


def lt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).long()


# ---------------------------------------------------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    from sslrec_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)       # a non-null HOST address: a call that got as far as a launch would fault, these return before
    bad = _lib.E_BADARG
    assert lib.sslrec_sddmm_f32(None, None, None, 4, 4, 4, None, None, 64, None, None, None, None) == bad
    assert lib.sslrec_sddmm_f32(p, p, p, 4, 4, 4, p, p, 64, None, None, None, None) == bad          # out is null
    for d in (0, 4, 48, 512):
        assert lib.sslrec_sddmm_f32(p, p, p, 4, 4, 4, p, p, d, None, None, p, None) == bad
        assert lib.sslrec_row_invnorm_f32(p, 4, d, p, None, None) == bad
        assert lib.sslrec_cosine_finish_f32(p, p, p, p, None, 4, d, p, None) == bad
    assert lib.sslrec_edge_rownorm_fwd_f32(None, None, 4, None, 0, None, None, None, None) == bad
    assert lib.sslrec_edge_rownorm_fwd_f32(p, p, 4, None, 0, p, p, None, None) == bad               # inv_s is null
    assert lib.sslrec_edge_rownorm_fwd_f32(p, p, 4, None, 2, p, p, p, None) == bad                  # long rows announced, list missing
    assert lib.sslrec_edge_rownorm_bwd_f32(None, None, 4, None, 0, None, None, 4, None, 0, None, None, None, None, None, None, None, None) == bad
    assert lib.sslrec_edge_rownorm_bwd_f32(p, p, 4, None, 0, p, p, 4, None, 0, p, p, p, p, p, p, None, None) == bad      # p_tail is null
    assert lib.sslrec_edge_rownorm_bwd_f32(p, p, 4, None, 0, p, p, 4, None, 1, p, p, p, p, p, p, p, None) == bad
    assert lib.sslrec_row_invnorm_f32(None, 4, 64, None, None, None) == bad
    assert lib.sslrec_cosine_finish_f32(None, None, None, None, None, 4, 64, None, None) == bad
    assert lib.sslrec_cosine_finish_f32(p, p, p, None, None, 4, 64, p, None) == bad                 # p_a is null


def test_adaptive_mask_refuses_cpu_tables_and_the_two_tensor_call():
    from sslrec_amd.models.aug_utils import AdaptiveMask
    heads, tails = square_lists()
    mask = AdaptiveMask(lt(heads), lt(tails), (N_NODE, N_NODE))
    assert mask.graph.nnz == heads.size and tuple(mask.graph.shape) == (N_NODE, N_NODE)
    with pytest.raises(RuntimeError, match='HIP device only'):
        mask(torch.zeros(N_NODE, 32))
    with pytest.raises(TypeError, match='NODE table'):
        mask(torch.zeros(heads.size, 32), torch.zeros(heads.size, 32))
    from sslrec_amd import ops
    with pytest.raises(RuntimeError, match='HIP device only'):
        ops.sddmm(mask.graph, torch.zeros(N_NODE, 32), torch.zeros(N_NODE, 32))
    with pytest.raises(RuntimeError, match='HIP device only'):
        ops.spmm_valued(mask.graph, torch.ones(heads.size), torch.zeros(N_NODE, 32))


def test_plan_csr_arrays_are_consistent_with_the_shuffled_coo_entries():
    from sslrec_amd.graph import EDGE_LONG_ROW, PropGraph
    heads, tails = square_lists()
    g = PropGraph(heads, tails, np.ones(heads.size, dtype=np.float32), (N_NODE, N_NODE), 'cpu')
    for plan, rows, cols in ((g.fwd, heads, tails), (g.bwd, tails, heads)):      # both plans number the entries alike
        h = plan.host_csr()
        rowptr, col, perm, roe = h['rowptr'], h['col'], h['perm'], h['row_of_entry']
        assert all(a.dtype == np.int32 for a in h.values())
        assert rowptr.shape == (N_NODE + 1,) and rowptr[0] == 0 and rowptr[-1] == heads.size and np.all(np.diff(rowptr) >= 0)
        assert np.array_equal(np.sort(perm), np.arange(heads.size))
        assert np.array_equal(rows[perm], roe) and np.array_equal(cols[perm], col)
        assert np.array_equal(roe, np.repeat(np.arange(N_NODE), np.diff(rowptr)))
        assert np.array_equal(np.diff(rowptr), np.bincount(rows, minlength=N_NODE))
        assert np.array_equal(h['long_rows'], np.flatnonzero(np.bincount(rows, minlength=N_NODE) > EDGE_LONG_ROW))
    deg = np.bincount(heads, minlength=N_NODE)
    assert deg[N_USER - 1] == 0 and deg[N_NODE - 1] == 0 and deg[0] >= 499 and deg[N_USER] > EDGE_LONG_ROW      # the fixture's promises
    assert g.fwd.host_csr()['long_rows'].tolist() == [N_USER]
    assert not np.array_equal(heads, np.sort(heads))


# ---------------------------------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------------------------------
DEV = 'cuda:0'


def square_graph(vals=None):
    from sslrec_amd.graph import PropGraph
    heads, tails = square_lists()
    vals = np.ones(heads.size, dtype=np.float32) if vals is None else vals
    return PropGraph(heads, tails, vals, (N_NODE, N_NODE), DEV)


def rect_graph():
    from sslrec_amd.graph import PropGraph
    u, i = rect_lists()
    return PropGraph(u, i, np.ones(u.size, dtype=np.float32), (N_USER, N_ITEM), DEV)


def gpu(x):
    return x.detach().float().to(DEV)


@functools.lru_cache(maxsize=None)
def ref_sddmm_square(d):
    heads, tails = (lt(a) for a in square_lists())
    a, b = table(N_NODE, d, 11), table(N_NODE, d, 12)
    fn = lambda dt: (a.to(dt)[heads] * b.to(dt)[tails]).sum(1)
    return (a, b) + both_precisions(fn)


@pytest.mark.gpu
@pytest.mark.parametrize('d', [8, 32, 64, 256])
def test_sddmm_matches_float64(d):
    from sslrec_amd import ops
    a, b, r64, r32 = ref_sddmm_square(d)
    g = square_graph()
    check('sddmm d=%d' % d, ops.sddmm(g, gpu(a), gpu(b)), r64, r32)
    a_dev = gpu(a)
    heads, tails = (lt(x) for x in square_lists())
    fn = lambda dt: (a.to(dt)[heads] * a.to(dt)[tails]).sum(1)
    check('sddmm a=b', ops.sddmm(g, a_dev, a_dev), *both_precisions(fn))                         # the operands may alias


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['fwd', 'bwd'])
def test_sddmm_rectangular_two_tables_and_factors(which):
    from sslrec_amd import ops
    d = 32
    users, items = (lt(x) for x in rect_lists())
    ut, it = table(N_USER, d, 21), table(N_ITEM, d, 22)
    uf, itf = rand_vec(N_USER, 23, 0.5), rand_vec(N_ITEM, 24, 0.5)
    g = rect_graph()
    plain = lambda dt: (ut.to(dt)[users] * it.to(dt)[items]).sum(1)
    scaled = lambda dt: (ut.to(dt)[users] * it.to(dt)[items]).sum(1) * uf.to(dt)[users] * itf.to(dt)[items]
    if which == 'fwd':
        check('rect fwd', ops.sddmm(g, gpu(ut), gpu(it), 'fwd'), *both_precisions(plain))
        check('rect fwd rc', ops.sddmm(g, gpu(ut), gpu(it), 'fwd', gpu(uf), gpu(itf)), *both_precisions(scaled))
    else:       # the transposed plan: rows are items, the entry numbering stays the caller's
        check('rect bwd', ops.sddmm(g, gpu(it), gpu(ut), 'bwd'), *both_precisions(plain))
        check('rect bwd rc', ops.sddmm(g, gpu(it), gpu(ut), 'bwd', gpu(itf), gpu(uf)), *both_precisions(scaled))
    with pytest.raises(ValueError):
        ops.sddmm(g, gpu(it), gpu(ut), 'fwd')


@functools.lru_cache(maxsize=None)
def ref_weights_square(d):
    heads, tails = (lt(a) for a in square_lists())
    s, dw = table(N_NODE, d, 31), rand_vec(heads.numel(), 32) - 0.5

    def fn(dt):
        x = leaf(s, dt)
        w = ref_weights(x, x, heads, tails, N_NODE)
        w.backward(dw.to(dt))
        return {'w': w.detach(), 'dS': x.grad}
    return (s, dw) + both_precisions(fn)


@pytest.mark.gpu
@pytest.mark.parametrize('d', [8, 32, 64, 256])
def test_edge_cosine_weights_forward_and_table_gradient(d):
    from sslrec_amd import ops
    s, dw, r64, r32 = ref_weights_square(d)
    x = gpu(s).requires_grad_(True)
    w = ops.edge_cosine_weights(square_graph(), x)
    w.backward(gpu(dw))
    check('w d=%d' % d, w, r64['w'], r32['w'])
    check('dS d=%d' % d, x.grad, r64['dS'], r32['dS'])


@pytest.mark.gpu
def test_edge_cosine_weights_two_tables_rectangular():
    from sslrec_amd import ops
    d = 32
    users, items = (lt(x) for x in rect_lists())
    ut, it, dw = table(N_USER, d, 41), table(N_ITEM, d, 42), rand_vec(users.numel(), 43) - 0.5

    def fn(dt):
        a, b = leaf(ut, dt), leaf(it, dt)
        w = ref_weights(a, b, users, items, N_USER)
        w.backward(dw.to(dt))
        return {'w': w.detach(), 'dH': a.grad, 'dT': b.grad}
    r64, r32 = both_precisions(fn)
    a, b = gpu(ut).requires_grad_(True), gpu(it).requires_grad_(True)
    w = ops.edge_cosine_weights(rect_graph(), a, b)
    w.backward(gpu(dw))
    check('rect w', w, r64['w'], r32['w'])
    check('rect dH', a.grad, r64['dH'], r32['dH'])
    check('rect dT', b.grad, r64['dT'], r32['dT'])


@functools.lru_cache(maxsize=None)
def ref_spmm_valued(d):
    heads, tails = (lt(a) for a in square_lists())
    vals, x, r = rand_vec(heads.numel(), 51, 0.1), table(N_NODE, d, 52), table(N_NODE, d, 53)

    def fn(dt):
        v, xx = leaf(vals, dt), leaf(x, dt)
        y = ref_spmm(v, heads, tails, xx, N_NODE)
        (y * r.to(dt)).sum().backward()
        return {'Y': y.detach(), 'dX': xx.grad, 'dvals': v.grad}
    return (vals, x, r) + both_precisions(fn)


@pytest.mark.gpu
@pytest.mark.parametrize('d,swept', [(32, True), (64, True), (32, False), (64, False), (48, True)])
def test_spmm_valued_product_and_both_gradients(d, swept, monkeypatch):
    from sslrec_amd import ops
    monkeypatch.setenv('SSLREC_SPMM_SWEPT', '1' if swept else '0')
    vals, x, r, r64, r32 = ref_spmm_valued(d)
    g = square_graph()                                            # a fresh graph: the choice of layout is cached per plan
    dk = 64 if d == 48 else d                                     # 48 runs zero-padded to 64
    assert (g.fwd.swept(dk) is not None) == swept and (g.bwd.swept(dk) is not None) == swept
    v, xx = gpu(vals).requires_grad_(True), gpu(x).requires_grad_(True)
    y = ops.spmm_valued(g, v, xx)
    assert tuple(y.shape) == (N_NODE, d)
    (y * gpu(r)).sum().backward()
    for name, got in (('Y', y), ('dX', xx.grad), ('dvals', v.grad)):
        check('%s d=%d %s' % (name, d, 'swept' if swept else 'streamed'), got, r64[name], r32[name])


def run_composition(d):
    """AdaptiveMask.forward + propagate on the GPU: (w, Y, dS, dX)"""
    from sslrec_amd.models.aug_utils import AdaptiveMask
    heads, tails = (lt(a) for a in square_lists())
    s, x, r = table(N_NODE, d, 61), table(N_NODE, d, 62), table(N_NODE, d, 63)
    mask = AdaptiveMask(heads.to(DEV), tails.to(DEV), (N_NODE, N_NODE))
    ss, xx = gpu(s).requires_grad_(True), gpu(x).requires_grad_(True)
    idx, w = mask(ss)
    assert torch.equal(idx.cpu(), torch.stack([heads, tails]))
    y = mask.propagate(w, xx)
    (y * gpu(r)).sum().backward()
    return {'w': w.detach(), 'Y': y.detach(), 'dS': ss.grad, 'dX': xx.grad}


@functools.lru_cache(maxsize=None)
def ref_composition(d):
    heads, tails = (lt(a) for a in square_lists())
    s, x, r = table(N_NODE, d, 61), table(N_NODE, d, 62), table(N_NODE, d, 63)

    def fn(dt):
        ss, xx = leaf(s, dt), leaf(x, dt)
        w = ref_weights(ss, ss, heads, tails, N_NODE)
        y = ref_spmm(w, heads, tails, xx, N_NODE)
        (y * r.to(dt)).sum().backward()
        return {'w': w.detach(), 'Y': y.detach(), 'dS': ss.grad, 'dX': xx.grad}
    return both_precisions(fn)


@pytest.mark.gpu
@pytest.mark.parametrize('d', [32, 64])
def test_adaptive_mask_forward_plus_propagate(d):
    r64, r32 = ref_composition(d)
    got = run_composition(d)
    for name in ('w', 'Y', 'dS', 'dX'):
        check('%s d=%d' % (name, d), got[name], r64[name], r32[name])


@pytest.mark.gpu
def test_dccf_graph_layer_half_gradient_through_three_paths():
    """gnn = A^ E, gaa = A(w(gnn)) E, loss on gnn + gaa + E (dccf.py:74, :83-89, :97 without the intent terms): E receives gradient
    through the normalized product, through the learned values and through the valued product's operand"""
    from sslrec_amd import ops
    from sslrec_amd.models.aug_utils import AdaptiveMask
    d = 64
    heads_np, tails_np = square_lists()
    heads, tails = lt(heads_np), lt(tails_np)
    deg = np.bincount(heads_np, minlength=N_NODE).astype(np.float64)
    a_hat = torch.from_numpy((deg[heads_np] ** -0.5) * (deg[tails_np] ** -0.5)).float()      # D^-1/2 A D^-1/2 (dccf.py:57-63), rounded once
    e, r = table(N_NODE, d, 71), table(N_NODE, d, 72)

    def fn(dt):
        ee = leaf(e, dt)
        gnn = ref_spmm(a_hat.to(dt), heads, tails, ee, N_NODE)
        gaa = ref_spmm(ref_weights(gnn, gnn, heads, tails, N_NODE), heads, tails, ee, N_NODE)
        out = gnn + gaa + ee
        (out * r.to(dt)).sum().backward()
        return {'out': out.detach(), 'dE': ee.grad}
    r64, r32 = both_precisions(fn)
    mask = AdaptiveMask(heads, tails, (N_NODE, N_NODE), device=DEV)
    ee = gpu(e).requires_grad_(True)
    gnn = ops.spmm(square_graph(a_hat.numpy()), ee)
    gaa = mask.propagate(mask(gnn)[1], ee)
    out = gnn + gaa + ee
    (out * gpu(r)).sum().backward()
    check('layer out', out, r64['out'], r32['out'])
    check('layer dE', ee.grad, r64['dE'], r32['dE'])


@pytest.mark.gpu
def test_empty_rows_give_zero_and_two_runs_give_the_same_bits():
    from sslrec_amd import ops
    from sslrec_amd.graph import DroppedView
    first, second = run_composition(64), run_composition(64)
    for name in first:
        assert torch.equal(first[name], second[name]), name          # no atomics anywhere: bit-reproducible
        assert torch.isfinite(first[name]).all(), name
    for empty in (N_USER - 1, N_NODE - 1):                           # the user and the item without interactions: inv_s = 0
        assert torch.all(first['Y'][empty] == 0)
        assert torch.all(first['dS'][empty] == 0) and torch.all(first['dX'][empty] == 0)
    g = square_graph()
    dropped = DroppedView(g, torch.ones(g.nnz, dtype=torch.bool))
    x = torch.zeros(N_NODE, 32, device=DEV)
    for call in (lambda: ops.sddmm(dropped, x, x), lambda: ops.edge_cosine_weights(dropped, x),
                 lambda: ops.spmm_valued(dropped, torch.ones(g.nnz, device=DEV), x)):
        with pytest.raises(ValueError, match='edge-dropped'):
            call()
