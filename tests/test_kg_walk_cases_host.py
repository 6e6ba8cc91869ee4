"""What the graphs of tests/kg_walk_cases.py and the restatements must meet on their own, without a GPU: every claimed degree, slot order,
n_long, n_chunks and work-item count holds in graph.RelGraph's three host lists, the masks keep what they claim per chunk, the prescribed
logits are what they claim in float64, the float64 and float32 restatements are finite on every case, and the composed float64 forms of
ops.rel_aggregate / ops.rel_attention agree with the restatements to 1e-12 (the bound of test_kgin_host.py / test_kgcl_host.py), which
validates the yardstick of test_kg_walk_edges.py on these graphs."""
import numpy as np
import pytest
import torch

import kg_walk_cases as K

BUILDERS = [('boundary', K.boundary), ('masks', K.masks), ('many_long', K.many_long), ('short', K.short), ('logit_order', K.logit_order)]
BUILDERS += [('stride-%d-%d' % s, (lambda s=s: K.stride(*s))) for s in K.STRIDE_SHAPES]
BUILDERS += [('lds_fit-%d-%d' % s, (lambda s=s: K.lds_fit(*s))) for s in K.LDS_SHAPES]
CASE_IDS = [b[0] for b in BUILDERS]
ORDERS = ('head', 'tail', 'rel')


def host_lists(case):
    from sslrec_amd.graph import RelGraph
    return dict(zip(ORDERS, RelGraph(*case.quintuple()).host_lists()))


def assert_close(name, got, want, rel=1e-12):
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= rel * max(scale, 1e-300), name


def test_constants_are_the_projects():
    from sslrec_amd import graph, ops
    assert K.CHUNK == graph.REL_CHUNK and K.DIMS == tuple(ops.KGIN_DIMS)
    assert len(K.all_cases()) == len(BUILDERS)
    a, b = K.boundary(), K.boundary()
    assert a is b                                           # built once
    K.boundary.cache_clear()
    c = K.boundary()                                        # and the same when built again
    assert all(np.array_equal(x, y) for x, y in zip(a.quintuple()[:3], c.quintuple()[:3])) and torch.equal(a.keep, c.keep)


@pytest.mark.parametrize('build', [b[1] for b in BUILDERS], ids=CASE_IDS)
def test_geometry_is_as_claimed_in_all_three_orders(build):
    case = build()
    lists = host_lists(case)
    assert case.E == case.head.size == case.tail.size == case.rel.size
    assert case.head.min() >= 0 and case.head.max() < case.N and case.tail.min() >= 0 and case.tail.max() < case.N
    assert case.rel.min() >= 0 and case.rel.max() < case.R
    for order in ORDERS:
        ls = lists[order]
        ptr, eid = ls.ptr.numpy().astype(np.int64), ls.eid.numpy().astype(np.int64)
        deg = np.diff(ptr)
        assert deg.size == case.n_dest(order) == ls.n_dest
        claimed = case.degree[order]
        for i, n in claimed.items():
            assert deg[i] == n, (order, i, int(deg[i]), n)
        rest = np.setdiff1d(np.arange(deg.size), np.fromiter(claimed.keys(), dtype=np.int64, count=len(claimed)))
        assert rest.size == 0 or deg[rest].max() <= K.CHUNK, order          # what has no claim is not long
        n_long, n_chunks, items = case.claimed_geometry(order)
        assert (ls.n_long, ls.n_chunks, ls.n_dest + ls.n_chunks) == (n_long, n_chunks, items), order
        # slot k of an engineered destination is the k-th edge of its group, and chunk c starts at slot c * CHUNK
        for (o, i), ids in case.slots.items():
            if o == order:
                assert np.array_equal(eid[ptr[i]:ptr[i + 1]], ids), (order, i)
        cd, cb = ls.chunk_dest.numpy().astype(np.int64), ls.chunk_begin.numpy().astype(np.int64)
        for j, i in enumerate(ls.long_dest.numpy()):
            c0, c1 = int(ls.long_ptr[j]), int(ls.long_ptr[j + 1])
            assert c1 - c0 == (deg[i] + K.CHUNK - 1) // K.CHUNK and np.all(cd[c0:c1] == i)
            assert np.array_equal(cb[c0:c1], ptr[i] + K.CHUNK * np.arange(c1 - c0))
    # engineered destinations take their partners from the plain ranges only: no engineered id occurs outside its own group
    for (o, i), ids in case.slots.items():
        assert np.array_equal(np.sort(np.nonzero(case.dest(o) == i)[0]), np.sort(ids)), (o, i)
    for label, (order, ids) in case.rows.items():
        assert len(ids) == 0 or (0 <= min(ids) and max(ids) < case.n_dest(order)), label


def test_boundary_claims():
    case = K.boundary()
    lists = host_lists(case)
    assert (case.N, case.R) == (1500, 40) and case.E == 2 * sum(K.DEGREES) + sum(K.REL_DEGREES) + 3000
    for order, want in (('head', K.DEGREES), ('tail', K.DEGREES), ('rel', K.REL_DEGREES)):
        assert sorted(n for i, n in case.degree[order].items() if i < (len(K.REL_DEGREES) if order == 'rel' else 2 * len(K.DEGREES))) == sorted(want)
        assert lists[order].n_long == sum(n > K.CHUNK for n in want) and lists[order].n_chunks == sum(-(-n // K.CHUNK) for n in want if n > K.CHUNK)
    assert np.bincount(case.rel, minlength=case.R)[len(K.REL_DEGREES):].min() >= 1          # every plain relation is used
    keep = case.keep.numpy()
    for order in ('head', 'tail'):
        one = case.info['single'][order]
        assert case.degree[order][one] == 1 and keep[case.slots[(order, one)]].all()
    for order in ORDERS:
        for i in case.info['masked_out'][order]:
            assert case.degree[order][i] >= 1 and not keep[case.slots[(order, i)]].any()
        for i in case.info['empty'][order]:
            assert case.degree[order][i] == 0


def test_mask_variants_keep_what_they_claim_per_chunk():
    case = K.masks()
    lists = host_lists(case)
    keep = case.keep.numpy()
    want = {'all kept': [512, 512, 512, 1], 'chunk 1 masked': [512, 0, 512, 1], 'chunk 0 masked': [0, 512, 512, 1], 'last slot only': [0, 0, 0, 1],
            'all masked': [0, 0, 0, 0], 'chunk 0 only': [512, 0, 0, 0], 'twin': [512]}
    assert set(want) == set(K.VARIANTS)
    for order in ORDERS:
        ls = lists[order]
        ptr, eid = ls.ptr.numpy().astype(np.int64), ls.eid.numpy().astype(np.int64)
        for name in K.VARIANTS:
            i = case.info['variant'][(order, name)]
            mine = np.nonzero(case.dest(order) == i)[0]                     # the caller's order: edge k lies in chunk k // CHUNK
            got = [int(keep[mine[c:c + K.CHUNK]].sum()) for c in range(0, mine.size, K.CHUNK)]
            assert got == want[name], (order, name, got)
            assert np.array_equal(eid[ptr[i]:ptr[i + 1]], mine)             # and the list walks it in that order
        # the twin repeats the first chunk of 'chunk 0 only': the same partners in the same slots
        _, src, dst = [t for t in case.twins if t[0] == order][0]
        a, b = case.slots[(order, src)][:K.CHUNK], case.slots[(order, dst)]
        for col in ORDERS:
            if col != order:
                assert np.array_equal(case.dest(col)[a], case.dest(col)[b]), (order, col)
        t = K.tables(case, 32)
        for name in (('r', 'w') if order == 'rel' else ('x', 'p', 'q', 'go')):
            assert torch.equal(t[name][src], t[name][dst])


def test_logit_order_sequences_are_as_claimed_in_float64():
    case = K.logit_order()
    assert len(case.logit) == len(K.SEQUENCES) == 7
    for d in K.DIMS:
        t = K.tables(case, d)
        for name, h in case.info['head_of'].items():
            ids = case.slots[('head', h)]
            tails = case.tail[ids]
            assert np.unique(tails).size == K.N_SLOTS == ids.size and np.all(case.rel[ids] == 0) and np.all(case.head[ids] == h)
            l64 = ((t['p'][h] + t['q'][tails]) * t['r'][0]).sum(-1)
            l32 = ((t['p'][h].float() + t['q'][tails].float()) * t['r'][0].float()).sum(-1)
            assert bool(((l64 - torch.from_numpy(case.logit[h])).abs() <= 1e-12 * 300).all())
            if name in ('ascending', 'descending'):
                step = l64[1:] - l64[:-1]
                assert bool((step > 0).all() if name == 'ascending' else (step < 0).all())
                assert float(l64.max() - l64.min()) >= 600 * (1 - 1e-12)
            elif name.startswith('maximum'):
                at = int(name.split()[-1])
                assert int(l64.argmax()) == at and int((l64 == l64.max()).sum()) == 1 and float(l64.max() - l64.min()) >= 600 * (1 - 1e-12)
                assert at // K.CHUNK == (1 if at else 0)
            elif name.startswith('all equal'):
                assert bool((l64 == l64[0]).all()) and bool((l32 == l32[0]).all()) and abs(abs(float(l64[0])) - 300) < 1e-9
            else:
                assert bool((l64[::2] == 0).all()) and bool((l32[::2] == 0).all()) and bool((l64[1::2] != 0).all())
                assert bool((l64[1::2] > 0).any()) and bool((l64[1::2] < 0).any())


@pytest.mark.parametrize('slope', [0.0, 0.2, 1.0])
def test_logit_dp_scale_bounds_the_terms_of_dp(slope):
    """the scale dP of logit_order is measured against is at least the sum of the magnitudes of dP's terms dl_e R[0] = dQ[t_e]"""
    case, d = K.logit_order(), 64
    for masked in (False, True):
        dq = K.reference(case, d, 'att', masked, slope)[0]['dq']
        for h in case.logit:
            scale = K.logit_dp_scale(case, d, h, masked, slope)
            terms = dq[torch.from_numpy(case.tail[case.slots[('head', h)]])]
            assert np.isfinite(scale) and scale > 0 and float(terms.abs().sum(0).max()) <= scale * (1 + 1e-9), (h, masked)


def _ops_of(case):
    return ('att',) if case.logit is not None else ('agg', 'att')


@pytest.mark.parametrize('build', [b[1] for b in BUILDERS], ids=CASE_IDS)
def test_restatements_are_finite_in_both_precisions(build):
    case = build()
    for d in case.dims:
        for op in _ops_of(case):
            for masked in (False, True):
                for ref in K.reference(case, d, op, masked):
                    assert set(ref) == set(K.AGG_ALL if op == 'agg' else K.ATT_ALL)
                    for k, v in ref.items():
                        assert bool(torch.isfinite(v).all()), (case.name, d, op, masked, k, v.dtype)
                r64, r32 = K.reference(case, d, op, masked)
                assert all(r64[k].dtype == torch.float64 and r32[k].dtype == torch.float32 for k in r64)
                assert K.reference(case, d, op, masked)[0] is r64          # computed once


@pytest.mark.parametrize('U,d,F', K.FM_SHAPES)
def test_factor_modulate_restatement_is_finite_and_the_loop_has_two_passes(U, d, F):
    r64, r32 = K.fm_reference(U, d, F)
    assert set(r64) == set(K.FM_OUT) and all(bool(torch.isfinite(v).all()) for ref in (r64, r32) for v in ref.values())
    G, rows, passes = K.fm_geometry(U, d)
    assert passes >= 2 and G <= K.MAX_ROW_BLOCKS and (G - 1) * rows < U < G * rows
    if F == 1:                                              # a softmax over one factor is the constant 1
        assert bool((r64['d_u'] == 0).all()) and bool((r64['d_latent'] == 0).all())


@pytest.mark.parametrize('slope', [0.0, 0.01, 1.0])
def test_slope_restatements_are_finite(slope):
    for case, d in ((K.boundary(), 64), (K.logit_order(), 64)):
        for ref in K.reference(case, d, 'att', False, slope):
            assert all(bool(torch.isfinite(v).all()) for v in ref.values())


@pytest.mark.parametrize('build', [b[1] for b in BUILDERS], ids=CASE_IDS)
def test_composed_float64_forms_agree_with_the_restatements(build):
    from sslrec_amd import ops
    from sslrec_amd.graph import RelGraph
    case = build()
    d = case.dims[0]
    graph = RelGraph(*case.quintuple())
    t = K.tables(case, d)
    for masked in (False, True):
        keep = case.keep if masked else None
        if 'agg' in _ops_of(case):
            x, w = K.leaf(t['x'], torch.float64), K.leaf(t['w'], torch.float64)
            y = ops.rel_aggregate(graph, x, w, keep)
            (y * t['go']).sum().backward()
            want = K.reference(case, d, 'agg', masked)[0]
            for k, got in zip(K.AGG_ALL, (y.detach(), x.grad, w.grad)):
                assert_close('%s agg %s' % (case.name, k), got, want[k])
        leaves = [K.leaf(t[n], torch.float64) for n in ('x', 'p', 'q', 'r')]
        y = ops.rel_attention(graph, *leaves, keep)
        (y * t['go']).sum().backward()
        want = K.reference(case, d, 'att', masked)[0]
        for k, got in zip(K.ATT_ALL, (y.detach(), leaves[0].grad, leaves[1].grad, leaves[2].grad, leaves[3].grad)):
            assert_close('%s att %s' % (case.name, k), got, want[k])


def test_equal_logits_give_the_mean_of_the_tail_rows():
    case = K.logit_order()
    t = K.tables(case, 32)
    for masked in (False, True):
        y = K.reference(case, 32, 'att', masked)[0]['y']
        for name in ('all equal +300', 'all equal -300'):
            h = case.info['head_of'][name]
            ids = case.slots[('head', h)]
            if masked:
                ids = ids[case.keep.numpy()[ids]]
            assert_close(name, y[h], t['x'][torch.from_numpy(case.tail[ids])].mean(0), 1e-12)
