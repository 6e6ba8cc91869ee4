"""The typed-edge walks of csrc/rmha.hip (ops.rel_mh_attention, ops.rel_rationale) on the GPU, at the edges of their geometry and of the
keep mask: degrees around the 512-slot chunk, masks defined per chunk, more long destinations than one finishing workgroup holds, more
work items than 2048 workgroups take in one pass, relation tables on both sides of the LDS fit, and a mask against the graph of the kept
edges.  The graphs come from the builders of tests/kg_walk_cases.py (tests/test_kg_walk_cases_host.py checks what they claim); the
tables of the new operation are drawn here.

Yardstick: the project's check(name, got, ref64, ref32) (tests/mhcn_reference.py) against the float64 restatement of
tests/kgrec_reference.py: the kernels' error is at most 4 x the float32 restatement's, floor 8 * 2^-23, both printed.  It is applied to
every whole output and again to the sub-tensor of every class of rows of the case, so that a long list cannot set the scale for a short
one.  Every test first asserts, on the device lists, the geometry it relies on, and ends by repeating its calls and asserting equal
bits."""
import numpy as np
import pytest
import torch

import kg_walk_cases as K
import kgrec_reference as R
from kgrec_reference import check

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

# which outputs carry one row per destination of an order (dt has a share from the walk by head and one from the walk by tail)
MH_OUT = {'head': ('y', 'dt', 'mean_head'), 'tail': ('dx', 'dt', 'mean_tail'), 'rel': ('dr',)}
MH_ALL = ('y', 'dx', 'dt', 'dr')
RAT_ALL = ('score', 'logits', 'mean_head', 'mean_tail')

_GRAPHS, _TABLES, _REFS = {}, {}, {}


def gpu(x):
    return x.detach().float().to(DEV)


def graph_of(case):
    from sslrec_amd.graph import RelGraph
    if case.name not in _GRAPHS:
        _GRAPHS[case.name] = RelGraph(*case.quintuple(), device=DEV)
    return _GRAPHS[case.name]


def assert_claimed_geometry(case, graph):
    """the device lists have the n_long, n_chunks and work items the case claims; -> order: (n_long, n_chunks, items)"""
    from sslrec_amd.graph import REL_CHUNK
    assert REL_CHUNK == K.CHUNK
    out = {}
    for order, ls in (('head', graph.by_head), ('tail', graph.by_tail), ('rel', graph.by_rel)):
        out[order] = (ls.n_long, ls.n_chunks, ls.n_dest + ls.n_chunks)
        assert out[order] == case.claimed_geometry(order), (case.name, order, out[order])
    return out


def tables(case, d):
    """float64 x, t, go [N, d] and r [R, d], the same for every test that asks; t and r are scaled by 0.9 (a logit is a sum of d / 2
    products of three factors over sqrt(d / 2): its standard deviation is 0.9^3).  A twin's rows are copies of its original's."""
    key = (case.name, d)
    if key not in _TABLES:
        t = {'x': R.randn((case.N, d), 21), 't': R.randn((case.N, d), 24, 0.9), 'go': R.randn((case.N, d), 23), 'r': R.randn((case.R, d), 22, 0.9)}
        for order, src, dst in case.twins:
            for name in (('r',) if order == 'rel' else ('x', 't', 'go')):
                t[name][dst] = t[name][src]
        _TABLES[key] = t
    return _TABLES[key]


def reference(case, d, masked):
    """(float64, float32) outputs of the restatement (rel_mh_attention with its four gradients, rel_rationale), computed once"""
    key = (case.name, d, bool(masked))
    if key not in _REFS:
        t = tables(case, d)
        keep = case.keep if masked else None

        def fn(dt):
            leaves = [R.leaf(t[n], dt) for n in ('x', 't', 'r')]
            y = R.rel_mh_attention(*leaves, case.edges, keep)
            (y * t['go'].to(dt)).sum().backward()
            out = dict(zip(MH_ALL, [y.detach()] + [a.grad for a in leaves]))
            out.update(zip(RAT_ALL, R.rel_rationale(t['t'].to(dt), t['r'].to(dt), case.edges, keep)))
            return out
        _REFS[key] = R.both_precisions(fn)
    return _REFS[key]


def run(graph, t, keep):
    from sslrec_amd import ops
    leaves = [gpu(t[n]).requires_grad_(True) for n in ('x', 't', 'r')]
    y = ops.rel_mh_attention(graph, *leaves, keep)
    assert type(y.grad_fn).__name__.startswith('_RelMhAttentionFn')           # the kernels, not the composed form
    (y * gpu(t['go'])).sum().backward()
    out = dict(zip(MH_ALL, [y.detach()] + [a.grad for a in leaves]))
    out.update(zip(RAT_ALL, ops.rel_rationale(graph, gpu(t['t']), gpu(t['r']), keep)))
    return out


def values(case, d):
    """both operations with and without the case's mask against the restatement, whole and per class of rows, every call twice with
    equal bits; -> masked: outputs"""
    graph, t, out = graph_of(case), tables(case, d), {}
    for masked in (False, True):
        keep = case.keep.to(DEV) if masked else None
        got = run(graph, t, keep)
        r64, r32 = reference(case, d, masked)
        tag = '%s d=%d%s' % (case.name, d, ' masked' if masked else '')
        for k in r64:
            check('%s %s' % (tag, k), got[k], r64[k], r32[k])
        for label, (order, ids) in case.rows.items():
            rows = torch.from_numpy(np.asarray(ids, dtype=np.int64))
            for k in (MH_OUT[order] if len(ids) else ()):
                check('%s %s | %s' % (tag, k, label), got[k][rows.to(DEV)], r64[k][rows], r32[k][rows])
        assert all(bool(torch.isfinite(v).all()) for v in got.values())
        if masked:
            off = (~case.keep).to(DEV)
            assert bool((got['score'][off] == 0).all()) and bool((got['logits'][off] == 0).all())
        again = run(graph, t, keep)
        for k in got:
            assert torch.equal(got[k], again[k]), (case.name, d, masked, k)
        out[masked] = got
    return out


def assert_unwritten(got, order, ids):
    """the rows of destinations without a kept slot are exact zeros in every output of that order"""
    ids = torch.as_tensor(list(ids), dtype=torch.long, device=DEV)
    for k in MH_OUT[order]:
        assert bool((got[k][ids] == 0).all()), (order, k)


def assert_one_kept_edge(case, t, got, h, e):
    """head h whose only kept edge is e: the float32 product x[t] * r[rel] bit for bit, and a score of exactly 1"""
    tail, rel = int(case.tail[e]), int(case.rel[e])
    assert int(case.head[e]) == h
    assert torch.equal(got['y'][h], gpu(t['x'])[tail] * gpu(t['r'])[rel])
    assert float(got['score'][e]) == 1.0 and float(got['mean_head'][h]) == 1.0


@pytest.mark.parametrize('d', K.DIMS)
def test_degrees_at_the_chunk_boundary(d):
    case = K.boundary()
    graph = graph_of(case)
    geom = assert_claimed_geometry(case, graph)
    assert geom['head'][:2] == (5, 13) and geom['tail'][:2] == (5, 13) and geom['rel'][:2] == (3, 7)
    assert {0, 1, 511, 512, 513, 1537} <= set(case.degree['head'].values()) and graph.by_head.max_len == 1537
    assert K.lds_fits(case.R, d) and case.R * (d // 4) > K.THREADS                  # the relation table is staged in more than one pass
    res = values(case, d)
    t = tables(case, d)
    nd = len(K.DEGREES)
    for masked, got in res.items():
        for order in ('head', 'tail', 'rel'):
            assert_unwritten(got, order, case.info['empty'][order])
            if masked:
                assert_unwritten(got, order, case.info['masked_out'][order])
        for k in ('dx', 'mean_tail'):                        # an engineered head is nobody's tail, an engineered tail nobody's head
            assert bool((got[k][:nd] == 0).all()), k
        for k in ('y', 'mean_head'):
            assert bool((got[k][nd:2 * nd] == 0).all()), k
        h = case.info['single']['head']
        assert_one_kept_edge(case, t, got, h, int(case.slots[('head', h)][0]))


@pytest.mark.parametrize('d', K.DIMS)
def test_masks_per_chunk(d):
    case = K.masks()
    geom = assert_claimed_geometry(case, graph_of(case))
    assert all(geom[o][:2] == (6, 24) for o in ('head', 'tail', 'rel')) and K.LONG == 3 * K.CHUNK + 1
    got = values(case, d)[True]
    t = tables(case, d)
    var = case.info['variant']
    for order in ('head', 'tail', 'rel'):
        assert_unwritten(got, order, [var[(order, 'all masked')]])                   # a long destination without a kept slot
    for order, src, dst in case.twins:                                               # chunks 1 .. 3 add +0 or merge with weight 0
        for k in MH_OUT[order]:
            assert torch.equal(got[k][src], got[k][dst]), (order, k)
            assert bool((got[k][src] != 0).any())
    h = var[('head', 'last slot only')]                                              # the merge multiplies by expf(0) = 1 and divides by 1
    assert_one_kept_edge(case, t, got, h, int(case.slots[('head', h)][-1]))


@pytest.mark.parametrize('d', K.DIMS)
def test_finishing_launch_of_several_workgroups(d):
    case = K.many_long()
    geom = assert_claimed_geometry(case, graph_of(case))
    for order in ('head', 'tail', 'rel'):
        assert geom[order][0] == 40 > 32 >= K.rpb(d) and -(-geom[order][0] // K.rpb(d)) >= 2
    values(case, d)


@pytest.mark.parametrize('N,d', K.STRIDE_SHAPES)
def test_second_pass_of_the_grid_stride_loop(N, d):
    case = K.stride(N, d)
    geom = assert_claimed_geometry(case, graph_of(case))
    first = K.MAX_BLOCKS * K.rpb(d)
    for order in ('head', 'tail'):
        assert geom[order][0] == 3 and geom[order][1] == 6 and geom[order][2] > first >= case.N - first       # two passes, no third
    assert case.N > first                                                            # so every chunk item falls in the second pass
    values(case, d)


@pytest.mark.parametrize('R_,d', K.LDS_SHAPES)
def test_relation_table_at_the_lds_fit(R_, d):
    case = K.lds_fit(R_, d)
    geom = assert_claimed_geometry(case, graph_of(case))
    assert all(geom[o][0] == 0 for o in geom)
    assert K.lds_fits(R_, d) == (R_ % 2 == 0) and K.lds_fits(R_ - R_ % 2, d) and not K.lds_fits(R_ - R_ % 2 + 1, d)
    assert R_ * (d // 4) > K.THREADS and R_ > case.info['staged_first']
    values(case, d)


@pytest.mark.parametrize('d', K.DIMS)
def test_mask_equals_the_graph_of_the_kept_edges(d):
    from sslrec_amd.graph import RelGraph
    case = K.short()
    graph = graph_of(case)
    sel = case.keep.numpy()
    sub = RelGraph(case.head[sel], case.tail[sel], case.rel[sel], case.N, case.R, device=DEV)
    for g in (graph, sub):
        assert g.by_head.n_long == 0 and g.by_tail.n_long == 0 and g.by_rel.n_long == 0
    assert sub.n_edges == int(sel.sum()) and 0 < sub.n_edges < graph.n_edges
    values(case, d)
    t = tables(case, d)
    masked, plain = run(graph, t, case.keep.to(DEV)), run(sub, t, None)
    for k in masked:                                         # the kept slots are added in the same sequence: the eid indirection
        a = masked[k][case.keep.to(DEV)] if k in ('score', 'logits') else masked[k]
        assert torch.equal(a, plain[k]), k
