"""The typed-edge walks of csrc/kgin.hip (ops.rel_aggregate, ops.factor_modulate) and csrc/rgat.hip (ops.rel_attention) on the GPU, at the
edges of their geometry and of the keep mask: degrees around the 512-slot chunk, masks defined per chunk, more long destinations than one
finishing workgroup holds, more work items than 2048 workgroups take in one pass, relation tables on both sides of the LDS fit and staged
in several passes, logits in a prescribed slot order, slopes 0 / 0.01 / 1, and factor_modulate with several passes per workgroup.  The
graphs come from tests/kg_walk_cases.py; tests/test_kg_walk_cases_host.py checks what they claim.

Yardstick: the project's check(name, got, ref64, ref32) (tests/mhcn_reference.py) against the float64 restatements of
tests/kgin_reference.py / tests/kgcl_reference.py: the kernels' error is at most 4 x the float32 restatement's, floor 8 * 2^-23, both
printed.  It is applied to every whole output and again to the sub-tensor of every class of rows of the case, so that a long list
cannot set the scale for a short one.  One output has no scale of its own: dP of the logit_order heads is 0 in exact arithmetic (one
relation per head, and the ds_e of a softmax add up to 0), so it is measured against the magnitude of its operands before they cancel,
with the same factor and floor (check_cancelling).  Every test first asserts, on the device lists, the geometry it relies on, and ends by repeating
its calls and asserting equal bits."""
import numpy as np
import pytest
import torch

import kg_walk_cases as K
from kgin_reference import FLOOR, check

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

_GRAPHS = {}


def gpu(x):
    return x.detach().float().to(DEV)


def graph_of(case):
    from sslrec_amd.graph import RelGraph
    if case.name not in _GRAPHS:
        _GRAPHS[case.name] = RelGraph(*case.quintuple(), device=DEV)
    return _GRAPHS[case.name]


def lists_of(graph):
    return {'head': graph.by_head, 'tail': graph.by_tail, 'rel': graph.by_rel}


def assert_claimed_geometry(case, graph):
    """the device lists have the n_long, n_chunks and work items the case claims; -> order: (n_long, n_chunks, items)"""
    from sslrec_amd.graph import REL_CHUNK
    assert REL_CHUNK == K.CHUNK
    out = {}
    for order, ls in lists_of(graph).items():
        out[order] = (ls.n_long, ls.n_chunks, ls.n_dest + ls.n_chunks)
        assert out[order] == case.claimed_geometry(order), (case.name, order, out[order])
    return out


def run_agg(graph, t, keep):
    """ops.rel_aggregate forward and backward: the outputs and the integer count of kept edges per head the kernel wrote"""
    from sslrec_amd import ops
    x, w = gpu(t['x']).requires_grad_(True), gpu(t['w']).requires_grad_(True)
    y = ops.rel_aggregate(graph, x, w, keep)
    assert type(y.grad_fn).__name__.startswith('_RelAggregateFn')           # the kernels, not the composed form
    cnt = y.grad_fn.saved_tensors[2].clone()
    (y * gpu(t['go'])).sum().backward()
    return {'y': y.detach(), 'dx': x.grad, 'dw': w.grad, 'cnt': cnt}


def run_att(graph, t, keep, slope=0.2):
    from sslrec_amd import ops
    leaves = [gpu(t[n]).requires_grad_(True) for n in ('x', 'p', 'q', 'r')]
    y = ops.rel_attention(graph, *leaves, keep, slope)
    assert type(y.grad_fn).__name__.startswith('_RelAttentionFn')
    (y * gpu(t['go'])).sum().backward()
    return dict(zip(K.ATT_ALL, [y.detach(), leaves[0].grad, leaves[1].grad, leaves[2].grad, leaves[3].grad]))


RUN = {'agg': run_agg, 'att': run_att}


def check_outputs(case, d, op, masked, got, slope=0.2):
    """check on every whole output, then on the rows of every class of the case"""
    r64, r32 = K.reference(case, d, op, masked, slope)
    tag = '%s d=%d %s%s%s' % (case.name, d, op, ' masked' if masked else '', '' if slope == 0.2 else ' slope %g' % slope)
    one_relation = case.logit is not None                  # logit_order: dP[h] is 0 in exact arithmetic, see check_cancelling
    for k in r64:
        if not (one_relation and k == 'dp'):
            check('%s %s' % (tag, k), got[k], r64[k], r32[k])
    for label, k, rows in K.row_groups(case, op):
        if not (one_relation and k == 'dp'):
            check('%s %s | %s' % (tag, k, label), got[k][rows.to(DEV)], r64[k][rows], r32[k][rows])
    if one_relation:
        nh = len(case.logit)
        assert bool((got['dp'][nh:] == 0).all())             # a tail has no outbound edge
        for name, h in case.info['head_of'].items():
            check_cancelling('%s dp | head: %s' % (tag, name), got['dp'][h], r64['dp'][h], r32['dp'][h], K.logit_dp_scale(case, d, h, masked, slope))


def check_cancelling(name, got, ref64, ref32, scale):
    """check's rule -- the kernel at most 4 x as far from float64 as the float32 restatement, floor 8 * 2^-23 -- for a row that is 0, or
    nearly, in exact arithmetic (kg_walk_cases.logit_order: dP[h] = R[0] sum_e dl_e with sum_e dl_e = 0).  max|ref| is then no scale:
    both errors are measured against `scale`, the magnitude of the operands before they cancel (kg_walk_cases.logit_dp_scale)."""
    e = float((got.detach().cpu().double() - ref64).abs().max()) / scale
    e32 = float((ref32.double() - ref64).abs().max()) / scale
    bound = max(4 * e32, FLOOR)
    print('%-40s kernel %.3e  fp32 torch %.3e  (%.2f / %.2f units of 2^-23 sum|operands|)  bound %.3e' % (name, e, e32, e * 2 ** 23, e32 * 2 ** 23, bound))
    assert torch.isfinite(got).all(), name
    assert e <= bound, '%s: kernel error %.3e > bound %.3e (fp32 torch: %.3e)' % (name, e, bound, e32)


def values(case, d, ops_=('agg', 'att')):
    """both operations with and without the case's mask against the restatements, every call twice with equal bits;
    -> (op, masked): outputs"""
    graph = graph_of(case)
    t = K.tables(case, d)
    out = {}
    for op in ops_:
        for masked in (False, True):
            keep = case.keep.to(DEV) if masked else None
            got = RUN[op](graph, t, keep)
            check_outputs(case, d, op, masked, got)
            assert all(bool(torch.isfinite(v).all()) for v in got.values())
            again = RUN[op](graph, t, keep)
            for k in got:
                assert torch.equal(got[k], again[k]), (case.name, d, op, masked, k)
            out[(op, masked)] = got
    return out


def assert_unwritten(got, order, ids):
    """the rows of destinations without a kept slot are exact zeros in every output of that order (and the kgin count is 0)"""
    ids = torch.as_tensor(list(ids), dtype=torch.long, device=DEV)
    outs = K.AGG_OUT if 'dw' in got else K.ATT_OUT
    for k in outs[order]:
        assert bool((got[k][ids] == 0).all()), (order, k)
    if order == 'head' and 'cnt' in got:
        assert bool((got['cnt'][ids] == 0).all())


def assert_one_kept_edge(case, t, res, masked, h, e):
    """head h whose only kept edge is e: rgat gives x[t] and kgin the float32 product x[t] * w[r], bit for bit"""
    x, w = gpu(t['x']), gpu(t['w'])
    tail, rel = int(case.tail[e]), int(case.rel[e])
    assert int(case.head[e]) == h
    assert torch.equal(res[('att', masked)]['y'][h], x[tail])
    assert torch.equal(res[('agg', masked)]['y'][h], x[tail] * w[rel]) and int(res[('agg', masked)]['cnt'][h]) == 1


# ---------------------------------------------------------------------------------------------------------------------
# degrees at the chunk boundary
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', K.DIMS)
def test_degrees_at_the_chunk_boundary(d):
    case = K.boundary()
    graph = graph_of(case)
    geom = assert_claimed_geometry(case, graph)
    assert geom['head'][:2] == (5, 13) and geom['tail'][:2] == (5, 13) and geom['rel'][:2] == (3, 7)      # 513, 1023, 1024, 1025, 1537 / 513, 1024, 1025
    assert {512, 513} <= set(case.degree['head'].values()) and graph.by_head.max_len == 1537
    assert K.lds_fits(case.R, d) and case.R * (d // 4) > K.THREADS                  # the relation table is staged in more than one pass
    res = values(case, d)
    t = K.tables(case, d)
    nd = len(K.DEGREES)
    for (op, masked), got in res.items():
        for order in ('head', 'tail', 'rel'):
            assert_unwritten(got, order, case.info['empty'][order])
            if masked:
                assert_unwritten(got, order, case.info['masked_out'][order])
        assert_unwritten(got, 'tail', range(nd))             # an engineered head is nobody's tail, an engineered tail nobody's head
        assert_unwritten(got, 'head', range(nd, 2 * nd))
    for masked in (False, True):
        h = case.info['single']['head']
        assert_one_kept_edge(case, t, res, masked, h, int(case.slots[('head', h)][0]))


# ---------------------------------------------------------------------------------------------------------------------
# masks defined per chunk
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', K.DIMS)
def test_masks_per_chunk(d):
    case = K.masks()
    graph = graph_of(case)
    geom = assert_claimed_geometry(case, graph)
    assert all(geom[o][:2] == (6, 24) for o in ('head', 'tail', 'rel'))              # six destinations of 512 + 512 + 512 + 1 slots; the twin is short
    assert K.LONG == 3 * K.CHUNK + 1
    res = values(case, d)
    t = K.tables(case, d)
    var = case.info['variant']
    for op in ('agg', 'att'):
        got = res[(op, True)]
        for order in ('head', 'tail', 'rel'):
            assert_unwritten(got, order, [var[(order, 'all masked')]])               # a long destination without a kept slot
        outs = K.AGG_OUT if op == 'agg' else K.ATT_OUT
        for order, src, dst in case.twins:                                           # chunks 1 .. 3 add +0 or merge with weight 0
            for k in outs[order]:
                assert torch.equal(got[k][src], got[k][dst]), (op, order, k)
                assert bool((got[k][src] != 0).any())
    h = var[('head', 'last slot only')]                                              # the merge multiplies by expf(0) = 1 and divides by 1
    assert_one_kept_edge(case, t, res, True, h, int(case.slots[('head', h)][-1]))


# ---------------------------------------------------------------------------------------------------------------------
# more long destinations than one finishing workgroup holds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', K.DIMS)
def test_finishing_launch_of_several_workgroups(d):
    case = K.many_long()
    geom = assert_claimed_geometry(case, graph_of(case))
    for order in ('head', 'tail', 'rel'):
        assert geom[order][0] == 40 > 32 >= K.rpb(d) and -(-geom[order][0] // K.rpb(d)) >= 2
    values(case, d)


# ---------------------------------------------------------------------------------------------------------------------
# more work items than the workgroups take in one pass
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,d', K.STRIDE_SHAPES)
def test_second_pass_of_the_grid_stride_loop(N, d):
    case = K.stride(N, d)
    geom = assert_claimed_geometry(case, graph_of(case))
    first = K.MAX_BLOCKS * K.rpb(d)
    for order in ('head', 'tail'):
        assert geom[order][0] == 3 and geom[order][1] == 6 and geom[order][2] > first >= case.N - first       # two passes, no third
    assert case.N > first                                                            # so every chunk item falls in the second pass
    values(case, d)


# ---------------------------------------------------------------------------------------------------------------------
# the relation table on both sides of the LDS fit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R,d', K.LDS_SHAPES)
def test_relation_table_at_the_lds_fit(R, d):
    case = K.lds_fit(R, d)
    geom = assert_claimed_geometry(case, graph_of(case))
    assert all(geom[o][0] == 0 for o in geom)
    assert K.lds_fits(R, d) == (R % 2 == 0) and K.lds_fits(R - R % 2, d) and not K.lds_fits(R - R % 2 + 1, d)
    assert R * (d // 4) > K.THREADS and R > max(case.info['staged_first'], 6)         # rows beyond the first staging pass and beyond relation 5
    values(case, d)


# ---------------------------------------------------------------------------------------------------------------------
# the online softmax in a prescribed order
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', K.DIMS)
def test_logits_in_a_prescribed_order(d):
    case = K.logit_order()
    geom = assert_claimed_geometry(case, graph_of(case))
    assert geom['head'][:2] == (7, 21) and geom['rel'][:2] == (1, -(-7 * K.N_SLOTS // K.CHUNK)) and geom['tail'][0] == 0
    res = values(case, d, ('att',))
    t = K.tables(case, d)
    for masked in (False, True):                             # equal logits: the mean of the kept tail rows, finite at +-300
        for name in ('all equal +300', 'all equal -300'):
            h = case.info['head_of'][name]
            ids = case.slots[('head', h)]
            if masked:
                ids = ids[case.keep.numpy()[ids]]
            rows = t['x'][torch.from_numpy(case.tail[ids])]
            got = res[('att', masked)]['y'][h:h + 1]
            assert bool(torch.isfinite(got).all())
            check('logit_order d=%d %s%s y against the mean' % (d, name, ' masked' if masked else ''), got, rows.mean(0, keepdim=True),
                  rows.float().mean(0, keepdim=True))


# ---------------------------------------------------------------------------------------------------------------------
# a mask on the full graph against the graph of the kept edges
# ---------------------------------------------------------------------------------------------------------------------
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
    t = K.tables(case, d)
    for op in ('agg', 'att'):
        masked, plain = RUN[op](graph, t, case.keep.to(DEV)), RUN[op](sub, t, None)
        for k in masked:                                     # the kept slots are added in the same sequence: the eid indirection
            assert torch.equal(masked[k], plain[k]), (op, k)


# ---------------------------------------------------------------------------------------------------------------------
# slope
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('slope', [0.0, 0.01, 1.0])
def test_slopes_zero_small_and_one(slope, monkeypatch):
    from sslrec_amd import ops
    lib = ops._lib.load()
    calls, fwd = [], lib.sslrec_rgat_fwd_f32

    def counted(*a):
        calls.append(1)
        return fwd(*a)
    monkeypatch.setattr(lib, 'sslrec_rgat_fwd_f32', counted)
    d = 64
    for case in (K.boundary(), K.logit_order()):
        graph = graph_of(case)
        assert_claimed_geometry(case, graph)
        t = K.tables(case, d)
        if case.logit is not None:                           # logits of exactly 0 take the slope's side of the derivative
            h = case.info['head_of']['half zero']
            l32 = (gpu(t['q'])[torch.from_numpy(case.tail[case.slots[('head', h)]]).to(DEV)] * gpu(t['r'])[0]).sum(-1)
            assert int((l32 == 0).sum()) == K.N_SLOTS // 2 and bool((gpu(t['p'])[h] == 0).all())
        for masked in (False, True):
            keep = case.keep.to(DEV) if masked else None
            before = len(calls)
            got = run_att(graph, t, keep, slope)
            assert len(calls) == before + 1                  # the kernels ran: slope >= 0 includes 0
            check_outputs(case, d, 'att', masked, got, slope)
            again = run_att(graph, t, keep, slope)
            for k in got:
                assert torch.equal(got[k], again[k]), k
    # and no edge-sized matrix on the way (as test_rel_attention_makes_no_edge_sized_matrix)
    case = K.boundary()
    graph, t = graph_of(case), K.tables(case, d)
    leaves = [gpu(t[n]).requires_grad_(True) for n in ('x', 'p', 'q', 'r')]
    go = gpu(t['go'])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    (ops.rel_attention(graph, *leaves, None, slope) * go).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print('rel_attention slope %g forward + backward, peak above the level before the call: %d bytes, E d 4 = %d' % (slope, peak, case.E * d * 4))
    assert peak < case.E * d * 4


# ---------------------------------------------------------------------------------------------------------------------
# ops.factor_modulate with several passes per workgroup
# ---------------------------------------------------------------------------------------------------------------------
def fm_run(U, d, F):
    from sslrec_amd import ops
    tens, go = K.fm_tables(U, d, F)
    return K.fm_outputs(ops.factor_modulate, tens, go, gpu)


@pytest.mark.parametrize('U,d,F', K.FM_SHAPES)
def test_factor_modulate_with_several_passes_per_workgroup(U, d, F):
    from sslrec_amd import ops
    G, rows, passes = K.fm_geometry(U, d)
    assert -(-U // K.rpb(d)) > K.MAX_ROW_BLOCKS and G <= K.MAX_ROW_BLOCKS and passes >= 2      # capped: the row loop runs at least twice
    assert (G - 1) * rows < U < G * rows                                                        # and the last workgroup is clipped
    assert ops.kgin_fused_ok(d) and 1 <= F <= ops.KGIN_FMAX
    r64, r32 = K.fm_reference(U, d, F)
    got = fm_run(U, d, F)
    for k in K.FM_OUT:
        check('factor_modulate %s (%d, %d, %d)' % (k, U, d, F), got[k], r64[k], r32[k])
    last = torch.arange((G - 1) * rows, U)
    for k in ('out', 'd_agg', 'd_u'):
        check('factor_modulate %s (%d, %d, %d) | rows of the clipped workgroup' % (k, U, d, F), got[k][last.to(DEV)], r64[k][last], r32[k][last])
    if F == 1:                                               # the softmax over one factor is the constant 1
        assert bool((got['d_u'] == 0).all()) and bool((got['d_latent'] == 0).all())
    again = fm_run(U, d, F)
    for k in got:
        assert torch.equal(got[k], again[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------
def _grads(fn, tens, needs):
    leaves = [a.clone().requires_grad_(n) for a, n in zip(tens, needs)]
    fn(*leaves).backward()
    return [a.grad for a in leaves]


def test_gradients_of_a_subset_of_the_inputs():
    from sslrec_amd import ops
    case, d = K.boundary(), 64
    graph, t = graph_of(case), K.tables(case, d)
    assert_claimed_geometry(case, graph)
    keep, go = case.keep.to(DEV), gpu(t['go'])
    att = [gpu(t[n]) for n in ('x', 'p', 'q', 'r')]
    full = _grads(lambda *a: (ops.rel_attention(graph, *a, keep) * go).sum(), att, (True,) * 4)
    assert all(g is not None for g in full)
    for needs in ((True, False, False, False), (False, False, False, True), (False, True, True, False)):
        part = _grads(lambda *a: (ops.rel_attention(graph, *a, keep) * go).sum(), att, needs)
        for n, g, f in zip(needs, part, full):
            assert (g is None) if not n else torch.equal(g, f), needs
    agg = [gpu(t['x']), gpu(t['w'])]
    full = _grads(lambda *a: (ops.rel_aggregate(graph, *a, keep) * go).sum(), agg, (True, True))
    for needs in ((True, False), (False, True)):
        part = _grads(lambda *a: (ops.rel_aggregate(graph, *a, keep) * go).sum(), agg, needs)
        for n, g, f in zip(needs, part, full):
            assert (g is None) if not n else torch.equal(g, f), needs


def test_keep_as_bool_uint8_or_on_the_host():
    case, d = K.boundary(), 64
    graph, t = graph_of(case), K.tables(case, d)
    assert_claimed_geometry(case, graph)
    assert case.keep.dtype == torch.bool and not case.keep.is_cuda
    for op in ('agg', 'att'):
        want = RUN[op](graph, t, case.keep.to(DEV))
        for keep in (case.keep.to(DEV).to(torch.uint8), case.keep, case.keep.to(torch.uint8)):
            got = RUN[op](graph, t, keep)
            for k in want:
                assert torch.equal(got[k], want[k]), (op, k, keep.dtype, keep.device)


def test_strided_inputs_and_a_broadcast_upstream_gradient():
    from sslrec_amd import ops
    case, d = K.boundary(), 64
    graph, t = graph_of(case), K.tables(case, d)
    assert_claimed_geometry(case, graph)
    keep = case.keep.to(DEV)

    def wide(a, col):
        """a as the column slice [col, col + d) of a [rows, 2 d + 4] tensor"""
        w = torch.full((a.shape[0], 2 * d + 4), 7.0, device=DEV)
        w[:, col:col + d] = a
        return w[:, col:col + d]
    for names, fn in ((('x', 'p', 'q', 'r'), lambda *a: ops.rel_attention(graph, *a, keep)), (('x', 'w'), lambda *a: ops.rel_aggregate(graph, *a, keep))):
        dense = [gpu(t[n]) for n in names]
        sliced = [wide(a, 4 * i) for i, a in enumerate(dense)]
        assert all(not s.is_contiguous() and torch.equal(s, a) for s, a in zip(sliced, dense))
        outs = []
        for tens in (dense, sliced):
            leaves = [a.detach().requires_grad_(True) for a in tens]
            y = fn(*leaves)
            y.sum().backward()                               # the upstream gradient is an expanded scalar: stride 0
            outs.append([y.detach()] + [a.grad for a in leaves])
        for a, b in zip(*outs):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all())
