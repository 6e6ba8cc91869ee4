"""The two by-products of the LightGCN step that ride on the column-swept kernel's flush (sslrec_spmm_swept_step_f32):
the regularizer's sum of squares from the first forward product (ops.REG_IN_FLUSH) and the batched axpy_x rows of the last
backward product (ops.AXPY_BATCH).  Both are compiled into the one-workgroup-per-CU (128-register) build only, so the graphs
here are the smallest that reach it: 256 workgroups whose accumulators take more than half the LDS (n_slots * d * 4 > 81,920),
with empty rows, rows of degree 1-5, enough rows of degree 17-40 that a workgroup has more chunked rows than one flush pass
covers (1024 / (d / 4) rows), and one row of 2,000-3,000 entries.  (A wave with more one-slot rows than its 12 prefetched
passes cover does not occur on a balanced layout -- 12 passes are more than the slot limit's share of a wave -- so the kernel's
loop behind them is not reached here; it runs the same flush_row as the chunked passes that are.)  Everything is compared with
the switches off, bit for bit; the regularizer, whose summation order changes, with the float64 sum.

Measured on one MI355X: reg is 3.3e-8 (relative) from weight * the float64 sum on both routes and at both widths -- both give
the fp32 number nearest to it; the bound is 1e-6."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIN_PART0 = 32 * 65          # floats of ticket counters in front of the partials (csrc/fin_reduce.h)
L, W = 3, 0.37


def _step_graph(n, n_heavy, n_giant, seed):
    """symmetric 0/1 pattern with the reference's normalization D^-1/2 A D^-1/2 (so the factorized chain applies): nodes
    [0, n_heavy) form a random graph of mean degree 26 among themselves, the next ones a random graph of mean degree 2, one node
    has n_giant neighbours among those, the last n / 45 nodes have no entry at all"""
    rng = np.random.default_rng(seed)
    n_empty = n // 45
    giant = n - n_empty - 1
    m = n_heavy * 13
    lo = [rng.integers(0, n_heavy, m), rng.integers(n_heavy, giant, giant - n_heavy), np.full(n_giant, giant)]
    hi = [rng.integers(0, n_heavy, m), rng.integers(n_heavy, giant, giant - n_heavy), rng.choice(np.arange(n_heavy, giant), n_giant, replace=False)]
    lo, hi = np.concatenate(lo), np.concatenate(hi)
    lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
    key = np.unique(lo[lo != hi] * n + hi[lo != hi])
    lo, hi = key // n, key % n
    rows, cols = np.concatenate([lo, hi]), np.concatenate([hi, lo])
    perm = rng.permutation(rows.size)
    rows, cols = rows[perm], cols[perm]
    deg = np.bincount(rows, minlength=n).astype(np.float64)
    vals = ((deg[rows] + 1e-10) ** -0.5 * (deg[cols] + 1e-10) ** -0.5).astype(np.float32)
    return rows, cols, vals, deg


class _Case:
    pass


_CASES = {}


@pytest.fixture(scope='module', params=[64, 128], ids=['d64', 'd128'])
def case(request):
    return _build_case(request.param)


@pytest.fixture(scope='module')
def case64():
    return _build_case(64)


def _build_case(d):
    """graph, tables and the float64 reference of one width, built once; the layout facts the tests rely on are asserted here, so a
    change of the layout builder fails loudly instead of emptying the tests"""
    from sslrec_amd import _lib
    from sslrec_amd.graph import PropGraph
    import ctypes as C
    if d in _CASES:
        return _CASES[d]
    # (the long row's 16-entry chunks must stay below half a workgroup's slots, or the builder cuts every row into longer chunks)
    n, n_heavy, n_giant = (90000, 18500, 3000) if d == 64 else (45000, 9500, 2000)
    c = _Case()
    c.d, c.n = d, n
    c.rows, c.cols, c.vals, deg = _step_graph(n, n_heavy, n_giant, seed=d)
    assert (deg == 0).sum() >= n // 45 and ((deg >= 1) & (deg <= 5)).sum() > 1000 and deg.max() >= n_giant
    assert ((deg >= 17) & (deg <= 40)).sum() > (17000 if d == 64 else 8500)
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv('SSLREC_SWEPT_BLOCKS', '256')
        mp.setenv('SSLREC_SPMM_SWEPT', '1')
        mp.delenv('SSLREC_SWEPT_WIDTH', raising=False)
        c.g = PropGraph(c.rows, c.cols, c.vals, (n, n), DEV)
        lays = [c.g.fwd.swept(d), c.g.bwd.swept(d)]
    finally:
        mp.undo()
    lib = _lib.load()
    for lay in lays:
        assert lay is not None and lay.n_pass == 1 and lay.n_blocks == 256
        assert lay.n_slots * d * 4 > 81920
        assert lib.sslrec_swept_step_ok(C.byref(lay.c_struct())) == 1
        assert int(np.diff(lay.cf_ptr.cpu().numpy()).max()) > 1024 // (d // 4)      # a second chunked pass in some workgroup
    assert c.g.factorization() is not None and c.g.factorization()[2]
    gen = torch.Generator().manual_seed(5)
    c.e0 = (torch.rand(n, d, generator=gen) - 0.5).to(DEV)
    c.wt = torch.randn(n, d, generator=gen).to(DEV)
    c.ref = W * float((c.e0.double() ** 2).sum().item())
    _CASES[d] = c
    return c


def _switches(monkeypatch, reg, axpy, factorized=None):
    from sslrec_amd import ops
    monkeypatch.setattr(ops, 'REG_IN_FLUSH', reg)
    monkeypatch.setattr(ops, 'AXPY_BATCH', axpy)
    if factorized is not None:
        monkeypatch.setattr(ops, 'FACTORIZED', factorized)


def _fwd_bwd(g, e0, wt, c=1.0, **kw):
    from sslrec_amd import ops
    a = e0.clone().requires_grad_(True)
    out = ops.propagate_sum(g, a, L, reg_weight=W, **kw)
    tot, reg = out[0], out[1]
    (c * ((tot * wt).sum() + reg)).backward()
    return tot.detach(), reg.detach(), a.grad


def _routes():
    from sslrec_amd import ops
    return dict(ops.REG_ROUTES), dict(ops.AXPY_ROUTES)


@pytest.mark.parametrize('factorized', [1, 0], ids=['factorized', 'valued'])
def test_regularizer_from_the_first_flush(case, factorized, monkeypatch):
    """A: tot and the gradient keep their bits, reg is within 1e-6 of the float64 sum on both routes and repeats bit for bit"""
    from sslrec_amd import ops
    _switches(monkeypatch, False, False, factorized)
    assert (ops._chain_scale(case.g, case.d, L) is not None) == bool(factorized)
    r0, _ = _routes()
    tot0, reg0, grad0 = _fwd_bwd(case.g, case.e0, case.wt)
    r1, _ = _routes()
    assert (r1['kernel'], r1['flush']) == (r0['kernel'] + 1, r0['flush'])
    _switches(monkeypatch, True, False, factorized)
    tot1, reg1, grad1 = _fwd_bwd(case.g, case.e0, case.wt)
    tot2, reg2, grad2 = _fwd_bwd(case.g, case.e0, case.wt)
    r2, _ = _routes()
    assert (r2['kernel'], r2['flush']) == (r1['kernel'], r1['flush'] + 2)
    err_flush, err_kernel = abs(reg1.item() - case.ref) / case.ref, abs(reg0.item() - case.ref) / case.ref
    print('d = %d %s: reg relative error, flush %.3g, kernel %.3g' % (case.d, 'factorized' if factorized else 'valued', err_flush, err_kernel))
    assert torch.equal(tot1, tot0) and torch.equal(grad1, grad0)
    assert err_kernel <= 1e-6
    assert err_flush <= 1e-6
    assert torch.equal(reg2, reg1) and torch.equal(tot2, tot1) and torch.equal(grad2, grad1)


def test_first_product_with_y_and_a_hundred_launches(case):
    """A, on the launch itself: Y and acc_out keep their bits; 100 back-to-back launches give one value and leave the tickets zero"""
    from sslrec_amd import _lib, ops
    g, e0, d = case.g, case.e0, case.d
    acc0, acc1 = torch.empty_like(e0), torch.empty_like(e0)
    y0 = ops.spmm_raw(g, e0, 'fwd', acc_in=e0, acc_out=acc0, want_y=True)
    ws = ops._ticket_ws(e0.device, _lib.load().sslrec_sumsq_ws_bytes(), 'sumsq')
    out = torch.full((101,), float('nan'), dtype=torch.float32, device=DEV)
    y1 = ops.spmm_raw(g, e0, 'fwd', acc_in=e0, acc_out=acc1, want_y=True, reg_sumsq=(ws, out[100:], W))
    assert torch.equal(y1, y0) and torch.equal(acc1, acc0)
    for i in range(100):
        ops.spmm_raw(g, e0, 'fwd', acc_in=e0, acc_out=acc1, want_y=False, reg_sumsq=(ws, out[i:i + 1], W))
    torch.cuda.synchronize()
    assert torch.equal(acc1, acc0)
    assert abs(out[0].item() - case.ref) <= 1e-6 * case.ref
    assert bool((out.view(torch.int32) == out.view(torch.int32)[0]).all())
    assert int(ws[:FIN_PART0].view(torch.int32).abs().max().item()) == 0


@pytest.mark.parametrize('factorized', [1, 0], ids=['factorized', 'valued'])
@pytest.mark.parametrize('c', [1.0, 3.0])
def test_axpy_rows_in_batches(case, c, factorized, monkeypatch):
    """B: the gradient under c * ((tot * wt).sum() + reg) keeps its bits (the last backward product is a pattern launch in the
    factorized chain, a valued one otherwise)"""
    _switches(monkeypatch, True, False, factorized)
    _, x0 = _routes()
    tot0, reg0, grad0 = _fwd_bwd(case.g, case.e0, case.wt, c)
    _, x1 = _routes()
    assert (x1['plain'], x1['batched']) == (x0['plain'] + 1, x0['batched'])
    _switches(monkeypatch, True, True, factorized)
    tot1, reg1, grad1 = _fwd_bwd(case.g, case.e0, case.wt, c)
    _, x2 = _routes()
    assert (x2['plain'], x2['batched']) == (x1['plain'], x1['batched'] + 1)
    assert torch.equal(grad1, grad0) and torch.equal(tot1, tot0) and torch.equal(reg1, reg0)
    # (the gradient really holds the regularizer's share: 2 W c e0 is far above the rounding of the rest)
    assert not torch.equal(grad1, _fwd_bwd(case.g, case.e0, case.wt, 2.0 * c)[2])


def _small_graph(n, nnz, seed):
    rng = np.random.default_rng(seed)
    key = rng.choice(n * n, size=nnz, replace=False)
    return key // n, key % n, rng.uniform(0.05, 1.0, size=nnz).astype(np.float32)


@pytest.mark.parametrize('which', ['small', 'streamed', 'passes', 'perturbed', 'layers'])
def test_fallbacks_keep_the_kernel_of_their_own(case64, which, monkeypatch):
    """layouts and chains the tagged builds do not cover: sslrec_sumsq_fwd_f32 runs (the route counter says so) and reg, tot and
    the gradient are those of the switches off"""
    from sslrec_amd.graph import PropGraph
    case = case64
    kw = {}
    if which in ('small', 'streamed'):       # the 64-register build of a 300-row graph / no swept layout at all
        monkeypatch.setenv('SSLREC_SPMM_SWEPT', '0' if which == 'streamed' else '1')
        r, c_, v = _small_graph(300, 4000, seed=7)
        g = PropGraph(r, c_, v * 0.2, (300, 300), DEV)
        assert (g.fwd.swept(64) is None) == (which == 'streamed')
        gen = torch.Generator().manual_seed(3)
        e0, wt = torch.randn(300, 64, generator=gen).to(DEV), torch.randn(300, 64, generator=gen).to(DEV)
    elif which == 'passes':                  # the step graph on a 32-column layout: two embedding-column passes per product
        monkeypatch.setenv('SSLREC_SWEPT_BLOCKS', '256')
        monkeypatch.setenv('SSLREC_SWEPT_WIDTH', '32')
        g = PropGraph(case.rows, case.cols, case.vals, (case.n, case.n), DEV)
        assert g.fwd.swept(64).n_pass == 2
        e0, wt = case.e0, case.wt
    else:                                    # the step graph itself: the arguments decide
        g, e0, wt = case.g, case.e0, case.wt
        if which == 'perturbed':
            gen = torch.Generator().manual_seed(9)
            kw = dict(noises=[torch.rand(case.n, 64, generator=gen).to(DEV) for _ in range(L)], eps=0.2)
        else:
            kw = dict(return_layers=True)
    _switches(monkeypatch, False, False)
    tot0, reg0, grad0 = _fwd_bwd(g, e0, wt, 3.0, **kw)
    r0, _ = _routes()
    _switches(monkeypatch, True, True)
    tot1, reg1, grad1 = _fwd_bwd(g, e0, wt, 3.0, **kw)
    r1, x1 = _routes()
    assert (r1['kernel'], r1['flush']) == (r0['kernel'] + 1, r0['flush'])
    assert torch.equal(reg1, reg0) and torch.equal(tot1, tot0) and torch.equal(grad1, grad0)


def test_whole_step(case, monkeypatch):
    """the benchmark's step expression with a batch of 257: BPR loss and gradient bit for bit, the loss within one fp32 ulp"""
    from sslrec_amd import ops
    n_user, B, reg_weight = case.n // 2, 257, 1.0e-8
    gen = torch.Generator().manual_seed(11)
    batch = [torch.randint(0, n_user, (B,), generator=gen).to(DEV), torch.randint(0, case.n - n_user, (B,), generator=gen).to(DEV),
             torch.randint(0, case.n - n_user, (B,), generator=gen).to(DEV)]
    one = torch.ones((), dtype=torch.float32, device=DEV)

    def step():
        e0 = case.e0.clone().requires_grad_(True)
        s, reg = ops.propagate_sum(case.g, e0, L, reg_weight=reg_weight)
        loss, bpr = ops.bpr_loss_stacked(s, n_user, *batch, divisor=B, add=reg)
        loss.backward(one)
        return loss.detach(), bpr.detach(), e0.grad
    _switches(monkeypatch, False, False)
    loss0, bpr0, grad0 = step()
    r0, x0 = _routes()
    _switches(monkeypatch, True, True)
    loss1, bpr1, grad1 = step()
    r1, x1 = _routes()
    assert r1['flush'] == r0['flush'] + 1 and x1['batched'] == x0['batched'] + 1
    assert torch.equal(bpr1, bpr0) and torch.equal(grad1, grad0)
    a, b = np.float32(loss0.item()), np.float32(loss1.item())
    print('loss off %r on %r' % (a, b))
    assert abs(np.float64(a) - np.float64(b)) <= np.spacing(max(abs(a), abs(b)))
