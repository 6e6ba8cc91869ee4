"""The LightGCN step's loss work folded into fewer launches: the BPR backward staged by the forward launch
(sslrec_bpr_fwd_staged_f32 + sslrec_bpr_bwd_from_staged_f32, switch SSLREC_BPR_STAGED / ops.BPR_STAGED) against the three-launch
form it replaces (bit for bit where the upstream gradient is 1) and against the oracle.
Needs an MI355X:  python -m pytest tests -m gpu"""
import os

import numpy as np
import pytest
import torch

from oracle import ref_expr as R
from tests import helpers as H

pytestmark = pytest.mark.gpu

DEV = os.environ.get('SSLREC_TEST_DEVICE', 'cuda')
N_USER, N_ITEM = 300, 600


def _indices(B, kind, gen):
    """index sets of B triples.  'dup3' / 'dup12': one item 3 / 12 times among the 2 B positives and negatives (short-list path /
    beyond DET_LIST = 8, the scanning path) -- or as often as 2 B slots allow (B = 1: twice, B = 5: ten times, still beyond the list);
    'anchor': one user as the anchor of several triples AND an item of the same stacked-table offset duplicated."""
    assert B <= N_USER and 2 * B <= N_ITEM
    ancs = torch.randperm(N_USER, generator=gen)[:B].clone()      # all distinct
    slots = torch.randperm(N_ITEM, generator=gen)[:2 * B].clone()      # p0 n0 p1 n1 ...
    if kind == 'dup3':
        slots[:min(3, 2 * B)] = 5
    elif kind == 'dup12':
        slots[:min(12, 2 * B)] = 9
    elif kind == 'anchor':
        ancs[:min(4, B)] = 3
        slots[:min(2, 2 * B)] = 3
    else:
        assert kind == 'none'
    poss, negs = slots.reshape(-1, 2)[:, 0].contiguous(), slots.reshape(-1, 2)[:, 1].contiguous()
    return ancs, poss, negs


def _oracle(table, ancs, poss, negs, B, up):
    t = table.clone().requires_grad_(True)
    loss = R.cal_bpr_loss(t[:N_USER][ancs], t[N_USER:][poss], t[N_USER:][negs]) / B
    (up * loss).backward()
    return loss.item(), t.grad.numpy()


def _generation(B, d):
    from sslrec_amd import ops
    ent = [v for k, v in ops._KEPT_WS.items() if k[1:] == (B, d)]
    return ent[0][0]._sslrec_stage[0] if ent else 0


def _run(table, idx, B, staged, monkeypatch, up=None, add=None):
    """loss (and total) + gradient of bpr_loss_stacked with the switch set; returns also by how much the staging generation moved"""
    from sslrec_amd import ops
    monkeypatch.setattr(ops, 'BPR_STAGED', staged)
    t = table.to(DEV).requires_grad_(True)
    gen0 = _generation(B, table.shape[1])
    out = ops.bpr_loss_stacked(t, N_USER, *[i.to(DEV) for i in idx], divisor=B, add=add)
    loss = out[0] if add is not None else out
    (loss if up is None else up * loss).backward()
    return [o.item() for o in (out if add is not None else (out,))], t.grad, _generation(B, table.shape[1]) - gen0


@pytest.mark.parametrize('kind', ['none', 'dup3', 'dup12', 'anchor'])
@pytest.mark.parametrize('d', [32, 64])
@pytest.mark.parametrize('B', [1, 5, 257])
def test_staged_bpr_has_the_bits_of_the_three_launch_form(B, d, kind, monkeypatch):
    """upstream gradient 1: gradient table and loss bitwise equal to the switch-off path (x * 1.0f is exact, the loss keeps its grid
    and order); upstream 0.37: within the existing BPR tests' tolerance of the oracle (rtol 1e-4, atol 1e-6)."""
    gen = torch.Generator().manual_seed(1000 * B + d + len(kind))
    table = torch.randn(N_USER + N_ITEM, d, generator=gen)
    idx = _indices(B, kind, gen)
    add = torch.tensor(0.25, device=DEV)
    off, g_off, moved_off = _run(table, idx, B, False, monkeypatch, add=add)
    on, g_on, moved_on = _run(table, idx, B, True, monkeypatch, add=add)
    assert moved_off == 0 and moved_on == 1                  # the path under test really ran
    assert on == off and torch.equal(g_on, g_off)
    on1, g_on1, _ = _run(table, idx, B, True, monkeypatch)   # without `add`
    assert on1[0] == off[1] and torch.equal(g_on1, g_off)
    ref_loss, ref_grad = _oracle(table, *idx, B, 1.0)
    np.testing.assert_allclose(on[1], ref_loss, rtol=1e-5)
    np.testing.assert_allclose(g_on.cpu().numpy(), ref_grad, rtol=1e-4, atol=1e-6)
    _, g_s, moved = _run(table, idx, B, True, monkeypatch, up=0.37)
    assert moved == 1
    np.testing.assert_allclose(g_s.cpu().numpy(), _oracle(table, *idx, B, 0.37)[1], rtol=1e-4, atol=1e-6)
    _, g_s2, _ = _run(table, idx, B, True, monkeypatch, up=0.37)
    assert torch.equal(g_s, g_s2)                            # reproducible


def test_staged_bpr_ownership_of_the_shared_workspace(monkeypatch):
    """The staging workspace is shared per (device, B, d): whoever cannot prove the rows are still its own takes the three-launch form."""
    from sslrec_amd import ops
    B, d = 37, 64
    gen = torch.Generator().manual_seed(5)
    tabs = [torch.randn(N_USER + N_ITEM, d, generator=gen) for _ in range(2)]
    idxs = [_indices(B, k, gen) for k in ('dup3', 'anchor')]
    want = [_run(tabs[k], idxs[k], B, False, monkeypatch)[1] for k in range(2)]
    monkeypatch.setattr(ops, 'BPR_STAGED', True)
    # two forwards, backwards in reverse order: the second forward cancels the first one's staging
    ts = [t.to(DEV).requires_grad_(True) for t in tabs]
    gen0 = _generation(B, d)
    losses = [ops.bpr_loss_stacked(ts[k], N_USER, *[i.to(DEV) for i in idxs[k]], divisor=B) for k in range(2)]
    assert _generation(B, d) - gen0 == 3                     # staged, cancelled, staged
    losses[1].backward()
    losses[0].backward()
    assert torch.equal(ts[0].grad, want[0]) and torch.equal(ts[1].grad, want[1])
    # one forward, two backwards under retain_graph
    t = tabs[0].to(DEV).requires_grad_(True)
    loss = ops.bpr_loss_stacked(t, N_USER, *[i.to(DEV) for i in idxs[0]], divisor=B)
    loss.backward(retain_graph=True)
    first = t.grad.clone()
    t.grad = None
    loss.backward()
    assert torch.equal(first, want[0]) and torch.equal(t.grad, want[0])
    # forward under no_grad / on a table that takes no gradient: nothing is staged, the value is the same
    gen0 = _generation(B, d)
    with torch.no_grad():
        v0 = ops.bpr_loss_stacked(t, N_USER, *[i.to(DEV) for i in idxs[0]], divisor=B)
    v1 = ops.bpr_loss_stacked(tabs[0].to(DEV), N_USER, *[i.to(DEV) for i in idxs[0]], divisor=B)
    assert _generation(B, d) == gen0 and v0.item() == loss.item() == v1.item()
    # a step right after all of this is staged again and right
    _, g, moved = _run(tabs[1], idxs[1], B, True, monkeypatch)
    assert moved == 1 and torch.equal(g, want[1])
    # the scatter table is clean afterwards (test_bpr_backward_keeps_its_scatter_table_clean_between_calls's check)
    (ws, _), = [v for k, v in ops._KEPT_WS.items() if k[1:] == (B, d)]
    torch.cuda.synchronize()
    tab = ws[3 * B * d:].view(torch.int32)
    base = (-(ws.data_ptr() + 3 * B * d * 4) % 16) // 4
    slots = 32768
    assert int(tab[base:base + 3 * slots].abs().max()) == 0 and bool((tab[base + 3 * slots:base + 4 * slots] == 0x7fffffff).all())


def test_staged_bpr_leaves_batches_beyond_the_scatter_table_to_the_atomic_form(monkeypatch):
    """3 B > DET_MAX = 16384: no staging, atomic adds; tolerance only (the adds' order is not fixed)"""
    B, d = 5462, 32
    gen = torch.Generator().manual_seed(11)
    table = torch.randn(N_USER + N_ITEM, d, generator=gen) * 0.3
    idx = (torch.randint(0, N_USER, (B,), generator=gen), torch.randint(0, N_ITEM, (B,), generator=gen),
           torch.randint(0, N_ITEM, (B,), generator=gen))
    out, g, moved = _run(table, idx, B, True, monkeypatch)
    assert moved == 0
    ref_loss, ref_grad = _oracle(table, *idx, B, 1.0)
    np.testing.assert_allclose(out[0], ref_loss, rtol=1e-5)
    np.testing.assert_allclose(g.cpu().numpy(), ref_grad, rtol=1e-4, atol=1e-6)


def test_lightgcn_step_with_the_staged_bpr_equals_the_step_without(monkeypatch):
    """LightGCN cal_loss + backward on `tiny`, d = 64, L = 3 (the reference's recorded draws): switch on against off -- gradients, `loss`
    and `bpr_loss` bitwise equal -- and both against the reference's recorded step."""
    import sslrec_amd.models.aug_utils as aug
    from sslrec_amd import ops
    from tests.test_gpu_parity import _check_step
    g, cfg = H.load_golden('tiny', 'lightgcn', 64, 3)
    res = {}
    for staged in (True, False):
        monkeypatch.setattr(ops, 'BPR_STAGED', staged)
        dh, model = H.setup_model('lightgcn', g, cfg, DEV, 64, 3)
        H.set_params_from_golden(model, g)
        monkeypatch.setattr(aug.t, 'rand', H.ReplayRand(H.golden_draws(g)))
        batch = H.batch_from_golden(g, DEV)
        gen0 = _generation(int(batch[0].numel()), 64)
        loss, parts = model.cal_loss(batch)
        loss.backward()
        assert (_generation(int(batch[0].numel()), 64) - gen0 == 1) == staged
        _check_step(g, model, loss, parts, full=True)
        res[staged] = (loss.item(), parts['bpr_loss'].item(), [p.grad.clone() for p in model.parameters()])
        monkeypatch.undo()
    assert res[True][0] == res[False][0] and res[True][1] == res[False][1]
    for a, b in zip(res[True][2], res[False][2]):
        assert torch.equal(a, b)
