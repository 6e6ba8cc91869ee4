#!/usr/bin/env python
"""HCCF on a synthetic graph of a real dataset's shape (K = 128, keep_rate 0.5), by HIP events:
  * ops.hyper_propagate_stacked forward and forward + backward, beside the PyTorch expression of the reference's hccf.py:43-49,
    105-107 (two GEMMs, F.dropout, HGNNLayer per row range, concat) on the same GPU in the same run, with the peak allocated memory
    of both forms and the forward's fraction of its fp32-MFMA FLOP bound (8 N d K FLOPs: E W twice, A^T X and A H);
  * one whole cal_loss + backward of the model, beside the same step written with plain torch ops (hccf.py:38-88 restated).
usage: python tools/hccf_bench.py [out_dir = profiles/hccf] [dataset = gowalla] [d ...  = 32]"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sslrec_amd import ops  # noqa: E402
from sslrec_amd.config.configurator import configs, load_config  # noqa: E402
from sslrec_amd.data_utils.data_handler_general_cf import DataHandlerGeneralCF  # noqa: E402
from sslrec_amd.models.bulid_model import build_model  # noqa: E402
from sslrec_amd.rng import PhiloxState  # noqa: E402

dev = 'cuda:0'
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'hccf')
dataset = sys.argv[2] if len(sys.argv) > 2 else 'gowalla'
dims = [int(a) for a in sys.argv[3:]] or [32]
assert torch.cuda.is_available(), 'this tool measures: it needs the GPU'
os.makedirs(out_dir, exist_ok=True)
K, BATCH, KEEP, LEAKY = 128, 4096, 0.5, 1.0          # hccf.yml's values (leaky 1.0: the shipped activation is the identity)
FP32_FLOPS = 157.3e12          # MI355X: fp32 matrix peak


def timed_us(fn, inner, reps=7, warmup=2):
    """median over `reps` windows of `inner` back-to-back calls between one event pair, per call, in microseconds"""
    for _ in range(warmup):
        fn()
    evs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 / inner for a, b in evs)
    return {'median_us': round(t[len(t) // 2], 2), 'min_us': round(t[0], 2), 'max_us': round(t[-1], 2), 'windows': reps, 'calls_per_window': inner}


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def torch_hyper(x, e, n_user, w_u, w_i, mult, leaky, keep_rate):
    """hccf.py:43-44, 48-49, 105-107 (F.dropout draws its own mask)"""
    out = []
    for rows, w in ((slice(0, n_user), w_u), (slice(n_user, None), w_i)):
        a = F.dropout(e[rows] @ w * mult, p=1 - keep_rate)
        out.append(F.leaky_relu(a @ F.leaky_relu(a.T @ x[rows], leaky), leaky))
    return torch.concat(out, dim=0)


def torch_spec_nodes(e1, e2, nodes, temp):
    e1, e2 = F.normalize(e1 + 1e-8, p=2), F.normalize(e2 + 1e-8, p=2)
    p1, p2 = e1[nodes], e2[nodes]
    nume = torch.exp(torch.sum(p1 * p2, dim=-1) / temp)
    deno = torch.exp(p1 @ e2.T / temp).sum(-1) + 1e-8
    return -torch.log(nume / deno).mean()


def torch_step(model, adj, batch):
    """hccf.py:38-88 with stock torch ops (EdgeDrop as a mask on the values of the coalesced adjacency)"""
    n_user, keep = model.user_num, model.keep_rate
    e0 = torch.concat([model.user_embeds, model.item_embeds], dim=0)
    lst, gcn, hyp = [e0], [], []
    idx, vals = adj.indices(), adj.values()
    for _ in range(model.layer_num):
        m = (torch.rand(vals.shape[0], device=vals.device) + keep).floor()
        dropped = torch.sparse_coo_tensor(idx, vals * m / keep, adj.shape)
        gcn.append(torch.sparse.mm(dropped, lst[-1]))
        hyp.append(torch_hyper(lst[-1], e0, n_user, model.user_hyper_embeds, model.item_hyper_embeds, model.mult, model.leaky, keep))
        lst.append(gcn[-1] + hyp[-1])
    final = sum(lst)
    ancs, poss, negs = batch
    a, p, ng = final[:n_user][ancs], final[n_user:][poss], final[n_user:][negs]
    bpr = -((a * p).sum(-1) - (a * ng).sum(-1)).sigmoid().log().mean()
    cl = 0
    for g, h in zip(gcn, hyp):
        g = g.detach()
        cl = cl + torch_spec_nodes(g[:n_user], h[:n_user], torch.unique(ancs), model.temperature) \
            + torch_spec_nodes(g[n_user:], h[n_user:], torch.unique(poss), model.temperature)
    reg = model.reg_weight * sum(w.norm(2).square() for w in model.parameters())
    return bpr + reg + model.cl_weight * cl


for d in dims:
    load_config('hccf', device=dev, overrides={'data': {'synthetic': dataset}, 'train': {'batch_size': BATCH},
                                              'model': {'embedding_size': d, 'hyper_num': K, 'keep_rate': KEEP, 'leaky': LEAKY, 'device_rng': True}})
    dh = DataHandlerGeneralCF()
    dh.trn_mat = dh._load_one_mat(dh.trn_file)
    configs['data']['user_num'], configs['data']['item_num'] = dh.trn_mat.shape
    dh.torch_adj = dh._make_torch_adj(dh.trn_mat)
    torch.manual_seed(d)
    model = build_model(dh).to(dev)
    n_user, n_item = model.user_num, model.item_num
    n = n_user + n_item
    rec = {'dataset': dataset, 'n_user': n_user, 'n_item': n_item, 'd': d, 'K': K, 'keep_rate': KEEP, 'leaky': LEAKY, 'batch': BATCH}

    # -- the hypergraph layer alone --------------------------------------------------------------------------------------
    gen = torch.Generator().manual_seed(d)
    x = (0.1 * torch.randn(n, d, generator=gen)).to(dev).requires_grad_(True)
    e = (0.1 * torch.randn(n, d, generator=gen)).to(dev).requires_grad_(True)
    r = (0.1 * torch.randn(n, d, generator=gen)).to(dev)
    w_u, w_i = model.user_hyper_embeds, model.item_hyper_embeds
    state = PhiloxState(dev, seed=1)

    def clear():
        x.grad = e.grad = w_u.grad = w_i.grad = None

    def hip_fwd():
        return ops.hyper_propagate_stacked(x, e, n_user, w_u, w_i, 1.0, LEAKY, KEEP, (state, 1))

    def hip_fwd_bwd():
        clear()
        (hip_fwd() * r).sum().backward()

    def torch_fwd():
        return torch_hyper(x, e, n_user, w_u, w_i, 1.0, LEAKY, KEEP)

    def torch_fwd_bwd():
        clear()
        (torch_fwd() * r).sum().backward()

    # agreement on the SAME mask: the composed expression fed ops.hyper_keep_mask (row range by row range: the mask is N x K)
    hip_fwd_bwd()
    got = [hip_fwd().detach(), x.grad.clone(), e.grad.clone(), w_u.grad.clone(), w_i.grad.clone()]
    clear()
    mask = ops.hyper_keep_mask(state, 1, n, K, KEEP)
    (ops._hyper_composed(x, e, n_user, w_u, w_i, 1.0, LEAKY, KEEP, mask) * r).sum().backward()
    with torch.no_grad():
        want = [ops._hyper_composed(x, e, n_user, w_u, w_i, 1.0, LEAKY, KEEP, mask), x.grad.clone(), e.grad.clone(), w_u.grad.clone(), w_i.grad.clone()]
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    rec['agreement_with_torch_fp32_same_mask'] = dict(zip(('Y', 'dX', 'dE', 'dW_u', 'dW_i'), (rel(a, b) for a, b in zip(got, want))))
    # random inputs put a few pre-activations within rounding of 0, where the two forms may pick different slopes (a discrete
    # difference, not an error of either): count the rows where that happened and compare the row gradients on the others
    same = ((got[0] > 0) == (want[0] > 0)).all(dim=1)
    rec['rows_with_an_output_of_another_sign'] = int((~same).sum())
    rec['agreement_on_the_other_rows'] = {'dX': rel(got[1][same], want[1][same]), 'dE': rel(got[2][same], want[2][same])}
    del got, want, mask
    with torch.no_grad():
        rec['hip_forward'] = timed_us(hip_fwd, 10)
        rec['torch_forward'] = timed_us(torch_fwd, 5)
    rec['hip_forward_backward'] = timed_us(hip_fwd_bwd, 5)
    rec['torch_forward_backward'] = timed_us(torch_fwd_bwd, 5)
    rec['hip_forward_backward_peak_MB'] = peak_mb(hip_fwd_bwd)
    rec['torch_forward_backward_peak_MB'] = peak_mb(torch_fwd_bwd)
    rec['torch_over_hip_forward'] = round(rec['torch_forward']['median_us'] / rec['hip_forward']['median_us'], 2)
    rec['torch_over_hip_forward_backward'] = round(rec['torch_forward_backward']['median_us'] / rec['hip_forward_backward']['median_us'], 2)
    flop_us = 8.0 * n * d * K / FP32_FLOPS * 1e6
    rec['forward_fp32_flop_bound_us'] = round(flop_us, 2)
    rec['forward_bound_over_time'] = round(flop_us / rec['hip_forward']['median_us'], 3)
    clear()

    # -- the whole step ------------------------------------------------------------------------------------------------
    rng = np.random.RandomState(d)
    batch = [torch.from_numpy(rng.randint(0, hi, BATCH)).to(dev) for hi in (n_user, n_item, n_item)]
    adj = dh.torch_adj.coalesce()

    def hip_step():
        for p in model.parameters():
            p.grad = None
        model.cal_loss(batch)[0].backward()

    def torch_step_():
        for p in model.parameters():
            p.grad = None
        torch_step(model, adj, batch).backward()

    rec['hip_step_loss'] = float(model.cal_loss(batch)[0].detach())
    rec['torch_step_loss'] = float(torch_step(model, adj, batch).detach())          # (another mask: the same distribution, not the same number)
    rec['hip_step'] = timed_us(hip_step, 3, reps=5)
    rec['torch_step'] = timed_us(torch_step_, 2, reps=5, warmup=1)
    rec['hip_step_peak_MB'] = peak_mb(hip_step)
    rec['torch_step_peak_MB'] = peak_mb(torch_step_)
    rec['torch_over_hip_step'] = round(rec['torch_step']['median_us'] / rec['hip_step']['median_us'], 2)
    print(json.dumps(rec))
    json.dump(rec, open(os.path.join(out_dir, '%s_d%d.json' % (dataset, d)), 'w'), indent=1)
    del model, x, e, r, adj
    torch.cuda.empty_cache()
