#!/usr/bin/env python
"""DCCF on the amazon-book-shaped synthetic graph at d = 32 and 64, K = 128, by HIP events:
  * ops.intent_aggregate_stacked forward and forward + backward, beside the PyTorch expression of the reference's dccf.py:77-80
    (split, two GEMM-softmax-GEMM chains, concat) on the same GPU in the same run, with the peak allocated memory of both forms and
    the distance of the kernel from the faster of its two bounds (HBM bytes of X in and Y out; 4 N d K fp32 FLOPs forward);
  * one whole cal_loss + backward of the model, beside the same step written with plain torch ops (dccf.py:65-146 restated).
usage: python tools/dccf_bench.py [out_dir = profiles/dccf] [dataset = amazon-book]"""
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

dev = 'cuda:0'
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'dccf')
dataset = sys.argv[2] if len(sys.argv) > 2 else 'amazon-book'
assert torch.cuda.is_available(), 'this tool measures: it needs the GPU'
os.makedirs(out_dir, exist_ok=True)
K, BATCH = 128, 4096
HBM_BPS, FP32_FLOPS = 8.0e12, 157.3e12          # MI355X: HBM3E peak, fp32 matrix / vector peak


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


def torch_intent(table, n_user, c_u, c_i):
    u, i = torch.split(table, [n_user, table.shape[0] - n_user], 0)
    return torch.concat([torch.softmax(u @ c_u, dim=1) @ c_u.T, torch.softmax(i @ c_i, dim=1) @ c_i.T], dim=0)


def torch_infonce(e1, e2, all2, temp):
    n1 = e1 / torch.sqrt(1e-8 + e1.square().sum(-1, keepdim=True))
    n2 = e2 / torch.sqrt(1e-8 + e2.square().sum(-1, keepdim=True))
    na = all2 / torch.sqrt(1e-8 + all2.square().sum(-1, keepdim=True))
    return (-(n1 * n2 / temp).sum(-1) + torch.log(torch.sum(torch.exp(n1 @ na.T / temp), dim=-1))).sum()


def torch_mask_values(emb, heads, tails, n):
    head_e, tail_e = F.normalize(torch.index_select(emb, 0, heads)), F.normalize(torch.index_select(emb, 0, tails))
    alpha = (torch.sum(head_e * tail_e, dim=1) + 1) / 2
    d_inv = torch.zeros(n, device=emb.device).index_add(0, heads, alpha).pow(-1).nan_to_num(0, 0, 0)
    return d_inv[heads] * alpha


def torch_spmm(vals, heads, tails, x, n):
    return torch.zeros(n, x.shape[1], device=x.device).index_add(0, heads, vals[:, None] * torch.index_select(x, 0, tails))


def torch_step(model, adj, heads, tails, batch):
    """dccf.py:65-146 with stock torch ops"""
    n_user, n = model.user_num, model.user_num + model.item_num
    all_e = [torch.concat([model.user_embeds, model.item_embeds], dim=0)]
    parts = []
    for l in range(model.layer_num):
        e = all_e[l]
        gnn = torch.sparse.mm(adj, e)
        inte = torch_intent(e, n_user, model.user_intent, model.item_intent)
        gaa = torch_spmm(torch_mask_values(gnn, heads, tails, n), heads, tails, e, n)
        iaa = torch_spmm(torch_mask_values(inte, heads, tails, n), heads, tails, e, n)
        parts.append((gnn, inte, gaa, iaa))
        all_e.append(gnn + inte + gaa + iaa + e)
    final = torch.stack(all_e, dim=1).sum(dim=1)
    ancs, poss, negs = batch
    ue, ie = final[:n_user], final[n_user:]
    a, p, ng = ue[ancs], ie[poss], ie[negs]
    bpr = torch.sum(F.softplus((a * ng).sum(-1) - (a * p).sum(-1))) / a.shape[0]
    reg = model.reg_weight * sum(w.norm(2).square() for w in model.parameters())
    users, items = torch.unique(ancs), torch.unique(torch.concat([poss, negs]))
    cl = 0.0
    for gnn, inte, gaa, iaa in parts:
        for idx, lo in ((users, 0), (items, n_user)):
            anchor = gnn[idx + lo]
            for other in (inte, gaa, iaa):
                view = other[idx + lo]
                cl = cl + torch_infonce(anchor, view, view, model.temperature) / users.shape[0]
    return bpr + reg + model.cl_weight * cl


for d in (32, 64):
    load_config('dccf', device=dev, overrides={'data': {'synthetic': dataset}, 'model': {'embedding_size': d, 'intent_num': K},
                                              'train': {'batch_size': BATCH}})
    dh = DataHandlerGeneralCF()
    dh.trn_mat = dh._load_one_mat(dh.trn_file)
    configs['data']['user_num'], configs['data']['item_num'] = dh.trn_mat.shape
    dh.torch_adj = dh._make_torch_adj(dh.trn_mat)
    torch.manual_seed(d)
    model = build_model(dh).to(dev)
    n_user, n_item = model.user_num, model.item_num
    n = n_user + n_item
    rec = {'dataset': dataset, 'n_user': n_user, 'n_item': n_item, 'd': d, 'K': K, 'batch': BATCH}

    # -- the intent aggregation alone ------------------------------------------------------------------------------------
    gen = torch.Generator().manual_seed(d)
    x = (0.1 * torch.randn(n, d, generator=gen)).to(dev).requires_grad_(True)
    r = (0.1 * torch.randn(n, d, generator=gen)).to(dev)
    c_u, c_i = model.user_intent, model.item_intent

    def clear():
        x.grad = c_u.grad = c_i.grad = None

    def hip_fwd():
        return ops.intent_aggregate_stacked(x, n_user, c_u, c_i)

    def hip_fwd_bwd():
        clear()
        (hip_fwd() * r).sum().backward()

    def torch_fwd():
        return torch_intent(x, n_user, c_u, c_i)

    def torch_fwd_bwd():
        clear()
        (torch_fwd() * r).sum().backward()

    hip_fwd_bwd()
    got = [hip_fwd().detach(), x.grad.clone(), c_u.grad.clone(), c_i.grad.clone()]
    torch_fwd_bwd()
    want = [torch_fwd().detach(), x.grad.clone(), c_u.grad.clone(), c_i.grad.clone()]
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    rec['agreement_with_torch_fp32'] = dict(zip(('Y', 'dX', 'dC_u', 'dC_i'), (rel(a, b) for a, b in zip(got, want))))
    del got, want
    with torch.no_grad():
        rec['hip_forward'] = timed_us(hip_fwd, 10)
        rec['torch_forward'] = timed_us(torch_fwd, 5)
    rec['hip_forward_backward'] = timed_us(hip_fwd_bwd, 5)
    rec['torch_forward_backward'] = timed_us(torch_fwd_bwd, 5)
    rec['hip_forward_backward_peak_MB'] = peak_mb(hip_fwd_bwd)
    rec['torch_forward_backward_peak_MB'] = peak_mb(torch_fwd_bwd)
    rec['torch_over_hip_forward'] = round(rec['torch_forward']['median_us'] / rec['hip_forward']['median_us'], 2)
    rec['torch_over_hip_forward_backward'] = round(rec['torch_forward_backward']['median_us'] / rec['hip_forward_backward']['median_us'], 2)
    hbm_us, flop_us = 2 * n * d * 4 / HBM_BPS * 1e6, 4.0 * n * d * K / FP32_FLOPS * 1e6
    rec['forward_bounds'] = {'hbm_us': round(hbm_us, 2), 'fp32_flop_us': round(flop_us, 2),
                             'what': 'X in + Y out at %.1f TB/s; 4 N d K FLOPs at %.1f TFLOPS; the larger of the two binds' % (HBM_BPS / 1e12, FP32_FLOPS / 1e12)}
    rec['forward_bound_over_time'] = round(max(hbm_us, flop_us) / rec['hip_forward']['median_us'], 3)
    clear()

    # -- the whole step ------------------------------------------------------------------------------------------------
    rng = np.random.RandomState(d)
    batch = [torch.from_numpy(rng.randint(0, hi, BATCH)).to(dev) for hi in (n_user, n_item, n_item)]
    heads, tails = model.all_h_list.to(dev), model.all_t_list.to(dev)
    adj = dh.torch_adj.coalesce()

    def hip_step():
        for p in model.parameters():
            p.grad = None
        model.cal_loss(batch)[0].backward()

    def torch_step_():
        for p in model.parameters():
            p.grad = None
        torch_step(model, adj, heads, tails, batch).backward()

    rec['hip_step_loss'] = float(model.cal_loss(batch)[0])
    rec['torch_step_loss'] = float(torch_step(model, adj, heads, tails, batch))
    rec['hip_step'] = timed_us(hip_step, 3, reps=5)
    rec['torch_step'] = timed_us(torch_step_, 2, reps=5, warmup=1)
    rec['hip_step_peak_MB'] = peak_mb(hip_step)
    rec['torch_step_peak_MB'] = peak_mb(torch_step_)
    rec['torch_over_hip_step'] = round(rec['torch_step']['median_us'] / rec['hip_step']['median_us'], 2)
    print(json.dumps(rec))
    json.dump(rec, open(os.path.join(out_dir, '%s_d%d.json' % (dataset, d)), 'w'), indent=1)
    del model, x, r, adj, heads, tails
    torch.cuda.empty_cache()
