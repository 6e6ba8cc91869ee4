#!/usr/bin/env python
"""DirectAU on a synthetic graph of a real dataset's shape (B = 4096, gamma = 2, L = 2), by HIP events:
  * ops.align_uniform_loss_stacked forward and forward + backward, beside the PyTorch expression of the reference's directau.py:42-47
    (two gathers, alignment, two uniformity calls with torch.pdist, backward with index_put) on the same GPU in the same run, with
    the peak allocated memory of both forms, and the fused form's peak memory again at B = 8192 (nothing in it grows with B^2);
  * one whole cal_loss + backward of the model, beside the same step written with plain torch ops (directau.py:27-47 restated).
usage: python tools/directau_bench.py [out_dir = profiles/directau] [dataset = gowalla] [d ...  = 32 64]"""
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
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'directau')
dataset = sys.argv[2] if len(sys.argv) > 2 else 'gowalla'
dims = [int(a) for a in sys.argv[3:]] or [32, 64]
assert torch.cuda.is_available(), 'this tool measures: it needs the GPU'
os.makedirs(out_dir, exist_ok=True)
BATCH, GAMMA, LAYERS = 4096, 2.0, 2          # directau.yml's values


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
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)


def torch_alignment(x, y):
    x, y = F.normalize(x, dim=-1), F.normalize(y, dim=-1)
    return (x - y).norm(p=2, dim=1).pow(2).mean()


def torch_uniformity(x):
    x = F.normalize(x, dim=-1)
    return torch.pdist(x, p=2).pow(2).mul(-2).exp().mean().log()


def torch_loss(user_embeds, item_embeds, ancs, poss, gamma):
    """directau.py:42-47"""
    anc, pos = user_embeds[ancs], item_embeds[poss]
    return torch_alignment(anc, pos) + gamma * (torch_uniformity(anc) + torch_uniformity(pos)) / 2


def torch_step(model, adj, batch):
    """directau.py:27-47 with stock torch ops"""
    embeds = torch.concat([model.user_embeds, model.item_embeds], dim=0)
    lst = [embeds]
    for _ in range(model.layer_num):
        lst.append(torch.sparse.mm(adj, lst[-1]))
    mean = sum(lst) / len(lst)
    return torch_loss(mean[:model.user_num], mean[model.user_num:], batch[0], batch[1], model.gamma)


for d in dims:
    load_config('directau', device=dev, overrides={'data': {'synthetic': dataset}, 'train': {'batch_size': BATCH},
                                                  'model': {'embedding_size': d, 'layer_num': LAYERS, 'gamma': GAMMA}})
    dh = DataHandlerGeneralCF()
    dh.trn_mat = dh._load_one_mat(dh.trn_file)
    configs['data']['user_num'], configs['data']['item_num'] = dh.trn_mat.shape
    dh.torch_adj = dh._make_torch_adj(dh.trn_mat)
    torch.manual_seed(d)
    model = build_model(dh).to(dev)
    n_user, n_item = model.user_num, model.item_num
    n = n_user + n_item
    rec = {'dataset': dataset, 'n_user': n_user, 'n_item': n_item, 'd': d, 'gamma': GAMMA, 'layer_num': LAYERS, 'batch': BATCH}

    # -- the loss alone ------------------------------------------------------------------------------------------------
    gen = torch.Generator().manual_seed(d)
    table = (0.1 * torch.randn(n, d, generator=gen)).to(dev).requires_grad_(True)
    rng = np.random.RandomState(d)
    scale = 1.0 / (LAYERS + 1)

    def draw(B):
        return [torch.from_numpy(rng.randint(0, hi, B)).to(dev) for hi in (n_user, n_item, n_item)]
    batch = draw(BATCH)

    def hip_fwd(b=batch):
        return ops.align_uniform_loss_stacked(table, n_user, b[0], b[1], GAMMA, scale)[0]

    def hip_fwd_bwd(b=batch):
        table.grad = None
        hip_fwd(b).backward()

    def torch_fwd(b=batch):
        mean = table * scale
        return torch_loss(mean[:n_user], mean[n_user:], b[0], b[1], GAMMA)

    def torch_fwd_bwd(b=batch):
        table.grad = None
        torch_fwd(b).backward()

    hip_fwd_bwd()
    got = [hip_fwd().detach(), table.grad.clone()]
    torch_fwd_bwd()
    want = [torch_fwd().detach(), table.grad.clone()]
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    rec['agreement_with_torch_fp32'] = {'loss': rel(got[0], want[0]), 'dT': rel(got[1], want[1])}
    del got, want
    with torch.no_grad():
        rec['hip_forward'] = timed_us(hip_fwd, 100)
        rec['torch_forward'] = timed_us(torch_fwd, 20)
    rec['hip_forward_backward'] = timed_us(hip_fwd_bwd, 50)
    rec['torch_forward_backward'] = timed_us(torch_fwd_bwd, 10)
    # peak memory beyond the inputs; the [N, d] gradient buffer is part of both
    rec['table_MB'] = round(n * d * 4 / 2 ** 20, 2)
    rec['hip_forward_backward_peak_MB'] = peak_mb(hip_fwd_bwd)
    rec['torch_forward_backward_peak_MB'] = peak_mb(torch_fwd_bwd)
    big = draw(2 * BATCH)
    rec['hip_forward_backward_peak_MB_at_2x_batch'] = peak_mb(lambda: hip_fwd_bwd(big))
    rec['torch_forward_backward_peak_MB_at_2x_batch'] = peak_mb(lambda: torch_fwd_bwd(big))
    rec['torch_over_hip_forward'] = round(rec['torch_forward']['median_us'] / rec['hip_forward']['median_us'], 2)
    rec['torch_over_hip_forward_backward'] = round(rec['torch_forward_backward']['median_us'] / rec['hip_forward_backward']['median_us'], 2)
    table.grad = None

    # -- the whole step ------------------------------------------------------------------------------------------------
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
    rec['torch_step_loss'] = float(torch_step(model, adj, batch).detach())
    rec['hip_step'] = timed_us(hip_step, 20, reps=5)
    rec['torch_step'] = timed_us(torch_step_, 5, reps=5, warmup=1)
    rec['hip_step_peak_MB'] = peak_mb(hip_step)
    rec['torch_step_peak_MB'] = peak_mb(torch_step_)
    rec['torch_over_hip_step'] = round(rec['torch_step']['median_us'] / rec['hip_step']['median_us'], 2)
    print(json.dumps(rec))
    json.dump(rec, open(os.path.join(out_dir, '%s_d%d.json' % (dataset, d)), 'w'), indent=1)
    del model, table, adj
    torch.cuda.empty_cache()
