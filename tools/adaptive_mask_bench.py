#!/usr/bin/env python
"""AdaptiveMask on the amazon-book-shaped synthetic graph (symmetric bipartite adjacency, both directions of every interaction as in
the reference's dccf.py:21-23) at d = 32 and 64: the SDDMM launch, forward AdaptiveMask + propagate, and forward + backward, by
HIP events -- beside the same expression written with plain PyTorch ops on the same GPU (index_select, F.normalize, index_add_: what the
reference's aug_utils.py:73-79 + dccf.py:83-89 do, restated here) and beside the project's measured gather ceiling (one random 4 d-byte
row per entry at the L2-resident rate, profiles/r02/gather_ceiling.json).
usage: python tools/adaptive_mask_bench.py [out_dir = profiles/adaptive_mask] [dataset = amazon-book]"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sslrec_amd import ops  # noqa: E402
from sslrec_amd.data_utils.synth import make_dataset  # noqa: E402
from sslrec_amd.models.aug_utils import AdaptiveMask  # noqa: E402

dev = 'cuda:0'
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'adaptive_mask')
dataset = sys.argv[2] if len(sys.argv) > 2 else 'amazon-book'
assert torch.cuda.is_available(), 'this tool measures: it needs the GPU'
os.makedirs(out_dir, exist_ok=True)


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


def l2_gather_rate(row_bytes):
    """bytes / s of random row gathers from a table that fits an L2 (0.5 - 4.2 MB), 16 waves per CU with 8 loads in flight: the mean
    of those records of the project's gather microbenchmark"""
    recs = json.load(open(os.path.join(ROOT, 'profiles', 'r02', 'gather_ceiling.json')))
    r = [x['TBps'] for x in recs if x['row_bytes'] == row_bytes and x['waves_per_cu'] == 16 and x['loads_in_flight'] == 8 and 0.5 <= x['table_MB'] <= 4.2]
    return float(np.mean(r)) * 1e12


def torch_weights(table, heads, tails, n):
    head_e, tail_e = F.normalize(torch.index_select(table, 0, heads)), F.normalize(torch.index_select(table, 0, tails))
    alpha = (torch.sum(head_e * tail_e, dim=1) + 1) / 2
    d_inv = torch.zeros(n, device=table.device).index_add_(0, heads, alpha).pow(-1).nan_to_num(0, 0, 0)
    return d_inv[heads] * alpha


def torch_propagate(vals, heads, tails, x, n):
    return torch.zeros(n, x.shape[1], device=x.device).index_add_(0, heads, vals[:, None] * torch.index_select(x, 0, tails))


trn = make_dataset(dataset).tocoo()
n_user, n_item = trn.shape
n = n_user + n_item
heads_np = np.concatenate([trn.row, trn.col + n_user]).astype(np.int64)
tails_np = np.concatenate([trn.col + n_user, trn.row]).astype(np.int64)
heads, tails = torch.from_numpy(heads_np).to(dev), torch.from_numpy(tails_np).to(dev)
mask = AdaptiveMask(heads, tails, (n, n))
nnz = mask.graph.nnz

for d in (32, 64):
    gen = torch.Generator().manual_seed(d)
    s = (0.1 * torch.randn(n, d, generator=gen)).to(dev).requires_grad_(True)
    x = (0.1 * torch.randn(n, d, generator=gen)).to(dev).requires_grad_(True)
    r = (0.1 * torch.randn(n, d, generator=gen)).to(dev)
    norms = ops.row_invnorm(s)
    sd = s.detach()

    def hip_fwd():
        return mask.propagate(mask(s)[1], x)

    def hip_fwd_bwd():
        s.grad = x.grad = None
        (hip_fwd() * r).sum().backward()

    def torch_fwd():
        return torch_propagate(torch_weights(s, heads, tails, n), heads, tails, x, n)

    def torch_fwd_bwd():
        s.grad = x.grad = None
        (torch_fwd() * r).sum().backward()

    # same numbers first: the two expressions on the same inputs (reordered fp32 sums differ in the last bits only)
    hip_fwd_bwd()
    y_h, ds_h, dx_h = hip_fwd().detach(), s.grad.clone(), x.grad.clone()
    torch_fwd_bwd()
    y_t, ds_t, dx_t = torch_fwd().detach(), s.grad.clone(), x.grad.clone()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    rec = {'dataset': dataset, 'n_user': n_user, 'n_item': n_item, 'entries': nnz, 'd': d,
           'swept_layout': mask.graph.fwd.swept(d) is not None,
           'agreement_with_torch_fp32': {'Y': rel(y_h, y_t), 'dS': rel(ds_h, ds_t), 'dX': rel(dx_h, dx_t)}}
    rec['sddmm'] = timed_us(lambda: ops.sddmm(mask.graph, sd, sd, 'fwd', norms, norms), 20)
    rate = l2_gather_rate(4 * d)
    ceiling_us = nnz * 4 * d / rate * 1e6
    rec['gather_ceiling'] = {'rate_TBps': round(rate / 1e12, 2), 'us_per_launch': round(ceiling_us, 2),
                             'what': 'entries x 4 d bytes (ONE random row per entry) at the L2-resident gather rate of profiles/r02/gather_ceiling.json'}
    rec['sddmm_ceiling_over_time'] = round(ceiling_us / rec['sddmm']['median_us'], 3)
    with torch.no_grad():
        rec['hip_forward'] = timed_us(hip_fwd, 5)
        rec['torch_forward'] = timed_us(torch_fwd, 3, reps=5)
    rec['hip_forward_backward'] = timed_us(hip_fwd_bwd, 5)
    rec['torch_forward_backward'] = timed_us(torch_fwd_bwd, 3, reps=5)
    rec['torch_over_hip_forward'] = round(rec['torch_forward']['median_us'] / rec['hip_forward']['median_us'], 2)
    rec['torch_over_hip_forward_backward'] = round(rec['torch_forward_backward']['median_us'] / rec['hip_forward_backward']['median_us'], 2)
    print(json.dumps(rec))
    json.dump(rec, open(os.path.join(out_dir, '%s_d%d.json' % (dataset, d)), 'w'), indent=1)
    del y_h, ds_h, dx_h, y_t, ds_t, dx_t
    torch.cuda.empty_cache()
