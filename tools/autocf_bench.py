#!/usr/bin/env python
"""AutoCF on the gowalla-shaped synthetic graph with autocf.yml's sizes (d = 32, H = 4), by HIP events:
  * the graph-transformer layer on a decoder graph produced by the masker: ops.edge_attention forward and forward + backward, the
    three [N, d] projections, and the reference's composed expression (autocf.py:109-129: [E, d] gathers, three [E, d] GEMMs,
    index_add_) in PyTorch on the same GPU in the same run, with the peak allocated memory of both forms, the pattern build, and
    the forward as a fraction of the L2-resident gather ceiling (one K row and one V row per entry; sslrec_debug_gather_rows);
  * one fix_steps resampling (sample_subgraphs + mask_subgraphs), and the reference's per-seed masker loop beside the set-operation
    masker on a graph small enough for the loop to finish in seconds (loop_dataset, default tiny);
  * one whole training step (cal_loss + backward).
usage: python tools/autocf_bench.py [out_dir = profiles/autocf] [dataset = gowalla] [loop_dataset = tiny]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sslrec_amd import _lib, ops  # noqa: E402
from sslrec_amd.config.configurator import configs, load_config  # noqa: E402
from sslrec_amd.data_utils.data_handler_general_cf import DataHandlerGeneralCF  # noqa: E402
from sslrec_amd.graph import EdgePattern  # noqa: E402
from sslrec_amd.models.bulid_model import build_model  # noqa: E402

dev = 'cuda:0'
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'autocf')
dataset = sys.argv[2] if len(sys.argv) > 2 else 'gowalla'
loop_dataset = sys.argv[3] if len(sys.argv) > 3 else 'tiny'
assert torch.cuda.is_available(), 'this tool measures: it needs the GPU'
os.makedirs(out_dir, exist_ok=True)
BATCH = 4096


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


def wall_ms(fn, reps=3):
    """host wall time with a synchronisation on both sides (the resampling synchronises by itself)"""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(sorted(out)[len(out) // 2], 3)


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def torch_gt_layer(rows, cols, embeds, wq, wk, wv, heads):
    """autocf.py:109-129 with stock torch ops"""
    n, d = embeds.shape
    row_e, col_e = embeds[rows], embeds[cols]
    qe, ke, ve = ((x @ w).view(-1, heads, d // heads) for x, w in ((row_e, wq), (col_e, wk), (col_e, wv)))
    att = torch.exp(torch.clamp(torch.einsum('ehd, ehd -> eh', qe, ke), -10.0, 10.0))
    norm = torch.zeros(n, heads, device=embeds.device).index_add_(0, rows, att)[rows]
    att = att / (norm + 1e-8)
    res = torch.einsum('eh, ehd -> ehd', att, ve).reshape(-1, d)
    return torch.zeros(n, d, device=embeds.device).index_add_(0, rows, res)


def loop_masker(rows, cols, seeds, mask_depth):
    """autocf.py:180-198: the per-seed loop (entry removal only)"""
    nxt = None
    for i in range(mask_depth):
        cur = seeds if i == 0 else nxt
        nxt = []
        for seed in cur:
            idct = torch.logical_or(rows == seed, cols == seed)
            if i != mask_depth - 1:
                nxt.append(rows[idct])
                nxt.append(cols[idct])
            rows, cols = rows[torch.logical_not(idct)], cols[torch.logical_not(idct)]
        if len(nxt) > 0:
            nxt = torch.unique(torch.concat(nxt))
    return rows, cols


def gather_rate_l2(d):
    """TB/s of random-row gathers of d floats out of a table that fits every L2 (what bench.py's roofline section measures)"""
    lib = _lib.load()
    x = torch.randn(2048 * d, device=dev)
    scratch = torch.zeros(4096, device=dev)
    cnt = C.c_int64(0)
    st = torch.cuda.current_stream().cuda_stream

    def run():
        _lib.check(lib.sslrec_debug_gather_rows(x.data_ptr(), 2048, 4 * d, 64, 256, scratch.data_ptr(), C.addressof(cnt), st), 'sslrec_debug_gather_rows')
    t = timed_us(run, 10)
    return cnt.value * 4 * d / (t['median_us'] * 1e-6) / 1e12


def make_model(name, over=None):
    load_config('autocf', device=dev, overrides={'data': {'synthetic': name}, 'train': {'batch_size': BATCH}, 'model': dict(over or {})})
    dh = DataHandlerGeneralCF()
    dh.trn_mat = dh._load_one_mat(dh.trn_file)
    configs['data']['user_num'], configs['data']['item_num'] = dh.trn_mat.shape
    dh.torch_adj = dh._make_torch_adj(dh.trn_mat)
    torch.manual_seed(2023)
    return dh, build_model(dh).to(dev)


dh, model = make_model(dataset)
m = configs['model']
d, heads = m['embedding_size'], m['head_num']
n = model.user_num + model.item_num
rec = {'dataset': dataset, 'n_user': model.user_num, 'n_item': model.item_num, 'nnz_adj': int(dh.torch_adj._values().shape[0]), 'd': d,
       'heads': heads, 'batch': BATCH}

# -- one resampling, and the decoder graph the rest runs on --------------------------------------------------------------
with torch.no_grad():
    scores, seeds = model.sample_subgraphs()
enc, dec = model.mask_subgraphs(seeds)
rec['decoder_entries'] = dec.nnz
rec['decoder_long_rows'], rec['decoder_long_cols'] = int(dec.long_rows.numel()), int(dec.long_cols.numel())
rec['decoder_max_row'] = int((dec.rowptr[1:] - dec.rowptr[:-1]).max())
rec['encoder_entries_kept'] = int(model.masker.last['keep'].sum())
rows, cols = dec.coo()


def resample():
    s, sd = model.sample_subgraphs()
    return model.mask_subgraphs(sd)


rec['resample_ms'] = wall_ms(resample)
rec['pattern_build_sorted_keys_ms'] = wall_ms(lambda: EdgePattern(rows, cols, n))
perm = torch.randperm(rows.shape[0], device=dev)
rec['pattern_build_random_order_ms'] = wall_ms(lambda: EdgePattern(rows[perm], cols[perm], n))

# -- the GT layer ----------------------------------------------------------------------------------------------------
gt = model.gtLayers[0]
gen = torch.Generator().manual_seed(d)
x = (0.1 * torch.randn(n, d, generator=gen)).to(dev).requires_grad_(True)
r = (0.1 * torch.randn(n, d, generator=gen)).to(dev)
params = (gt.qTrans, gt.kTrans, gt.vTrans)


def clear():
    x.grad = None
    for p in params:
        p.grad = None


def projections():
    return x @ gt.qTrans, x @ gt.kTrans, x @ gt.vTrans


q0, k0, v0 = (t.detach().requires_grad_(True) for t in projections())


def hip_op():
    return ops.edge_attention(dec, q0, k0, v0, heads)


def hip_op_fwd_bwd():
    q0.grad = k0.grad = v0.grad = None
    (hip_op() * r).sum().backward()


def hip_layer():
    return gt(dec, x)


def hip_layer_fwd_bwd():
    clear()
    (hip_layer() * r).sum().backward()


def torch_layer():
    return torch_gt_layer(rows, cols, x, gt.qTrans, gt.kTrans, gt.vTrans, heads)


def torch_layer_fwd_bwd():
    clear()
    (torch_layer() * r).sum().backward()


hip_layer_fwd_bwd()
got = [hip_layer().detach(), x.grad.clone()] + [p.grad.clone() for p in params]
torch_layer_fwd_bwd()
want = [torch_layer().detach(), x.grad.clone()] + [p.grad.clone() for p in params]
rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
rec['agreement_with_torch_fp32'] = dict(zip(('Y', 'dX', 'dWq', 'dWk', 'dWv'), (rel(a, b) for a, b in zip(got, want))))
del got, want
with torch.no_grad():
    rec['hip_operator_forward'] = timed_us(hip_op, 10)
    rec['projections_forward'] = timed_us(projections, 10)
    rec['hip_layer_forward'] = timed_us(hip_layer, 10)
    rec['torch_layer_forward'] = timed_us(torch_layer, 3)
rec['hip_operator_forward_backward'] = timed_us(hip_op_fwd_bwd, 5)
rec['hip_layer_forward_backward'] = timed_us(hip_layer_fwd_bwd, 5)
rec['torch_layer_forward_backward'] = timed_us(torch_layer_fwd_bwd, 3)
rec['hip_layer_forward_backward_peak_MB'] = peak_mb(hip_layer_fwd_bwd)
rec['torch_layer_forward_backward_peak_MB'] = peak_mb(torch_layer_fwd_bwd)
rec['torch_over_hip_layer_forward'] = round(rec['torch_layer_forward']['median_us'] / rec['hip_layer_forward']['median_us'], 2)
rec['torch_over_hip_layer_forward_backward'] = round(rec['torch_layer_forward_backward']['median_us'] / rec['hip_layer_forward_backward']['median_us'], 2)
rate = gather_rate_l2(d)
floor_us = 2.0 * dec.nnz * 4 * d / (rate * 1e12) * 1e6
rec['gather_ceiling'] = {'gather_TBps_L2_resident': round(rate, 3), 'rows_per_entry': 2, 'forward_floor_us': round(floor_us, 2),
                         'operator_forward_fraction_of_ceiling': round(floor_us / rec['hip_operator_forward']['median_us'], 3)}
clear()

# -- the whole step ------------------------------------------------------------------------------------------------------
rng = np.random.RandomState(d)
batch = [torch.from_numpy(rng.randint(0, hi, BATCH)).to(dev) for hi in (model.user_num, model.item_num, model.item_num)]


def hip_step():
    for p in model.parameters():
        p.grad = None
    model.cal_loss(batch, enc, dec)[0].backward()


rec['step_loss'] = float(model.cal_loss(batch, enc, dec)[0])
rec['hip_step'] = timed_us(hip_step, 3, reps=5)
rec['hip_step_peak_MB'] = peak_mb(hip_step)
print(json.dumps(rec))
json.dump(rec, open(os.path.join(out_dir, '%s_d%d.json' % (dataset, d)), 'w'), indent=1)
del model, dh, enc, dec, rows, cols
torch.cuda.empty_cache()

# -- the masker: the reference's loop beside the set operations, at a size where the loop finishes in seconds --------------
dh, model = make_model(loop_dataset, {'seed_num': 20})
idx = dh.torch_adj._indices().to(dev).long()
with torch.no_grad():
    _, seeds = model.sample_subgraphs()
masker = model.masker
n_small = model.user_num + model.item_num
loop = {'dataset': loop_dataset, 'nodes': n_small, 'entries': int(idx.shape[1]), 'seeds': int(seeds.numel()), 'mask_depth': masker.mask_depth}
k_rows, k_cols = loop_masker(idx[0], idx[1], seeds, masker.mask_depth)
keep, _ = masker.masked_entries(idx[0], idx[1], seeds, n_small, masker.mask_depth)
loop['same_kept_entries'] = bool(torch.equal(torch.sort(k_rows * n_small + k_cols)[0], torch.sort(idx[0][keep] * n_small + idx[1][keep])[0]))
loop['reference_loop_ms'] = wall_ms(lambda: loop_masker(idx[0], idx[1], seeds, masker.mask_depth))
loop['set_operations_ms'] = wall_ms(lambda: masker.masked_entries(idx[0], idx[1], seeds, n_small, masker.mask_depth))
loop['loop_over_set_operations'] = round(loop['reference_loop_ms'] / max(loop['set_operations_ms'], 1e-6), 1)
print(json.dumps(loop))
json.dump(loop, open(os.path.join(out_dir, 'masker_%s.json' % loop_dataset), 'w'), indent=1)
