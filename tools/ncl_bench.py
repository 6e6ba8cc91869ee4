#!/usr/bin/env python
"""NCL on the gowalla- and amazon-book-shaped synthetic graphs at d = 32 and 64, K = 50, on one GPU in one process:
  * one clustering call of each table (ops.kmeans, 1000 iterations as KMeansClustering asks for) by the kernels of csrc/kmeans.hip and by
    the composed row-chunked torch expression (SSLREC_KMEANS_FUSED=0's path), with the early exit on and off, wall time with a device
    synchronisation at both ends (the early exit's host looks are part of the cost).  The tables are the model's xavier initialisation,
    the regime of the first clustering of a run.  The composed path without the early exit is timed over COMPOSED_FULL_ITERS iterations
    and reported per iteration;
  * the iteration count at the exit and whether both paths return the same assignment;
  * bytes per iteration: the ALGORITHMIC bytes (the table once, idx, the centroids), what the three launches move by construction
    (the table twice: assignment and update; idx three times; the slab partials written and read) and what the reference expression
    moves ([N, K, d] written and read, two index_add_) -- computed from the shapes, not counters -- and the rate they imply;
  * one NCL training step (zero_grad, cal_loss, backward, Adam) without and with the clustering of both tables in it.
usage: python tools/ncl_bench.py [out_dir = profiles/ncl] [dataset ... = gowalla amazon-book]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sslrec_amd import ops  # noqa: E402
from sslrec_amd.config.configurator import configs, load_config  # noqa: E402
from sslrec_amd.data_utils.data_handler_general_cf import DataHandlerGeneralCF  # noqa: E402
from sslrec_amd.models.bulid_model import build_model  # noqa: E402
from sslrec_amd.trainer.trainer import Trainer  # noqa: E402

dev = 'cuda:0'
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'ncl')
datasets = sys.argv[2:] or ['gowalla', 'amazon-book']
assert torch.cuda.is_available(), 'this tool measures: it needs the GPU'
os.makedirs(out_dir, exist_ok=True)
BATCH, K, MAX_ITER, COMPOSED_FULL_ITERS = 4096, 50, 1000, 40


class _Log:
    def log(self, *a, **k):
        pass

    log_loss = log_eval = log


def wall_ms(fn, reps=3, warmup=1):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    return {'median_ms': round(t[len(t) // 2], 3), 'min_ms': round(t[0], 3), 'max_ms': round(t[-1], 3), 'calls': reps}, out


def cluster_record(x, c0):
    N, d = x.shape
    rec = {'N': N}

    def call(fused, early, iters=MAX_ITER):
        ops.KMEANS_FUSED = fused
        try:
            return ops.kmeans(x, c0, max_iter=iters, early_exit=early)
        finally:
            ops.KMEANS_FUSED = True

    rec['fused_early_exit'], fe = wall_ms(lambda: call(True, True))
    rec['fused_1000_iterations'], ff = wall_ms(lambda: call(True, False))
    rec['composed_early_exit'], ce = wall_ms(lambda: call(False, True), reps=1, warmup=1)
    rec['composed_%d_iterations' % COMPOSED_FULL_ITERS], _ = wall_ms(lambda: call(False, False, COMPOSED_FULL_ITERS), reps=1, warmup=0)
    rec['iterations_at_exit'] = {'fused': fe[3], 'composed': ce[3]}
    rec['early_exit_bitwise_equal_to_1000_iterations'] = all(torch.equal(a, b) for a, b in zip(fe[:3], ff[:3]))
    rec['fused_and_composed_same_assignment'] = bool(torch.equal(fe[1], ce[1]))
    rec['non_empty_clusters'] = int((fe[2] > 0).sum())
    us_fused = rec['fused_1000_iterations']['median_ms'] * 1e3 / MAX_ITER
    us_comp = rec['composed_%d_iterations' % COMPOSED_FULL_ITERS]['median_ms'] * 1e3 / COMPOSED_FULL_ITERS
    slabs = min((N + 63) // 64, 256)
    algorithmic = N * d * 4 + N * 4 + 2 * K * d * 4
    launches = 2 * N * d * 4 + 3 * N * 4 + 2 * slabs * K * (d + 1) * 4 + 2 * K * d * 4
    reference = 2 * N * K * d * 4 + N * d * 4 + 2 * N * K * 4 + 2 * (N * d * 4 + N * 8) + 4 * K * d * 4
    rec['per_iteration'] = {
        'fused_us': round(us_fused, 2), 'composed_us': round(us_comp, 2), 'composed_over_fused': round(us_comp / us_fused, 1),
        'algorithmic_bytes': algorithmic, 'fused_bytes_by_construction': launches, 'reference_expression_bytes': reference,
        'fused_bytes_over_algorithmic': round(launches / algorithmic, 2),
        'fused_GBps_of_its_bytes': round(launches / us_fused / 1e3, 1), 'note': 'bytes computed from the shapes, not from counters'}
    return rec


for dataset in datasets:
    for d in (32, 64):
        load_config('ncl', device=dev, overrides={'data': {'synthetic': dataset}, 'train': {'batch_size': BATCH},
                                                  'model': {'embedding_size': d, 'cluster_num': K}})
        dh = DataHandlerGeneralCF()
        dh.trn_mat = dh._load_one_mat(dh.trn_file)
        configs['data']['user_num'], configs['data']['item_num'] = dh.trn_mat.shape
        dh.torch_adj = dh._make_torch_adj(dh.trn_mat)
        torch.manual_seed(d)
        np.random.seed(d)
        model = build_model(dh).to(dev)
        trainer = Trainer(dh, _Log())
        trainer.create_optimizer(model)
        rec = {'dataset': dataset, 'n_user': model.user_num, 'n_item': model.item_num, 'nnz': int(dh.trn_mat.nnz), 'd': d, 'K': K, 'batch': BATCH,
               'max_iter': MAX_ITER, 'poll': ops.KMEANS_POLL}
        gen = torch.Generator().manual_seed(d)
        for name, table in (('users', model.user_embeds), ('items', model.item_embeds)):
            rec['cluster_' + name] = cluster_record(table.detach(), torch.rand(K, d, generator=gen).to(dev))
        rng = np.random.RandomState(d)
        batch = [torch.from_numpy(rng.randint(0, hi, BATCH)).to(dev) for hi in (model.user_num, model.item_num, model.item_num)]
        quiet, flagged = batch + [torch.zeros(BATCH, dtype=torch.int64, device=dev)], batch + [torch.ones(BATCH, dtype=torch.int64, device=dev)]
        trainer._eager_step(model, flagged)                      # the first step clusters in any case
        rec['step_without_clustering'], _ = wall_ms(lambda: [trainer._eager_step(model, quiet) for _ in range(20)], reps=5, warmup=1)
        rec['step_without_clustering'] = {k: (round(v / 20, 4) if k.endswith('_ms') else v) for k, v in rec['step_without_clustering'].items()}
        rec['step_with_clustering'], _ = wall_ms(lambda: trainer._eager_step(model, flagged), reps=5, warmup=1)
        rec['iterations_in_step'] = model.kmeans.iters_run
        print(json.dumps(rec))
        json.dump(rec, open(os.path.join(out_dir, '%s_d%d.json' % (dataset, d)), 'w'), indent=1)
        del model, trainer
        torch.cuda.empty_cache()
