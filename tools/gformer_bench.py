#!/usr/bin/env python
"""GFormer on the gowalla- and amazon-book-shaped synthetic graphs at d = 32 (and 64 on request), A = 64 anchors, on one GPU in one process,
every fused op against its composed torch path in the same run (wall time with a device synchronisation at both ends):
  * ops.anchor_hops: total, number of levels and time per level, by csrc/bfs.hip and by the composed torch loop, and whether both agree;
  * ops.anchor_position_features: forward + backward by csrc/pnn.hip and by the composed expression (SSLREC_PNN_FUSED=0's path);
  * ops.edge_attention_scores on LocalGraph's widened adjacency, fused and composed;
  * one resampling (LocalGraph + masker), split into the host parts (numpy draws and masks, the native plan) and the rest (device);
  * one training step (cal_loss, zero_grad, backward, Adam) without and with a resampling in front of it.
usage: python tools/gformer_bench.py [out_dir = profiles/gformer] [dims = 32] [dataset ... = gowalla amazon-book]"""
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
from sslrec_amd.graph import PropGraph  # noqa: E402
from sslrec_amd.models.bulid_model import build_model  # noqa: E402
from sslrec_amd.models.general_cf import gformer as G  # noqa: E402
from sslrec_amd.trainer.trainer import Trainer  # noqa: E402

dev = 'cuda:0'
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'gformer')
dims = [int(x) for x in sys.argv[2].split(',')] if len(sys.argv) > 2 else [32]
datasets = sys.argv[3:] or ['gowalla', 'amazon-book']
assert torch.cuda.is_available(), 'this tool measures: it needs the GPU'
os.makedirs(out_dir, exist_ok=True)
BATCH = 4096


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


def switched(name, value, fn):
    old = getattr(ops, name)
    setattr(ops, name, value)
    try:
        return fn()
    finally:
        setattr(ops, name, old)


class HostClock:
    """wall time spent inside wrapped host functions"""

    def __init__(self):
        self.ms = 0.0

    def wrap(self, fn):
        def inner(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                self.ms += (time.perf_counter() - t0) * 1e3
        return inner


for dataset in datasets:
    for d in dims:
        load_config('gformer', device=dev, overrides={'data': {'synthetic': dataset}, 'train': {'batch_size': BATCH}, 'model': {'embedding_size': d}})
        dh = DataHandlerGeneralCF()
        dh.trn_mat = dh._load_one_mat(dh.trn_file)
        configs['data']['user_num'], configs['data']['item_num'] = dh.trn_mat.shape
        dh.torch_adj = dh._make_torch_adj(dh.trn_mat)
        torch.manual_seed(d)
        np.random.seed(d)
        model = build_model(dh).to(dev)
        trainer = Trainer(dh, _Log())
        trainer.create_optimizer(model)
        N, A = model.user_num + model.item_num, configs['model']['anchor_set_num']
        rec = {'dataset': dataset, 'n_user': model.user_num, 'n_item': model.item_num, 'nnz': int(dh.trn_mat.nnz), 'd': d, 'A': A, 'batch': BATCH,
               'head': configs['model']['head'], 'poll': ops.ANCHOR_HOPS_POLL}

        # ---- anchors ----
        anchors = np.random.choice(N, size=A, replace=False)
        ops.anchor_hops(model.adj, anchors)                      # (builds and uploads the plan's CSR once)
        fused, (hops, levels) = wall_ms(lambda: ops.anchor_hops(model.adj, anchors, return_levels=True))
        composed, (hops_c, levels_c) = wall_ms(lambda: switched('ANCHOR_HOPS_FUSED', False, lambda: ops.anchor_hops(model.adj, anchors, return_levels=True)),
                                               reps=1, warmup=1)
        rec['anchor_hops'] = {'fused': fused, 'composed': composed, 'levels': levels, 'levels_composed': levels_c,
                              'fused_us_per_level_launched': round(fused['median_ms'] * 1e3 / (-(-(levels + 1) // ops.ANCHOR_HOPS_POLL) * ops.ANCHOR_HOPS_POLL), 2),
                              'equal': bool(torch.equal(hops, hops_c)), 'unreached_share': round(float((hops < 0).float().mean()), 4),
                              'composed_over_fused': round(composed['median_ms'] / fused['median_ms'], 1)}
        model.preSelect_anchor_set()

        # ---- position features, forward + backward ----
        x = model.getEgoEmbeds().detach().clone().requires_grad_(True)
        gz = torch.randn(N, 2 * d, device=dev)

        def pnn_pass():
            x.grad = None
            z = ops.anchor_position_features(x, dh.anchor_ids_device, dh.anchor_hops)
            z.backward(gz)
            return z.detach(), x.grad
        fused, (z_f, dx_f) = wall_ms(pnn_pass, reps=5)
        composed, (z_c, dx_c) = wall_ms(lambda: switched('PNN_FUSED', False, pnn_pass), reps=3)
        rec['anchor_position_features'] = {'fused_fwd_bwd': fused, 'composed_fwd_bwd': composed,
                                           'composed_over_fused': round(composed['median_ms'] / fused['median_ms'], 1),
                                           'max_abs_diff_z': float((z_f - z_c).abs().max()), 'max_abs_diff_dx': float((dx_f - dx_c).abs().max()),
                                           'reference_tensor_bytes': N * A * 3 * d * 4}

        # ---- one resampling, host and device parts ----
        clock = HostClock()
        local, masker = model.localGraph, model.masker
        local.add_adj_entries = clock.wrap(local.add_adj_entries)
        masker.mask_entries = clock.wrap(masker.mask_entries)
        plan_clock = HostClock()
        G.PropGraph = plan_clock.wrap(PropGraph)

        def resample():
            att_edge, add_adj = local(dh.torch_adj, model.getEgoEmbeds(), dh)
            return (att_edge, add_adj) + tuple(masker(add_adj, att_edge))
        resample()
        clock.ms = plan_clock.ms = 0.0
        n_res = 3 if dh.trn_mat.nnz < 1000000 else 1            # (a resampling at amazon-book size is tens of seconds of numpy on the host)
        total, out = wall_ms(resample, reps=n_res, warmup=0)
        att_edge, add_adj, enc, dec, sub, cmp = out
        rec['resampling'] = {'total': total, 'host_draws_and_masks_ms': round(clock.ms / n_res, 3), 'host_native_plan_ms': round(plan_clock.ms / n_res, 3),
                             'rest_ms': round(total['median_ms'] - (clock.ms + plan_clock.ms) / n_res, 3), 'add_adj_entries': add_adj.nnz,
                             'decoder_entries': dec.pattern.nnz, 'sub_entries': sub.pattern.nnz}

        # ---- per-entry attention on add_adj ----
        emb = model.getEgoEmbeds().detach()
        q, k = emb @ model.gtLayers.qTrans.detach(), emb @ model.gtLayers.kTrans.detach()
        fused, s_f = wall_ms(lambda: ops.edge_attention_scores(add_adj.pattern, q, k, model.gtLayers.head), reps=5)
        composed, s_c = wall_ms(lambda: switched('EDGE_SCORES_FUSED', False, lambda: ops.edge_attention_scores(add_adj.pattern, q, k, model.gtLayers.head)),
                                reps=5)
        rec['edge_attention_scores'] = {'fused': fused, 'composed': composed, 'composed_over_fused': round(composed['median_ms'] / fused['median_ms'], 1),
                                        'max_abs_diff': float((s_f - s_c).abs().max())}

        # ---- the training step ----
        rng = np.random.RandomState(d)
        batch = [torch.from_numpy(rng.randint(0, hi, BATCH)).to(dev) for hi in (model.user_num, model.item_num, model.item_num)]

        def step(graphs):
            loss, _ = model.cal_loss(batch, *graphs)
            trainer.optimizer.zero_grad()
            trainer._backward(loss)
            trainer.optimizer.step()
        graphs = (enc, dec, sub, cmp)
        step(graphs)
        plain, _ = wall_ms(lambda: [step(graphs) for _ in range(10)], reps=3, warmup=1)
        rec['step_without_resampling'] = {k_: (round(v / 10, 4) if k_.endswith('_ms') else v) for k_, v in plain.items()}

        def resampled_step():
            o = resample()
            step((o[2], o[3], o[4], o[5]))
        rec['step_with_resampling'], _ = wall_ms(resampled_step, reps=n_res, warmup=0)
        for name, flag in (('step_without_resampling_composed_pnn', 'PNN_FUSED'),):
            comp, _ = wall_ms(lambda: switched(flag, False, lambda: [step(graphs) for _ in range(10)]), reps=3, warmup=1)
            rec[name] = {k_: (round(v / 10, 4) if k_.endswith('_ms') else v) for k_, v in comp.items()}
        G.PropGraph = PropGraph
        print(json.dumps(rec))
        json.dump(rec, open(os.path.join(out_dir, '%s_d%d.json' % (dataset, d)), 'w'), indent=1)
        del model, trainer, out, enc, dec, sub, cmp, add_adj
        torch.cuda.empty_cache()
