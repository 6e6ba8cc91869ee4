#!/usr/bin/env python
"""MHCN on the two synthetic social shapes (synth.SOCIAL_SHAPES: social-yelp, social-epinions) at d = 32 and 64, on one GPU in one
process, the kernels (csrc/mhcn.hip, csrc/mhcn_gate.hip) against the composed torch expressions (SSLREC_MHCN_FUSED=0's path):
  * per op -- ops.self_gate (4 gates), ops.channel_mix with the layer sums, ops.hier_ssl_loss -- forward + backward, both ways,
    alternating, timed with device events around REPS calls after a warm-up of both;
  * the ALGORITHMIC bytes of each op, forward + backward, computed from the shapes (every input read once, every output and every
    gradient written once; not counters), and the rate they imply at the measured time;
  * the whole training step (zero_grad, cal_loss, backward, Adam) both ways, and the kernel launches of one step both ways as the
    profiler counts them (null where it cannot);
  * the nnz of H_s, H_j, H_p and R and the seconds the host took to build them.
usage: python tools/mhcn_bench.py [out_dir = profiles/mhcn] [shape ... = social-yelp social-epinions]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sslrec_amd import ops  # noqa: E402
from sslrec_amd.config.configurator import load_config  # noqa: E402
from sslrec_amd.data_utils.data_handler_social import DataHandlerSocial  # noqa: E402
from sslrec_amd.models.bulid_model import build_model  # noqa: E402
from sslrec_amd.trainer.trainer import Trainer  # noqa: E402

dev = 'cuda:0'
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'mhcn')
shapes = sys.argv[2:] or ['social-yelp', 'social-epinions']
assert torch.cuda.is_available(), 'this tool measures: it needs the GPU'
os.makedirs(out_dir, exist_ok=True)
BATCH, REPS, ROUNDS = 2000, 20, 5


class _Log:
    def log(self, *a, **k):
        pass

    log_loss = log_eval = log


def event_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def ab(fn, reps=REPS, rounds=ROUNDS):
    """{'fused': ..., 'composed': ...} ms per call: both warmed up, then `rounds` alternating windows of `reps` calls each"""
    def run(fused):
        ops.MHCN_FUSED = fused
        try:
            return fn()
        finally:
            ops.MHCN_FUSED = True
    for fused in (True, False):
        for _ in range(3):
            run(fused)
    t = {True: [], False: []}
    for _ in range(rounds):
        for fused in (True, False):
            t[fused].append(event_ms(lambda: run(fused), reps))
    out = {}
    for fused, name in ((True, 'fused'), (False, 'composed')):
        v = sorted(t[fused])
        out[name] = {'median_ms': round(v[len(v) // 2], 4), 'min_ms': round(v[0], 4), 'max_ms': round(v[-1], 4), 'windows': rounds, 'calls_per_window': reps}
    out['composed_over_fused'] = round(out['composed']['median_ms'] / out['fused']['median_ms'], 2)
    return out


def with_rate(rec, n_bytes):
    rec['algorithmic_bytes'] = int(n_bytes)
    for name in ('fused', 'composed'):
        rec[name]['GBps_of_algorithmic_bytes'] = round(n_bytes / rec[name]['median_ms'] / 1e6, 1)
    rec['note'] = 'bytes computed from the shapes (inputs read once, outputs and gradients written once), not from counters'
    return rec


def count_launches(fn, fused):
    ops.MHCN_FUSED = fused
    try:
        fn()
        torch.cuda.synchronize()
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).lower().endswith('cuda') and 'memcpy' not in e.name.lower()
                and 'memset' not in e.name.lower())
        return n or None
    except Exception as exc:          # the count is a by-product: the timings do not depend on it
        print('launch count not available: %r' % (exc,))
        return None
    finally:
        ops.MHCN_FUSED = True


for shape in shapes:
    for d in (32, 64):
        load_config('mhcn', device=dev, overrides={'data': {'synthetic': shape}, 'train': {'batch_size': BATCH}, 'model': {'embedding_size': d}})
        t0 = time.perf_counter()
        dh = DataHandlerSocial()
        dh.load_data()
        build_s = time.perf_counter() - t0
        torch.manual_seed(d)
        np.random.seed(d)
        model = build_model(dh).to(dev)
        trainer = Trainer(dh, _Log())
        trainer.create_optimizer(model)
        U, I = model.user_num, model.item_num
        rec = {'shape': shape, 'n_user': U, 'n_item': I, 'interactions': int(dh.trn_mat.nnz), 'trust_edges': int(dh.trust_mat.nnz), 'd': d,
               'batch': BATCH, 'layer_num': model.layer_num, 'nnz': dh.nnz, 'host_load_and_build_seconds': round(build_s, 2)}
        fb = 4 * U * d                                           # bytes of one [U, d] table
        gen = torch.Generator().manual_seed(d)

        def table(scale=0.1):
            return (scale * torch.randn(U, d, generator=gen)).to(dev).requires_grad_(True)

        # (a) self_gate, four gates
        x = table()
        ws = [m.weight for m in (model.gating1, model.gating2, model.gating3, model.gating4)]
        bs = [m.bias for m in (model.gating1, model.gating2, model.gating3, model.gating4)]
        gys = [torch.randn(U, d, device=dev) for _ in range(4)]

        def gate():
            ys = ops.self_gate(x, ws, bs)
            torch.autograd.backward(ys, gys, inputs=[x] + ws + bs)
        rec['self_gate_4'] = with_rate(ab(gate), fb * (1 + 4) + fb * (1 + 4 + 1) + 3 * 4 * d * (d + 1) * 4)      # fwd: x, 4 y; bwd: x, 4 dy, dx; W, b, dW, db

        # (b) channel_mix with the layer sums
        tabs, sums = [table() for _ in range(4)], [table(1.0) for _ in range(4)]
        v = (model.attn_mat @ model.attn.t()).reshape(-1).detach().requires_grad_(True)
        gm = [torch.randn(U, d, device=dev) for _ in range(5)]

        def mix():
            mixed, outs = ops.channel_mix(*tabs, v, sums=sums)
            torch.autograd.backward([mixed] + list(outs), gm, inputs=tabs + sums + [v])
        rec['channel_mix_sums'] = with_rate(ab(mix), fb * (8 + 5) + fb * (4 + 5 + 4))      # fwd: 4 e, 4 a, 5 out; bwd: 4 e, 5 g, 4 de (da = g)

        # (c) hier_ssl_loss on H_s
        em = table(0.3)
        perms = [torch.randperm(n, generator=gen).to(dev) for n in (U, d, U, d, U)]

        def ssl_only():          # (edge = H_s em is the caller's SpMM, the same both ways: not in the window)
            ops.hier_ssl_loss(em_l, edge_l, perms).backward(inputs=[em_l, edge_l])
        em_l = em.detach().requires_grad_(True)
        edge_l = ops.spmm(dh.H_s, em_l).detach().requires_grad_(True)
        rec['hier_ssl_loss'] = with_rate(ab(ssl_only), fb * 5 + fb * (5 + 2 + 2))      # fwd: em, em[p], edge, 2 shuffled edge; bwd: those, + 2 gathers, 2 grads

        # the whole step
        rng = np.random.RandomState(d)
        batch = [torch.from_numpy(rng.randint(0, hi, BATCH)).to(dev) for hi in (U, I, I)]
        rec['step'] = ab(lambda: trainer._eager_step(model, batch), reps=10)
        rec['launches_per_step'] = {'fused': count_launches(lambda: trainer._eager_step(model, batch), True),
                                    'composed': count_launches(lambda: trainer._eager_step(model, batch), False)}
        print(json.dumps(rec))
        json.dump(rec, open(os.path.join(out_dir, '%s_d%d.json' % (shape, d)), 'w'), indent=1)
        del model, trainer, dh
        torch.cuda.empty_cache()
