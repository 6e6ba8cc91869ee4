#!/usr/bin/env python
"""KGIN on the two synthetic kg shapes (synth.KG_SHAPES: kg-last-fm, kg-alibaba) at d = 32 and 64, on one GPU in one process, the
kernels (csrc/kgin.hip) against the composed torch expressions (SSLREC_KGIN_FUSED=0's path):
  * per op -- ops.rel_aggregate with a half keep mask, ops.factor_modulate -- forward and forward + backward, both ways, alternating,
    timed with device events around REPS calls after a warm-up of both;
  * for rel_aggregate the bytes it must move forward (kept edges x (one table row + the slot's three indices and its mask byte), the
    relation table once, the output rows and counts; computed from the shapes, not counters) and the time those bytes take at the
    HBM peak of 8 TB/s;
  * the whole training step (zero_grad, cal_loss, backward, Adam) both ways, and the kernel launches of one step both ways as the
    profiler counts them (null where it cannot);
  * the host time of the step's np.random.choice(E, E / 2, replace=False) draw, and the seconds the host took to load and build.
usage: python tools/kgin_bench.py [out_dir = profiles/kgin] [shape ... = kg-last-fm kg-alibaba]"""
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
from sslrec_amd.data_utils.data_handler_kg import DataHandlerKG  # noqa: E402
from sslrec_amd.models.bulid_model import build_model  # noqa: E402
from sslrec_amd.trainer.trainer import Trainer  # noqa: E402

dev = 'cuda:0'
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'kgin')
shapes = sys.argv[2:] or ['kg-last-fm', 'kg-alibaba']
assert torch.cuda.is_available(), 'this tool measures: it needs the GPU'
os.makedirs(out_dir, exist_ok=True)
BATCH, REPS, ROUNDS = 1024, 10, 5
HBM_BYTES_PER_S = 8e12


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
        ops.KGIN_FUSED = fused
        try:
            return fn()
        finally:
            ops.KGIN_FUSED = True
    for fused in (True, False):
        for _ in range(2):
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


def count_launches(fn, fused):
    ops.KGIN_FUSED = fused
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
        ops.KGIN_FUSED = True


for shape in shapes:
    dh, build_s = None, None
    for d in (32, 64):
        load_config('kgin', device=dev, overrides={'data': {'synthetic': shape}, 'train': {'batch_size': BATCH}, 'model': {'embedding_size': d}})
        if dh is None:
            t0 = time.perf_counter()
            dh = DataHandlerKG()
            dh.load_data()
            build_s = time.perf_counter() - t0
            data_cfg = dict(configs['data'])
        else:
            configs['data'].update(data_cfg)
        torch.manual_seed(d)
        np.random.seed(d)
        model = build_model(dh).to(dev)
        trainer = Trainer(dh, _Log())
        trainer.create_optimizer(model)
        g = dh.rel_graph
        U, N, E, Rn = model.n_users, model.n_entities, g.n_edges, g.n_rel
        rec = {'shape': shape, 'n_user': U, 'n_item': model.n_items, 'n_entity': N, 'relations': Rn, 'kg_edges': E,
               'interactions': int(dh.interact_mat._nnz()), 'd': d, 'batch': BATCH, 'layer_num': model.context_hops,
               'longest_list': {'by_head': g.by_head.max_len, 'by_tail': g.by_tail.max_len, 'by_rel': g.by_rel.max_len},
               'chunks': {'by_head': g.by_head.n_chunks, 'by_tail': g.by_tail.n_chunks, 'by_rel': g.by_rel.n_chunks},
               'host_load_and_build_seconds': round(build_s, 2)}
        gen = torch.Generator().manual_seed(d)

        # (a) rel_aggregate under a half mask
        x = (0.1 * torch.randn(N, d, generator=gen)).to(dev).requires_grad_(True)
        w = model.gcn.weight.detach().clone().requires_grad_(True)
        keep = (torch.rand(E, generator=gen) < 0.5).to(dev).to(torch.uint8)
        gy = torch.randn(N, d, device=dev)

        def rel_fwd():
            with torch.no_grad():
                ops.rel_aggregate(g, x, w, keep)

        def rel_both():
            ops.rel_aggregate(g, x, w, keep).backward(gy, inputs=[x, w])
        n_kept = int(keep.sum())
        fwd_bytes = n_kept * (4 * d + 12) + E + Rn * d * 4 + N * (4 * d + 4 + 4)
        rec['rel_aggregate'] = {'forward': ab(rel_fwd), 'forward_backward': ab(rel_both), 'kept_edges': n_kept, 'forward_bytes': int(fwd_bytes),
                                'forward_ms_at_8TBps': round(fwd_bytes / HBM_BYTES_PER_S * 1e3, 4),
                                'note': 'bytes computed from the shapes (a table row, three indices and a mask byte per kept edge, the mask '
                                        'byte of every edge, W once, Y and the counts), not from counters'}
        rec['rel_aggregate']['forward_GBps_of_those_bytes'] = round(fwd_bytes / rec['rel_aggregate']['forward']['fused']['median_ms'] / 1e6, 1)

        def rel_atomics():          # the same expression as plain autograd: index_add_ and the gathers' backward with float atomics
            h, t, r = ops._kept_edges(g, keep)
            y = torch.zeros(N, d, device=dev).index_add_(0, h, x[t] * w[r])
            cnt = torch.zeros(N, device=dev).index_add_(0, h, torch.ones(h.numel(), device=dev))
            (y / cnt.clamp(min=1).unsqueeze(1)).backward(gy, inputs=[x, w])
        rel_atomics()
        rec['rel_aggregate']['forward_backward_plain_autograd_with_float_atomics_ms'] = round(sorted(event_ms(rel_atomics, REPS) for _ in range(3))[1], 4)

        # (b) factor_modulate
        agg = (0.1 * torch.randn(U, d, generator=gen)).to(dev).requires_grad_(True)
        ue = (0.1 * torch.randn(U, d, generator=gen)).to(dev).requires_grad_(True)
        lat = model.latent_emb.detach().clone().requires_grad_(True)
        dm = (torch.softmax(model.gcn.disen_weight_att, -1) @ model.gcn.weight).detach().clone().requires_grad_(True)
        gu = torch.randn(U, d, device=dev)

        def fm_fwd():
            with torch.no_grad():
                ops.factor_modulate(agg, ue, lat, dm)

        def fm_both():
            ops.factor_modulate(agg, ue, lat, dm).backward(gu, inputs=[agg, ue, lat, dm])
        rec['factor_modulate'] = {'forward': ab(fm_fwd), 'forward_backward': ab(fm_both)}

        # (c) the host draw of the edge sample
        t0 = time.perf_counter()
        for _ in range(3):
            np.random.choice(E, size=int(E * 0.5), replace=False)
        rec['host_edge_sample_ms'] = round((time.perf_counter() - t0) / 3 * 1e3, 2)

        # the whole step
        rng = np.random.RandomState(d)
        batch = [torch.from_numpy(rng.randint(0, hi, BATCH)).to(dev) for hi in (U, model.n_items, model.n_items)]
        rec['step'] = ab(lambda: trainer._eager_step(model, batch), reps=5)
        rec['launches_per_step'] = {'fused': count_launches(lambda: trainer._eager_step(model, batch), True),
                                    'composed': count_launches(lambda: trainer._eager_step(model, batch), False)}
        print(json.dumps(rec))
        json.dump(rec, open(os.path.join(out_dir, '%s_d%d.json' % (shape, d)), 'w'), indent=1)
        del model, trainer
        torch.cuda.empty_cache()
    del dh
