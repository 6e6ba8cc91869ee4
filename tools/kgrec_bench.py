#!/usr/bin/env python
"""KGRec on the two synthetic kg shapes (synth.KG_SHAPES: kg-last-fm, kg-alibaba) at d = 32 and 64, on one GPU in one process, the
kernels (csrc/rmha.hip) against the composed torch expressions (SSLREC_KGREC_FUSED=0's path):
  * ops.rel_mh_attention over the handler's graph with a half keep mask, forward and forward + backward, both ways, alternating, timed
    with device events around REPS calls after a warm-up of both;
  * ops.rel_rationale under the same mask, both ways;
  * the bytes the forward must move (every slot's edge id and mask byte; per kept edge two more indices, a row of T and a row of X and
    the two logits written; T, Y, the maxima, the sums and the row pointer per entity; the relation table once -- computed from the
    shapes, not counters) and the time those bytes take at the HBM peak of 8 TB/s;
  * the whole training step (zero_grad, cal_loss, backward, Adam) both ways, and the kernel launches of one step both ways as the
    profiler counts them (null where it cannot);
  * the share of the fused step spent in torch.topk, torch.multinomial and the Gumbel draws (device events around each call).
usage: python tools/kgrec_bench.py [out_dir = profiles/kgrec] [shape ... = kg-last-fm kg-alibaba]"""
import json
import os
import random
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
from sslrec_amd.models.kg import kgrec as kgrec_module  # noqa: E402
from sslrec_amd.trainer.trainer import Trainer  # noqa: E402

dev = 'cuda:0'
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'kgrec')
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
        ops.KGREC_FUSED = fused
        try:
            return fn()
        finally:
            ops.KGREC_FUSED = True
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
    ops.KGREC_FUSED = fused
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
        ops.KGREC_FUSED = True


def timed_calls(step):
    """ms per step spent inside torch.topk, torch.multinomial and the model's gumbel_like, by device events around every call of one
    fused step (after a warm-up step), and the ms of that step"""
    spans = {'topk': [], 'multinomial': [], 'gumbel': []}

    def wrap(name, fn):
        def inner(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            spans[name].append((e0, e1))
            return out
        return inner
    saved = (torch.topk, torch.multinomial, kgrec_module.gumbel_like)
    step()
    torch.topk, torch.multinomial, kgrec_module.gumbel_like = wrap('topk', saved[0]), wrap('multinomial', saved[1]), wrap('gumbel', saved[2])
    try:
        whole = event_ms(step, 1)
    finally:
        torch.topk, torch.multinomial, kgrec_module.gumbel_like = saved
    out = {k: round(sum(a.elapsed_time(b) for a, b in v), 4) for k, v in spans.items()}
    out['calls'] = {k: len(v) for k, v in spans.items()}
    out['step_ms'] = round(whole, 4)
    out['share_of_step'] = {k: round(out[k] / whole, 4) for k in spans}
    return out


for shape in shapes:
    dh, build_s = None, None
    for d in (32, 64):
        load_config('kgrec', device=dev, overrides={'data': {'synthetic': shape}, 'train': {'batch_size': BATCH}, 'model': {'embedding_size': d}})
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
        random.seed(d)
        model = build_model(dh).to(dev)
        trainer = Trainer(dh, _Log())
        trainer.create_optimizer(model)
        g = dh.rel_graph
        U, N, E, Rn = model.n_users, model.n_entities, g.n_edges, g.n_rel
        rec = {'shape': shape, 'n_user': U, 'n_item': model.n_items, 'n_entity': N, 'relations': Rn, 'kg_edges': E,
               'interaction_entries': int(dh.interact_mat._nnz()), 'd': d, 'batch': BATCH, 'layer_num': model.context_hops,
               'mae_msize': model.mae_msize,
               'longest_list': {'by_head': g.by_head.max_len, 'by_tail': g.by_tail.max_len, 'by_rel': g.by_rel.max_len},
               'chunks': {'by_head': g.by_head.n_chunks, 'by_tail': g.by_tail.n_chunks, 'by_rel': g.by_rel.n_chunks},
               'host_load_and_build_seconds': round(build_s, 2)}
        gen = torch.Generator().manual_seed(d)

        # (a) rel_mh_attention and rel_rationale under a half mask
        x = (0.1 * torch.randn(N, d, generator=gen)).to(dev).requires_grad_(True)
        tq = (0.1 * torch.randn(N, d, generator=gen)).to(dev).requires_grad_(True)
        r = model.gcn.relation_emb.detach().clone().requires_grad_(True)
        keep = (torch.rand(E, generator=gen) < 0.5).to(dev).to(torch.uint8)
        gy = torch.randn(N, d, device=dev)

        def att_fwd():
            with torch.no_grad():
                ops.rel_mh_attention(g, x, tq, r, keep)

        def att_both():
            ops.rel_mh_attention(g, x, tq, r, keep).backward(gy, inputs=[x, tq, r])

        def rationale():
            ops.rel_rationale(g, tq, r, keep)
        n_kept = int(keep.sum())
        fwd_bytes = E * 5 + n_kept * (8 + 8 * d + 8) + N * (8 * d + 20) + Rn * d * 4
        rec['rel_mh_attention'] = {'forward': ab(att_fwd), 'forward_backward': ab(att_both), 'kept_edges': n_kept, 'forward_bytes': int(fwd_bytes),
                                   'forward_ms_at_8TBps': round(fwd_bytes / HBM_BYTES_PER_S * 1e3, 4),
                                   'note': 'bytes computed from the shapes (edge id and mask byte per slot; two indices, a row of T, a row of X '
                                           'and two logits per kept edge; T, Y, two maxima, two sums and pointer per entity; R once), not from '
                                           'counters'}
        rec['rel_mh_attention']['forward_GBps_of_those_bytes'] = round(fwd_bytes / rec['rel_mh_attention']['forward']['fused']['median_ms'] / 1e6, 1)
        rec['rel_rationale'] = ab(rationale)

        # (b) the whole step
        rng = np.random.RandomState(d)
        batch = [torch.from_numpy(rng.randint(0, hi, BATCH)).to(dev) for hi in (U, model.n_items, model.n_items)]
        rec['step'] = ab(lambda: trainer._eager_step(model, batch), reps=3, rounds=3)
        rec['launches_per_step'] = {'fused': count_launches(lambda: trainer._eager_step(model, batch), True),
                                    'composed': count_launches(lambda: trainer._eager_step(model, batch), False)}
        rec['draws_in_a_fused_step'] = timed_calls(lambda: trainer._eager_step(model, batch))
        print(json.dumps(rec))
        json.dump(rec, open(os.path.join(out_dir, '%s_d%d.json' % (shape, d)), 'w'), indent=1)
        del model, trainer, batch
        torch.cuda.empty_cache()
    del dh
