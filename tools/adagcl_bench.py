#!/usr/bin/env python
"""AdaGCL on the amazon-book-shaped synthetic graph at d = 32 and 64, by HIP events, each beside the composed torch expression of the
same reference lines (models/general_cf/adagcl.py) on the same GPU in the same process:
  * the VGAE edge decoder over all entries and the generated view: ops.edge_mlp_logits + ops.edge_keep_view beside :224-237 (two
    [nnz, d] gathers, the [nnz, d] GEMM, the boolean index and a new sparse tensor);
  * DenoiseNet's gate of one layer, forward + backward down to the layer's weights: two [N, d] GEMMs + ops.edge_gate beside
    :274-311, :382-394, :340-347 on the [nnz, d] gathers;
  * one whole AdaGCLTrainer step beside the same four phases written with stock torch ops (torch.sparse.mm on rebuilt tensors).
Peak allocated memory (torch.cuda.max_memory_allocated above the resident state) is recorded for both forms of each.
usage: python tools/adagcl_bench.py [out_dir = profiles/adagcl] [dataset = amazon-book] [d ... = 32 64]"""
import json
import math
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
from sslrec_amd.graph import graph_of  # noqa: E402
from sslrec_amd.models.bulid_model import build_model  # noqa: E402
from sslrec_amd.trainer.build_trainer import build_trainer  # noqa: E402

dev = 'cuda:0'
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'adagcl')
dataset = sys.argv[2] if len(sys.argv) > 2 else 'amazon-book'
dims = [int(a) for a in sys.argv[3:]] or [32, 64]
assert torch.cuda.is_available(), 'this tool measures: it needs the GPU'
os.makedirs(out_dir, exist_ok=True)
BATCH = 4096


class _Log:
    def log(self, *a, **k):
        pass

    log_loss = log_eval = log


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


def sparse_mm(idx, vals, n, x):
    return torch.sparse.mm(torch.sparse_coo_tensor(idx, vals, (n, n)), x)


def torch_generate(vgae, x, idx, vals, n):
    """adagcl.py:224-237"""
    edge_pred = torch.sigmoid(vgae.decoder(x[idx[0]] * x[idx[1]]))[:, 0]
    mask = (edge_pred + 0.5).floor().type(torch.bool)
    new_vals = vals[mask]
    new_vals = new_vals / (new_vals.shape[0] / vals.shape[0])
    return torch.sparse_coo_tensor(idx[:, mask], new_vals, (n, n))


def torch_gate(net, x, idx, layer, m, noise, beta, eps, n):
    """adagcl.py:274-311, :382-394, :340-347: (values, l0 term)"""
    f1 = getattr(net, 'nblayers_%d' % layer)(x[idx[0]])
    f2 = getattr(net, 'selflayers_%d' % layer)(x[idx[1]])
    la = getattr(net, 'attentions_%d' % layer)(torch.concat([f1, f2], dim=1)).view(-1)
    g = torch.sigmoid(la if noise is None else (noise + la) / beta)
    mask = torch.clamp(g * (m['zeta'] - m['gamma']) + m['gamma'], 0.0, 1.0)
    rowsum = torch.zeros(n, device=x.device).index_add(0, idx[0], mask) + eps
    dinv = torch.clamp(torch.pow(rowsum, -0.5), 0.0, 10.0)
    return mask * dinv[idx[0]] * dinv[idx[1]], torch.sigmoid(la - beta * math.log(-m['gamma'] / m['zeta'])).mean()


def torch_bpr(x, n_user, batch):
    a, p, ng = x[batch[0]], x[n_user + batch[1]], x[n_user + batch[2]]
    return F.softplus((a * ng).sum(-1) - (a * p).sum(-1)).sum() / batch[0].shape[0]


class TorchStep:
    """the four phases of reference trainer/trainer.py:1153-1186 with stock torch ops and the modules' own parameters"""

    def __init__(self, model, trainer, idx, vals):
        self.model, self.t, self.idx, self.vals = model, trainer, idx, vals
        self.n, self.m = model.user_num + model.item_num, configs['model']

    def forward(self, adj):
        lst = [torch.concat([self.model.user_embeds, self.model.item_embeds], dim=0)]
        for _ in range(self.model.layer_num):
            lst.append(torch.sparse.mm(adj, lst[-1]))
        return sum(lst)

    def forward_(self):
        lst = [torch.concat([self.model.user_embeds, self.model.item_embeds], dim=0)]
        for i in range(self.model.layer_num):
            with torch.no_grad():
                v, _ = torch_gate(self.t.generator_2, lst[-1], self.idx, i, self.m, None, 1.0, 0.0, self.n)
            lst.append(sparse_mm(self.idx, v, self.n, lst[-1]))
        return sum(lst)

    def encoder(self, adj):
        vg = self.t.generator_1
        x = self.forward(adj).detach()
        mean, std = vg.encoder_mean(x), vg.encoder_std(x)
        return torch.randn(mean.shape, device=x.device) * std + mean, mean, std

    def __call__(self, batch, temperature):
        model, t, m, n = self.model, self.t, self.m, self.n
        opts = (t.optimizer, t.optimizer_gen_1, t.optimizer_gen_2)
        for o in opts:
            o.zero_grad()
        adj = torch.sparse_coo_tensor(self.idx, self.vals, (n, n))
        with torch.no_grad():
            data1 = torch_generate(t.generator_1, self.encoder(adj)[0], self.idx, self.vals, n)
        out1, out2 = self.forward(data1), self.forward_()
        (model.loss_graphcl(out1, out2, batch[0], batch[1]).mean() * model.cl_weight).backward()
        t.optimizer.step()
        t.optimizer.zero_grad()
        n1, n2 = self.forward(data1), self.forward_()
        ((model.loss_graphcl(n1, out1.detach(), batch[0], batch[1]) + model.loss_graphcl(n2, out2.detach(), batch[0], batch[1])).mean()
         * model.ib_weight).backward()
        t.optimizer.step()
        t.optimizer.zero_grad()
        reg = model.reg_weight * sum(w.norm(2).square() for w in model.parameters())
        (torch_bpr(self.forward(adj), model.user_num, batch) + reg).backward()
        vg = t.generator_1
        x, mean, std = self.encoder(adj)
        xu, xi = x[:model.user_num], x[model.user_num:]
        pos = torch.sigmoid(vg.decoder(xu[batch[0]] * xi[batch[1]]))
        neg = torch.sigmoid(vg.decoder(xu[batch[0]] * xi[batch[2]]))
        rec = vg.bceloss(pos, torch.ones_like(pos)) + vg.bceloss(neg, torch.zeros_like(neg))
        kl = -0.5 * (1 + 2 * torch.log(std) - mean ** 2 - std ** 2).sum(dim=1)
        loss_vgae = (rec + 0.1 * kl.mean() + torch_bpr(x, model.user_num, batch)).mean()
        net = t.generator_2
        x = net.features.detach()
        lst, l0 = [x], 0
        for i in range(model.layer_num):
            noise = net.hard_concrete_sample(self.idx.shape[1], x.device)
            v, l0_i = torch_gate(net, x, self.idx, i, m, noise, temperature, 1e-6, n)
            l0 = l0 + l0_i
            x = sparse_mm(self.idx, v, n, x)
            lst.append(x)
        (loss_vgae + torch_bpr(sum(lst), model.user_num, batch) + l0 * m['lambda0']).backward()
        for o in opts:
            o.step()


for d in dims:
    load_config('adagcl', device=dev, overrides={'data': {'synthetic': dataset}, 'train': {'batch_size': BATCH}, 'model': {'embedding_size': d}})
    dh = DataHandlerGeneralCF()
    dh.trn_mat = dh._load_one_mat(dh.trn_file)
    configs['data']['user_num'], configs['data']['item_num'] = dh.trn_mat.shape
    dh.torch_adj = dh._make_torch_adj(dh.trn_mat)
    torch.manual_seed(d)
    np.random.seed(d)
    model = build_model(dh).to(dev)
    trainer = build_trainer(dh, _Log())
    trainer.create_optimizer(model)
    n_user, n = model.user_num, model.user_num + model.item_num
    graph = graph_of(dh.torch_adj)
    idx, vals = dh.torch_adj._indices().to(dev), dh.torch_adj._values().to(dev)
    nnz = idx.shape[1]
    m = configs['model']
    rec = {'dataset': dataset, 'n_user': n_user, 'n_item': model.item_num, 'nnz': nnz, 'd': d, 'batch': BATCH}
    vgae, net = trainer.generator_1, trainer.generator_2
    gen = torch.Generator().manual_seed(d)
    x = (0.5 * torch.randn(n, d, generator=gen)).to(dev)
    with torch.no_grad():                            # a decoder bias that keeps about half of the entries, as a trained one does
        probe = ops.edge_mlp_logits(graph, x, vgae.decoder[1].weight, vgae.decoder[1].bias, vgae.decoder[3].weight, vgae.decoder[3].bias)
        vgae.decoder[3].bias -= probe.median()

    # -- the decoder over all entries and the generated view ------------------------------------------------------------------
    dec1, dec2 = vgae.decoder[1], vgae.decoder[3]

    def hip_decoder():
        return ops.edge_keep_view(graph, ops.edge_mlp_logits(graph, x, dec1.weight, dec1.bias, dec2.weight, dec2.bias))

    def torch_decoder():
        return torch_generate(vgae, x, idx, vals, n)

    with torch.no_grad():
        view, keep, kept = hip_decoder()
        ref = torch_decoder().coalesce()
        rec['decoder_kept'] = {'hip': int(kept.item()), 'torch': int(ref.values().numel())}
        rec['decoder_hip'] = timed_us(hip_decoder, 10)
        rec['decoder_torch'] = timed_us(torch_decoder, 3)
        rec['decoder_hip_peak_MB'] = peak_mb(hip_decoder)
        rec['decoder_torch_peak_MB'] = peak_mb(torch_decoder)
        del view, keep, kept, ref
    rec['decoder_torch_over_hip'] = round(rec['decoder_torch']['median_us'] / rec['decoder_hip']['median_us'], 2)

    # -- the gate of layer 0, forward + backward down to the layer's weights ---------------------------------------------------
    noise = net.hard_concrete_sample(nnz, dev)
    dvals = (torch.randn(nnz, generator=gen)).to(dev)
    gate_params = [p for name, p in net.named_parameters() if name.endswith('_0.0.weight') or name.endswith('_0.0.bias')]

    def clear():
        for p in gate_params:
            p.grad = None

    def hip_gate():
        clear()
        p, q, bias = net.get_attention(x, x, 0)
        v, l0 = ops.edge_gate(graph, p, q, bias, m['gamma'], m['zeta'], beta=2.0, noise=noise, eps=1e-6)
        ((v * dvals).sum() + 0.7 * l0).backward()

    def torch_gate_():
        clear()
        v, l0 = torch_gate(net, x, idx, 0, m, noise, 2.0, 1e-6, n)
        ((v * dvals).sum() + 0.7 * l0).backward()

    hip_gate()
    got = [p.grad.clone() for p in gate_params]
    torch_gate_()
    rec['gate_agreement_with_torch_fp32'] = [float((a - p.grad).abs().max() / p.grad.abs().max()) for a, p in zip(got, gate_params)]
    rec['gate_hip_forward_backward'] = timed_us(hip_gate, 5)
    rec['gate_torch_forward_backward'] = timed_us(torch_gate_, 3)
    rec['gate_hip_peak_MB'] = peak_mb(hip_gate)
    rec['gate_torch_peak_MB'] = peak_mb(torch_gate_)
    rec['gate_torch_over_hip'] = round(rec['gate_torch_forward_backward']['median_us'] / rec['gate_hip_forward_backward']['median_us'], 2)
    clear()
    del got

    # -- the whole trainer step --------------------------------------------------------------------------------------------
    rng = np.random.RandomState(d)
    batch = [torch.from_numpy(rng.randint(0, hi, BATCH)).to(dev) for hi in (n_user, model.item_num, model.item_num)]
    torch_step = TorchStep(model, trainer, idx, vals)
    rec['hip_step'] = timed_us(lambda: trainer.train_step(model, batch, 2.0), 2, reps=5, warmup=2)
    rec['hip_step_peak_MB'] = peak_mb(lambda: trainer.train_step(model, batch, 2.0))
    rec['torch_step'] = timed_us(lambda: torch_step(batch, 2.0), 1, reps=5, warmup=1)
    rec['torch_step_peak_MB'] = peak_mb(lambda: torch_step(batch, 2.0))
    rec['torch_over_hip_step'] = round(rec['torch_step']['median_us'] / rec['hip_step']['median_us'], 2)
    print(json.dumps(rec))
    json.dump(rec, open(os.path.join(out_dir, '%s_d%d.json' % (dataset, d)), 'w'), indent=1)
    del model, trainer, torch_step, x, idx, vals, graph
    torch.cuda.empty_cache()
