"""KGRec on the GPU: ops.rel_mh_attention and ops.rel_rationale (sslrec_amd/csrc/rmha.hip), the model (sslrec_amd/models/kg/kgrec.py) on
the kg data handler, and two epochs through the generic Trainer.

Yardstick (tests/kgrec_reference.py): a float64 torch restatement of the reference's expressions.  The same restatement runs in fp32 on
the CPU; its error against float64 is measured per tensor as max|x - ref| / max|ref|, and what runs on the GPU may be at most 4 x as far
off, with a floor of 8 * 2^-23.  Both errors are printed per tensor."""
import random

import numpy as np
import pytest
import torch

import kgrec_reference as R
from test_kgcl import HUB_EDGES, MASKED_HEAD, ONE_HEAD, att_case

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu


def gpu(x):
    return x.detach().float().to(DEV)


# ---------------------------------------------------------------------------------------------------------------------
# ops.rel_mh_attention
# ---------------------------------------------------------------------------------------------------------------------
OUTPUTS = ('y', 'dx', 'dt', 'dr')
SHAPES = [(1, 1, 1, 32), (33, 200, 3, 32), (300, 4000, 7, 64), (300, 4000, 1100, 64), (257, 3000, 5, 128), (300, 4000, 7, 48)]

_REFS, _GRAPHS = {}, {}


def mh_case(N, E, Rn, d, scale=1.0):
    """(head, tail, rel, half mask, x, t, r, upstream gradient): the arrays of test_kgcl.att_case (an entity without edges, a head fully
    masked, a head with one kept edge, a pair under two relations, 5,000-edge hubs as head and as tail for N >= 257), its table p as the
    node table t; t and r are scaled by `scale`"""
    head, tail, rel, keep, x, p, _, r, go = att_case(N, E, Rn, d, scale)
    return head, tail, rel, keep, x, p, r, go


def mh_graph(key):
    from sslrec_amd.graph import RelGraph
    if key[:4] not in _GRAPHS:
        head, tail, rel = mh_case(*key)[:3]
        _GRAPHS[key[:4]] = RelGraph(head, tail, rel, key[0], key[2], device=DEV)
    return _GRAPHS[key[:4]]


def mh_reference(key, masked):
    """(float64, float32) restatement outputs, computed once per case"""
    if (key, masked) not in _REFS:
        head, tail, rel, keep, x, t, r, go = mh_case(*key)
        edges = tuple(torch.from_numpy(a) for a in (head, tail, rel))

        def fn(dt):
            leaves = [R.leaf(a, dt) for a in (x, t, r)]
            y = R.rel_mh_attention(*leaves, edges, keep if masked else None)
            (y * go.to(dt)).sum().backward()
            return dict(zip(OUTPUTS, [y.detach()] + [a.grad for a in leaves]))
        _REFS[(key, masked)] = R.both_precisions(fn)
    return _REFS[(key, masked)]


def mh_run(graph, case, masked, fused=True):
    from sslrec_amd import ops
    keep, go = case[3], case[7]
    leaves = [gpu(a).requires_grad_(True) for a in case[4:7]]
    y = ops.rel_mh_attention(graph, *leaves, keep.to(DEV) if masked else None)
    assert ('_RelMhAttentionFn' in type(y.grad_fn).__name__) == fused, type(y.grad_fn).__name__
    (y * gpu(go)).sum().backward()
    return dict(zip(OUTPUTS, [y.detach()] + [a.grad for a in leaves]))


def mh_check(key, label):
    from sslrec_amd import ops
    from sslrec_amd.graph import REL_CHUNK
    N, E, Rn, d = key[:4]
    fused = d != 48
    assert ops.kgin_fused_ok(d) == fused
    case = mh_case(*key)
    head, tail, rel = case[:3]
    graph = mh_graph(key)
    if N >= 257:                    # the chunked softmax merge, the long tails and the long relation lists are taken
        assert graph.by_head.n_long >= 1 and graph.by_tail.n_long >= 1 and graph.by_rel.n_long >= 1
        assert graph.by_head.max_len > HUB_EDGES > REL_CHUNK
    for masked in (False, True):
        r64, r32 = mh_reference(key, masked)
        got = mh_run(graph, case, masked, fused)
        for k in OUTPUTS:
            R.check('%s %s %s%s' % (label, k, key[:4], ' masked' if masked else ''), got[k], r64[k], r32[k])
        if N > 1:
            for k in ('y', 'dx', 'dt'):                                                                       # the entity without edges
                assert bool((got[k][N - 1] == 0).all()), k
            if masked:                                                                                       # no 0 / 0
                assert bool((got['y'][MASKED_HEAD] == 0).all())
                assert all(bool(torch.isfinite(got[k]).all()) for k in OUTPUTS)
                one = int(np.nonzero(head == ONE_HEAD)[0][0])
                assert int((head == ONE_HEAD).sum()) == 1
                want = gpu(case[4])[int(tail[one])] * gpu(case[6])[int(rel[one])]
                assert torch.equal(got['y'][ONE_HEAD], want)                                                 # softmax of one edge: x[t] r[rel]
            unused = np.setdiff1d(np.arange(Rn), rel[case[3].numpy()] if masked else rel)
            assert Rn < 1000 or unused.size > 1000
            assert bool((got['dr'][torch.from_numpy(unused).to(DEV)] == 0).all())                            # exactly 0
        again = mh_run(graph, case, masked, fused)
        for k in OUTPUTS:
            assert torch.equal(got[k], again[k]), k


@pytest.mark.parametrize('N,E,Rn,d', SHAPES)
def test_rel_mh_attention_values_and_gradients(N, E, Rn, d):
    mh_check((N, E, Rn, d, 1.0), 'rel_mh_attention')


def test_rel_mh_attention_with_logits_beyond_300():
    """t and r scaled by 5: a logit is a sum of 32 products of three factors over sqrt(32), its standard deviation 5^3 = 125, where exp
    overflows without the subtraction of the maximum"""
    key = (300, 4000, 7, 64, 5.0)
    head, tail, rel, _, _, t, r, _ = mh_case(*key)
    logits = R.mh_logits(t, r, tuple(torch.from_numpy(a) for a in (head, tail, rel)))
    assert float(logits.max()) > 300 and float(logits.min()) < -300
    mh_check(key, 'rel_mh_attention +-300')


def test_a_subset_of_the_gradients_has_the_bits_of_the_full_set():
    from sslrec_amd import ops
    key = (300, 4000, 7, 64, 1.0)
    case, graph = mh_case(*key), mh_graph(key)
    full = mh_run(graph, case, True)
    for wanted in ((0,), (1,), (2,), (0, 2)):
        leaves = [gpu(a).requires_grad_(i in wanted) for i, a in enumerate(case[4:7])]
        y = ops.rel_mh_attention(graph, *leaves, case[3].to(DEV))
        (y * gpu(case[7])).sum().backward()
        for i, a in enumerate(leaves):
            assert (a.grad is not None) == (i in wanted)
            if i in wanted:
                assert torch.equal(a.grad, full[OUTPUTS[1 + i]]), (wanted, i)


def test_attn_hgcn_aggregate_carries_the_gradient_to_w_q():
    """T = x @ w_q inside autograd against the literal shared_layer_agg with its [E, d] gathers through `@ W_Q`"""
    from sslrec_amd import ops
    key = (300, 4000, 7, 64, 1.0)
    head, tail, rel, keep, x, _, r, go = mh_case(*key)
    graph = mh_graph(key)
    w = R.randn((64, 64), 11, 0.2)
    edges = tuple(torch.from_numpy(a) for a in (head, tail, rel))
    names = ('y', 'dx', 'dw', 'dr')

    def fn(dt):
        leaves = [R.leaf(a, dt) for a in (x, w, r)]
        y = R.shared_layer_agg_kg(*leaves, edges, keep)
        (y * go.to(dt)).sum().backward()
        return dict(zip(names, [y.detach()] + [a.grad for a in leaves]))
    r64, r32 = R.both_precisions(fn)
    leaves = [gpu(a).requires_grad_(True) for a in (x, w, r)]
    y = ops.attn_hgcn_aggregate(graph, *leaves, keep.to(DEV))
    (y * gpu(go)).sum().backward()
    got = dict(zip(names, [y.detach()] + [a.grad for a in leaves]))
    for k in names:
        R.check('attn_hgcn_aggregate %s' % k, got[k], r64[k], r32[k])


# ---------------------------------------------------------------------------------------------------------------------
# ops.rel_rationale
# ---------------------------------------------------------------------------------------------------------------------
RAT = ('score', 'logits', 'mean_head', 'mean_tail')


@pytest.mark.parametrize('N,E,Rn,d', SHAPES)
def test_rel_rationale_against_the_restatement(N, E, Rn, d):
    from sslrec_amd import ops
    key = (N, E, Rn, d, 1.0)
    head, tail, rel, keep, _, t, r, _ = mh_case(*key)
    graph = mh_graph(key)
    edges = tuple(torch.from_numpy(a) for a in (head, tail, rel))
    for masked in (False, True):
        k_cpu = keep if masked else None
        r64, r32 = R.both_precisions(lambda dt: dict(zip(RAT, R.rel_rationale(t.to(dt), r.to(dt), edges, k_cpu))))
        run = lambda: dict(zip(RAT, ops.rel_rationale(graph, gpu(t), gpu(r), keep.to(DEV) if masked else None)))
        got = run()
        assert all(not v.requires_grad for v in got.values())
        for k in RAT:
            R.check('rel_rationale %s %s%s' % (k, key[:4], ' masked' if masked else ''), got[k], r64[k], r32[k])
        kept = keep.numpy() if masked else np.ones(head.size, dtype=bool)
        assert bool((got['score'].cpu()[torch.from_numpy(~kept)] == 0).all()) and bool((got['logits'].cpu()[torch.from_numpy(~kept)] == 0).all())
        # each head's scores sum to its kept degree
        deg = torch.from_numpy(np.bincount(head[kept], minlength=N)).double()
        sums = lambda s: torch.zeros(N, dtype=torch.float64).index_add_(0, torch.from_numpy(head), s.cpu().double())
        assert torch.equal(sums(r64['score']).round(), deg)
        R.check('rel_rationale head sums %s' % (key[:4],), sums(got['score']), sums(r64['score']), sums(r32['score']))
        if N > 1:
            assert float(got['mean_head'][N - 1]) == 0 and float(got['mean_tail'][N - 1]) == 0
            if masked:
                assert float(got['mean_head'][MASKED_HEAD]) == 0
                one = int(np.nonzero(head == ONE_HEAD)[0][0])
                assert float(got['score'][one]) == 1.0 and float(got['mean_head'][ONE_HEAD]) == 1.0
        again = run()
        for k in RAT:
            assert torch.equal(got[k], again[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# memory
# ---------------------------------------------------------------------------------------------------------------------
def test_rel_mh_attention_makes_no_edge_sized_matrix(monkeypatch):
    from sslrec_amd import ops
    from sslrec_amd.graph import RelGraph
    N, E, Rn, d = 2000, 200000, 7, 64
    rng = np.random.RandomState(9)
    graph = RelGraph(rng.randint(0, N, E), rng.randint(0, N, E), rng.randint(0, Rn, E), N, Rn, device=DEV)
    leaves = [gpu(R.randn(s, i, 0.3)).requires_grad_(True) for i, s in enumerate([(N, d), (N, d), (Rn, d)])]
    go = gpu(R.randn((N, d), 7))
    keep = torch.from_numpy(rng.rand(E) < 0.5).to(DEV).to(torch.uint8)

    def peak():
        for a in leaves:
            a.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        (ops.rel_mh_attention(graph, *leaves, keep) * go).sum().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before
    fused = peak()
    monkeypatch.setattr(ops, 'KGREC_FUSED', False)
    composed = peak()
    print('rel_mh_attention forward + backward, peak above the level before the call: kernels %d bytes, composed %d bytes, E d 4 = %d' %
          (fused, composed, E * d * 4))
    assert fused < E * d * 4
    assert composed > E * d * 4


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def kg_handler(d, overrides=None):
    from sslrec_amd.config.configurator import load_config
    from sslrec_amd.data_utils.data_handler_kg import DataHandlerKG
    model = {'embedding_size': d, 'mae_msize': 32}
    model.update(overrides or {})
    load_config('kgrec', device=DEV, overrides={'data': {'synthetic': 'kg-tiny'}, 'model': model, 'train': {'batch_size': 128},
                                                'test': {'batch_size': 32}})
    dh = DataHandlerKG()
    dh.load_data()
    return dh


PARTS = ('rec_loss', 'mae_loss', 'cl_loss')


def model_run(model, batch):
    model.zero_grad()
    loss, parts = model.cal_loss(batch)
    loss.backward()
    res = {'loss': loss.detach().reshape(-1, 1)}
    res.update({k: parts[k].detach().reshape(-1, 1) for k in PARTS})
    res.update({'grad ' + n: p.grad.clone() for n, p in model.named_parameters()})
    return res


def model_reference(model, dh, params, batch):
    from test_kgrec_host import restatement_inputs

    def fn(dt):
        p = {n: R.leaf(v.cpu(), dt) for n, v in params.items()}
        edges, sel, mats, hp, masks = restatement_inputs(model, dh, dt)
        out = R.model_loss(p, (model.n_users, model.n_items), edges, sel, mats, batch, hp, masks)
        out['loss'].backward()
        res = {k: out[k].detach().reshape(-1, 1) for k in ('loss',) + PARTS}
        res.update({'grad ' + n: p[n].grad for n in R.PARAM_NAMES})
        return res
    return R.both_precisions(fn)


@pytest.mark.parametrize('d', [32, 64])
def test_model_against_the_float64_restatement(d, monkeypatch):
    from sslrec_amd import ops
    from sslrec_amd.models.bulid_model import build_model
    dh = kg_handler(d)
    torch.manual_seed(d)
    model = build_model(dh).to(DEV)
    params = {n: p.detach().clone() for n, p in model.named_parameters()}
    rng = np.random.RandomState(d)
    ui = np.asarray(dh.ui_edges)
    pick = rng.randint(0, len(ui), 100)
    batch_cpu = (torch.from_numpy(ui[pick, 0]).long(), torch.from_numpy(ui[pick, 1]).long(), torch.from_numpy(rng.randint(0, 50, 100)).long())
    batch = [b.to(DEV) for b in batch_cpu]
    calls, fwd = [], ops._lib.load().sslrec_rmha_fwd_f32

    def counted(*a):
        calls.append(1)
        return fwd(*a)
    monkeypatch.setattr(ops._lib.load(), 'sslrec_rmha_fwd_f32', counted)
    np.random.seed(5)
    torch.manual_seed(5)
    got = model_run(model, batch)
    assert len(calls) == model.context_hops                                    # the kernels ran, once per hop
    recorded = [model.last_sample_ids.clone(), model.last_enc_keep.clone(), model.last_cl_keep.clone(), model.last_masked_ids.clone(),
                model.last_ui_keep.clone(), model.last_cl_ui_ids.clone(), model.last_rand_item.clone()]
    assert len(model.last_mess_masks) == 5 * model.context_hops
    r64, r32 = model_reference(model, dh, params, batch_cpu)
    assert set(got) == set(r64)
    for k in sorted(r64):
        R.check('kgrec fused %s (d = %d)' % (k, d), got[k], r64[k], r32[k])
    # the composed expressions on the same shapes (SSLREC_KGREC_FUSED=0), the same draws
    monkeypatch.setattr(ops, 'KGREC_FUSED', False)
    np.random.seed(5)
    torch.manual_seed(5)
    composed = model_run(model, batch)
    assert len(calls) == model.context_hops
    now = [model.last_sample_ids, model.last_enc_keep, model.last_cl_keep, model.last_masked_ids, model.last_ui_keep, model.last_cl_ui_ids,
           model.last_rand_item]
    if all(torch.equal(a, b) for a, b in zip(recorded, now)):                  # (a score within rounding of another may swap a top-k pick)
        for k in sorted(r64):
            R.check('kgrec composed %s (d = %d)' % (k, d), composed[k], r64[k], r32[k])
    else:
        c64, c32 = model_reference(model, dh, params, batch_cpu)
        for k in sorted(c64):
            R.check('kgrec composed, its own selections, %s (d = %d)' % (k, d), composed[k], c64[k], c32[k])
    monkeypatch.setattr(ops, 'KGREC_FUSED', True)


def test_device_rng_leaves_the_host_generators_alone():
    """model.device_rng: the sample, the random mask, the interaction dropout and the permutation are drawn on the device"""
    from sslrec_amd.models.bulid_model import build_model
    dh = kg_handler(32, {'device_rng': True})
    torch.manual_seed(3)
    model = build_model(dh).to(DEV)
    ui = np.asarray(dh.ui_edges)
    batch = [torch.from_numpy(ui[:100, 0]).long().to(DEV), torch.from_numpy(ui[:100, 1]).long().to(DEV), torch.arange(100).remainder(50).to(DEV)]
    np_before, torch_before = np.random.get_state(), torch.get_rng_state()
    loss, _ = model.cal_loss(batch)
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    # neither host generator moved
    assert all(np.array_equal(a, b) for a, b in zip(np_before, np.random.get_state())) and torch.equal(torch_before, torch.get_rng_state())
    # the sample keeps the reference's counts: int(n_r / 2) edges of every type but the last, none of the last
    edge_type = np.asarray(dh.kg_edges)[:, 2]
    ids = model.last_sample_ids.cpu().numpy()
    n_rel = model.n_relations
    assert np.unique(ids).size == ids.size
    assert np.array_equal(np.bincount(edge_type[ids], minlength=n_rel)[1:n_rel - 1], np.bincount(edge_type, minlength=n_rel)[1:n_rel - 1] // 2)
    assert not np.any(edge_type[ids] == n_rel - 1)
    nnz = dh.interact_mat._nnz()
    assert model.last_ui_keep.is_cuda and 0.3 * nnz < int(model.last_ui_keep.sum()) < 0.7 * nnz
    assert model.last_rand_item.is_cuda and sorted(model.last_rand_item.tolist()) == list(range(model.n_items))
    assert 32 <= model.last_masked_ids.numel() <= 64


class _Log:
    def log(self, *a, **k):
        pass

    log_loss = log_eval = log


def test_two_epochs_through_the_generic_trainer_on_kg_tiny():
    from sslrec_amd.config.configurator import configs, load_config
    from sslrec_amd.data_utils.build_data_handler import build_data_handler
    from sslrec_amd.models.bulid_model import build_model
    from sslrec_amd.trainer.build_trainer import build_trainer
    from sslrec_amd.trainer.trainer import Trainer
    load_config('kgrec', device=DEV, overrides={'data': {'synthetic': 'kg-tiny'}, 'train': {'epoch': 2, 'batch_size': 128, 'save_model': False, 'test_step': 1},
                                                'model': {'embedding_size': 32, 'mae_msize': 32}, 'test': {'batch_size': 32}})
    torch.manual_seed(2020)
    np.random.seed(2020)
    random.seed(2020)
    dh = build_data_handler()
    dh.load_data()
    model = build_model(dh).to(DEV)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    seen, cal_loss = [], model.cal_loss

    def spy(batch):
        loss, parts = cal_loss(batch)
        seen.append(torch.stack([loss.detach()] + [parts[k].detach().reshape(()) for k in PARTS]))
        return loss, parts
    model.cal_loss = spy
    trainer = build_trainer(dh, _Log())
    assert type(trainer) is Trainer
    trainer.train(model)
    assert len(seen) == 2 * len(dh.train_dataloader) and bool(torch.isfinite(torch.stack(seen)).all())
    for n, p in model.named_parameters():
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), before[n]), n
    result = trainer.evaluate(model)                                         # through predict_topk on the device
    assert set(result) == set(configs['test']['metrics']) and all(np.isfinite(v).all() and len(v) == 3 for v in result.values())
    assert all(0.0 <= float(x) <= 1.0 for v in result.values() for x in v)
