"""KGCL without a GPU: the yml, the construction sample, the parameter draws, the composed torch form of ops.rel_attention /
ops.rgat_aggregate in float64 against the restatement (tests/kgcl_reference.py) with gradcheck, the per-epoch views (weights and the
re-normalised adjacency against scipy), the model's cal_loss on the CPU in float64, the trainer factory and the refusals."""
import random

import numpy as np
import pytest
import torch

import kgcl_reference as R


def cfg(overrides=None, dataset=None, model='kgcl'):
    from sslrec_amd.config.configurator import load_config
    return load_config(model, dataset=dataset, device='cpu', overrides=overrides)


def tiny_handler(model=None, train=None, name='kgcl'):
    from sslrec_amd.data_utils.data_handler_kg import DataHandlerKG
    cfg({'data': {'synthetic': 'kg-tiny'}, 'model': dict({'embedding_size': 32}, **(model or {})), 'train': dict({'batch_size': 128}, **(train or {})),
         'test': {'batch_size': 32}}, model=name)
    dh = DataHandlerKG()
    dh.load_data()
    return dh


def tiny_batch(dh, B=100, seed=1):
    rng = np.random.RandomState(seed)
    ui = np.asarray(dh.ui_edges)
    pick = rng.randint(0, len(ui), B)
    return (torch.from_numpy(ui[pick, 0]).long(), torch.from_numpy(ui[pick, 1]).long(), torch.from_numpy(rng.randint(0, 50, B)).long())


def assert_close(name, got, want, rel=1e-12):
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= rel * max(scale, 1e-300), name


def test_yml_holds_the_reference_keys():
    c = cfg()
    assert c['optimizer'] == {'name': 'adam', 'lr': 1.0e-3, 'weight_decay': 0}
    assert c['train']['trainer'] == 'kgcl_trainer' and c['train']['epoch'] == 500 and c['train']['batch_size'] == 1024
    assert c['train']['kg_batch_size'] == 4096 and c['train']['loss'] == 'pairwise' and c['train']['test_step'] == 1 and c['train']['seed'] == 2020
    assert c['test'] == {'metrics': ['recall', 'ndcg'], 'k': [10, 20, 40], 'batch_size': 1024, 'eval_at_one_forward': True}
    assert c['data'] == {'type': 'kg', 'name': 'last-fm'}
    assert c['model'] == {'name': 'kgcl', 'train_trans': False, 'layer_num': 2, 'layer_num_kg': 2, 'decay_weight': 1.0e-5, 'embedding_size': 64,
                          'node_dropout': True, 'node_dropout_rate': 0.5, 'mess_dropout': True, 'mess_dropout_rate': 0.1, 'tau': 0.2,
                          'cl_weight': 0.1, 'mu': 0.7}


def test_construction_sample_is_the_references():
    from sslrec_amd.models.bulid_model import build_model
    from sslrec_amd.models.kg.kgcl import samp_edge_from_dict
    dh = tiny_handler()
    assert max(len(v) for v in dh.kg_dict.values()) > 15 and min(len(v) for v in dh.kg_dict.values()) <= 15          # both branches
    random.seed(11)
    model = build_model(dh)
    random.seed(11)
    want = np.asarray(R.samp_edge_from_dict(dh.kg_dict, 15))
    assert type(model).__name__ == 'KGCL' and np.array_equal(model.kg_sample, want)
    assert len(want) < len(dh.kg_edges) and np.bincount(want[:, 0]).max() == 15
    g = model.rel_graph
    assert g.n == 90 and g.n_rel == 8 and g.n_edges == len(want) and g is not dh.rel_graph
    assert np.array_equal(g.head.numpy(), want[:, 0]) and np.array_equal(g.tail.numpy(), want[:, 1]) and np.array_equal(g.rel.numpy(), want[:, 2] - 1)
    # a dict with one long and one short head
    random.seed(3)
    got = samp_edge_from_dict({4: [(1, t) for t in range(40)], 9: [(2, 5), (1, 5)]}, 15)
    random.seed(3)
    assert np.array_equal(got, np.asarray(R.samp_edge_from_dict({4: [(1, t) for t in range(40)], 9: [(2, 5), (1, 5)]}, 15))) and len(got) == 17


@pytest.mark.parametrize('seed', [3, 2020])
def test_parameter_names_shapes_and_draws(seed):
    from sslrec_amd.models.bulid_model import build_model
    dh = tiny_handler()
    torch.manual_seed(seed)
    model = build_model(dh)
    got = dict(model.named_parameters())
    want = R.draw_params(150, 9, 32, seed)
    assert list(got) == R.PARAM_NAMES
    for n in R.PARAM_NAMES:
        assert got[n].shape == want[n].shape and torch.equal(got[n].detach(), want[n]), n
    assert tuple(got['rgat.W'].shape) == (32, 32) and tuple(got['rgat.a'].shape) == (64, 1) and tuple(got['rgat.fc.weight'].shape) == (32, 64)
    assert sorted(model.state_dict()) == sorted(R.PARAM_NAMES)
    model.load_state_dict({k: v + 0.5 for k, v in want.items()})
    assert (model.tau, model.cl_weight, model.mu) == (0.2, 0.1, 0.95)                    # the code's constants, not the yml's mu = 0.7


# ---------------------------------------------------------------------------------------------------------------------
# ops.rel_attention, composed, float64
# ---------------------------------------------------------------------------------------------------------------------
def small_graph():
    """6 nodes, 20 edges: head 0 has a single edge, every edge of head 1 is masked, (2, 3) occurs under relations 0 and 1, node 5 has no
    edge at all"""
    rng = np.random.RandomState(2)
    head = np.array([0, 1, 1, 2, 2] + list(rng.randint(2, 5, 15)))
    tail = np.array([4, 0, 3, 3, 3] + list(rng.randint(0, 5, 15)))
    rel = np.array([1, 0, 2, 0, 1] + list(rng.randint(0, 3, 15)))
    keep = rng.rand(20) < 0.7
    keep[0], keep[1:3], keep[3:5] = True, False, True
    return head, tail, rel, torch.from_numpy(keep)


@pytest.mark.parametrize('masked', [False, True])
def test_composed_rel_attention_in_float64(masked):
    from sslrec_amd import ops
    from sslrec_amd.graph import RelGraph
    head, tail, rel, keep = small_graph()
    keep = keep if masked else None
    N, Rn, d = 6, 3, 8
    g = RelGraph(head, tail, rel, N, Rn)
    edges = tuple(torch.from_numpy(a) for a in (head, tail, rel))
    tens = [R.randn((N, d), 1), R.randn((N, d), 2), R.randn((N, d), 3), R.randn((Rn, d), 4)]
    go = R.randn((N, d), 5)
    a = [R.leaf(x, torch.float64) for x in tens]
    b = [R.leaf(x, torch.float64) for x in tens]
    ya, yb = ops.rel_attention(g, *a, keep), R.rel_attention(*b, edges, keep)
    (ya * go).sum().backward()
    (yb * go).sum().backward()
    assert_close('y', ya.detach(), yb.detach())
    for name, u, v in zip(('dx', 'dp', 'dq', 'dr'), a, b):
        assert_close(name, u.grad, v.grad)
    assert bool((ya[5] == 0).all()) and torch.equal(ya[0].detach(), tens[0][4])            # no edge: 0; one edge: x[t]
    if masked:
        assert bool((ya[1] == 0).all()) and bool((a[1].grad[1] == 0).all())
    # the backward of the formulas, written out per edge
    kept = np.ones(20, dtype=bool) if keep is None else keep.numpy()
    x, p, q, r = (t.numpy() for t in tens)
    G, Y = go.numpy(), ya.detach().numpy()
    l = np.array([(p[head[e]] + q[tail[e]]) @ r[rel[e]] for e in range(20)])
    s = np.where(l > 0, l, 0.2 * l)
    dx, dp, dq, dr = np.zeros((N, d)), np.zeros((N, d)), np.zeros((N, d)), np.zeros((Rn, d))
    for e in np.nonzero(kept)[0]:
        mine = kept & (head == head[e])
        alpha = np.exp(s[e] - s[mine].max()) / np.exp(s[mine] - s[mine].max()).sum()
        dl = alpha * (G[head[e]] @ x[tail[e]] - G[head[e]] @ Y[head[e]]) * (1.0 if l[e] > 0 else 0.2)
        dx[tail[e]] += alpha * G[head[e]]
        dp[head[e]] += dl * r[rel[e]]
        dq[tail[e]] += dl * r[rel[e]]
        dr[rel[e]] += dl * (p[head[e]] + q[tail[e]])
    for name, u, v in zip(('dx', 'dp', 'dq', 'dr'), a, (dx, dp, dq, dr)):
        assert_close(name + ' formula', u.grad, torch.from_numpy(v), 1e-11)
    assert torch.autograd.gradcheck(lambda *z: ops.rel_attention(g, *z, keep), [R.leaf(x, torch.float64) for x in tens])
    with pytest.raises(ValueError):
        ops.rel_attention(g, *a, torch.ones(19, dtype=torch.bool))
    with pytest.raises(ValueError):
        ops.rel_attention(g, a[0], a[1], a[2], a[3][:2])


@pytest.mark.parametrize('masked', [False, True])
def test_rgat_aggregate_is_the_literal_fc_of_the_concatenation(masked):
    from sslrec_amd import ops
    from sslrec_amd.graph import RelGraph
    head, tail, rel, keep = small_graph()
    keep = keep if masked else None
    N, Rn, d = 6, 3, 8
    g = RelGraph(head, tail, rel, N, Rn)
    edges = tuple(torch.from_numpy(a) for a in (head, tail, rel))
    tens = [R.randn((N, d), 1), R.randn((d, 2 * d), 2), R.randn((d,), 3), R.randn((Rn, d), 4)]
    go = R.randn((N, d), 5)
    a = [R.leaf(x, torch.float64) for x in tens]
    b = [R.leaf(x, torch.float64) for x in tens]
    ya = ops.rgat_aggregate(g, *a, keep)
    yb = R.rgat_agg(b[0], b[3], b[1], b[2], edges, keep)
    (ya * go).sum().backward()
    (yb * go).sum().backward()
    assert_close('y', ya.detach(), yb.detach())
    for name, u, v in zip(('dx', 'dW', 'db', 'dr'), a, b):
        assert_close(name, u.grad, v.grad, 1e-11)
    assert not ops.kgin_fused_ok(48) and all(ops.kgin_fused_ok(x) for x in (32, 64, 128))


# ---------------------------------------------------------------------------------------------------------------------
# the per-epoch views
# ---------------------------------------------------------------------------------------------------------------------
def test_aug_view_weights_and_adjacency():
    from sslrec_amd.models.bulid_model import build_model
    from sslrec_amd.models.kg.kgcl import ui_aug_weights
    stab = torch.tensor([-1.0, -0.2, 0.0, 0.3, 0.9, 1.0])
    assert torch.equal(ui_aug_weights(stab, 0.95), R.aug_weights(stab, 0.95))
    w = ui_aug_weights(stab, 0.95)
    assert float(w.max()) == pytest.approx(0.95) and float(w.min()) > 0.3
    dh = tiny_handler()
    torch.manual_seed(6)
    random.seed(6)
    model = build_model(dh)
    # norm_adj itself is `_get_norm_adj_mat(ui_mat)`, entry for entry and in its order
    want = R.norm_adj_mat(dh.ui_mat, 60, 50)
    idx = model.norm_adj._indices().numpy()
    assert np.array_equal(idx[0], want.row) and np.array_equal(idx[1], want.col)
    assert np.array_equal(model.norm_adj._values().numpy(), want.data.astype(np.float32))
    np.random.seed(8)
    views = model.get_aug_views()
    E, nnz, m = model.rel_graph.n_edges, 800, 400
    assert all(v.dtype == torch.uint8 and tuple(v.shape) == (E,) and int(v.sum()) == E // 2 for v in views[:2])
    assert not torch.equal(views[0], views[1])
    assert torch.allclose(model.last_aug_weights, R.aug_weights(_stability(model, views), 0.95), rtol=1e-5, atol=0)      # (fp32; another order of sums)
    for view, mask in zip(views[2:], model.last_aug_masks):
        assert view.is_sparse and view._nnz() == nnz and tuple(mask.shape) == (m,) and 0.5 * m < int(mask.sum()) < m
        want = R.masked_norm_adj(dh.ui_mat, mask.numpy(), 60, 50).tocsr()
        want = np.asarray(want[idx[0], idx[1]]).reshape(-1).astype(np.float32)
        got = view._values().numpy()
        assert got.dtype == np.float32 and np.all(np.abs(got - want) <= 2.0 ** -23 * np.abs(want))          # one float32 ulp
        entry = model._inter_entry.numpy()
        dropped = np.ones(m, dtype=bool)
        dropped[entry[mask.numpy()]] = False
        assert dropped.any() and np.all(got[:m][dropped] == 0) and np.all(got[:m][~dropped] > 0)                # dropped entries: exactly 0
        dense = view.to_dense().numpy()
        assert np.array_equal(dense, dense.T) and np.array_equal(got[m:], got[:m][model._mirror.numpy()])       # both halves
    # a repeated interaction is kept when any copy is
    from sslrec_amd.models.kg.kgcl import ui_view_values
    vals, kept = ui_view_values(torch.tensor([False, True, False]), torch.tensor([0, 0, 1]), torch.tensor([0, 1]), torch.tensor([0, 0]),
                                torch.tensor([0, 1]), 2, 1)
    assert kept.tolist() == [True, False] and vals.tolist() == [np.float32((1 + 1e-7) ** -1.0), 0.0] * 2


def _stability(model, views):
    """the cosine per item of the two kg views, from the restatement"""
    import torch.nn.functional as F
    edges = tuple(torch.from_numpy(model.kg_sample[:, c] - s) for c, s in ((0, 0), (1, 0), (2, 1)))
    p = {n: v.detach() for n, v in model.named_parameters()}
    out = [R.rgat_forward(p['all_embed'][60:], p['relation_embed'][1:], p['rgat.fc.weight'], p['rgat.fc.bias'], edges, v, 2)[:50] for v in views[:2]]
    return F.cosine_similarity(out[0], out[1], dim=-1)


# ---------------------------------------------------------------------------------------------------------------------
# the model's step
# ---------------------------------------------------------------------------------------------------------------------
def test_order_of_draws_in_a_step():
    from sslrec_amd.models.bulid_model import build_model
    dh = tiny_handler(model={'mess_dropout': False})
    torch.manual_seed(1)
    random.seed(1)
    model = build_model(dh)
    views = model.get_aug_views()
    E = model.rel_graph.n_edges
    np.random.seed(77)
    torch.manual_seed(78)
    model.cal_loss(list(tiny_batch(dh)) + list(views))
    np_after, torch_after = np.random.get_state(), torch.get_rng_state()
    np.random.seed(77)
    torch.manual_seed(78)
    flags = torch.floor(0.5 + torch.rand(800)).type(torch.bool)                          # `_sparse_dropout` first (:255)
    picked = np.random.choice(E, size=int(E * 0.5), replace=False)                        # then `_edge_sampling` (:256-257)
    keep = np.zeros(E, dtype=bool)
    keep[picked] = True
    assert np.array_equal(model.last_keep.numpy().astype(bool), keep) and torch.equal(model.last_ui_keep, flags)
    assert all(np.array_equal(a, b) for a, b in zip(np_after, np.random.get_state())) and torch.equal(torch_after, torch.get_rng_state())


@pytest.mark.parametrize('node_dropout', [True, False])
def test_cal_loss_on_the_cpu_in_float64(node_dropout):
    from sslrec_amd.models.bulid_model import build_model
    dh = tiny_handler(model={'node_dropout': node_dropout, 'mess_dropout': False, 'embedding_size': 16})
    torch.manual_seed(4)
    random.seed(4)
    model = build_model(dh).double()
    batch = tiny_batch(dh)
    np.random.seed(9)
    views = model.get_aug_views()
    loss, parts = model.cal_loss(list(batch) + list(views))
    loss.backward()
    assert sorted(parts) == ['cl_loss', 'rec_loss']
    named = dict(model.named_parameters())
    assert named['rgat.W'].grad is None and named['rgat.a'].grad is None
    if node_dropout:
        keep, ui_keep = model.last_keep.bool(), model.last_ui_keep
        assert int(keep.sum()) == model.rel_graph.n_edges // 2
    else:
        keep = ui_keep = None
        assert model.last_keep is None and model.last_ui_keep is None
    p = {n: R.leaf(v, torch.float64) for n, v in model.named_parameters()}
    edges = tuple(torch.from_numpy(model.kg_sample[:, c] - s) for c, s in ((0, 0), (1, 0), (2, 1)))
    graphs = [R.sparse_dropout_dense(model.norm_adj, ui_keep, 0.5, torch.float64)] + [v.to_dense().double() for v in views[2:]]
    out = R.model_loss(p, 60, 50, edges, (keep, views[0], views[1]), graphs, 2, 2, batch, model.decay)
    out['loss'].backward()
    for k in ('loss', 'rec_loss', 'cl_loss'):
        assert_close(k, (loss if k == 'loss' else parts[k]).detach().reshape(1), out[k].detach().reshape(1), 1e-11)
    for n in ('all_embed', 'relation_embed', 'rgat.fc.weight', 'rgat.fc.bias'):
        assert_close('grad ' + n, named[n].grad, p[n].grad, 1e-9)
    assert bool((named['relation_embed'].grad[0] == 0).all())                            # the interact relation's row is never indexed
    # generate() in eval mode: no dropout of any kind, the full graphs
    model.eval()
    with torch.no_grad():
        u, i = model.generate()
        wu, wi = R.kgcl_forward({n: v.detach() for n, v in named.items()}, 60, 50, edges, None,
                                R.sparse_dropout_dense(model.norm_adj, None, 0.5, torch.float64), 2, 2)
    assert_close('generate users', u, wu, 1e-11)
    assert_close('generate items', i, wi, 1e-11)
    kg_loss = model.cal_kg_loss((torch.tensor([0, 1]), torch.tensor([1, 2]), torch.tensor([2, 3]), torch.tensor([4, 5])))
    assert kg_loss.dim() == 0 and bool(torch.isfinite(kg_loss))


# ---------------------------------------------------------------------------------------------------------------------
# trainer and refusals
# ---------------------------------------------------------------------------------------------------------------------
class _Log:
    def log(self, *a, **k):
        pass

    log_loss = log_eval = log


def test_trainer_factory():
    from sslrec_amd.trainer.build_trainer import build_trainer
    from sslrec_amd.trainer.trainer import KGCLTrainer, Trainer
    dh = tiny_handler()
    trainer = build_trainer(dh, _Log())
    assert type(trainer) is KGCLTrainer and isinstance(trainer, Trainer)
    dh = tiny_handler(train={'trainer': 'kgcl_trainer'}, name='kgin')
    with pytest.raises(NotImplementedError, match='kgcl_trainer'):
        build_trainer(dh, _Log())


def test_refusals_by_name():
    from sslrec_amd.data_utils.data_handler_kg import DataHandlerKG
    from sslrec_amd.models.bulid_model import build_model
    dh = tiny_handler(train={'hip_graph': True})
    with pytest.raises(NotImplementedError, match='hip_graph'):
        build_model(dh)
    cfg({'data': {'synthetic': 'kg-tiny'}, 'model': {'train_trans': True}})
    with pytest.raises(NotImplementedError, match='train_trans'):
        DataHandlerKG()
