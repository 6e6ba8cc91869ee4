"""KGIN without a GPU: the yml, the kg data handler (synthetic and from text files), graph.RelGraph's three orders, the refusals, the
parameter draws, the step's order of random draws, and the composed torch forms of ops.rel_aggregate / ops.factor_modulate and the
model's cal_loss on the CPU in float64 against the restatement (tests/kgin_reference.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kgin_reference as R


def cfg(overrides=None, dataset=None):
    from sslrec_amd.config.configurator import load_config
    return load_config('kgin', dataset=dataset, device='cpu', overrides=overrides)


def tiny_handler(model=None, train=None):
    from sslrec_amd.data_utils.data_handler_kg import DataHandlerKG
    cfg({'data': {'synthetic': 'kg-tiny'}, 'model': dict({'embedding_size': 32}, **(model or {})), 'train': dict({'batch_size': 128}, **(train or {})),
         'test': {'batch_size': 32}})
    dh = DataHandlerKG()
    dh.load_data()
    return dh


def test_yml_holds_the_reference_values():
    c = cfg()
    assert c['optimizer'] == {'name': 'adam', 'lr': 1.0e-4, 'weight_decay': 0}
    assert c['train']['epoch'] == 500 and c['train']['batch_size'] == 1024 and c['train']['loss'] == 'pairwise' and c['train']['test_step'] == 10
    assert c['train']['seed'] == 2020 and c['train']['reproducible'] is True and c['train']['trainer'] == 'trainer'
    assert c['test'] == {'metrics': ['recall', 'ndcg'], 'k': [10, 20, 40], 'batch_size': 1024, 'eval_at_one_forward': True}
    assert c['data'] == {'type': 'kg', 'name': 'last-fm'}
    assert c['model'] == {'name': 'kgin', 'layer_num': 2, 'decay_weight': 1.0e-5, 'embedding_size': 64, 'node_dropout': True,
                          'node_dropout_rate': 0.5, 'mess_dropout': True, 'mess_dropout_rate': 0.1, 'n_factors': 4, 'ind': 'distance',
                          'sim_regularity': 1.0e-4}


def test_kg_shapes():
    from sslrec_amd.data_utils import synth
    assert synth.KG_SHAPES['kg-tiny'] == (60, 50, 90, 4, 400, 300)
    assert synth.KG_SHAPES['kg-last-fm'] == (23566, 48123, 106389, 9, 3034796, 464567)
    assert synth.KG_SHAPES['kg-alibaba'] == (114737, 30040, 89196, 51, 1781093, 279155)


def test_handler_on_kg_tiny():
    from sslrec_amd.config.configurator import configs
    from sslrec_amd.graph import RelGraph
    dh = tiny_handler()
    d = configs['data']
    assert (d['user_num'], d['item_num'], d['entity_num'], d['node_num'], d['relation_num'], d['triplet_num']) == (60, 50, 90, 150, 9, 600)
    kg = np.asarray(dh.kg_edges)
    assert kg.shape == (600, 3) and len(dh.ui_edges) == 400 and dh.ui_mat.shape == (60, 50) and dh.ui_mat.nnz == 400
    h, t, r = kg[:, 0], kg[:, 1], kg[:, 2]
    assert r.min() == 1 and r.max() == 8
    # the canonical half and its inverse
    assert np.array_equal(h[:300], t[300:]) and np.array_equal(t[:300], h[300:]) and np.array_equal(r[:300] + 4, r[300:])
    assert len({tuple(x) for x in kg.tolist()}) == 600
    # an entity with no edge, a (head, tail) pair under two relations, a relation that occurs once
    touched = np.zeros(90, dtype=bool)
    touched[h] = touched[t] = True
    assert (~touched).sum() >= 1 and not touched[50 + 20]
    pairs = {}
    for hh, tt, rr in kg.tolist():
        pairs.setdefault((hh, tt), set()).add(rr)
    assert any(len(v) >= 2 for v in pairs.values())
    counts = np.bincount(r, minlength=9)
    assert counts[0] == 0 and (counts[1:] >= 1).all() and (counts == 1).sum() == 2          # the rare relation and its inverse
    assert dict(dh.kg_dict)[int(h[0])][0] == (int(r[0]), int(t[0]))
    assert sum(len(v) for v in dh.train_user_dict.values()) == 400 and len(dh.test_user_dict) >= 1
    # the model's two graphs, built once
    g = dh.rel_graph
    assert isinstance(g, RelGraph) and (g.n, g.n_rel, g.n_edges) == (90, 8, 600) and g.by_head is None      # (no HIP device: no device lists)
    assert np.array_equal(g.rel.numpy(), r - 1) and np.array_equal(g.head.numpy(), h) and np.array_equal(g.tail.numpy(), t)
    im = dh.interact_mat
    assert tuple(im.shape) == (60, 90) and im._nnz() == 400
    dense = im.to_dense().double().numpy()
    ui = dh.ui_mat.toarray()
    deg = ui.sum(1, keepdims=True)
    want = np.zeros((60, 90))
    want[:, :50] = ui / np.where(deg == 0, 1, deg)
    assert np.allclose(dense, want, rtol=1e-7, atol=0)
    # the loaders: train pairs in file order, all-rank evaluation
    ds = dh.train_dataloader.dataset
    assert np.array_equal(ds.rows, np.asarray(dh.ui_edges)[:, 0]) and np.array_equal(ds.cols, np.asarray(dh.ui_edges)[:, 1])
    assert type(dh.test_dataloader.dataset).__name__ == 'AllRankTstData'


def write_kg_files(root):
    d = root / 'datasets' / 'kg' / 'last-fm_kg'
    d.mkdir(parents=True)
    (d / 'train.txt').write_text('0 1 2 2 5\n1 0\n2 3 4 1\n3 5\n')                      # a repeated item in a line
    (d / 'test.txt').write_text('0 3\n2 0 5\n4 2\n')                                    # user 4 occurs in the test file only
    # (h, r, t) lines with a repeated triplet, a pair under two relations, entity 7 untouched, relation 2 once
    (d / 'kg_final.txt').write_text('0 0 6\n1 0 6\n0 0 6\n0 1 6\n2 1 8\n5 2 9\n3 0 8\n6 1 9\n')
    return d


def test_handler_on_text_files_against_a_dense_construction(tmp_path, monkeypatch):
    from sslrec_amd.config.configurator import configs
    from sslrec_amd.data_utils.build_data_handler import build_data_handler
    write_kg_files(tmp_path)
    monkeypatch.chdir(tmp_path)
    cfg({'train': {'batch_size': 4}, 'test': {'batch_size': 4}}, dataset='last-fm')
    dh = build_data_handler()
    assert type(dh).__name__ == 'DataHandlerKG'
    dh.load_data()
    d = configs['data']
    # dense construction: T[h, r, t] over the canonical relations, then the inverse block and the shift by one
    canonical = {(0, 0, 6), (1, 0, 6), (0, 1, 6), (2, 1, 8), (5, 2, 9), (3, 0, 8), (6, 1, 9)}
    T = np.zeros((10, 7, 10), dtype=bool)
    for h, r, t in canonical:
        T[h, r + 1, t] = True
        T[t, r + 3 + 1, h] = True
    assert (d['user_num'], d['item_num'], d['entity_num'], d['node_num'], d['relation_num'], d['triplet_num']) == (5, 6, 10, 15, 7, 14)
    assert d['dir'] == './datasets/kg/last-fm_kg/'
    kg = np.asarray(dh.kg_edges)
    got = np.zeros_like(T)
    got[kg[:, 0], kg[:, 2], kg[:, 1]] = True
    assert kg.shape == (14, 3) and np.array_equal(got, T) and int(T.sum()) == 14
    # canonical triplets first, in np.unique's row order, then their inverses in the same order
    assert kg[:7, [0, 2, 1]].tolist() == [[h, r + 1, t] for h, r, t in sorted(canonical)]
    assert np.array_equal(kg[7:, 0], kg[:7, 1]) and np.array_equal(kg[7:, 1], kg[:7, 0]) and np.array_equal(kg[7:, 2], kg[:7, 2] + 3)
    assert {k: sorted(v) for k, v in dh.kg_dict.items()} == {h: sorted((int(r), int(t)) for hh, t, r in kg.tolist() if hh == h) for h in set(kg[:, 0].tolist())}
    # interactions: the repeated item counts once, pairs in line order
    ui = np.asarray(dh.ui_edges)
    assert ui[:, 0].tolist() == [0, 0, 0, 1, 2, 2, 2, 3] and sorted(ui[:3, 1].tolist()) == [1, 2, 5] and sorted(ui[4:7, 1].tolist()) == [1, 3, 4]
    assert dict(dh.train_user_dict)[1] == [0] and sorted(dh.test_user_dict[2]) == [0, 5] and dh.test_user_dict[4] == [2]
    assert dh.ui_mat.shape == (5, 6) and dh.ui_mat.nnz == 8
    # RelGraph's three orders against a stable sort
    g = dh.rel_graph
    assert (g.n, g.n_rel, g.n_edges) == (10, 6, 14)
    head, tail, rel = kg[:, 0], kg[:, 1], kg[:, 2] - 1
    for lst, dest, ia, ib, n_dest in zip(g.host_lists(), (head, tail, rel), (tail, head, head), (rel, rel, tail), (10, 10, 6)):
        order = np.argsort(dest, kind='stable')
        assert np.array_equal(lst.eid.numpy(), order) and np.array_equal(lst.ia.numpy(), ia[order]) and np.array_equal(lst.ib.numpy(), ib[order])
        assert np.array_equal(lst.ptr.numpy(), np.concatenate([[0], np.cumsum(np.bincount(dest, minlength=n_dest))]))
        assert lst.n_chunks == 0 and lst.n_long == 0


def test_rel_graph_chunks_of_long_destinations():
    from sslrec_amd.graph import REL_CHUNK, RelGraph
    rng = np.random.RandomState(0)
    n_long_a, n_long_b = 2 * REL_CHUNK + 7, REL_CHUNK + 1
    head = np.concatenate([np.full(n_long_a, 3), np.full(n_long_b, 9), np.full(REL_CHUNK, 5), rng.randint(6, 12, 100)])          # 5: exactly REL_CHUNK, not long
    perm = rng.permutation(head.size)
    head = head[perm]
    tail, rel = rng.randint(0, 12, head.size), rng.randint(0, 2, head.size)
    by_head = RelGraph(head, tail, rel, 12, 2).host_lists()[0]
    deg = np.bincount(head, minlength=12)
    longs = np.nonzero(deg > REL_CHUNK)[0]
    assert by_head.long_dest.tolist() == longs.tolist() == [3, 9] and deg[5] == REL_CHUNK
    ptr = by_head.ptr.numpy()
    want_dest, want_begin = [], []
    for x in longs:
        for b in range(ptr[x], ptr[x + 1], REL_CHUNK):
            want_dest.append(x)
            want_begin.append(b)
    assert by_head.chunk_dest.tolist() == want_dest and by_head.chunk_begin.tolist() == want_begin
    assert by_head.long_ptr.tolist() == np.concatenate([[0], np.cumsum([-(-deg[x] // REL_CHUNK) for x in longs])]).tolist()
    with pytest.raises(ValueError, match='relation id'):
        RelGraph([0], [0], [2], 3, 2)
    with pytest.raises(ValueError, match='entity id'):
        RelGraph([0], [3], [0], 3, 2)


def test_refusals_by_name():
    from sslrec_amd.data_utils.data_handler_kg import DataHandlerKG
    from sslrec_amd.models.bulid_model import build_model
    cfg({'data': {'synthetic': 'kg-tiny'}, 'model': {'diff_model': 1}})
    with pytest.raises(NotImplementedError, match='diff_model'):
        DataHandlerKG()
    cfg({'data': {'synthetic': 'kg-tiny'}, 'model': {'train_trans': True}})
    with pytest.raises(NotImplementedError, match='train_trans'):
        DataHandlerKG()
    cfg({'data': {'synthetic': 'kg-huge'}})
    with pytest.raises(ValueError, match='kg-huge'):
        DataHandlerKG()
    cfg(dataset='yelp')
    with pytest.raises(ValueError, match='yelp'):
        DataHandlerKG()
    dh = tiny_handler(train={'hip_graph': True})
    with pytest.raises(NotImplementedError, match='hip_graph'):
        build_model(dh)


@pytest.mark.parametrize('seed', [3, 2020])
def test_parameter_names_shapes_and_draws(seed):
    from sslrec_amd.models.bulid_model import build_model
    dh = tiny_handler()
    torch.manual_seed(seed)
    model = build_model(dh)
    assert type(model).__name__ == 'KGIN'
    got = dict(model.named_parameters())
    want = R.draw_params(150, 32, 4, 9, seed)
    assert list(got) == R.PARAM_NAMES
    for n in R.PARAM_NAMES:
        assert got[n].shape == want[n].shape and torch.equal(got[n].detach(), want[n]), n
    assert tuple(got['gcn.weight'].shape) == (8, 32) and tuple(got['gcn.disen_weight_att'].shape) == (4, 8)
    assert sorted(model.state_dict()) == sorted(R.PARAM_NAMES)
    model.load_state_dict({k: v + 0.5 for k, v in want.items()})


def tiny_batch(dh, B=100, seed=1):
    rng = np.random.RandomState(seed)
    ui = np.asarray(dh.ui_edges)
    pick = rng.randint(0, len(ui), B)
    return (torch.from_numpy(ui[pick, 0]).long(), torch.from_numpy(ui[pick, 1]).long(), torch.from_numpy(rng.randint(0, 50, B)).long())


def test_order_of_draws_in_a_step():
    from sslrec_amd.models.bulid_model import build_model
    dh = tiny_handler()
    torch.manual_seed(1)
    model = build_model(dh)
    batch = tiny_batch(dh)
    np.random.seed(77)
    torch.manual_seed(78)
    model.cal_loss(batch)
    np_after, torch_after = np.random.get_state(), torch.get_rng_state()
    # the restatement's draws: the edge sample, the sparse-dropout flags, then per hop the two message dropouts
    np.random.seed(77)
    torch.manual_seed(78)
    keep = R.edge_sample_mask(600, 0.5)
    flags = R.sparse_dropout_flags(400, 0.5)
    for _ in range(2):
        F.dropout(torch.ones(90, 32), p=0.1)
        F.dropout(torch.ones(60, 32), p=0.1)
    assert int(keep.sum()) == 300 and np.array_equal(model.last_keep.numpy().astype(bool), keep)
    assert torch.equal(model.last_ui_keep, flags)
    assert all(np.array_equal(a, b) for a, b in zip(np_after, np.random.get_state())) and torch.equal(torch_after, torch.get_rng_state())


# ---------------------------------------------------------------------------------------------------------------------
# the composed forms against the restatement, float64
# ---------------------------------------------------------------------------------------------------------------------
def assert_close(name, got, want, rel=1e-12):
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= rel * max(scale, 1e-300), name


@pytest.mark.parametrize('masked', [False, True])
def test_composed_rel_aggregate_in_float64(masked):
    from sslrec_amd import ops
    from sslrec_amd.graph import RelGraph
    N, E, Rn, d = 40, 300, 5, 24
    rng = np.random.RandomState(5)
    head, tail, rel = rng.randint(0, N - 1, E), rng.randint(0, N - 1, E), rng.randint(0, Rn, E)          # entity N - 1 has no edge
    head[:2], tail[:2], rel[:2] = 7, 9, [0, 1]                                                            # a pair under two relations
    keep = torch.from_numpy(rng.rand(E) < 0.5) if masked else None
    if masked:
        keep[torch.from_numpy(head == 7)] = False                                                         # a head with every edge masked
    g = RelGraph(head, tail, rel, N, Rn)
    x, w, go = R.randn((N, d), 1), R.randn((Rn, d), 2), R.randn((N, d), 3)
    xa, wa = R.leaf(x, torch.float64), R.leaf(w, torch.float64)
    ya = ops.rel_aggregate(g, xa, wa, keep)
    (ya * go).sum().backward()
    xb, wb = R.leaf(x, torch.float64), R.leaf(w, torch.float64)
    yb = R.kg_aggregate(xb, wb, torch.from_numpy(head), torch.from_numpy(tail), torch.from_numpy(rel), keep)
    (yb * go).sum().backward()
    assert_close('y', ya.detach(), yb.detach())
    assert_close('dx', xa.grad, xb.grad)
    assert_close('dw', wa.grad, wb.grad)
    assert bool((ya[N - 1] == 0).all()) and (not masked or bool((ya[7] == 0).all()))
    # the backward of the issue's formulas, written out
    cnt = np.zeros(N)
    kept = np.ones(E, dtype=bool) if keep is None else keep.numpy()
    np.add.at(cnt, head[kept], 1)
    inv = 1.0 / np.maximum(cnt, 1)
    dx, dw = np.zeros((N, d)), np.zeros((Rn, d))
    for e in np.nonzero(kept)[0]:
        dx[tail[e]] += go[head[e]].numpy() * w[rel[e]].numpy() * inv[head[e]]
        dw[rel[e]] += go[head[e]].numpy() * x[tail[e]].numpy() * inv[head[e]]
    assert_close('dx formula', xa.grad, torch.from_numpy(dx), 1e-11)
    assert_close('dw formula', wa.grad, torch.from_numpy(dw), 1e-11)
    with pytest.raises(ValueError):
        ops.rel_aggregate(g, xa, wa, torch.ones(E - 1, dtype=torch.bool))


@pytest.mark.parametrize('U,d,Fn', [(1, 8, 4), (37, 24, 4), (50, 32, 8), (20, 16, 11)])
def test_composed_factor_modulate_in_float64(U, d, Fn):
    from sslrec_amd import ops
    tens = [R.randn((U, d), 1), R.randn((U, d), 2), R.randn((Fn, d), 3), R.randn((Fn, d), 4)]
    go = R.randn((U, d), 5)
    a = [R.leaf(x, torch.float64) for x in tens]
    b = [R.leaf(x, torch.float64) for x in tens]
    ya, yb = ops.factor_modulate(*a), R.factor_modulate(*b)
    (ya * go).sum().backward()
    (yb * go).sum().backward()
    assert_close('out', ya.detach(), yb.detach())
    for name, p, q in zip(('d_agg', 'd_u', 'd_latent', 'd_D'), a, b):
        assert_close(name, p.grad, q.grad)
    assert not ops.kgin_fused_ok(48) and all(ops.kgin_fused_ok(x) for x in (32, 64, 128))


@pytest.mark.parametrize('ind', ['distance', 'cosine', 'mi'])
def test_cal_loss_on_the_cpu_in_float64(ind):
    from sslrec_amd.models.bulid_model import build_model
    dh = tiny_handler(model={'node_dropout': False, 'mess_dropout': False, 'ind': ind, 'embedding_size': 16})
    torch.manual_seed(4)
    model = build_model(dh).double()
    batch = tiny_batch(dh)
    loss, parts = model.cal_loss(batch)
    loss.backward()
    assert sorted(parts) == ['cor', 'loss', 'rec_loss', 'reg_loss'] and model.last_keep is None and model.last_ui_keep is None
    p = {n: R.leaf(v, torch.float64) for n, v in model.named_parameters()}
    kg = np.asarray(dh.kg_edges)
    edges = tuple(torch.from_numpy(kg[:, c] - s) for c, s in ((0, 0), (1, 0), (2, 1)))
    interact = R.sparse_dropout_dense(dh.interact_mat, None, 0.5, torch.float64)
    out = R.model_loss(p, 60, edges, None, interact, 2, ind, batch, model.decay, model.sim_decay)
    out['loss'].backward()
    for k in ('loss', 'rec_loss', 'reg_loss', 'cor'):
        assert_close(k, (loss if k == 'loss' else parts[k]).detach().reshape(1), out[k].detach().reshape(1), 1e-11)
    assert_close('user', model.final_user_embeds.detach(), out['user'].detach(), 1e-11)
    assert_close('entity', model.final_entity_embeds.detach(), out['entity'].detach(), 1e-11)
    for n, v in model.named_parameters():
        assert_close('grad ' + n, v.grad, p[n].grad, 1e-9)
