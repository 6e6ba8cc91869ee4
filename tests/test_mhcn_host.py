"""MHCN without a GPU: the configuration, the social data handler (motif counts exactly against dense numpy, the four matrices'
patterns and values, the pickle path with ratings, the synthetic trust graph), the refusals by name, the parameters' names / shapes /
draw order, the order of the 15 permutations, and the composed (torch) forms of the three ops in float64 against the literal
restatement of the reference (tests/mhcn_reference.py), values and every gradient to 1e-12 relative."""
import os
import pickle

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import mhcn_reference as R

TINY_U, TINY_I = 150, 120


def config(device='cpu', over=None, synthetic='social-tiny'):
    from sslrec_amd.config.configurator import load_config
    overrides = {'data': {'synthetic': synthetic} if synthetic else {}}
    for k, v in (over or {}).items():
        overrides.setdefault(k, {}).update(v)
    return load_config('mhcn', device=device, overrides=overrides)


def handler(device='cpu', over=None):
    from sslrec_amd.data_utils.build_data_handler import build_data_handler
    config(device, over)
    dh = build_data_handler()
    dh.load_data()
    return dh


def test_mhcn_config_holds_the_reference_values():
    from sslrec_amd.config.configurator import load_config
    cfg = load_config('mhcn', device='cpu')
    o, tr, te, da, m, tu = (cfg[k] for k in ('optimizer', 'train', 'test', 'data', 'model', 'tune'))
    assert (o['name'], o['lr'], o['weight_decay']) == ('adam', 1.0e-3, 0)
    assert (tr['epoch'], tr['batch_size'], tr['save_model'], tr['loss'], tr['test_step']) == (30, 2000, True, 'pairwise', 1)
    assert (tr['reproducible'], tr['seed'], tr['tensorboard'], tr['log_loss'], tr['early_stop']) == (True, 2023, True, True, False)
    assert 'patience' not in tr and 'pretrain_path' not in tr
    assert (te['metrics'], te['k'], te['batch_size']) == (['recall', 'ndcg'], [10, 20, 40], 512)
    assert da == {'type': 'social', 'name': 'yelp'}
    assert m == {'name': 'mhcn', 'layer_num': 2, 'reg_weight': 1.0e-3, 'embedding_size': 64, 'ss_rate': 1.0e-2}
    assert tu == {'enable': False, 'hyperparameters': ['layer_num', 'reg_weight'], 'layer_num': [1, 2, 3], 'reg_weight': [1.0e-1, 1.0e-2, 1.0e-3]}


def dense_of(adj):
    return adj.coalesce().to_dense().double().numpy() if adj.is_sparse else np.asarray(adj)


def compare_handler_with_dense(dh):
    from sslrec_amd.data_utils.data_handler_social import motif_matrices
    S = np.asarray(sp.coo_matrix(dh.trust_mat).todense(), dtype=np.float64)
    Y = np.asarray(sp.coo_matrix(dh.trn_mat).todense(), dtype=np.float64)
    want_A = R.dense_motifs(S, Y)
    got_A = motif_matrices(dh.trust_mat, dh.trn_mat)
    for k, (g, w) in enumerate(zip(got_A, want_A)):
        assert np.array_equal(np.asarray(g.todense()), w), 'A%d' % (k + 1)          # integer counts: exact
        assert g.nnz == int((w != 0).sum()), 'A%d holds explicit zeros' % (k + 1)
    want = R.dense_adjacencies(S, Y)
    for name, w in zip(('H_s', 'H_j', 'H_p', 'R'), want):
        adj = getattr(dh, name)
        assert adj.dtype == torch.float32 and tuple(adj.shape) == w.shape, name
        vals = adj._values().numpy()
        assert np.isfinite(vals).all(), name
        idx = adj._indices().numpy()
        got = np.zeros(w.shape)
        got[idx[0], idx[1]] = vals                                                   # (no entry is stored twice: asserted next)
        assert np.unique(idx[0].astype(np.int64) * w.shape[1] + idx[1]).size == vals.size, name
        assert np.array_equal(got != 0, w != 0), name + ' pattern'
        w32 = w.astype(np.float32)
        ulp = np.spacing(np.abs(w32))
        assert np.all(np.abs(got.astype(np.float32) - w32) <= ulp), name + ' values'
    return got_A, want


@pytest.mark.parametrize('seed', [2023, 7])
def test_social_handler_matrices_equal_the_dense_restatement(seed):
    dh = handler(over={'data': {'synthetic_seed': seed}})
    from sslrec_amd.config.configurator import configs
    assert (configs['data']['user_num'], configs['data']['item_num']) == (TINY_U, TINY_I)
    assert not hasattr(dh, 'valid_dataloader') and hasattr(dh, 'test_dataloader') and hasattr(dh, 'train_dataloader')
    got_A, (H_s, H_j, H_p, Rm) = compare_handler_with_dense(dh)
    if seed == 2023:          # the shipped tiny graph: every motif occurs, and H_s / H_j have rows without entries
        assert all(a.nnz > 0 for a in got_A), [a.nnz for a in got_A]
        assert ((H_s != 0).sum(1) == 0).any() and ((H_j != 0).sum(1) == 0).any()
        assert (H_p != 0).sum() > 0
    for H in (H_s, H_j, H_p):
        sums = H.sum(1)
        assert np.allclose(sums[sums != 0], 1.0, atol=1e-12)


def test_synthetic_trust_graph_is_seeded_directed_and_has_isolated_users():
    from sslrec_amd.data_utils import synth
    a, b = synth.trust_graph(150, 700, 0.3, 5, seed=9), synth.trust_graph(150, 700, 0.3, 5, seed=9)
    assert np.array_equal(a.row, b.row) and np.array_equal(a.col, b.col)
    S = np.asarray(a.todense())
    assert S.shape == (150, 150) and set(np.unique(S)) == {0.0, 1.0} and a.nnz == int(S.sum())      # no duplicate entry
    assert np.trace(S) == 0
    assert abs(a.nnz - 700) <= 2
    recip = (S * S.T).sum() / S.sum()
    assert 0.25 < recip < 0.35
    assert int(((S.sum(0) + S.sum(1)) == 0).sum()) >= 5
    assert not np.array_equal(synth.trust_graph(150, 700, 0.3, 5, seed=10).row, a.row)
    assert set(synth.SOCIAL_SHAPES) >= {'social-tiny', 'social-yelp', 'social-epinions'}
    assert synth.SOCIAL_SHAPES['social-yelp'][:2] == (43043, 66576) and synth.SOCIAL_SHAPES['social-epinions'][:2] == (18081, 251722)


def test_pickle_path_gives_the_same_matrices_and_uses_the_ratings(tmp_path, monkeypatch):
    from sslrec_amd.data_utils import synth
    from sslrec_amd.data_utils.build_data_handler import build_data_handler
    trn, trust = synth.make_social_dataset('social-tiny', 11)
    rng = np.random.default_rng(5)
    rated = sp.coo_matrix((rng.integers(1, 6, trn.nnz).astype(np.float64), (trn.row, trn.col)), shape=trn.shape)
    tst = synth.split_holdout(trn, 0.05, 13)
    d = tmp_path / 'datasets' / 'social' / 'ciao'
    os.makedirs(d)
    for name, mat in (('trn_mat', rated), ('tst_mat', tst.tocsr()), ('trust_mat', trust.tocsr())):      # coo and csr pickles both load
        with open(d / (name + '.pkl'), 'wb') as f:
            pickle.dump(mat, f)
    monkeypatch.chdir(tmp_path)
    from sslrec_amd.config.configurator import load_config
    load_config('mhcn', dataset='ciao', device='cpu')
    dh = build_data_handler()
    dh.load_data()
    assert dh.trn_file == './datasets/social/ciao/trn_mat.pkl'
    compare_handler_with_dense(dh)
    Y = np.asarray(rated.todense())
    Rm = dense_of(dh.R)
    r, c = int(rated.row[0]), int(rated.col[0])
    assert Y.max() == 5 and abs(Rm[r, c] - Y[r, c] / np.sqrt(Y[r].sum()) / np.sqrt(Y[:, c].sum())) < 1e-6
    # the in-memory path on the same matrices
    from sslrec_amd.data_utils import data_handler_social as S
    H = S.motif_adjacencies(trust, rated)
    for name, h in zip(('H_s', 'H_j', 'H_p'), H):
        assert np.array_equal(dense_of(getattr(dh, name)), np.asarray(h.todense()).astype(np.float32).astype(np.float64)), name
    binary = S.motif_adjacencies(trust, trn)
    assert not np.array_equal(np.asarray(binary[1].todense()), np.asarray(H[1].todense()))      # the ratings are used as values
    batch = next(iter(dh.test_dataloader))
    assert len(batch) == 2 and batch[1].shape[1] == TINY_I


@pytest.mark.parametrize('name', ['dsl', 'dcrec', 'kcgn', 'smin'])
def test_other_social_models_are_refused_by_name(name):
    from sslrec_amd.config.configurator import configs
    from sslrec_amd.data_utils.build_data_handler import build_data_handler
    config()
    configs['model']['name'] = name
    with pytest.raises(NotImplementedError, match=name):
        build_data_handler()


def test_hip_graph_is_refused_by_name():
    from sslrec_amd.models.bulid_model import build_model
    dh = handler(over={'train': {'hip_graph': True}})
    with pytest.raises(NotImplementedError, match='train.hip_graph'):
        build_model(dh)


def test_parameters_have_the_reference_names_shapes_and_draws():
    from sslrec_amd.models.bulid_model import build_model
    dh = handler(over={'model': {'embedding_size': 32}})
    for seed in (5, 2023):
        torch.manual_seed(seed)
        model = build_model(dh)
        after = torch.get_rng_state()
        assert type(model).__name__ == 'MHCN'
        want = R.draw_params(TINY_U, TINY_I, 32, seed)
        assert torch.equal(torch.get_rng_state(), after)
        assert sorted(n for n, _ in model.named_parameters()) == sorted(R.PARAM_NAMES)
        for n, p in model.named_parameters():
            assert p.shape == want[n].shape and torch.equal(p.detach(), want[n]), n
        assert sorted(model.state_dict()) == sorted(R.PARAM_NAMES)
        model.load_state_dict({k: v + 1 for k, v in want.items()})
        assert torch.equal(model.attn.detach(), want['attn'] + 1)
    assert (model.layer_num, model.reg_weight, model.ss_rate) == (2, 1.0e-3, 1.0e-2)


def test_the_fifteen_permutations_are_the_reference_draws():
    from sslrec_amd.models.bulid_model import build_model
    dh = handler(over={'model': {'embedding_size': 32}})
    model = build_model(dh)
    torch.manual_seed(41)
    perms = model._draw_perms('cpu')
    after = torch.get_rng_state()
    torch.manual_seed(41)
    for k in range(3):          # per channel: row_shuffle (:135), row_col_shuffle (:136), row_col_shuffle (:141)
        want = [torch.randperm(TINY_U), torch.randperm(32), torch.randperm(TINY_U), torch.randperm(32), torch.randperm(TINY_U)]
        assert len(perms[k]) == 5
        for got, w in zip(perms[k], want):
            assert torch.equal(got, w)
    assert torch.equal(torch.get_rng_state(), after)


# ---- the composed forms against the literal restatement, float64 on the CPU ---------------------------------------------------------
def close(got, want, what):
    scale = float(want.detach().abs().max().clamp_min(1e-300))
    assert float((got.detach() - want.detach()).abs().max()) <= 1e-12 * scale, what


def grads(fn, leaves):
    for x in leaves:
        x.grad = None
    fn().backward()
    return [x.grad.clone() for x in leaves]


def test_composed_self_gate_in_float64():
    from sslrec_amd import ops
    N, d, C = 37, 48, 4
    x = R.leaf(R.randn((N, d), 1), torch.float64)
    ws = [R.leaf(R.randn((d, d), 10 + c, 0.3), torch.float64) for c in range(C)]
    bs = [R.leaf(R.randn((d,), 20 + c), torch.float64) for c in range(C)]
    gs = [R.randn((N, d), 30 + c) for c in range(C)]
    leaves = [x] + ws + bs
    got = ops.self_gate(x, ws, bs)
    want = [R.self_gating(x, w, b) for w, b in zip(ws, bs)]
    assert len(got) == C
    for c in range(C):
        close(got[c], want[c], 'self_gate %d' % c)
    g_got = grads(lambda: sum((y * g).sum() for y, g in zip(ops.self_gate(x, ws, bs), gs)), leaves)
    g_want = grads(lambda: sum((R.self_gating(x, w, b) * g).sum() for w, b, g in zip(ws, bs, gs)), leaves)
    for a, b in zip(g_got, g_want):
        close(a, b, 'self_gate gradient')
    with pytest.raises(ValueError):
        ops.self_gate(x, ws + ws[:1], bs + bs[:1])


@pytest.mark.parametrize('with_sums', [False, True])
def test_composed_channel_mix_and_normalize_add_in_float64(with_sums):
    from sslrec_amd import ops
    N, d = 41, 24
    tabs = [R.leaf(R.randn((N, d), 40 + k), torch.float64) for k in range(4)]
    with torch.no_grad():
        tabs[1][5] = 0                                       # a zero row in a channel and in simp
        tabs[3][7] = 0
    sums = [R.leaf(R.randn((N, d), 50 + k), torch.float64) for k in range(4)]
    attn, attn_mat = R.leaf(R.randn((1, d), 60, 0.4), torch.float64), R.leaf(R.randn((d, d), 61, 0.4), torch.float64)
    g = [R.randn((N, d), 70 + k) for k in range(5)]
    leaves = tabs + sums + [attn, attn_mat] if with_sums else tabs + [attn, attn_mat]

    def ours():
        v = (attn_mat @ attn.t()).reshape(-1)
        if with_sums:
            mixed, outs, scores = ops.channel_mix(*tabs, v, sums=sums, return_scores=True)
            return mixed, scores, outs
        mixed, scores = ops.channel_mix(*tabs, v, return_scores=True)
        return mixed, scores, ()

    def theirs():
        mixed, scores = R.channel_attention(attn, attn_mat, *tabs[:3])
        mixed = mixed + tabs[3] / 2
        outs = tuple(a + torch.nn.functional.normalize(e, p=2, dim=1) for a, e in zip(sums, tabs)) if with_sums else ()
        return mixed, scores, outs

    (m1, s1, o1), (m2, s2, o2) = ours(), theirs()
    close(m1, m2, 'mixed')
    close(s1, s2, 'scores')
    assert tuple(s1.shape) == (N, 3)
    for a, b in zip(o1, o2):
        close(a, b, 'sums')
    if with_sums:
        assert bool((o1[1][5] == sums[1][5]).all()) and bool((o1[3][7] == sums[3][7]).all())      # zero rows add zeros

    def total(res):
        mixed, scores, outs = res
        return (mixed * g[0]).sum() + sum((o * gk).sum() for o, gk in zip(outs, g[1:]))
    for a, b in zip(grads(lambda: total(ours()), leaves), grads(lambda: total(theirs()), leaves)):
        close(a, b, 'channel_mix gradient')
    if with_sums:
        grads(lambda: total(ours()), leaves)
        assert torch.equal(tabs[3].grad[7], g[0][7] / 2 + g[4][7] / 1e-12)                         # the clamp's gradient: g / eps
        y = R.leaf(tabs[0], torch.float64)
        acc = R.leaf(sums[0], torch.float64)
        close(ops.normalize_add(acc, y), acc + torch.nn.functional.normalize(y, p=2, dim=1), 'normalize_add')
        ga = grads(lambda: (ops.normalize_add(acc, y) * g[1]).sum(), [acc, y])
        gb = grads(lambda: ((acc + torch.nn.functional.normalize(y, p=2, dim=1)) * g[1]).sum(), [acc, y])
        close(ga[0], gb[0], 'normalize_add d acc')
        close(ga[1], gb[1], 'normalize_add d y')


@pytest.mark.parametrize('N,d', [(1, 8), (2, 8), (53, 24)])
def test_composed_hier_ssl_loss_in_float64(N, d):
    from sslrec_amd import ops
    gen = torch.Generator().manual_seed(N)
    perms = [torch.randperm(n, generator=gen) for n in (N, d, N, d, N)]
    em, edge = R.leaf(R.randn((N, d), 80, 0.5), torch.float64), R.leaf(R.randn((N, d), 81, 0.5), torch.float64)
    got, want = ops.hier_ssl_loss(em, edge, perms), R.hierarchical_self_supervision(em, edge, perms)
    close(got, want, 'hier_ssl_loss')
    for a, b in zip(grads(lambda: ops.hier_ssl_loss(em, edge, perms), [em, edge]),
                    grads(lambda: R.hierarchical_self_supervision(em, edge, perms), [em, edge])):
        close(a, b, 'hier_ssl_loss gradient')
    # far negative arguments: the reference's form is -inf, the stable form is finite and equals -x there
    big = ops.hier_ssl_loss((em * 40).detach(), (edge * 40).detach().abs() * -1 if N == 1 else (edge * 40).detach(), perms)
    assert torch.isfinite(big)
    x = torch.tensor([-800.0, -200.0, -30.0, 0.0, 30.0], dtype=torch.float64)
    assert torch.isinf(R.log_sigmoid_reference(x)[0]) and torch.isfinite(ops.log_sigmoid_stable(x)).all()
    close(ops.log_sigmoid_stable(x)[1:], R.log_sigmoid_reference(x)[1:], 'log sigmoid where the reference is finite')
    with pytest.raises(ValueError):
        ops.hier_ssl_loss(em, edge, perms[:4])


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from sslrec_amd import _lib, ops
    lib = _lib.load()
    E = _lib.E_BADARG
    assert lib.sslrec_mhcn_gate_fwd_f32(None, 8, 64, None, None, 4, None, None, None, None, None) == E
    assert lib.sslrec_mhcn_gate_bwd_f32(None, 8, 64, None, None, 4, None, None, None, None, None, None, None, None, None) == E
    assert lib.sslrec_mhcn_mix_fwd_f32(None, None, None, None, None, 8, 64, None, None, None, None, None, None, None, None, None, None, None) == E
    assert lib.sslrec_mhcn_mix_bwd_f32(*([None] * 6), 8, 64, *([None] * 12)) == E
    assert lib.sslrec_mhcn_normadd_fwd_f32(None, None, 8, 64, None, None) == E and lib.sslrec_mhcn_normadd_bwd_f32(None, None, 8, 64, None, None) == E
    assert lib.sslrec_mhcn_ssl_fwd_f32(*([None] * 7), 8, 64, *([None] * 5)) == E
    assert lib.sslrec_mhcn_ssl_bwd_f32(*([None] * 15), 8, 64, *([None] * 4)) == E
    for d in (32, 64, 128):
        assert lib.sslrec_mhcn_ws_bytes(1000, d) > 0 and lib.sslrec_mhcn_gate_ws_bytes(1000, d, 4) >= 4 * d * (d + 1) * 4
        assert ops.mhcn_fused_ok(d)
    assert lib.sslrec_mhcn_ws_bytes(1000, 48) == 0 and lib.sslrec_mhcn_ws_bytes(0, 64) == 0
    assert lib.sslrec_mhcn_gate_ws_bytes(1000, 64, 5) == 0 and lib.sslrec_mhcn_gate_ws_bytes(1000, 48, 4) == 0
    assert not ops.mhcn_fused_ok(48) and not ops.mhcn_fused_ok(256)
