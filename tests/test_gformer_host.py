"""GFormer without a GPU: the model builds from its config with the reference's parameters and draw order, the trainer factory hands
out GFormerTrainer for this model only, train.hip_graph is refused, the in-kernel hop weight equals the reference's float64 -> float32
array, the collapsed PNN expression equals the literal [N, A, 2d] restatement (and would not with the row itself as self feature), the
masker's and LocalGraph's host logic reproduce the restatement entry for entry with the same number of numpy draws, and the C entry
points refuse bad arguments before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

import gformer_reference as R

TINY_U, TINY_I = 300, 220


def tiny_handler(device, over=None):
    from helpers import FixtureHandler
    from sslrec_amd.config.configurator import load_config
    from sslrec_amd.data_utils import synth
    overrides = {'data': {'synthetic': 'tiny'}}
    overrides.update(over or {})
    load_config('gformer', device=device, overrides=overrides)
    return FixtureHandler(synth.make_dataset('tiny', 2023)).load_adj_only()


def test_gformer_config_holds_the_reference_values():
    from sslrec_amd.config.configurator import configs
    tiny_handler('cpu')
    o, tr, te, da, m, tu = (configs[k] for k in ('optimizer', 'train', 'test', 'data', 'model', 'tune'))
    assert (o['name'], o['lr'], o['weight_decay']) == ('adam', 1.0e-3, 0)
    assert (tr['epoch'], tr['batch_size'], tr['save_model'], tr['loss'], tr['log_loss']) == (300, 4096, False, 'pairwise', False)
    assert (tr['test_step'], tr['patience'], tr['reproducible'], tr['seed'], tr['trainer']) == (3, 5, True, 2023, 'gformer_trainer')
    assert (te['metrics'], te['k'], te['batch_size']) == (['recall', 'ndcg'], [10, 20, 40], 1024)
    assert (da['type'], da['name']) == ('general_cf', 'gowalla')
    want = {'name': 'gformer', 'keep_rate': 0.9, 'layer_num': 2, 'reg_weight': 1.0e-6, 'cl_weight': 1.0, 'temperature': 0.1,
            'embedding_size': 32, 'gtw': 0.1, 'anchor_set_num': 64, 'fix_steps': 10, 'ctra': 1.0e-3, 'ssl_reg': 1.0, 'b2': 1.0,
            'reRate': 0.8, 'head': 4, 'ext': 0.5, 'addRate': 0.01, 'pnn_layer': 1, 'sub': 0.1}
    assert {k: m[k] for k in want} == want
    assert tu['enable'] is False and tu['hyperparameters'] == ['layer_num', 'reg_weight', 'ssl_reg']
    assert tu['layer_num'] == [2, 3] and tu['reg_weight'] == [1.0e-6, 1.0e-7, 1.0e-8] and tu['ssl_reg'] == [1.0e-1, 1, 2, 5]


def test_gformer_builds_with_the_reference_parameters_and_draw_order():
    from sslrec_amd.models.bulid_model import build_model
    import sslrec_amd.models.general_cf.gformer as G
    dh = tiny_handler('cpu', {'model': {'pnn_layer': 2}})
    torch.manual_seed(77)
    model = build_model(dh)
    assert type(model).__name__ == 'GFormer'
    for cls in ('GCNLayer', 'PNNLayer', 'GTLayer', 'LocalGraph', 'RandomMaskSubgraphs'):
        assert hasattr(G, cls)
    for fn in ('forward', 'cal_loss', 'full_predict', 'getEgoEmbeds', 'preSelect_anchor_set', 'get_random_anchorset'):
        assert callable(getattr(model, fn))
    lin = lambda prefix: [(prefix + '.linear_out.weight', (32, 32)), (prefix + '.linear_out.bias', (32,)),
                          (prefix + '.linear_hidden.weight', (32, 64)), (prefix + '.linear_hidden.bias', (32,))]
    want = [('uEmbeds', (TINY_U, 32)), ('iEmbeds', (TINY_I, 32))] + [('gtLayers.%sTrans' % c, (32, 32)) for c in 'qkv'] + \
        lin('pnnLayers.0') + lin('pnnLayers.1') + lin('localGraph.pnn')
    assert [(n, tuple(p.shape)) for n, p in model.named_parameters()] == want          # gtLayers is shared with localGraph: counted once
    assert model.localGraph.gt_layer is model.gtLayers
    after = torch.get_rng_state()
    # the reference's draws, gformer.py:37-44: the tables, GTLayer (:224-226), then two nn.Linear per PNNLayer (:198-199)
    torch.manual_seed(77)
    init = nn.init.xavier_uniform_
    drawn = [init(torch.empty(TINY_U, 32)), init(torch.empty(TINY_I, 32))] + [init(torch.empty(32, 32)) for _ in range(3)]
    for _ in range(3):
        for lin_ in (nn.Linear(32, 32), nn.Linear(64, 32)):
            drawn += [lin_.weight.detach(), lin_.bias.detach()]
    assert torch.equal(torch.get_rng_state(), after)                                   # ... and nothing more
    for (n, p), ref in zip(model.named_parameters(), drawn):
        assert torch.equal(p.detach(), ref), n
    model.load_state_dict({n: torch.full_like(p, 0.25) for n, p in model.state_dict().items()})      # a reference checkpoint's names
    assert torch.all(model.localGraph.gt_layer.vTrans == 0.25)


def test_trainer_factory_builds_gformer_trainer_for_gformer_only():
    from sslrec_amd.config.configurator import configs, load_config
    from sslrec_amd.trainer.build_trainer import build_trainer
    from sslrec_amd.trainer.trainer import GFormerTrainer
    dh = tiny_handler('cpu')
    trainer = build_trainer(dh, None)
    assert type(trainer) is GFormerTrainer and trainer.fixSteps == 10
    configs['train']['hip_graph'] = True
    with pytest.raises(NotImplementedError, match='train.hip_graph'):
        build_trainer(dh, None)
    load_config('lightgcn', device='cpu', overrides={'data': {'synthetic': 'tiny'}, 'train': {'trainer': 'gformer_trainer'}})
    with pytest.raises(NotImplementedError, match='gformer_trainer'):
        build_trainer(dh, None)


def test_the_in_kernel_hop_weight_equals_the_float64_array_rounded_to_float32():
    """csrc/pnn.hip computes 1.0f / (float)(h + 1); the reference stores float64 1 / (h + 1) and converts with t.tensor(..., float32)"""
    from sslrec_amd import ops
    h = np.arange(0, 32767, dtype=np.int64)
    in_kernel = np.float32(1.0) / (h + 1).astype(np.float32)
    assert in_kernel.dtype == np.float32
    reference = torch.tensor(1 / (h + 1), dtype=torch.float32).numpy()                 # gformer.py:174, :205
    assert np.array_equal(in_kernel, reference)
    hops = torch.from_numpy(np.concatenate([[-1], h]).astype(np.int16))
    w = ops.hop_weights(hops).numpy()
    assert w[0] == 0 and np.array_equal(w[1:], reference)


def _pnn_case(N, A, d, seed):
    rng = np.random.RandomState(seed)
    x = R.randn((N, d), seed)
    anchors = rng.choice(N, A, replace=A > N)                   # (more anchors than nodes: ids repeat)
    hops = rng.randint(-1, 6, size=(N, A)).astype(np.int16)
    hops[np.asarray(anchors), np.arange(A)] = 0
    hops[N // 2] = -1
    return x, anchors, torch.from_numpy(hops)


@pytest.mark.parametrize('N,A,d', [(257, 64, 32), (33, 64, 32), (200, 7, 32)])
def test_collapsed_pnn_equals_the_literal_restatement_and_needs_the_cyclic_window(N, A, d):
    from sslrec_amd.models.general_cf.gformer import PNNLayer
    x, anchors, hops = _pnn_case(N, A, d, 11 + N)
    w, b = R.randn((d, 2 * d), 5, 0.3), R.randn((d,), 6, 0.3)
    x1, x2 = R.leaf(x, torch.float64), R.leaf(x, torch.float64)
    want = R.ref_pnn(x1, anchors, R.ref_dists(hops, torch.float64), w, b)
    z = PNNLayer.position_features(x2, anchors, hops)
    got = torch.nn.functional.linear(z, w, b)
    g = R.randn((N, d), 9)
    (want * g).sum().backward()
    (got * g).sum().backward()
    e_fwd, e_bwd = R.rel_err(got, want.detach()), R.rel_err(x2.grad, x1.grad)
    print('collapsed PNN (%d, %d, %d): forward %.2e gradient %.2e' % (N, A, d, e_fwd, e_bwd))
    assert e_fwd <= 1e-13 and e_bwd <= 1e-13
    z_self = torch.cat([z.detach()[:, :d], x], dim=1)                                  # u_n = x_n: what the layer was meant to be
    assert R.rel_err(torch.nn.functional.linear(z_self, w, b), want.detach()) > 1e-2


GRAPH_U, GRAPH_I = 120, 90
GRAPH_N = GRAPH_U + GRAPH_I
MASK_SEED = 5


def _masker_case():
    from sslrec_amd.config.configurator import load_config
    from helpers import FixtureHandler
    import scipy.sparse as sp
    rows, cols = R.small_bipartite(GRAPH_U, GRAPH_I, 700, 3, isolated=(7, GRAPH_U + 4))
    half = rows.shape[0] // 2
    trn = sp.coo_matrix((np.ones(half, dtype=np.float32), (rows[:half], cols[:half] - GRAPH_U)), shape=(GRAPH_U, GRAPH_I))
    load_config('gformer', device='cpu', overrides={'model': {'addRate': 0.05}})
    dh = FixtureHandler(trn).load_adj_only()
    idx = dh.torch_adj._indices().numpy().astype(np.int64)
    return dh, idx[0], idx[1]


def test_local_graph_and_masker_host_logic_equal_the_restatement_draw_for_draw():
    from sslrec_amd.config.configurator import configs
    from sslrec_amd.models.general_cf.gformer import LocalGraph, GTLayer, RandomMaskSubgraphs
    dh, rows, cols = _masker_case()
    m = configs['model']
    local, masker = LocalGraph(dh, GTLayer(dh)), RandomMaskSubgraphs(dh)
    np.random.seed(MASK_SEED)
    a_rows, a_cols = local.add_adj_entries(rows, cols)
    E = a_rows.shape[0]
    att0 = (torch.rand(E, generator=torch.Generator().manual_seed(1)) * 4.5).float()   # scores in [0, 4.5): a third of them above the clamp
    assert int((att0 > 3).sum()) > E // 5
    att = att0.clone()
    out = masker.mask_entries(a_rows, a_cols, att)
    after = np.random.rand()
    assert torch.equal(att, att0.clamp(max=3))                                         # clamped in place, as upstream

    np.random.seed(MASK_SEED)
    r_rows, r_cols = R.ref_add_adj(rows, cols, GRAPH_N, m['addRate'])
    assert int(len(rows) * m['addRate']) >= 10
    assert np.array_equal(a_rows, r_rows) and np.array_equal(a_cols, r_cols)           # sorted, unique, diagonal included
    assert np.all(np.diff(a_rows * GRAPH_N + a_cols) > 0) and int((a_rows == a_cols).sum()) == GRAPH_N
    r_att = att0.clone()
    ref = R.ref_masker(r_rows, r_cols, r_att, GRAPH_N, m)
    assert after == np.random.rand()                                                   # exactly as many numpy draws
    twice = 0
    for key in ('enc', 'sub', 'cmp'):
        vals, has = out[key]
        w_rows, w_cols, w_vals, w_raw = ref[key]
        assert np.array_equal(a_rows[has], w_rows) and np.array_equal(a_cols[has], w_cols), key
        assert vals.dtype == np.float32 and np.array_equal(vals[has], w_vals), key
        assert np.all(vals[~has] == 0)
        twice += int(((w_raw == 2) & (w_rows == w_cols)).sum())
        assert set(np.unique(w_raw)) <= {1.0, 2.0}
    assert int(((ref['enc'][3] == 2) & (ref['enc'][0] == ref['enc'][1])).sum()) >= 1   # a kept diagonal entry counts twice (seed chosen so)
    assert twice >= 1
    assert np.array_equal(out['dec'][0], ref['dec'][0]) and np.array_equal(out['dec'][1], ref['dec'][1])
    assert int(out['keep'].sum()) == int(E * m['keep_rate'])

    # flag=True saw the CLAMPED scores: with the unclamped ones its draw would differ
    np.random.seed(MASK_SEED + 1)
    clamped = masker.create_sub_adj_entries(a_rows, a_cols, att0.clamp(max=3), True, GRAPH_N)
    np.random.seed(MASK_SEED + 1)
    unclamped = masker.create_sub_adj_entries(a_rows, a_cols, att0.clone(), True, GRAPH_N)
    assert not np.array_equal(clamped[1], unclamped[1])
    np.random.seed(MASK_SEED)
    local.add_adj_entries(rows, cols)
    again = masker.mask_entries(a_rows, a_cols, att0.clamp(max=3))                     # already clamped input: the same result
    assert np.array_equal(again['sub'][0], out['sub'][0]) and np.array_equal(again['cmp'][0], out['cmp'][0])


def test_ops_refuse_cpu_tensors_and_report_their_fused_shapes():
    from sslrec_amd import ops
    x, anchors, hops = _pnn_case(40, 8, 32, 1)
    with pytest.raises(RuntimeError, match='HIP device only'):
        ops.anchor_position_features(x.float(), anchors, hops)
    with pytest.raises(RuntimeError, match='HIP device only'):
        ops.edge_attention_scores(None, x.float(), x.float(), 4)
    assert ops.anchor_position_fused_ok(32, 64) and ops.anchor_position_fused_ok(128, 256) and ops.anchor_position_fused_ok(64, 1)
    assert not ops.anchor_position_fused_ok(48, 64) and not ops.anchor_position_fused_ok(32, 257) and not ops.anchor_position_fused_ok(32, 0)
    assert ops.anchor_hops_fused_ok(1, 1) and ops.anchor_hops_fused_ok(10, 256) and not ops.anchor_hops_fused_ok(10, 257)
    assert not ops.anchor_hops_fused_ok(10, 0)


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    from sslrec_amd import _lib
    lib = _lib.load()
    assert lib.sslrec_abi_version() == 7
    assert lib.sslrec_anchor_hops_ws_bytes(210, 64) > 0 and lib.sslrec_anchor_hops_ws_bytes(1, 256) > 0
    assert lib.sslrec_pnn_bwd_ws_bytes(210, 64, 32) > 0 and lib.sslrec_pnn_bwd_ws_bytes(1, 256, 128) > 0
    assert lib.sslrec_gt_scores_ws_bytes(210, 32, 4) == 210 * 4 * 4
    for A in (0, 257):
        assert lib.sslrec_anchor_hops_ws_bytes(210, A) == 0 and lib.sslrec_pnn_bwd_ws_bytes(210, A, 32) == 0, A
    assert lib.sslrec_anchor_hops_ws_bytes(0, 64) == 0 and lib.sslrec_pnn_bwd_ws_bytes(0, 64, 32) == 0
    assert lib.sslrec_pnn_bwd_ws_bytes(210, 64, 48) == 0 and lib.sslrec_pnn_bwd_ws_bytes(210, 1, 256) == 0
    assert lib.sslrec_gt_scores_ws_bytes(210, 48, 4) == 0 and lib.sslrec_gt_scores_ws_bytes(210, 32, 5) == 0 and lib.sslrec_gt_scores_ws_bytes(0, 32, 4) == 0
    buf = (C.c_float * 64)()                                    # host memory: every call below must return before touching it
    ptr = C.addressof(buf) + (-C.addressof(buf)) % 16
    levels, conv = C.c_int32(-1), C.c_int32(-1)
    good = dict(rowptr=ptr, col=ptr, n=1, long_rows=None, n_long=0, anchors=ptr, A=1, hops=ptr, poll=8, levels=C.byref(levels),
                conv=C.byref(conv), ws=ptr)
    for change in (dict(rowptr=None), dict(col=None), dict(anchors=None), dict(hops=None), dict(levels=None), dict(conv=None), dict(ws=None),
                   dict(n=0), dict(A=0), dict(A=257), dict(poll=0), dict(poll=65), dict(n_long=1), dict(n_long=-1)):
        a = dict(good, **change)
        rc = lib.sslrec_anchor_hops(a['rowptr'], a['col'], a['n'], a['long_rows'], a['n_long'], a['anchors'], a['A'], a['hops'], a['poll'],
                                    a['levels'], a['conv'], a['ws'], None)
        assert rc == _lib.E_BADARG, change
    assert levels.value == -1 and conv.value == -1
    good = dict(X=ptr, N=1, d=32, anchors=ptr, A=1, hops=ptr, Z=ptr)
    for change in (dict(X=None), dict(anchors=None), dict(hops=None), dict(Z=None), dict(N=0), dict(d=48), dict(A=0), dict(A=257),
                   dict(d=128, A=257), dict(X=ptr + 4), dict(Z=ptr + 8)):
        a = dict(good, **change)
        assert lib.sslrec_pnn_fwd_f32(a['X'], a['N'], a['d'], a['anchors'], a['A'], a['hops'], a['Z'], None) == _lib.E_BADARG, change
        assert lib.sslrec_pnn_bwd_f32(a['X'], a['N'], a['d'], a['anchors'], a['A'], a['hops'], a['Z'], ptr, None) == _lib.E_BADARG, change
    assert lib.sslrec_pnn_bwd_f32(ptr, 1, 32, ptr, 1, ptr, ptr, None, None) == _lib.E_BADARG
    good = dict(rowptr=ptr, col=ptr, n=1, long_rows=None, n_long=0, Q=ptr, K=ptr, d=32, heads=4, out=ptr, z=ptr)
    for change in (dict(rowptr=None), dict(col=None), dict(Q=None), dict(K=None), dict(out=None), dict(z=None), dict(n=-1), dict(d=48),
                   dict(heads=5), dict(heads=0), dict(n_long=1)):
        a = dict(good, **change)
        rc = lib.sslrec_gt_scores_f32(a['rowptr'], a['col'], a['n'], a['long_rows'], a['n_long'], a['Q'], a['K'], a['d'], a['heads'], a['out'],
                                      a['z'], None)
        assert rc == _lib.E_BADARG, change
