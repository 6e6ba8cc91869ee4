"""NCL without a GPU: the model builds from its config with the reference's parameters and draw order, the data handler feeds it
4-tuple batches with the epoch flag, train.hip_graph is refused by name, ops.kmeans refuses CPU tensors, the C entry points refuse bad
arguments before any launch, and the composed (torch) k-means path -- plain tensor code, so it runs on the CPU when called directly --
holds the invariants test_ncl.py holds the kernels to."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

import ncl_reference as R

TINY_U, TINY_I = 300, 220


def tiny_handler(device, over=None):
    from helpers import FixtureHandler
    from sslrec_amd.config.configurator import load_config
    from sslrec_amd.data_utils import synth
    overrides = {'data': {'synthetic': 'tiny'}}
    overrides.update(over or {})
    load_config('ncl', device=device, overrides=overrides)
    return FixtureHandler(synth.make_dataset('tiny', 2023)).load_adj_only()


def test_ncl_config_holds_the_reference_values():
    from sslrec_amd.config.configurator import configs
    tiny_handler('cpu')
    o, tr, te, da, m, tu = (configs[k] for k in ('optimizer', 'train', 'test', 'data', 'model', 'tune'))
    assert (o['name'], o['lr'], o['weight_decay']) == ('adam', 1.0e-3, 0)
    assert (tr['epoch'], tr['batch_size'], tr['save_model'], tr['loss'], tr['log_loss']) == (300, 4096, False, 'pairwise_with_epoch_flag', False)
    assert (tr['test_step'], tr['patience'], tr['reproducible'], tr['seed']) == (3, 5, True, 2023)
    assert (te['metrics'], te['k'], te['batch_size']) == (['recall', 'ndcg'], [10, 20, 40], 1024)
    assert (da['type'], da['name']) == ('general_cf', 'gowalla')
    want = {'name': 'ncl', 'keep_rate': 1.0, 'layer_num': 3, 'high_order': 2, 'reg_weight': 1.0e-7, 'proto_weight': 1.0e-4,
            'struct_weight': 1.0e-3, 'temperature': 0.1, 'embedding_size': 32, 'epoch_period': 3, 'cluster_num': 50}
    assert {k: m[k] for k in want} == want
    assert tu['hyperparameters'] == ['temperature', 'proto_weight', 'struct_weight']
    assert tu['temperature'] == [0.1, 0.2, 0.3, 0.5, 1.0] and tu['proto_weight'] == [1.0e-2, 1.0e-3, 1.0e-4] and tu['struct_weight'] == [1.0e-1, 1.0e-2, 1.0e-3]
    assert tu['enable'] is False          # (the one departure: the reference ships true, main.py here refuses grid search)


def test_ncl_builds_with_the_reference_parameters_and_draw_order():
    from sslrec_amd.models.bulid_model import build_model
    dh = tiny_handler('cpu')
    torch.manual_seed(77)
    model = build_model(dh)
    assert type(model).__name__ == 'NCL'
    assert {n: tuple(p.shape) for n, p in model.named_parameters()} == {'user_embeds': (TINY_U, 32), 'item_embeds': (TINY_I, 32)}
    assert (model.layer_num, model.high_order, model.temperature, model.proto_weight, model.struct_weight) == (3, 2, 0.1, 1.0e-4, 1.0e-3)
    assert (model.kmeans.cluster_num, model.kmeans.embedding_size, model.kmeans.max_iter) == (50, 32, 1000)
    assert model.device_rng is None and not hasattr(model, 'user2cluster')
    drawn = [model.kmeans.draw_centroids('cpu'), model.kmeans.draw_centroids('cpu')]      # what _cluster draws, users first (ncl.py:27-28)
    after = torch.get_rng_state()
    torch.manual_seed(77)                                                                  # the reference's draws: ncl.py:13, aug_utils.py:147
    init = nn.init.xavier_uniform_
    want = [init(torch.empty(TINY_U, 32)), init(torch.empty(TINY_I, 32)), torch.rand([50, 32]), torch.rand([50, 32])]
    for (n, p), w in zip(model.named_parameters(), want):
        assert torch.equal(p, w), n
    assert torch.equal(drawn[0], want[2]) and torch.equal(drawn[1], want[3])
    assert torch.equal(torch.get_rng_state(), after)                                       # ... and nothing more


def test_the_handler_feeds_ncl_four_tuples_with_the_epoch_flag():
    from sslrec_amd.config.configurator import load_config
    from sslrec_amd.data_utils.build_data_handler import build_data_handler
    from sslrec_amd.data_utils.datasets_general_cf import PairwiseWEpochFlagTrnData
    load_config('ncl', device='cpu', overrides={'data': {'synthetic': 'tiny'}, 'train': {'batch_size': 512}, 'model': {'epoch_period': 2}})
    np.random.seed(3)
    torch.manual_seed(3)
    dh = build_data_handler()
    dh.load_data()
    loader = dh.train_dataloader
    assert type(loader.dataset) is PairwiseWEpochFlagTrnData
    flagged = []
    for epoch in range(3):
        loader.dataset.sample_negs()
        sums = []
        for batch in loader:
            assert len(batch) == 4 and all(b.shape == batch[0].shape for b in batch)
            sums.append(int(batch[3].sum()))
        flagged.append(sums)
    assert flagged[0][0] == 1 and sum(flagged[0]) == 1          # the very first sample ever drawn
    assert sum(flagged[1]) == 1 and sum(flagged[2]) == 0        # epoch_period = 2: sample 0 of the epoch whose counter reaches 2


def test_ncl_refuses_a_captured_step_by_name():
    from sslrec_amd.models.bulid_model import build_model
    dh = tiny_handler('cpu', {'train': {'hip_graph': True}})
    with pytest.raises(NotImplementedError, match='train.hip_graph'):
        build_model(dh)


def test_kmeans_refuses_cpu_tensors_like_the_other_ops():
    from sslrec_amd import ops
    x, c0 = R.xavier_like(40, 32, 5, 1)
    with pytest.raises(RuntimeError, match='HIP device only'):
        ops.kmeans(x, c0)
    assert ops.kmeans_fused_ok(50, 32) and ops.kmeans_fused_ok(50, 64) and ops.kmeans_fused_ok(128, 128) and ops.kmeans_fused_ok(512, 32)
    assert not ops.kmeans_fused_ok(50, 48) and not ops.kmeans_fused_ok(129, 128) and not ops.kmeans_fused_ok(513, 32) and not ops.kmeans_fused_ok(0, 32)


def test_kmeans_entry_points_reject_bad_arguments_without_a_gpu():
    from sslrec_amd import _lib
    lib = _lib.load()
    assert lib.sslrec_kmeans_ws_bytes(1500, 50, 32) > 0 and lib.sslrec_kmeans_ws_bytes(1, 1, 128) > 0
    for N, K, d in ((0, 50, 32), (100, 0, 32), (100, 50, 48), (100, 513, 32), (100, 129, 128)):
        assert lib.sslrec_kmeans_ws_bytes(N, K, d) == 0, (N, K, d)
    buf = (C.c_float * 64)()                                    # host memory: every call below must return before touching it
    ptr = C.addressof(buf) + (-C.addressof(buf)) % 16
    iters = C.c_int32(-1)
    good = dict(X=ptr, N=1, d=32, K=1, cent=ptr, idx=ptr, counts=ptr, max_iter=1, early=1, poll=8, iters=C.byref(iters), ws=ptr)
    for change in (dict(X=None), dict(cent=None), dict(idx=None), dict(counts=None), dict(ws=None), dict(iters=None), dict(N=0), dict(d=48),
                   dict(K=0), dict(K=513), dict(max_iter=0), dict(poll=0), dict(poll=65), dict(X=ptr + 4), dict(cent=ptr + 8)):
        a = dict(good, **change)
        rc = lib.sslrec_kmeans_f32(a['X'], a['N'], a['d'], a['K'], a['cent'], a['idx'], a['counts'], a['max_iter'], a['early'], a['poll'],
                                   a['iters'], a['ws'], None)
        assert rc == _lib.E_BADARG, change
    assert iters.value == -1


# ---- the composed path is tensor code: called directly it runs on the CPU -------------------------------------------
COMPOSED_SHAPES = [(1500, 32, 50), (777, 64, 50), (300, 48, 9), (1, 32, 3), (65, 32, 128)]


@pytest.mark.parametrize('N,d,K', COMPOSED_SHAPES)
def test_composed_kmeans_one_step_tie_rule_and_exact_early_exit(N, d, K, monkeypatch):
    from sslrec_amd import ops
    monkeypatch.setattr(ops, 'KMEANS_CHUNK_ELEMS', 211 * K * d)               # several row chunks, the last one ragged
    x, c0 = R.xavier_like(N, d, K, 100 + N)
    R.check_step(x, c0, ops._kmeans_composed(x, c0, 1, True, 8), 'composed one step %s' % ((N, d, K),))
    dup = torch.cat([c0, c0[:min(4, K)]])
    _, idx, counts, _ = ops._kmeans_composed(x, dup, 1, True, 8)
    assert int(idx.max()) < K and float(counts[K:].sum()) == 0                # nobody is assigned to the later copy
    early = ops._kmeans_composed(x, c0, 200, True, 8)
    full = ops._kmeans_composed(x, c0, 200, False, 8)
    assert early[3] < 200 and full[3] == 200
    for a, b in zip(early[:3], full[:3]):
        assert torch.equal(a, b)
    R.check_step(x, early[0], early, 'composed fixed point %s' % ((N, d, K),))
