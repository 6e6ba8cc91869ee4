"""NCL on the GPU: ops.kmeans (csrc/kmeans.hip and the composed path) by invariants against float64 -- one step, the tie rule, the
exactness of the early exit, the fixed point, separated blobs, determinism -- and the model: loss parts and gradients against a
float64 restatement of ncl.py:51-86 fed with the model's own clustering, three epochs through the default Trainer, evaluation.

Shapes (N, d, K): the five of the feature's specification, d = 48, which the kernels do not take (the composed path), and for the
update kernel's other paths one that needs two cluster chunks (K d > 4096 sums) and one at the LDS limit K d 4 = 64 KiB (four chunks).
The checks of one shape share one test: the suite runs again for every later change, and a test costs its set-up every time."""
import numpy as np
import pytest
import torch

import ncl_reference as R

DEV = 'cuda:0'
TINY_U, TINY_I = 300, 220
# (N, d, K).  SPEC: the shapes every check runs on -- five kernel shapes and d = 48, which the kernels do not take (the composed path).
# CHUNKED: two further kernel shapes, for the paths of the update kernel the others do not reach (one step and determinism only).
SPEC = [(1500, 32, 50), (777, 64, 50), (1000, 128, 7), (1, 32, 3), (65, 32, 128), (500, 48, 9)]
CHUNKED = [(300, 128, 40), (200, 32, 512)]
pytestmark = pytest.mark.gpu


def run(x, c0, **kw):
    from sslrec_amd import ops
    cent, idx, counts, iters = ops.kmeans(x, c0, **kw)
    return cent.cpu(), idx.cpu(), counts.cpu(), iters


def same_bits(a, b):
    return all(torch.equal(p, q) for p, q in zip(a[:3], b[:3]))


@pytest.mark.parametrize('N,d,K', SPEC + CHUNKED)
def test_one_step_tie_rule_early_exit_fixed_point_and_determinism(N, d, K):
    from sslrec_amd import ops
    what = str((N, d, K))
    assert ops.KMEANS_FUSED and ops.kmeans_fused_ok(K, d) == (d != 48)
    x, c0 = R.xavier_like(N, d, K, 100 + N)
    xd, cd = x.to(DEV), c0.to(DEV)
    # 1. one step
    one = run(xd, cd, max_iter=1)
    assert one[3] == 1
    R.check_step(x, c0, one, 'one step ' + what)
    assert same_bits(one, run(xd, cd, max_iter=1))               # 6. two calls give the same bits
    if (N, d, K) in CHUNKED:
        a, b = run(xd, cd, max_iter=12, early_exit=False), run(xd, cd, max_iter=12, early_exit=False)
        assert a[3] == b[3] == 12 and same_bits(a, b)
        R.check_update(x, a[1], a[0], a[2], '12 steps ' + what)
        return
    # 2. exact duplicates of the first rows appended: nobody is assigned to the later copy
    dup = torch.cat([cd, cd[:min(4, K)]])
    cent, idx, counts, _ = run(xd, dup, max_iter=1)
    assert int(idx.max()) < K and float(counts[K:].sum()) == 0 and bool((cent[K:] == 0).all()) and torch.equal(idx, one[1])
    # 3. the early exit returns the bits of 1000 iterations (and of a second call: 6.)
    early = run(xd, cd, max_iter=1000, early_exit=True)
    full = run(xd, cd, max_iter=1000, early_exit=False)
    print('%s: %d iterations run with the early exit' % (what, early[3]))
    assert early[3] < 1000 and full[3] == 1000 and same_bits(early, full)
    for poll in (1, 64):                                         # when the host looks changes how many iterations run, not what comes out
        again = run(xd, cd, max_iter=1000, poll=poll)
        assert again[3] < 1000 and (poll != 1 or again[3] <= early[3]) and same_bits(again, early)
    # 4. the fixed point: idx is nearest to, and averaged into, the returned centroids
    R.check_step(x, early[0], early, 'fixed point ' + what)


def test_separated_blobs_cluster_like_the_float64_run(monkeypatch):
    from sslrec_amd import ops
    x, c0 = R.blobs()
    xd, cd = x.to(DEV), c0.to(DEV)
    _, idx64, counts64 = R.lloyd64(x, c0, 50)
    assert int((counts64 > 0).sum()) == 8 and float(counts64[8:].sum()) == 0
    for kw in ({}, {'early_exit': False, 'max_iter': 40}):
        out = run(xd, cd, **kw)
        assert torch.equal(out[1], idx64)
        R.check_update(x, idx64, out[0], out[2], 'blobs')       # to the one-step bound; over idx64 its float64 means ARE the float64 run's centroids
    monkeypatch.setattr(ops, 'KMEANS_FUSED', False)             # the measurement switch: the composed path on a kernel shape
    out = run(xd, cd)
    assert torch.equal(out[1], idx64)
    R.check_update(x, idx64, out[0], out[2], 'blobs, composed')


def test_kmeans_refuses_what_it_cannot_take():
    from sslrec_amd import ops
    x, c0 = (t.to(DEV) for t in R.xavier_like(65, 32, 128, 1))
    for args, kw in (((x, c0[:, :16]), {}), ((x[0], c0), {}), ((x[:0], c0), {}), ((x, c0), {'max_iter': 0}), ((x, c0), {'poll': 0}), ((x, c0), {'poll': 65})):
        with pytest.raises(ValueError):
            ops.kmeans(*args, **kw)
    with pytest.raises(TypeError):
        ops.kmeans(x.double(), c0.double())
    xg = x.clone().requires_grad_(True)
    assert not ops.kmeans(xg, c0, max_iter=2)[0].requires_grad  # not differentiable (ncl.py:27-28 detaches)


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def tiny_handler(device, over=None):
    from helpers import FixtureHandler
    from sslrec_amd.config.configurator import load_config
    from sslrec_amd.data_utils import synth
    overrides = {'data': {'synthetic': 'tiny'}}
    overrides.update(over or {})
    load_config('ncl', device=device, overrides=overrides)
    return FixtureHandler(synth.make_dataset('tiny', 2023)).load_adj_only()


# struct_weight / proto_weight: the largest of the reference's tuning grid, so that both contrastive terms carry weight in the gradient
MODEL_CFG = {'embedding_size': 32, 'layer_num': 3, 'high_order': 2, 'struct_weight': 1.0e-1, 'proto_weight': 1.0e-2}


def tiny_model(cluster_num):
    from sslrec_amd.models.bulid_model import build_model
    dh = tiny_handler(DEV, {'model': dict(MODEL_CFG, cluster_num=cluster_num)})
    model = build_model(dh).to(DEV)
    with torch.no_grad():
        for p, f in zip(model.parameters(), R.fills(TINY_U, TINY_I, 32)):
            p.copy_(f.to(DEV))
    return dh, model


def tiny_batch():
    rng = np.random.RandomState(5)
    return [torch.from_numpy(rng.randint(0, n, 256)).long() for n in (120, TINY_I, TINY_I)]


def tiny_graph(dh):
    adj = dh.torch_adj.cpu()
    return adj._values().double(), adj._indices()[0], adj._indices()[1]


@pytest.mark.parametrize('cluster_num', [7, 50])
def test_ncl_loss_parts_and_gradients_given_its_own_clustering(cluster_num):
    """Tolerances: those of the InfoNCE-carrying whole-step tests of tests/test_gpu_parity.py (_check_step, as
    test_training_step_matches_reference_tiny[simgcl] uses it): loss and parts rtol 1e-5 (parts atol 1e-9, reg_loss rtol 2e-6 against
    the float64 sum), gradients rtol 1e-4, atol 1e-7."""
    from sslrec_amd.config.configurator import configs
    torch.manual_seed(91)
    dh, model = tiny_model(cluster_num)
    model._cluster()
    assert tuple(model.user_centroids.shape) == tuple(model.item_centroids.shape) == (cluster_num, 32)
    assert tuple(model.user2cluster.shape) == (TINY_U,) and tuple(model.item2cluster.shape) == (TINY_I,)
    assert model.kmeans.iters_run < 1000
    batch = tiny_batch()
    flags = torch.zeros(256, dtype=torch.int64)
    calls = []
    model._cluster = lambda: calls.append(1)                    # flags all zero and a clustering at hand: cal_loss must not cluster
    loss, parts = model.cal_loss([b.to(DEV) for b in batch + [flags]])
    loss.backward()
    torch.cuda.synchronize()
    assert not calls and sorted(parts) == ['bpr_loss', 'proto_loss', 'reg_loss', 'struct_loss']
    ue, ie = (f.double().requires_grad_(True) for f in R.fills(TINY_U, TINY_I, 32))
    clusters = (model.user_centroids.double().cpu(), model.user2cluster.cpu(), model.item_centroids.double().cpu(), model.item2cluster.cpu())
    ref, ref_parts = R.ref_ncl_loss(ue, ie, tiny_graph(dh), batch, clusters, configs['model'])
    ref.backward()
    R.np_allclose(loss.item(), ref.item(), 1e-5, 0, 'loss')
    for k, v in parts.items():
        print('%s: got %.9g, float64 %.9g' % (k, float(v.detach()), float(ref_parts[k].detach())))
        R.np_allclose(float(v.detach()), float(ref_parts[k].detach()), 2e-6 if k == 'reg_loss' else 1e-5, 1e-9, k)
    for (name, p), want in zip(model.named_parameters(), (ue.grad, ie.grad)):
        err = (p.grad.cpu().double() - want).abs().max().item()
        print('d %s: largest gradient element %.3e, largest error %.3e' % (name, want.abs().max().item(), err))
        R.np_allclose(p.grad.cpu().numpy(), want.numpy(), 1e-4, 1e-7, 'd ' + name)


def test_cluster_leaves_the_cpu_generator_behind_two_centroid_draws():
    torch.manual_seed(91)
    dh, model = tiny_model(50)
    torch.manual_seed(123)
    model._cluster()
    torch.cuda.synchronize()
    got = torch.get_rng_state()
    torch.manual_seed(123)
    u0, i0 = torch.rand([50, 32]), torch.rand([50, 32])
    assert torch.equal(torch.get_rng_state(), got)
    # ... and the clustering started from exactly these draws: one step from them gives the assignment the model's run began with
    from sslrec_amd import ops
    want = ops.kmeans(model.user_embeds.detach(), u0.to(DEV))
    assert torch.equal(want[0], model.user_centroids) and torch.equal(want[1], model.user2cluster)
    want = ops.kmeans(model.item_embeds.detach(), i0.to(DEV))
    assert torch.equal(want[0], model.item_centroids) and torch.equal(want[1], model.item2cluster)
    # the default Trainer replays the CPU generator on the device: the same numbers, and after the flush the same generator state
    from sslrec_amd import rng
    first = (model.user_centroids.clone(), model.item_centroids.clone())
    rng.enable_host_replay(DEV)
    try:
        torch.manual_seed(123)
        model._cluster()
        rng.flush_host_replay()
        assert torch.equal(torch.get_rng_state(), got)
        assert torch.equal(model.user_centroids, first[0]) and torch.equal(model.item_centroids, first[1])
    finally:
        rng.disable_host_replay(DEV)


class _Log:
    def log(self, *a, **k):
        pass

    log_loss = log_eval = log


def test_ncl_trains_three_epochs_through_the_trainer_and_evaluates_from_its_cache():
    from sslrec_amd.config.configurator import configs, load_config
    from sslrec_amd.data_utils.build_data_handler import build_data_handler
    from sslrec_amd.models.bulid_model import build_model
    from sslrec_amd.trainer.trainer import Trainer
    load_config('ncl', device=DEV, overrides={'data': {'synthetic': 'tiny'}, 'train': {'epoch': 3, 'test_step': 3, 'batch_size': 1024},
                                              'model': {'epoch_period': 2, 'cluster_num': 7}})
    configs['train']['early_stop'] = False                      # (no best-model rebuild: three epochs, one evaluation, the test)
    torch.manual_seed(2023)
    np.random.seed(2023)
    dh = build_data_handler()
    dh.load_data()
    model = build_model(dh).to(DEV)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    log = []                                                    # per training batch: [flag sum, clustered?, loss parts]
    cal_loss, cluster = model.cal_loss, model._cluster

    def spy_cluster():
        log[-1][1] = True
        cluster()

    def spy_cal_loss(batch):
        log.append([int(batch[3].sum()), False, None])
        loss, parts = cal_loss(batch)
        log[-1][2] = [loss.detach()] + [v.detach() for v in parts.values()]
        return loss, parts

    model._cluster, model.cal_loss = spy_cluster, spy_cal_loss
    trainer = Trainer(dh, _Log())
    trainer.train(model)
    n_batches = len(dh.train_dataloader)
    assert len(log) == 3 * n_batches
    assert [row[1] for row in log] == [row[0] != 0 for row in log]            # clustered exactly on the flagged batches ...
    assert [i for i, row in enumerate(log) if row[1]] == [0] + [i for i in range(n_batches, 2 * n_batches) if log[i][0]]
    assert sum(row[1] for row in log) == 2                                    # ... the first batch ever and one batch of the second epoch
    assert all(bool(torch.isfinite(torch.stack(row[2])).all()) for row in log)
    for n, p in model.named_parameters():
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), before[n]), n
    result = trainer.evaluate(model)
    assert all(np.isfinite(v).all() for v in result.values()) and set(result) == set(configs['test']['metrics'])
    # evaluation: the first call after training propagates anew, the later ones reuse final_embeds_list (ncl.py:31-32)
    model._cluster, model.cal_loss = cluster, cal_loss
    model.is_training = True
    model.eval()
    users = torch.tensor([0, 5, 17, 299, 150, 5])
    mask = torch.from_numpy(dh.trn_mat.tocsr()[users.numpy()].toarray()).float()
    got = model.full_predict((users.to(DEV), mask.to(DEV)))
    cached = model.final_embeds_list
    assert cached is not None and len(cached) == 5 and not model.is_training
    again = model.full_predict((users.to(DEV), mask.to(DEV)))
    assert model.final_embeds_list is cached and torch.equal(got, again)
    adj = dh.torch_adj.cpu()
    final, _ = R.ref_ncl_forward(model.user_embeds.detach().double().cpu(), model.item_embeds.detach().double().cpu(),
                                 (adj._values().double(), adj._indices()[0], adj._indices()[1]), 3, 2)
    U = model.user_num
    scores = (final[:U][users] @ final[U:].T) * (1 - mask.double()) - 1e8 * mask.double()
    assert torch.allclose(got.cpu().double(), scores, rtol=1e-4, atol=1e-5)
