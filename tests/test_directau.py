"""DirectAU: the fused alignment + uniformity loss (sslrec_amd/csrc/au.hip, ops.align_uniform_loss_stacked, loss_utils.alignment /
uniformity) and the model (sslrec_amd/models/general_cf/directau.py).

Yardstick of the GPU tests, as in tests/test_hccf.py: a float64 torch restatement of the reference's expressions
(models/general_cf/directau.py:27-59, models/loss_utils.py:75-86) written out below -- torch.pdist itself, the call the reference makes,
the propagation with index_add -- gradients by torch autograd.  The same restatement runs in fp32 on the CPU; its error against float64
is measured per tensor as max|x - ref| / max|ref|, and the kernels may be at most 4 x as far off, with a floor of 8 * 2^-23.  Both
errors are printed per tensor.

Shapes of the loss tests.  The kernels give a lane one batch row and a workgroup 64 of them (B = 63 / 64 / 65), cut the columns into
4 S parts of ceil(B / 4 S) columns, S = 8 up to B = 1024 (so B = 2, 3, 31, 33 leave most parts empty and 257, 1000 give ragged last
parts), and stage 2048 / d columns at a time: a part longer than that (d = 128 at B = 1000; d = 32 and 64 only at B = 2100, where
S = 3) takes several tiles with a ragged last one."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

FLOOR = 8 * 2.0 ** -23
DEV = 'cuda:0'
N_USER, N_ITEM = 400, 300
TINY_U, TINY_I = 300, 220


def randn(shape, seed, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def lt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).long()


def leaf(x, dt):
    return x.detach().to(dt).clone().requires_grad_(True)


def gpu(x):
    return x.detach().float().to(DEV)


def rel_err(x, ref):
    ref = ref.double()
    return float((x.detach().cpu().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def check(name, got, ref64, ref32):
    e32, e = rel_err(ref32, ref64), rel_err(got, ref64)
    bound = max(4 * e32, FLOOR)
    print('%-44s kernel %.3e  fp32 torch %.3e  (%.2f / %.2f units of 2^-23 max|ref|)  bound %.3e' % (name, e, e32, e * 2 ** 23, e32 * 2 ** 23, bound))
    assert torch.isfinite(got).all(), name
    assert e <= bound, '%s: kernel error %.3e > bound %.3e (fp32 torch: %.3e)' % (name, e, bound, e32)


def both_precisions(fn):
    return fn(torch.float64), fn(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement (any dtype, CPU)
# ---------------------------------------------------------------------------------------------------------------------
def ref_alignment(x, y, alpha=2):
    """loss_utils.py:75-79"""
    x, y = F.normalize(x, dim=-1), F.normalize(y, dim=-1)
    return (x - y).norm(p=2, dim=1).pow(alpha).mean()


def ref_uniformity(x):
    """loss_utils.py:82-86"""
    x = F.normalize(x, dim=-1)
    return torch.pdist(x, p=2).pow(2).mul(-2).exp().mean().log()


def ref_loss(user_embeds, item_embeds, ancs, poss, gamma):
    """directau.py:43-47"""
    anc, pos = user_embeds[ancs], item_embeds[poss]
    align = ref_alignment(anc, pos)
    uniform = gamma * (ref_uniformity(anc) + ref_uniformity(pos)) / 2
    return align + uniform, align, uniform


def ref_spmm(vals, heads, tails, x, n_rows):
    return torch.zeros(n_rows, x.shape[1], dtype=x.dtype).index_add(0, heads, vals[:, None] * torch.index_select(x, 0, tails))


def ref_forward(ue, ie, g, L):
    """directau.py:30-37: the mean of the L + 1 layers"""
    vals, heads, tails = g
    e0 = torch.concat([ue, ie], dim=0)
    lst = [e0]
    for _ in range(L):
        lst.append(ref_spmm(vals, heads, tails, lst[-1], e0.shape[0]))
    return sum(lst) / len(lst)


# ---------------------------------------------------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------------------------------------------------
def tiny_handler(device, over=None):
    from helpers import FixtureHandler
    from sslrec_amd.config.configurator import load_config
    from sslrec_amd.data_utils import synth
    overrides = {'data': {'synthetic': 'tiny'}}
    overrides.update(over or {})
    load_config('directau', device=device, overrides=overrides)
    return FixtureHandler(synth.make_dataset('tiny', 2023)).load_adj_only()


def test_directau_builds_from_its_config_with_the_reference_draw_order():
    from torch import nn
    from sslrec_amd.config.configurator import configs
    from sslrec_amd.models.bulid_model import build_model
    dh = tiny_handler('cpu')
    o, tr, te, da, m, tu = (configs[k] for k in ('optimizer', 'train', 'test', 'data', 'model', 'tune'))
    assert (o['name'], o['lr'], o['weight_decay']) == ('adam', 1.0e-3, 1.0e-6)
    assert (tr['epoch'], tr['batch_size'], tr['save_model'], tr['loss'], tr['log_loss']) == (300, 4096, False, 'pairwise', False)
    assert (tr['test_step'], tr['patience'], tr['reproducible'], tr['seed']) == (3, 5, True, 2023)
    assert (te['metrics'], te['k'], te['batch_size']) == (['recall', 'ndcg'], [10, 20, 40], 1024)
    assert (da['type'], da['name']) == ('general_cf', 'gowalla')
    assert (m['name'], m['layer_num'], m['gamma'], m['embedding_size']) == ('directau', 2, 2.0, 32)
    assert 'reg_weight' not in m
    assert tu['enable'] is False and tu['hyperparameters'] == ['layer_num', 'gamma']
    assert tu['layer_num'] == [2, 3] and tu['gamma'] == [0.5, 1, 1.5, 2, 2.5]
    torch.manual_seed(77)
    model = build_model(dh)
    after_build = torch.get_rng_state()
    assert type(model).__name__ == 'DirectAU'
    assert {n: tuple(p.shape) for n, p in model.named_parameters()} == {'user_embeds': (300, 32), 'item_embeds': (220, 32)}
    assert (model.layer_num, model.gamma) == (2, 2.0)
    torch.manual_seed(77)                                                       # the reference's draws, directau.py:19-20
    init = nn.init.xavier_uniform_
    want = [init(torch.empty(300, 32)), init(torch.empty(220, 32))]
    for (n, p), w in zip(model.named_parameters(), want):
        assert torch.equal(p, w), n
    assert torch.equal(torch.get_rng_state(), after_build)                      # ... and nothing more
    assert model.device_rng is None


def test_au_entry_points_reject_bad_arguments_without_a_gpu():
    from sslrec_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)       # a non-null HOST address: a call that got as far as a launch would fault, these return before
    bad = _lib.E_BADARG
    ws = lib.sslrec_au_ws_bytes
    nan, inf = float('nan'), float('inf')

    def fwd(T=p, N=10, n_user=4, d=32, ancs=p, poss=p, B=8, scale=1.0, gamma=2.0, terms=7, out=p, w=p):
        return lib.sslrec_au_fwd_f32(T, N, n_user, d, ancs, poss, B, scale, gamma, terms, out, w, None)

    def bwd(N=10, n_user=4, d=32, ancs=p, poss=p, B=8, scale=1.0, gamma=2.0, terms=7, out=p, g_align=p, g_uniform=p, dT=p, w=p):
        return lib.sslrec_au_bwd_f32(N, n_user, d, ancs, poss, B, scale, gamma, terms, out, g_align, g_uniform, dT, w, None)
    for name in ('T', 'ancs', 'poss', 'out', 'w'):
        assert fwd(**{name: None}) == bad, name
    for name in ('ancs', 'poss', 'out', 'g_align', 'g_uniform', 'dT', 'w'):
        assert bwd(**{name: None}) == bad, name
    for d in (0, 16, 48, 256):
        assert fwd(d=d) == bad and bwd(d=d) == bad and ws(8, d) == 0
    for B in (-1, 0, 1, 8193):
        assert fwd(B=B) == bad and bwd(B=B) == bad and ws(B, 32) == 0
    for n_user in (-1, 11):
        assert fwd(n_user=n_user) == bad and bwd(n_user=n_user) == bad
    assert fwd(N=-1, n_user=0) == bad and bwd(N=-1, n_user=0) == bad
    for v in (nan, inf, -inf):
        assert fwd(scale=v) == bad and bwd(scale=v) == bad and fwd(gamma=v) == bad and bwd(gamma=v) == bad
    for terms in (0, 8, -1):
        assert fwd(terms=terms) == bad and bwd(terms=terms) == bad
    # normalised rows + staged gradient rows alone are 4 B d floats; nothing grows with B^2
    assert ws(4096, 32) > 4 * 4096 * 32 * 4 and ws(2, 32) > 0 and ws(8192, 128) > 0
    assert ws(8192, 32) < 4 * ws(4096, 32)


class Meta:                         # shape checks come before any device work: a stand-in that claims to be on the GPU
    is_cuda = True

    def __init__(self, *shape):
        self.shape = shape

    def dim(self):
        return len(self.shape)


def test_au_ops_refuse_bad_arguments_before_loading_the_library(monkeypatch):
    from sslrec_amd import _lib, ops
    from sslrec_amd.models import loss_utils

    def no_load():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_lib, 'load', no_load)
    t, idx = torch.zeros(8, 32), torch.arange(4)
    with pytest.raises(RuntimeError, match='HIP device only'):
        ops.align_uniform_loss_stacked(t, 3, idx, idx, 2.0)
    with pytest.raises(RuntimeError, match='HIP device only'):
        loss_utils.alignment(t, t)
    with pytest.raises(RuntimeError, match='HIP device only'):
        loss_utils.uniformity(t)
    tm, im = Meta(8, 32), Meta(4)
    for bad in ((Meta(8), 3, im, im), (Meta(8, 32, 2), 3, im, im), (tm, 9, im, im), (tm, -1, im, im), (tm, 3, im, Meta(5)), (tm, 3, Meta(4, 1), Meta(4, 1)),
                (tm, 3, Meta(), Meta())):
        with pytest.raises(ValueError, match='align_uniform_loss_stacked'):
            ops.align_uniform_loss_stacked(*bad, 2.0)
    for gamma, scale in ((float('nan'), 1.0), (2.0, float('inf'))):
        with pytest.raises(ValueError, match='align_uniform_loss_stacked'):
            ops.align_uniform_loss_stacked(tm, 3, im, im, gamma, scale)
    for x, y in ((Meta(8, 32), Meta(8, 64)), (Meta(8), Meta(8)), (Meta(8, 32), Meta(7, 32))):
        with pytest.raises(ValueError, match='alignment'):
            loss_utils.alignment(x, y)
    for x in (Meta(8), Meta(8, 4, 2)):
        with pytest.raises(ValueError, match='uniformity'):
            loss_utils.uniformity(x)


# ---------------------------------------------------------------------------------------------------------------------
# GPU tests: the loss alone
# ---------------------------------------------------------------------------------------------------------------------
def loss_indices(B):
    """anchors among the first 120 users, positives among all items: destinations repeat; positions 3 and B - 1 hold the rows of
    position 1 (same user AND same item: a real pair of term 1 on both sides)"""
    rng = np.random.RandomState(1000 + B)
    ancs, poss = rng.randint(0, 120, B), rng.randint(0, N_ITEM, B)
    for pos in (3, B - 1):
        if 1 < pos < B:
            ancs[pos], poss[pos] = ancs[1], poss[1]
    return lt(ancs), lt(poss)


@functools.lru_cache(maxsize=None)
def loss_table(d):
    return randn((N_USER + N_ITEM, d), 11, 0.3).float().double()                # exactly representable in fp32


def loss_reference(table, ancs, poss, scale, gamma):
    def fn(dt):
        t_ = leaf(table, dt)
        mean = t_ * scale
        loss, align, uniform = ref_loss(mean[:N_USER], mean[N_USER:], ancs, poss, gamma)
        loss.backward()
        return {'loss': loss.detach(), 'align_loss': align.detach(), 'uniform_loss': uniform.detach(), 'dT': t_.grad}
    return both_precisions(fn)


def run_loss(table, ancs, poss, scale, gamma):
    from sslrec_amd import ops
    t_ = gpu(table).requires_grad_(True)
    loss, align, uniform = ops.align_uniform_loss_stacked(t_, N_USER, ancs.to(DEV), poss.to(DEV), gamma, scale)
    assert loss.dim() == 0 and align.dim() == 0 and uniform.dim() == 0
    loss.backward()
    return {'loss': loss.detach(), 'align_loss': align.detach(), 'uniform_loss': uniform.detach(), 'dT': t_.grad}


LOSS_SHAPES = [(B, d) for B in (2, 3, 31, 32, 33, 63, 64, 65, 257, 1000) for d in (32, 64, 128)] + [(300, 48), (2100, 32), (2100, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize('B,d', LOSS_SHAPES)
def test_align_uniform_loss_and_its_gradient(B, d):
    table = loss_table(d)
    ancs, poss = loss_indices(B)
    for scale, gamma in ((1.0, 2.0), (1.0 / 3.0, 0.5)):
        r64, r32 = loss_reference(table, ancs, poss, scale, gamma)
        got = run_loss(table, ancs, poss, scale, gamma)
        for name in ('loss', 'align_loss', 'uniform_loss', 'dT'):
            check('B=%d d=%d scale=%.3g gamma=%g %s' % (B, d, scale, gamma, name), got[name], r64[name], r32[name])
        untouched = torch.ones(N_USER + N_ITEM, dtype=torch.bool)
        untouched[ancs] = False
        untouched[N_USER + poss] = False
        assert torch.all(got['dT'].cpu()[untouched] == 0)                      # rows outside the batch get exact zeros


@pytest.mark.gpu
def test_a_zero_table_row_picked_as_anchor():
    B, d, zero_user = 65, 32, 200                                               # (loss_indices draws among the first 120 users)
    table = loss_table(d).clone()
    table[zero_user] = 0.0
    ancs, poss = loss_indices(B)
    assert not (ancs == zero_user).any()
    ancs[10] = zero_user                                                        # picked once
    r64, r32 = loss_reference(table, ancs, poss, 1.0, 2.0)
    got = run_loss(table, ancs, poss, 1.0, 2.0)
    assert 1e9 < float(r64['dT'][zero_user].abs().max()) < 1e12               # division by the 1e-12 clamp
    others = torch.ones(N_USER + N_ITEM, dtype=torch.bool)
    others[zero_user] = False
    for name in ('loss', 'align_loss', 'uniform_loss'):
        check('zero row %s' % name, got[name], r64[name], r32[name])
    check('zero row dT[zero row]', got['dT'][zero_user], r64['dT'][zero_user], r32['dT'][zero_user])
    check('zero row dT[other rows]', got['dT'][others.to(DEV)], r64['dT'][others], r32['dT'][others])


@pytest.mark.gpu
@pytest.mark.parametrize('B,d', [(33, 32), (257, 64)])
def test_dense_alignment_and_uniformity_drop_ins(B, d):
    from sslrec_amd.models import loss_utils
    x, y = randn((B, d), 21, 0.3).float().double(), randn((B, d), 22, 0.3).float().double()
    x[B - 1] = x[1]                                                             # equal rows at two positions: a pair of term 1

    def fn(dt):
        xx, yy = leaf(x, dt), leaf(y, dt)
        uni, ali, ali3 = ref_uniformity(xx), ref_alignment(xx, yy), ref_alignment(xx, yy, 3)
        (uni + 2 * ali + 3 * ali3).backward()
        return {'uniformity': uni.detach(), 'alignment': ali.detach(), 'alignment alpha=3': ali3.detach(), 'dx': xx.grad, 'dy': yy.grad}
    r64, r32 = both_precisions(fn)
    xx, yy = gpu(x).requires_grad_(True), gpu(y).requires_grad_(True)
    uni, ali, ali3 = loss_utils.uniformity(xx), loss_utils.alignment(xx, yy), loss_utils.alignment(xx, yy, alpha=3)
    (uni + 2 * ali + 3 * ali3).backward()
    got = {'uniformity': uni.detach(), 'alignment': ali.detach(), 'alignment alpha=3': ali3.detach(), 'dx': xx.grad, 'dy': yy.grad}
    for name in got:
        check('dense B=%d d=%d %s' % (B, d, name), got[name], r64[name], r32[name])


@pytest.mark.gpu
def test_au_two_runs_give_the_same_bits():
    table = loss_table(64)
    ancs, poss = loss_indices(1000)
    first, second = (run_loss(table, ancs, poss, 1.0 / 3.0, 2.0) for _ in range(2))
    for name in first:
        assert torch.equal(first[name], second[name]), name


@pytest.mark.gpu
def test_a_batch_of_one_is_nan_like_the_reference_and_launches_no_kernel(monkeypatch):
    from sslrec_amd import _lib, ops
    lib = _lib.load()

    def not_me(*a):
        raise AssertionError('B = 1 reached the library')
    monkeypatch.setattr(lib, 'sslrec_au_fwd_f32', not_me, raising=False)
    monkeypatch.setattr(lib, 'sslrec_au_bwd_f32', not_me, raising=False)
    table = loss_table(32)
    ancs, poss = lt(np.array([5])), lt(np.array([9]))
    ref = ref_loss(table[:N_USER], table[N_USER:], ancs, poss, 2.0)
    assert torch.isnan(ref[0]) and torch.isnan(ref[2]) and torch.isfinite(ref[1])
    t_ = gpu(table).requires_grad_(True)
    loss, align, uniform = ops.align_uniform_loss_stacked(t_, N_USER, ancs.to(DEV), poss.to(DEV), 2.0)
    assert torch.isnan(loss) and torch.isnan(uniform)
    assert abs(float(align) - float(ref[1])) <= 1e-5 * abs(float(ref[1]))
    loss.backward()
    torch.cuda.synchronize()
    assert tuple(t_.grad.shape) == tuple(table.shape)


# ---------------------------------------------------------------------------------------------------------------------
# GPU tests: the whole step, evaluation and training
# ---------------------------------------------------------------------------------------------------------------------
def tiny_fills(d):
    return [randn((TINY_U, d), 300, 0.1).float().double(), randn((TINY_I, d), 301, 0.1).float().double()]


def tiny_model(d, L):
    from sslrec_amd.models.bulid_model import build_model
    dh = tiny_handler(DEV, {'model': {'embedding_size': d, 'layer_num': L}})
    model = build_model(dh).to(DEV)
    with torch.no_grad():
        for p, f in zip(model.parameters(), tiny_fills(d)):
            p.copy_(gpu(f))
    return dh, model


def tiny_batch():
    rng = np.random.RandomState(5)
    return lt(rng.randint(0, 120, 256)), lt(rng.randint(0, TINY_I, 256)), lt(rng.randint(0, TINY_I, 256))


def tiny_graph(dh):
    adj = dh.torch_adj
    return adj._values(), adj._indices()[0], adj._indices()[1]


@functools.lru_cache(maxsize=None)
def ref_tiny_step(d, L):
    from sslrec_amd.config.configurator import configs
    dh = tiny_handler('cpu', {'model': {'embedding_size': d, 'layer_num': L}})
    gamma = configs['model']['gamma']
    g = tiny_graph(dh)
    fills, (ancs, poss, _) = tiny_fills(d), tiny_batch()

    def fn(dt):
        ue, ie = (leaf(f, dt) for f in fills)
        mean = ref_forward(ue, ie, (g[0].to(dt), g[1], g[2]), L)
        loss, align, uniform = ref_loss(mean[:TINY_U], mean[TINY_U:], ancs, poss, gamma)
        loss.backward()
        return {'loss': loss.detach(), 'align_loss': align.detach(), 'uniform_loss': uniform.detach(), 'd user_embeds': ue.grad,
                'd item_embeds': ie.grad}
    return both_precisions(fn)


@pytest.mark.gpu
@pytest.mark.parametrize('d,L', [(32, 2), (64, 3)])
def test_directau_whole_step(d, L):
    torch.manual_seed(91)
    dh, model = tiny_model(d, L)
    cpu_state = torch.get_rng_state()
    loss, parts = model.cal_loss([b.to(DEV) for b in tiny_batch()])
    loss.backward()
    assert torch.equal(torch.get_rng_state(), cpu_state)                        # the step draws nothing
    assert sorted(parts) == ['align_loss', 'uniform_loss']
    got = {'loss': loss.detach()}
    got.update({k: v.detach() for k, v in parts.items()})
    got.update({'d ' + n: p.grad for n, p in model.named_parameters()})
    r64, r32 = ref_tiny_step(d, L)
    for name in ('loss', 'align_loss', 'uniform_loss', 'd user_embeds', 'd item_embeds'):
        check('%s d=%d L=%d' % (name, d, L), got[name], r64[name], r32[name])


class _Log:
    def log(self, *a, **k):
        pass

    log_loss = log_eval = log


@pytest.mark.gpu
def test_directau_evaluation_and_checkpoint(tmp_path, monkeypatch):
    from sslrec_amd.config.configurator import configs
    from sslrec_amd.trainer.trainer import Trainer
    d, L = 32, 2
    torch.manual_seed(5)
    g = tiny_graph(tiny_handler('cpu'))
    dh, model = tiny_model(d, L)
    final = ref_forward(*tiny_fills(d), (g[0].double(), g[1], g[2]), L)
    users = lt(np.array([0, 5, 17, 299, 150, 5]))
    trn = dh.trn_mat.tocsr()
    mask = torch.from_numpy(trn[users.numpy()].toarray()).double()
    scores = (final[:TINY_U][users] @ final[TINY_U:].T) * (1 - mask) - 1e8 * mask
    model.eval()
    cpu_state = torch.get_rng_state()
    got = model.full_predict((users.to(DEV), mask.float().to(DEV)))
    assert torch.equal(torch.get_rng_state(), cpu_state)                        # draw-free
    assert torch.allclose(got.cpu().double(), scores, rtol=1e-4, atol=1e-5)     # the VALUES: final_embeds holds the mean of the layers
    cached = model.final_embeds
    assert cached is not None and not model.is_training
    assert torch.allclose(cached.cpu().double(), final, rtol=1e-4, atol=1e-6)
    rowptr, col = lt(trn.indptr).to(DEV), lt(trn.indices).to(DEV)
    top = model.predict_topk(users.to(DEV), 10, (rowptr, col)).cpu()
    assert model.final_embeds is cached                                         # the second evaluation call reuses the tables
    assert torch.allclose(scores.gather(1, top), scores.topk(10).values, rtol=1e-4, atol=1e-5)
    # save_model / load_model round trip
    trainer = Trainer(dh, _Log())
    _, fresh = tiny_model(d, L)
    with torch.no_grad():
        fresh.user_embeds.zero_()
    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(configs['train'], 'save_model', True)
    trainer.save_model(model)
    saved = list((tmp_path / 'checkpoint' / 'directau').glob('*.pth'))
    assert len(saved) == 1
    monkeypatch.setitem(configs['train'], 'pretrain_path', str(saved[0]))
    trainer.load_model(fresh)
    for (n, p), (_, q) in zip(model.named_parameters(), fresh.named_parameters()):
        assert torch.equal(p, q), n


@pytest.mark.gpu
def test_directau_trains_two_epochs_through_the_trainer():
    from sslrec_amd.config.configurator import configs, load_config
    from sslrec_amd.data_utils.build_data_handler import build_data_handler
    from sslrec_amd.models.bulid_model import build_model
    from sslrec_amd.trainer.trainer import Trainer
    load_config('directau', device=DEV, overrides={'data': {'synthetic': 'tiny'}, 'train': {'epoch': 2, 'test_step': 1, 'batch_size': 512}})
    torch.manual_seed(2023)
    np.random.seed(2023)
    dh = build_data_handler()
    dh.load_data()
    model = build_model(dh).to(DEV)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    trainer = Trainer(dh, _Log())
    trainer.train(model)
    result = trainer.evaluate(model)
    assert all(np.isfinite(v).all() for v in result.values()) and set(result) == set(configs['test']['metrics'])
    for n, p in model.named_parameters():
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), before[n]), n
