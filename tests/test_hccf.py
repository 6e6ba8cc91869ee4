"""HCCF: the fused hypergraph layer (sslrec_amd/csrc/hyper.hip, ops.hyper_propagate_stacked / hyper_keep_mask), the spec-nodes InfoNCE
(loss_utils.cal_infonce_loss_spec_nodes) and the model (sslrec_amd/models/general_cf/hccf.py).

Yardstick of the GPU tests, as in tests/test_dccf.py: a float64 torch restatement of the reference's expressions
(models/general_cf/hccf.py:38-88, :100-108, models/loss_utils.py:42-51) written out below, gradients by torch autograd, fed the dropout
mask of ops.hyper_keep_mask and, for EdgeDrop, the draws of rng.philox_uniforms (device_rng mode).  The same restatement runs in fp32 on
the CPU; its error against float64 is measured per tensor as max|x - ref| / max|ref|, and the kernels may be at most 4 x as far off, with
a floor of 8 * 2^-23.  Both errors are printed per tensor.

LeakyReLU's derivative jumps at 0, so every fixture asserts on the CPU that each float64 pre-activation (Q = A^T X and P = A H) is
further from 0 than 64 * 2^-23 times the sum of the absolute products behind it.  The fixtures get there by construction rather than by
luck with a seed.  In the layer fixtures E[n, j] and X[n, j] have sign r_n s_j and W[j, k] has sign s_j c_k (r, s, c random signs), so
(E W)[n, k] is r_n c_k times a sum of positive products, Q[k, j] = sum_n A[n, k] X[n, j] has sign c_k s_j and P[n, j] = sum_k A[n, k]
H[k, j] has sign r_n s_j: no sum cancels to rounding level, and the slopes act'(H) and act'(Y) change along k, along the rows and
along the columns, so a kernel that read a slope from the wrong row of Y or the wrong k of H would fail.  The whole-step fixtures
carry s_j and c_k only (the adjacency mixes rows, so row signs would cancel in the second layer's input): H has mixed signs along
k, Y one sign per column.  A pre-activation with no product behind it at all (at K = 4 and keep_rate 0.5 one row in 16 loses all its
hyperedges) is exactly 0 in every precision and is left out of the condition.

The whole step with the DEFAULT InfoNCE arithmetic is held to the same bound where it holds; a tensor on the cl path that exceeds it is
held to DESIGN §2's whole-step bars instead (losses rtol 1e-5, gradients rtol 1e-4 / atol 1e-7).  With infonce_precision = fp32 the 4 x
bound applies to everything."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

N_USER, N_ITEM = 700, 500
N_NODE = N_USER + N_ITEM
FLOOR = 8 * 2.0 ** -23
MARGIN = 64 * 2.0 ** -23
DEV = 'cuda:0'
STATE_SEED, STREAM = 4242, 3


def randn(shape, seed, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def signs(d, seed=7):
    return torch.from_numpy(np.random.RandomState(seed).choice([-1.0, 1.0], d))


def signed(shape, seed, s, axis, lo=0.05, scale=0.3):
    """entries of magnitude lo + |N(0, scale)|, the sign of s along `axis`"""
    mag = lo + randn(shape, seed, scale).abs()
    return (mag * (s[None, :] if axis == 1 else s[:, None])).float().double()       # exactly representable in fp32


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
    print('%-30s kernel %.3e  fp32 torch %.3e  (%.2f / %.2f units of 2^-23 max|ref|)  bound %.3e' % (name, e, e32, e * 2 ** 23, e32 * 2 ** 23, bound))
    assert torch.isfinite(got).all(), name
    assert e <= bound, '%s: kernel error %.3e > bound %.3e (fp32 torch: %.3e)' % (name, e, bound, e32)


def both_precisions(fn):
    return fn(torch.float64), fn(torch.float32)


def philox(advances=1, seed=STATE_SEED):
    from sslrec_amd.rng import PhiloxState
    st = PhiloxState(DEV, seed=seed)
    for _ in range(advances):
        st.advance()
    return st


# ---------------------------------------------------------------------------------------------------------------------
# the restatement (any dtype, CPU)
# ---------------------------------------------------------------------------------------------------------------------
def ref_hgnn(a, x, leaky, margins):
    """hccf.py:105-107; margins collects min |pre-activation| / sum |products| of Q and P"""
    q = a.T @ x
    h = F.leaky_relu(q, leaky)
    p = a @ h
    if margins is not None and a.numel() and x.numel():
        with torch.no_grad():
            for pre, behind in ((q, a.abs().T @ x.abs()), (p, a.abs() @ h.abs())):
                some = behind > 0          # (a row whose K entries were all dropped has NO product behind it: exactly 0 in every precision,
                if some.any():             #  and both torch and the kernels take the slope `leaky` there -- nothing to disagree about)
                    margins.append(float((pre.abs()[some] / behind[some]).min()))
    return F.leaky_relu(p, leaky)


def ref_hyper(x, e, n_user, w_u, w_i, mult, leaky, keep_rate, mask, margins=None):
    """hccf.py:43-44, 48-49, 51 with F.dropout's mask given: kept entries are scaled by 1 / keep_rate"""
    out = []
    for rows, w in ((slice(0, n_user), w_u), (slice(n_user, None), w_i)):
        a = e[rows] @ w * mult
        if mask is not None:
            a = a * mask[rows].to(a.dtype) / keep_rate
        out.append(ref_hgnn(a, x[rows], leaky, margins))
    return torch.concat(out, dim=0)


def ref_spmm(vals, heads, tails, x, n_rows):
    return torch.zeros(n_rows, x.shape[1], dtype=x.dtype).index_add(0, heads, vals[:, None] * torch.index_select(x, 0, tails))


def ref_spec_nodes(embeds1, embeds2, nodes, temp):
    """loss_utils.py:42-51"""
    embeds1 = F.normalize(embeds1 + 1e-8, p=2)
    embeds2 = F.normalize(embeds2 + 1e-8, p=2)
    pck1, pck2 = embeds1[nodes], embeds2[nodes]
    nume = torch.exp(torch.sum(pck1 * pck2, dim=-1) / temp)
    deno = torch.exp(pck1 @ embeds2.T / temp).sum(-1) + 1e-8
    return -torch.log(nume / deno).mean()


def ref_step(params, n_user, L, g, edge_masks, hyper_masks, batch, cfg, margins=None):
    """hccf.py:38-88"""
    ue, ie, w_u, w_i = params
    g_vals, g_heads, g_tails = g
    keep = cfg['keep_rate']
    e0 = torch.concat([ue, ie], dim=0)
    lst, gcn, hyp = [e0], [], []
    for l in range(L):
        vals = g_vals if edge_masks is None else g_vals * edge_masks[l].to(g_vals.dtype) / keep          # EdgeDrop(resize_val=True)
        gcn.append(ref_spmm(vals, g_heads, g_tails, lst[-1], e0.shape[0]))
        hyp.append(ref_hyper(lst[-1], e0, n_user, w_u, w_i, cfg['mult'], cfg['leaky'], keep, None if hyper_masks is None else hyper_masks[l],
                             margins))
        lst.append(gcn[-1] + hyp[-1])
    final = sum(lst)
    if batch is None:
        return final
    ancs, poss, negs = batch
    a, p, n = final[:n_user][ancs], final[n_user:][poss], final[n_user:][negs]
    bpr = -((a * p).sum(-1) - (a * n).sum(-1)).sigmoid().log().mean()
    cl = 0
    for l in range(L):
        e1, e2 = gcn[l].detach(), hyp[l]
        cl = cl + ref_spec_nodes(e1[:n_user], e2[:n_user], torch.unique(ancs), cfg['temperature']) \
            + ref_spec_nodes(e1[n_user:], e2[n_user:], torch.unique(poss), cfg['temperature'])
    reg = sum(w.norm(2).square() for w in params) * cfg['reg_weight']
    cl = cl * cfg['cl_weight']
    return bpr + reg + cl, bpr, reg, cl, final


# ---------------------------------------------------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------------------------------------------------
def test_hyper_entry_points_reject_bad_arguments_without_a_gpu():
    from sslrec_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)       # a non-null HOST address: a call that got as far as a launch would fault, these return before
    bad = _lib.E_BADARG
    ws = lib.sslrec_hyper_ws_bytes

    def fwd(X=p, E=p, N=4, n_split=2, d=32, W_u=p, W_i=p, K=8, mult=1.0, leaky=0.5, keep=0.5, state=p, H_u=p, H_i=p, Y=p, w=p):
        return lib.sslrec_hyper_fwd_f32(X, E, N, n_split, d, W_u, W_i, K, mult, leaky, keep, state, 1, H_u, H_i, Y, w, None)

    def bwd(X=p, E=p, dY=p, Y=p, N=4, n_split=2, d=32, W_u=p, W_i=p, H_u=p, H_i=p, K=8, leaky=0.5, keep=0.5, state=p, dX=p, dE=p, dW_u=p,
            dW_i=p, w=p):
        return lib.sslrec_hyper_bwd_f32(X, E, dY, Y, N, n_split, d, W_u, W_i, H_u, H_i, K, 1.0, leaky, keep, state, 1, dX, dE, dW_u, dW_i, w, None)
    for name in ('X', 'E', 'W_u', 'W_i', 'H_u', 'H_i', 'Y', 'w', 'state'):
        assert fwd(**{name: None}) == bad, name
    for name in ('X', 'E', 'dY', 'Y', 'W_u', 'W_i', 'H_u', 'H_i', 'dX', 'dE', 'dW_u', 'dW_i', 'w', 'state'):
        assert bwd(**{name: None}) == bad, name
    for d in (0, 16, 48, 256):
        assert fwd(d=d) == bad and bwd(d=d) == bad and ws(4, 2, d, 8) == 0
    for k in (0, -1, 257):
        assert fwd(K=k) == bad and bwd(K=k) == bad and ws(4, 2, 32, k) == 0
    assert fwd(d=128, K=129) == bad and bwd(d=128, K=129) == bad and ws(4, 2, 128, 129) == 0      # two [d, K] matrices exceed LDS
    assert ws(4, 2, 128, 128) > 0 and ws(4, 2, 64, 256) > 0
    for n_split in (-1, 5):
        assert fwd(n_split=n_split) == bad and bwd(n_split=n_split) == bad and ws(4, n_split, 32, 8) == 0
    for leaky in (0.0, -0.5, float('nan')):
        assert fwd(leaky=leaky) == bad and bwd(leaky=leaky) == bad
    for keep in (0.0, -0.1, 1.5, float('nan')):
        assert fwd(keep=keep) == bad and bwd(keep=keep) == bad
    assert fwd(N=-1, n_split=0) == bad
    assert fwd(N=0, n_split=0, W_u=None, W_i=None, H_u=None, H_i=None, w=None, keep=1.0, state=None) == 0      # N = 0: success without a launch
    assert bwd(N=0, n_split=0, W_u=None, W_i=None, H_u=None, H_i=None, dW_u=None, dW_i=None, w=None, keep=1.0, state=None) == 0
    assert ws(1200, 700, 32, 128) >= (6 + 4) * 2 * 32 * 128 * 4


def test_hyper_ops_and_spec_nodes_loss_refuse_bad_arguments_before_loading_the_library(monkeypatch):
    from sslrec_amd import _lib, ops
    from sslrec_amd.models.loss_utils import cal_infonce_loss_spec_nodes

    def no_load():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_lib, 'load', no_load)
    x, w = torch.zeros(8, 32), torch.zeros(32, 16)
    with pytest.raises(RuntimeError, match='HIP device only'):
        ops.hyper_propagate_stacked(x, x, 3, w, w, 1.0, 0.5, 1.0)
    with pytest.raises(RuntimeError, match='HIP device only'):
        cal_infonce_loss_spec_nodes(x, x, torch.arange(4), 0.1)

    class Meta:                     # shape checks come before any device work: a stand-in that claims to be on the GPU
        is_cuda = True

        def __init__(self, *shape):
            self.shape = shape

        def dim(self):
            return len(self.shape)
    xm, wm = Meta(8, 32), Meta(32, 16)
    with pytest.raises(ValueError, match='leaky'):
        ops.hyper_propagate_stacked(xm, xm, 3, wm, wm, 1.0, 0.0, 1.0)
    with pytest.raises(ValueError, match='leaky'):
        ops.hyper_propagate_stacked(xm, xm, 3, wm, wm, 1.0, -0.2, 1.0)
    for keep in (0.0, 1.01, -1.0):
        with pytest.raises(ValueError, match='keep_rate'):
            ops.hyper_propagate_stacked(xm, xm, 3, wm, wm, 1.0, 0.5, keep)
    with pytest.raises(ValueError, match='rng'):
        ops.hyper_propagate_stacked(xm, xm, 3, wm, wm, 1.0, 0.5, 0.5)
    for bad in ((xm, Meta(8, 64), 3, wm, wm), (xm, xm, 9, wm, wm), (xm, xm, -1, wm, wm), (xm, xm, 3, wm, Meta(32, 8)), (xm, xm, 3, Meta(16, 16), Meta(16, 16)),
                (xm, xm, 3, Meta(32, 257), Meta(32, 257)), (Meta(8), Meta(8), 3, wm, wm)):
        with pytest.raises(ValueError, match='hyper_propagate_stacked'):
            ops.hyper_propagate_stacked(*bad, 1.0, 0.5, 1.0)


def tiny_handler(device, over=None):
    from helpers import FixtureHandler
    from sslrec_amd.config.configurator import load_config
    from sslrec_amd.data_utils import synth
    overrides = {'data': {'synthetic': 'tiny'}}
    overrides.update(over or {})
    load_config('hccf', device=device, overrides=overrides)
    return FixtureHandler(synth.make_dataset('tiny', 2023)).load_adj_only()


def test_hccf_builds_from_its_config_with_the_reference_draw_order():
    from torch import nn
    from sslrec_amd.config.configurator import configs
    from sslrec_amd.models.bulid_model import build_model
    dh = tiny_handler('cpu')
    m = configs['model']
    assert (m['layer_num'], m['hyper_num'], m['embedding_size'], m['keep_rate']) == (2, 128, 32, 0.5)
    assert (m['reg_weight'], m['cl_weight'], m['temperature'], m['mult'], m['leaky']) == (1.0e-7, 1.0, 0.1, 1.0, 1.0)
    torch.manual_seed(77)
    model = build_model(dh)
    after_build = torch.get_rng_state()
    assert type(model).__name__ == 'HCCF'
    assert {n: tuple(p.shape) for n, p in model.named_parameters()} == {
        'user_embeds': (300, 32), 'item_embeds': (220, 32), 'user_hyper_embeds': (32, 128), 'item_hyper_embeds': (32, 128)}
    torch.manual_seed(77)                                                       # the reference's draws, hccf.py:27-31
    init = nn.init.xavier_uniform_
    want = [init(torch.empty(300, 32)), init(torch.empty(220, 32)), init(torch.empty(32, 128)), init(torch.empty(32, 128))]
    for (n, p), w in zip(model.named_parameters(), want):
        assert torch.equal(p, w), n
    # ... and nothing more: the seed of the model's own dropout state is read (torch.initial_seed), not drawn, so EdgeDrop's parity
    # masks and everything after them get the numbers the reference's run gets
    assert torch.equal(torch.get_rng_state(), after_build) and model._hyper_seed == 77
    assert model.device_rng is None and model.edge_drop.resize_val


# ---------------------------------------------------------------------------------------------------------------------
# GPU tests: the layer
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layer_fixture(d, k, leaky, keep, mult=1.0, n=N_NODE, n_split=N_USER, same=False):
    """inputs, the mask the kernels compute, and the float64 / fp32 restatement of one layer with all its gradients"""
    from sslrec_amd import ops
    s, rs = signs(d), signs(n, 8)[:, None]                                      # column signs s_j, row signs r_n, hyperedge signs c_k
    e = signed((n, d), 1, s, 1) * rs
    x = e if same else signed((n, d), 2, s, 1) * rs
    w_u, w_i, r = signed((d, k), 3, s, 0) * signs(k, 9)[None, :], signed((d, k), 4, s, 0) * signs(k, 10)[None, :], randn((n, d), 5)
    mask = None if keep == 1.0 else ops.hyper_keep_mask(philox(), STREAM, n, k, keep).cpu()

    def fn(dt):
        margins = [] if dt == torch.float64 else None
        ee, wu, wi = leaf(e, dt), leaf(w_u, dt), leaf(w_i, dt)
        xx = ee if same else leaf(x, dt)
        y = ref_hyper(xx, ee, n_split, wu, wi, mult, leaky, keep, mask, margins)
        (y * r.to(dt)).sum().backward()
        if margins:
            assert min(margins) > MARGIN, 'a pre-activation within rounding of 0: %.3e' % min(margins)
        out = {'Y': y.detach(), 'dE': ee.grad, 'dW_u': wu.grad, 'dW_i': wi.grad}
        if not same:
            out['dX'] = xx.grad
        return out
    return (x, e, w_u, w_i, r, mask) + both_precisions(fn)


def run_layer(x, e, w_u, w_i, r, n_split, mult, leaky, keep, same=False):
    from sslrec_amd import ops
    ee, wu, wi = (gpu(v).requires_grad_(True) for v in (e, w_u, w_i))
    xx = ee if same else gpu(x).requires_grad_(True)
    y = ops.hyper_propagate_stacked(xx, ee, n_split, wu, wi, mult, leaky, keep, None if keep == 1.0 else (philox(), STREAM))
    assert tuple(y.shape) == tuple(e.shape)
    (y * gpu(r)).sum().backward()
    out = {'Y': y.detach(), 'dE': ee.grad, 'dW_u': wu.grad, 'dW_i': wi.grad}
    if not same:
        out['dX'] = xx.grad
    return out


def check_layer(tag, d, k, leaky, keep, mult=1.0, n=N_NODE, n_split=N_USER, same=False):
    x, e, w_u, w_i, r, _, r64, r32 = layer_fixture(d, k, leaky, keep, mult, n, n_split, same)
    got = run_layer(x, e, w_u, w_i, r, n_split, mult, leaky, keep, same)
    for name in r64:
        if r64[name].numel() == 0 or float(r64[name].abs().max()) == 0.0:      # (an empty range: its matrix gets a zero gradient)
            assert got[name].numel() == r64[name].numel() and torch.all(got[name] == 0), name
            continue
        check('%s %s%s' % (tag, name, ' X is E' if same else ''), got[name], r64[name], r32[name])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('keep', [1.0, 0.5])
@pytest.mark.parametrize('leaky', [1.0, 0.5, 0.01])
@pytest.mark.parametrize('d,k', [(32, 128), (64, 128), (128, 128), (32, 100), (64, 4), (32, 256), (48, 128), (128, 256), (64, 256)])
def test_hyper_layer_forward_and_all_five_gradients(d, k, leaky, keep):
    mult = 2.5 if (d, k, leaky, keep) == (64, 128, 0.5, 0.5) else 1.0
    tag = 'd=%d K=%d leaky=%g keep=%g' % (d, k, leaky, keep)
    check_layer(tag, d, k, leaky, keep, mult)                   # Y, dX, dE (X distinct from E), dW_u, dW_i
    check_layer(tag, d, k, leaky, keep, mult, same=True)        # X is E: autograd adds dX and dE


@pytest.mark.gpu
@pytest.mark.parametrize('n,n_split', [(N_NODE, 0), (N_NODE, N_NODE), (1, 1), (1, 0), (33, 20), (96, 32), (64, 32)])
def test_hyper_layer_edge_shapes(n, n_split):
    check_layer('N=%d n_user=%d' % (n, n_split), 32, 128, 0.5, 0.5, 1.0, n, n_split)
    check_layer('N=%d n_user=%d' % (n, n_split), 64, 100, 0.01, 1.0, 1.0, n, n_split, same=True)


@pytest.mark.gpu
def test_hyper_layer_without_rows_returns_empty_tensors():
    from sslrec_amd import ops
    d, k = 32, 16
    xx = torch.zeros(0, d, device=DEV, requires_grad=True)
    ee = torch.zeros(0, d, device=DEV, requires_grad=True)
    wu, wi = (gpu(randn((d, k), s)).requires_grad_(True) for s in (1, 2))
    y = ops.hyper_propagate_stacked(xx, ee, 0, wu, wi, 1.0, 0.5, 0.5, (philox(), STREAM))
    assert tuple(y.shape) == (0, d)
    y.sum().backward()
    assert tuple(xx.grad.shape) == (0, d) and tuple(ee.grad.shape) == (0, d) and torch.all(wu.grad == 0) and torch.all(wi.grad == 0)


@pytest.mark.gpu
def test_hyper_dropout_mask_is_the_one_hyper_keep_mask_writes_out():
    from sslrec_amd import ops
    d, k, leaky, keep = 32, 128, 0.5, 0.5
    x, e, w_u, w_i, r, mask, r64, r32 = layer_fixture(d, k, leaky, keep)
    got = run_layer(x, e, w_u, w_i, r, N_USER, 1.0, leaky, keep)
    check('mask Y', got['Y'], r64['Y'], r32['Y'])
    other = ref_hyper(x, e, N_USER, w_u, w_i, 1.0, leaky, keep, ~mask)          # the complementary mask gives another layer altogether
    assert rel_err(got['Y'], other) > 1e-2
    # the kept fraction: 700 x 128 Bernoulli(keep) draws, within 5 standard deviations
    n_el = 700 * 128
    kept = int(mask[:700].sum())
    assert abs(kept - keep * n_el) <= 5 * (n_el * keep * (1 - keep)) ** 0.5, kept
    st = philox()
    m3 = ops.hyper_keep_mask(st, STREAM, N_NODE, k, keep)
    assert torch.equal(m3.cpu(), mask) and m3.dtype == torch.bool and tuple(m3.shape) == (N_NODE, k)
    m4 = ops.hyper_keep_mask(st, STREAM + 1, N_NODE, k, keep)
    assert 0.4 < float((m3 != m4).float().mean()) < 0.6                         # another stream: another mask
    st.advance()
    m5 = ops.hyper_keep_mask(st, STREAM, N_NODE, k, keep)
    assert 0.4 < float((m3 != m5).float().mean()) < 0.6                         # the next step: another mask
    # ... and the kernels follow: the same call one step later differs from the first
    xx, ee, wu, wi = (gpu(v) for v in (x, e, w_u, w_i))
    y_next = ops.hyper_propagate_stacked(xx, ee, N_USER, wu, wi, 1.0, leaky, keep, (st, STREAM))
    assert rel_err(y_next, r64['Y']) > 1e-2
    ref_next = ref_hyper(x, e, N_USER, w_u, w_i, 1.0, leaky, keep, m5.cpu())
    assert rel_err(y_next, ref_next) < 1e-5
    # K that is no multiple of 4: rows of the mask are 4 ceil(K / 4) uniforms apart
    m100 = ops.hyper_keep_mask(philox(), STREAM, N_NODE, 100, keep)
    assert tuple(m100.shape) == (N_NODE, 100) and torch.equal(m100[0], m3[0, :100]) and not torch.equal(m100[1], m3[1, :100])


@pytest.mark.gpu
@pytest.mark.parametrize('d,k', [(64, 128), (128, 128)])
def test_hyper_two_runs_give_the_same_bits(d, k):
    x, e, w_u, w_i, r, _, _, _ = layer_fixture(d, k, 0.5, 0.5)
    first, second = (run_layer(x, e, w_u, w_i, r, N_USER, 1.0, 0.5, 0.5) for _ in range(2))
    for name in first:
        assert torch.equal(first[name], second[name]), name


# ---------------------------------------------------------------------------------------------------------------------
# GPU tests: the loss
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('temp', [0.1, 1.0])
def test_spec_nodes_infonce_against_the_restatement(temp):
    from sslrec_amd.models.loss_utils import cal_infonce_loss_spec_nodes
    m, d = 220, 32
    e1, e2 = randn((m, d), 31, 0.4), randn((m, d), 32, 0.4)
    e1[17] = 0.0                                                                # a zero row in each table: normalize(0 + 1e-8)
    e2[40] = 0.0
    picks = lt(np.random.RandomState(3).randint(0, m, 300))
    picks[:2] = torch.tensor([17, 40])
    nodes = torch.unique(picks)                                                 # duplicate-free, as hccf.py:80-81 passes them

    def fn(dt):
        b = leaf(e2, dt)
        loss = ref_spec_nodes(e1.to(dt), b, nodes, temp)
        loss.backward()
        return {'loss': loss.detach(), 'd embeds2': b.grad}
    r64, r32 = both_precisions(fn)
    a, b = gpu(e1), gpu(e2).requires_grad_(True)
    loss = cal_infonce_loss_spec_nodes(a, b, nodes.to(DEV), temp, precision='fp32')
    loss.backward()
    assert a.grad is None                                                       # gradients reach only embeds2
    check('spec_nodes loss temp=%g' % temp, loss, r64['loss'], r32['loss'])
    check('spec_nodes d embeds2 temp=%g' % temp, b.grad, r64['d embeds2'], r32['d embeds2'])


# ---------------------------------------------------------------------------------------------------------------------
# GPU tests: the whole step, evaluation and training
# ---------------------------------------------------------------------------------------------------------------------
TINY_U, TINY_I = 300, 220
STEP_LEAKY = 0.5


def tiny_fills(d, K):
    s = signs(d, 11)
    # magnitudes at which a layer neither grows nor shrinks the table much: no sum cancels here, so Y ~ N K A^2 X with A ~ d E W
    return [signed((TINY_U, d), 300, s, 1, 0.02, 0.05), signed((TINY_I, d), 301, s, 1, 0.02, 0.05),
            signed((d, K), 302, s, 0, 0.001, 0.003) * signs(K, 12)[None, :], signed((d, K), 303, s, 0, 0.001, 0.003) * signs(K, 13)[None, :]]


def tiny_model(d, L, K, precision=None, device_rng=True):
    from sslrec_amd.models.bulid_model import build_model
    model_over = {'embedding_size': d, 'layer_num': L, 'hyper_num': K, 'leaky': STEP_LEAKY, 'device_rng': device_rng}
    if precision:
        model_over['infonce_precision'] = precision
    dh = tiny_handler(DEV, {'model': model_over})
    model = build_model(dh).to(DEV)
    with torch.no_grad():
        for p, f in zip(model.parameters(), tiny_fills(d, K)):
            p.copy_(gpu(f))
    return dh, model


def tiny_batch():
    rng = np.random.RandomState(5)
    return lt(rng.randint(0, 120, 256)), lt(rng.randint(0, TINY_I, 256)), lt(rng.randint(0, TINY_I, 256))


def tiny_graph(dh):
    """values, rows, cols in the adjacency's OWN entry order (uncoalesced, sorted by column: entry k is what EdgeDrop's draw k decides)"""
    adj = dh.torch_adj
    return adj._values(), adj._indices()[0], adj._indices()[1]


@functools.lru_cache(maxsize=None)
def ref_tiny_step(d, L, K, seed):
    """float64 and fp32 restatement of one cal_loss + backward on `tiny`, with the masks the step's Philox state gives: after
    _begin_step's advance, layer l draws EdgeDrop from stream 2 l + 1 and the hypergraph dropout from stream 2 l + 2"""
    from sslrec_amd import ops
    from sslrec_amd.config.configurator import configs
    from sslrec_amd.rng import philox_uniforms
    dh = tiny_handler('cpu', {'model': {'embedding_size': d, 'layer_num': L, 'hyper_num': K, 'leaky': STEP_LEAKY}})
    cfg = dict(configs['model'])
    g = tiny_graph(dh)
    st = philox(1, seed)
    keep = cfg['keep_rate']
    edge_masks = [(philox_uniforms(st, 2 * l + 1, g[0].numel()) + keep).floor().bool().cpu() for l in range(L)]
    hyper_masks = [ops.hyper_keep_mask(st, 2 * l + 2, TINY_U + TINY_I, K, keep).cpu() for l in range(L)]
    fills, batch = tiny_fills(d, K), tiny_batch()

    def fn(dt):
        margins = [] if dt == torch.float64 else None
        params = [leaf(f, dt) for f in fills]
        loss, bpr, reg, cl, _ = ref_step(params, TINY_U, L, (g[0].to(dt), g[1], g[2]), edge_masks, hyper_masks, batch, cfg, margins)
        loss.backward()
        if margins:
            assert min(margins) > MARGIN, 'a pre-activation within rounding of 0: %.3e' % min(margins)
        out = {'loss': loss.detach(), 'bpr_loss': bpr.detach(), 'reg_loss': reg.detach(), 'cl_loss': cl.detach()}
        out.update({'d ' + n: p.grad for n, p in zip(('user_embeds', 'item_embeds', 'user_hyper_embeds', 'item_hyper_embeds'), params)})
        return out
    return both_precisions(fn)


def run_tiny_step(d, L, K, precision):
    dh, model = tiny_model(d, L, K, precision)
    seed = int(model.device_rng.state[0].item())
    loss, parts = model.cal_loss([b.to(DEV) for b in tiny_batch()])
    loss.backward()
    got = {'loss': loss.detach()}
    got.update({k: v.detach() for k, v in parts.items()})
    got.update({'d ' + n: p.grad for n, p in model.named_parameters()})
    return seed, got


STEP_TENSORS = ('bpr_loss', 'reg_loss', 'cl_loss', 'loss', 'd user_embeds', 'd item_embeds', 'd user_hyper_embeds', 'd item_hyper_embeds')


@pytest.mark.gpu
@pytest.mark.parametrize('d,L,K', [(32, 2, 128), (64, 3, 16)])
def test_hccf_whole_step_fp32_infonce(d, L, K):
    torch.manual_seed(91)
    seed, got = run_tiny_step(d, L, K, 'fp32')
    r64, r32 = ref_tiny_step(d, L, K, seed)
    assert sorted(k for k in got if k.endswith('_loss')) == ['bpr_loss', 'cl_loss', 'reg_loss']
    for name in STEP_TENSORS:
        check('%s d=%d L=%d' % (name, d, L), got[name], r64[name], r32[name])


@pytest.mark.gpu
@pytest.mark.parametrize('d,L,K', [(32, 2, 128), (64, 3, 16)])
def test_hccf_whole_step_default_infonce(d, L, K):
    torch.manual_seed(91)
    seed, got = run_tiny_step(d, L, K, None)
    r64, r32 = ref_tiny_step(d, L, K, seed)
    for name in STEP_TENSORS:
        on_cl_path = name not in ('bpr_loss', 'reg_loss')
        try:
            check('%s d=%d L=%d' % (name, d, L), got[name], r64[name], r32[name])
        except AssertionError:
            if not on_cl_path:
                raise
            ref, x = r64[name], got[name].cpu().double()                        # DESIGN §2's whole-step bars
            rtol, atol = (1e-5, 0.0) if name.endswith('loss') else (1e-4, 1e-7)
            worst = float(((x - ref).abs() - rtol * ref.abs()).max())
            print('%-30s beyond 4 x fp32; whole-step bar rtol %g atol %g: worst excess %.3e' % (name, rtol, atol, worst))
            assert torch.allclose(x, ref, rtol=rtol, atol=atol), name


class _Log:
    def log(self, *a, **k):
        pass

    log_loss = log_eval = log


@pytest.mark.gpu
def test_hccf_evaluation_training_and_checkpoint(tmp_path, monkeypatch):
    from sslrec_amd.config.configurator import configs
    from sslrec_amd.trainer.trainer import Trainer
    d, L, K = 32, 2, 128
    torch.manual_seed(5)
    g = tiny_graph(tiny_handler('cpu'))
    dh, model = tiny_model(d, L, K, device_rng=False)                           # the model's own dropout state, EdgeDrop in parity mode
    assert model.device_rng is None
    cfg = dict(configs['model'])
    final = ref_step(tiny_fills(d, K), TINY_U, L, (g[0].double(), g[1], g[2]), None, None, None,
                     dict(cfg, keep_rate=1.0))                                  # evaluation: keep_rate 1.0, nothing drawn
    users = lt(np.array([0, 5, 17, 299, 150, 5]))
    trn = dh.trn_mat.tocsr()
    mask = torch.from_numpy(trn[users.numpy()].toarray()).double()
    scores = (final[:TINY_U][users] @ final[TINY_U:].T) * (1 - mask) - 1e8 * mask
    model.eval()
    cpu_state = torch.get_rng_state()
    got = model.full_predict((users.to(DEV), mask.float().to(DEV)))
    assert torch.equal(torch.get_rng_state(), cpu_state)                        # draw-free
    assert torch.allclose(got.cpu().double(), scores, rtol=1e-4, atol=1e-5)
    cached = model.final_embeds
    assert cached is not None and not model.is_training
    rowptr, col = lt(trn.indptr).to(DEV), lt(trn.indices).to(DEV)
    top = model.predict_topk(users.to(DEV), 10, (rowptr, col)).cpu()
    assert model.final_embeds is cached                                         # the second evaluation call reuses the tables
    assert torch.allclose(scores.gather(1, top), scores.topk(10).values, rtol=1e-4, atol=1e-5)
    # two epochs of three steps with the Trainer's optimizer change all four parameters; the losses stay finite
    trainer = Trainer(dh, _Log())
    trainer.create_optimizer(model)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    model.train()
    batch = [b.to(DEV) for b in tiny_batch()]
    seen = []
    for _ in range(2):
        for _ in range(3):
            trainer.optimizer.zero_grad()
            loss, _ = model.cal_loss(batch)
            loss.backward()
            trainer.optimizer.step()
            seen.append(float(loss.detach()))
    assert all(np.isfinite(seen)) and len(set(seen)) == len(seen)               # (a fresh mask every step)
    for n, p in model.named_parameters():
        assert not torch.equal(p.detach(), before[n]), n
    # save_model / load_model round trip
    _, fresh = tiny_model(d, L, K, device_rng=False)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(configs['train'], 'save_model', True)
    trainer.save_model(model)
    saved = list((tmp_path / 'checkpoint' / 'hccf').glob('*.pth'))
    assert len(saved) == 1
    monkeypatch.setitem(configs['train'], 'pretrain_path', str(saved[0]))
    trainer.load_model(fresh)
    for (n, p), (_, q) in zip(model.named_parameters(), fresh.named_parameters()):
        assert torch.equal(p, q), n


@pytest.mark.gpu
def test_hccf_trains_two_epochs_through_the_trainer():
    from sslrec_amd.config.configurator import configs, load_config
    from sslrec_amd.data_utils.build_data_handler import build_data_handler
    from sslrec_amd.models.bulid_model import build_model
    from sslrec_amd.trainer.trainer import Trainer
    load_config('hccf', device=DEV, overrides={'data': {'synthetic': 'tiny'}, 'train': {'epoch': 2, 'test_step': 1, 'batch_size': 512}})
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
