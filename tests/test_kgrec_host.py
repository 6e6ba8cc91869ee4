"""KGRec without a GPU: the yml, the parameter draws, the composed torch forms of ops.rel_mh_attention / ops.attn_hgcn_aggregate /
ops.rel_rationale in float64 against the restatement (tests/kgrec_reference.py) with gradcheck, the relation-aware sample and the three
masks against the reference's np.random.choice calls, the model's cal_loss on the CPU in float64 against model_loss on the recorded
selections, the trainer factory and the command line."""
import numpy as np
import pytest
import torch

import kgrec_reference as R

U, I, N_ENT, N_REL = 60, 50, 90, 9                      # kg-tiny


def cfg(overrides=None, dataset=None, model='kgrec'):
    from sslrec_amd.config.configurator import load_config
    return load_config(model, dataset=dataset, device='cpu', overrides=overrides)


def tiny_handler(model=None, train=None, name='kgrec'):
    from sslrec_amd.data_utils.data_handler_kg import DataHandlerKG
    cfg({'data': {'synthetic': 'kg-tiny'}, 'model': dict({'embedding_size': 32, 'mae_msize': 32}, **(model or {})),
         'train': dict({'batch_size': 128}, **(train or {})), 'test': {'batch_size': 32}}, model=name)
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
    assert c['optimizer'] == {'name': 'adam', 'lr': 1.0e-4, 'weight_decay': 0}
    train = {'trainer': 'trainer', 'epoch': 500, 'batch_size': 1024, 'save_model': True, 'loss': 'pairwise', 'test_step': 10,
             'reproducible': True, 'seed': 2020}
    assert {k: c['train'].get(k) for k in train} == train                           # (load_config adds its own defaults beside them)
    assert c['test'] == {'metrics': ['recall', 'ndcg'], 'k': [10, 20, 40], 'batch_size': 1024, 'eval_at_one_forward': True}
    assert c['data'] == {'type': 'kg', 'name': 'last-fm'}
    assert c['model'] == {'name': 'kgrec', 'layer_num': 2, 'decay_weight': 1.0e-5, 'embedding_size': 64, 'node_dropout': True,
                          'node_dropout_rate': 0.5, 'mess_dropout': True, 'mess_dropout_rate': 0.1, 'mae_coef': 0.1, 'mae_msize': 256,
                          'cl_coef': 0.001, 'tau': 0.2, 'cl_drop_ratio': 0.5, 'samp_func': 'torch'}
    assert c['tune'] == {'enable': False, 'hyperparameters': ['layer_num'], 'layer_num': [1, 2, 3]}


@pytest.mark.parametrize('seed', [3, 2020])
def test_parameter_names_shapes_and_draws(seed):
    from sslrec_amd.models.bulid_model import build_model
    dh = tiny_handler()
    torch.manual_seed(seed)
    model = build_model(dh)
    assert type(model).__name__ == 'KGRec' and type(model.gcn).__name__ == 'AttnHGCN' and type(model.contrast_fn).__name__ == 'Contrast'
    got = dict(model.named_parameters())
    want = R.draw_params(U + N_ENT, N_REL, 32, seed)
    assert list(got) == R.PARAM_NAMES
    for n in R.PARAM_NAMES:
        assert got[n].shape == want[n].shape and torch.equal(got[n].detach(), want[n]), n
    assert tuple(got['gcn.relation_emb'].shape) == (N_REL - 1, 32) and tuple(got['gcn.W_Q'].shape) == (32, 32)
    assert sorted(model.state_dict()) == sorted(R.PARAM_NAMES)
    model.load_state_dict({k: v + 0.5 for k, v in want.items()})
    assert (model.gcn.n_heads, model.gcn.d_k, model.contrast_fn.tau, model.mae_msize) == (2, 16, 0.2, 32)
    for name in ('cal_loss', 'generate', 'rating', 'full_predict', 'generate_global_attn_score', 'predict_topk'):
        assert callable(getattr(model, name))


# ---------------------------------------------------------------------------------------------------------------------
# the ops, composed, float64
# ---------------------------------------------------------------------------------------------------------------------
def small_graph():
    """7 entities, 24 edges: head 0 has a single edge, every edge of head 1 is masked, (2, 3) occurs under relations 0 and 1, entity 6 has
    no edge at all"""
    rng = np.random.RandomState(2)
    head = np.array([0, 1, 1, 2, 2] + list(rng.randint(2, 6, 19)))
    tail = np.array([4, 0, 3, 3, 3] + list(rng.randint(0, 6, 19)))
    rel = np.array([1, 0, 2, 0, 1] + list(rng.randint(0, 3, 19)))
    keep = rng.rand(24) < 0.7
    keep[0], keep[1:3], keep[3:5] = True, False, True
    return head, tail, rel, torch.from_numpy(keep)


@pytest.mark.parametrize('masked', [False, True])
def test_composed_rel_mh_attention_in_float64(masked):
    from sslrec_amd import ops
    from sslrec_amd.graph import RelGraph
    head, tail, rel, keep = small_graph()
    keep = keep if masked else None
    N, Rn, d = 7, 3, 8
    g = RelGraph(head, tail, rel, N, Rn)
    edges = tuple(torch.from_numpy(a) for a in (head, tail, rel))
    tens = [R.randn((N, d), 1), R.randn((N, d), 2), R.randn((Rn, d), 4)]
    w = R.randn((d, d), 6)
    go = R.randn((N, d), 5)
    a = [R.leaf(x, torch.float64) for x in tens]
    b = [R.leaf(x, torch.float64) for x in tens]
    ya, yb = ops.rel_mh_attention(g, *a, keep), R.rel_mh_attention(*b, edges, keep)
    (ya * go).sum().backward()
    (yb * go).sum().backward()
    assert_close('y', ya.detach(), yb.detach())
    for name, u, v in zip(('dx', 'dt', 'dr'), a, b):
        assert_close(name, u.grad, v.grad)
    assert bool((ya[6] == 0).all()) and torch.equal(ya[0].detach(), tens[0][4] * tens[2][1])          # no edge: 0; one edge: x[t] r[rel]
    if masked:
        assert bool((ya[1] == 0).all()) and bool(torch.isfinite(ya).all()) and all(bool(torch.isfinite(u.grad).all()) for u in a)
    # the literal shared_layer_agg, with its gathers through `@ W_Q`
    c = [R.leaf(x, torch.float64) for x in (tens[0], w, tens[2])]
    e = [R.leaf(x, torch.float64) for x in (tens[0], w, tens[2])]
    yc, ye = ops.attn_hgcn_aggregate(g, *c, keep), R.shared_layer_agg_kg(*e, edges, keep)
    (yc * go).sum().backward()
    (ye * go).sum().backward()
    assert_close('agg y', yc.detach(), ye.detach())
    for name, u, v in zip(('dx', 'dW_Q', 'dr'), c, e):
        assert_close('agg ' + name, u.grad, v.grad, 1e-11)
    # the backward of the formulas, written out per edge
    kept = np.ones(24, dtype=bool) if keep is None else keep.numpy()
    x, t, r = (z.numpy() for z in tens)
    G, Y = go.numpy(), ya.detach().numpy()
    half, cc = d // 2, 1 / np.sqrt(d // 2)
    dx, dt, dr = np.zeros((N, d)), np.zeros((N, d)), np.zeros((Rn, d))
    for hd in range(2):
        C = slice(hd * half, (hd + 1) * half)
        l = np.array([cc * (t[head[e_], C] * t[tail[e_], C] * r[rel[e_], C]).sum() for e_ in range(24)])
        for e_ in np.nonzero(kept)[0]:
            mine = kept & (head == head[e_])
            alpha = np.exp(l[e_] - l[mine].max()) / np.exp(l[mine] - l[mine].max()).sum()
            h_, t_, r_ = head[e_], tail[e_], rel[e_]
            dl = alpha * ((G[h_, C] * x[t_, C] * r[r_, C]).sum() - (G[h_, C] * Y[h_, C]).sum())
            dt[h_, C] += cc * dl * t[t_, C] * r[r_, C]
            dt[t_, C] += cc * dl * t[h_, C] * r[r_, C]
            dx[t_, C] += alpha * G[h_, C] * r[r_, C]
            dr[r_, C] += cc * dl * t[h_, C] * t[t_, C] + alpha * G[h_, C] * x[t_, C]
    for name, u, v in zip(('dx', 'dt', 'dr'), a, (dx, dt, dr)):
        assert_close(name + ' formula', u.grad, torch.from_numpy(v), 1e-11)
    assert torch.autograd.gradcheck(lambda *z: ops.rel_mh_attention(g, *z, keep), [R.leaf(z, torch.float64) for z in tens])
    with pytest.raises(ValueError):
        ops.rel_mh_attention(g, *a, torch.ones(23, dtype=torch.bool))
    with pytest.raises(ValueError):
        ops.rel_mh_attention(g, a[0], a[1], a[2][:2])
    # keep as uint8, and a strided table
    if masked:
        wide = torch.cat([tens[0], tens[0]], dim=1)[:, :d]
        assert not wide.is_contiguous()
        assert torch.equal(ops.rel_mh_attention(g, wide, tens[1], tens[2], keep.to(torch.uint8)), ya.detach())


@pytest.mark.parametrize('masked', [False, True])
def test_composed_rel_rationale_in_float64(masked):
    from sslrec_amd import ops
    from sslrec_amd.graph import RelGraph
    head, tail, rel, keep = small_graph()
    keep = keep if masked else None
    N, Rn, d = 7, 3, 8
    g = RelGraph(head, tail, rel, N, Rn)
    edges = tuple(torch.from_numpy(a) for a in (head, tail, rel))
    x, w, r = R.randn((N, d), 1), R.randn((d, d), 2), R.randn((Rn, d), 4)
    got = ops.rel_rationale(g, (x @ w).requires_grad_(True), r, keep)
    want = R.rel_rationale(x @ w, r, edges, keep)
    for name, u, v in zip(('score', 'logits', 'mean_head', 'mean_tail'), got, want):
        assert not u.requires_grad
        assert_close(name, u, v)
    # the literal norm_attn_computer on the kept edges, and the two scatter_mean of cal_loss
    sc, lg = R.norm_attn_computer(x, w, r, edges, keep)
    sel = torch.ones(24, dtype=torch.bool) if keep is None else keep
    h_k, t_k = edges[0][sel], edges[1][sel]
    assert_close('score literal', got[0][sel], sc)
    assert_close('logits literal', got[1][sel], lg)
    assert_close('mean_head literal', got[2], R.scatter_mean(sc, h_k, N))
    assert_close('mean_tail literal', got[3], R.scatter_mean(sc, t_k, N))
    assert bool((got[0][~sel] == 0).all()) and bool((got[1][~sel] == 0).all())
    assert float(got[0][0]) == 1.0 and float(got[2][6]) == 0 and float(got[3][6]) == 0            # one kept edge: 1; no edge: 0
    deg = torch.zeros(N, dtype=torch.float64).index_add_(0, h_k, torch.ones(h_k.numel(), dtype=torch.float64))
    assert_close('head sums', torch.zeros(N, dtype=torch.float64).index_add_(0, edges[0], got[0]), deg)
    if masked:
        assert float(got[2][1]) == 0 and bool(torch.isfinite(got[0]).all())                        # head 1: every edge masked


# ---------------------------------------------------------------------------------------------------------------------
# the sample and the three masks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 7])
def test_sample_and_masks_follow_the_reference(seed):
    from sslrec_amd.models.bulid_model import build_model
    dh = tiny_handler()
    torch.manual_seed(1)
    model = build_model(dh)
    edge_type = np.asarray(dh.kg_edges)[:, 2].astype(np.int64)
    E = edge_type.size
    assert edge_type.min() == 1 and edge_type.max() == N_REL - 1
    np.random.seed(seed)
    torch.manual_seed(seed)
    model.cal_loss(tiny_batch(dh))
    np_after = np.random.get_state()
    np.random.seed(seed)
    want = R.relation_aware_edge_sampling(edge_type, N_REL, 0.5)
    sample_ids = model.last_sample_ids.numpy()
    assert np.array_equal(sample_ids, want)
    n_s = sample_ids.size
    counts = np.bincount(edge_type, minlength=N_REL)
    assert n_s == sum(int(counts[r] * 0.5) for r in range(1, N_REL - 1)) and counts[N_REL - 1] > 0
    assert not np.any(edge_type[sample_ids] == N_REL - 1) and np.unique(sample_ids).size == n_s          # the last type is never sampled
    # the random group of the MAE mask is the next draw of numpy's generator
    rand_pos = np.random.choice(n_s, size=32, replace=False)
    assert all(np.array_equal(a, b) for a, b in zip(np_after, np.random.get_state()))
    s_keep = np.zeros(E, dtype=bool)
    s_keep[sample_ids] = True
    enc, cl, masked = model.last_enc_keep.numpy().astype(bool), model.last_cl_keep.numpy().astype(bool), model.last_masked_ids.numpy()
    assert n_s - 2 * 32 <= enc.sum() <= n_s - 32 and cl.sum() == n_s - int(0.5 * n_s)
    assert not np.any(enc & ~s_keep) and not np.any(cl & ~s_keep)
    assert np.array_equal(np.sort(masked), np.nonzero(s_keep & ~enc)[0]) and 32 <= masked.size <= 64
    assert np.all(np.isin(sample_ids[rand_pos], masked))
    # masked edges in position order, as edge_index[:, mask] lists them
    pos = {e: i for i, e in enumerate(sample_ids)}
    assert [pos[e] for e in masked] == sorted(pos[e] for e in masked)
    ui_keep, cl_ui = model.last_ui_keep.numpy(), model.last_cl_ui_ids.numpy()
    assert ui_keep.size == 400 and np.all(ui_keep[cl_ui]) and np.unique(cl_ui).size == cl_ui.size == int(0.5 * ui_keep.sum())
    assert sorted(model.last_rand_item.tolist()) == list(range(I))


def test_samp_func_np_draws_with_numpys_choice():
    from sslrec_amd.models.bulid_model import build_model
    dh = tiny_handler(model={'samp_func': 'np'})
    torch.manual_seed(1)
    model = build_model(dh)
    np.random.seed(3)
    torch.manual_seed(3)
    loss, _ = model.cal_loss(tiny_batch(dh))
    cl_ui = model.last_cl_ui_ids.numpy()
    assert bool(torch.isfinite(loss)) and np.unique(cl_ui).size == cl_ui.size == int(0.5 * int(model.last_ui_keep.sum()))


# ---------------------------------------------------------------------------------------------------------------------
# the model's step
# ---------------------------------------------------------------------------------------------------------------------
def restatement_inputs(model, dh, dt):
    """what model_loss needs, from the selections the step recorded (tensors on the CPU)"""
    adj = dh.interact_mat.cpu()
    idx, val = adj._indices(), adj._values().to(dt)
    ui_keep = model.last_ui_keep.cpu()
    cl_ids = model.last_cl_ui_ids.cpu()
    rate, cl_rate = 1 - model.node_dropout_rate, 1 - model.cl_drop
    dropped = torch.sparse_coo_tensor(idx[:, ui_keep], val[ui_keep] * (1. / rate), adj.shape).to_dense()
    cl_view = torch.sparse_coo_tensor(idx[:, cl_ids], val[cl_ids] * (1. / rate / cl_rate), adj.shape).to_dense()[:, :model.n_items]
    sel = {'enc_keep': model.last_enc_keep.cpu().bool(), 'cl_keep': model.last_cl_keep.cpu().bool(), 'masked_ids': model.last_masked_ids.cpu(),
           'rand_item': model.last_rand_item.cpu()}
    masks, flat = {}, [None if m is None else m.detach().cpu().to(dt) for m in model.last_mess_masks]
    hops = model.context_hops
    if len(flat) == 5 * hops:                                   # the recommendation forward dropped messages too
        masks['gcn'] = [(flat[2 * h], flat[2 * h + 1]) for h in range(hops)]
        flat = flat[2 * hops:]
    assert len(flat) == 3 * hops
    masks['ui'] = [(flat[2 * h], flat[2 * h + 1]) for h in range(hops)]
    masks['kg'] = flat[2 * hops:]
    hp = {'layer_num': hops, 'decay': model.decay, 'mae_coef': model.mae_coef, 'cl_coef': model.cl_coef, 'tau': model.tau}
    g = dh.rel_graph
    edges = (g.head.cpu(), g.tail.cpu(), g.rel.cpu())
    return edges, sel, (dropped, cl_view), hp, masks


@pytest.mark.parametrize('mess_dropout', [True, False])
def test_cal_loss_on_the_cpu_in_float64(mess_dropout):
    from sslrec_amd.models.bulid_model import build_model
    dh = tiny_handler(model={'mess_dropout': mess_dropout, 'embedding_size': 16})
    torch.manual_seed(4)
    model = build_model(dh).double()
    batch = tiny_batch(dh)
    np.random.seed(9)
    loss, parts = model.cal_loss(batch)
    loss.backward()
    assert sorted(parts) == ['cl_loss', 'mae_loss', 'rec_loss']
    assert len(model.last_mess_masks) == (10 if mess_dropout else 6) and all(m is not None for m in model.last_mess_masks)
    named = dict(model.named_parameters())
    p = {n: R.leaf(v, torch.float64) for n, v in model.named_parameters()}
    edges, sel, mats, hp, masks = restatement_inputs(model, dh, torch.float64)
    out = R.model_loss(p, (U, I), edges, sel, mats, batch, hp, masks)
    out['loss'].backward()
    for k in ('loss', 'rec_loss', 'mae_loss', 'cl_loss'):
        assert_close(k, (loss if k == 'loss' else parts[k]).detach().reshape(1), out[k].detach().reshape(1), 1e-10)
    for n in R.PARAM_NAMES:
        assert_close('grad ' + n, named[n].grad, p[n].grad, 1e-10)
    assert bool((named['gcn.relation_emb'].grad[N_REL - 2] == 0).all())                  # the last type is in no sub-graph of a step
    # generate() in eval mode: no dropout of any kind, the full graphs
    model.eval()
    with torch.no_grad():
        u, i = model.generate()
        q = {n: v.detach() for n, v in named.items()}
        we, wu = R.gcn_forward(q['all_embed'][:U], q['all_embed'][U:], q['gcn.W_Q'], q['gcn.relation_emb'], edges, None,
                               dh.interact_mat.to_dense().double(), 2)
        score, index, types = model.generate_global_attn_score()
    assert_close('generate users', u, wu, 1e-11)
    assert_close('generate items', i, we[:I], 1e-11)
    assert_close('global scores', score, R.norm_attn_computer(q['all_embed'][U:], q['gcn.W_Q'], q['gcn.relation_emb'], edges)[0], 1e-11)
    assert torch.equal(index[0], edges[0]) and torch.equal(types, edges[2] + 1)
    assert tuple(model.rating(u[:3], i).shape) == (3, I)


# ---------------------------------------------------------------------------------------------------------------------
# trainer and command line
# ---------------------------------------------------------------------------------------------------------------------
class _Log:
    def log(self, *a, **k):
        pass

    log_loss = log_eval = log


def test_trainer_factory_and_refusal():
    from sslrec_amd.models.bulid_model import build_model
    from sslrec_amd.trainer.build_trainer import build_trainer
    from sslrec_amd.trainer.trainer import Trainer
    dh = tiny_handler()
    assert type(build_trainer(dh, _Log())) is Trainer
    dh = tiny_handler(train={'hip_graph': True})
    with pytest.raises(NotImplementedError, match='hip_graph'):
        build_model(dh)


def test_command_line_parses():
    """`main.py --model kgrec --synthetic kg-tiny`: what main() does up to the model, on the CPU"""
    from sslrec_amd.config.configurator import configs, parse_configure
    from sslrec_amd.data_utils.build_data_handler import build_data_handler
    from sslrec_amd.models.bulid_model import build_model
    import main                                        # noqa: F401  (the module imports)
    parse_configure(['--model', 'kgrec', '--device', 'cpu'])
    configs['data']['synthetic'] = 'kg-tiny'
    configs['model']['mae_msize'] = 32
    assert configs['model']['name'] == 'kgrec' and configs['data']['type'] == 'kg' and configs['train']['trainer'] == 'trainer'
    dh = build_data_handler()
    dh.load_data()
    assert type(build_model(dh)).__name__ == 'KGRec'
