"""AdaGCL on the HIP path; interface of the reference's models/general_cf/adagcl.py (:14-429): AdaGCL(data_handler) with forward(adj),
forward_(), loss_graphcl, cal_loss_cl, cal_loss_ib, cal_loss, full_predict and set_denoiseNet; VGAE() with set_adagcl, forward_encoder,
cal_loss_vgae and vgae_generate; DenoiseNet() with set_adagcl, get_attention, hard_concrete_sample, denoise_generate, l0_norm, call,
lossl0 and cal_loss_denoise; the loss dictionary keys and the parameter names (user_embeds, item_embeds; encoder_mean.{0,2},
encoder_std.{0,2}, decoder.{1,3}; nblayers_{0,1}.0, selflayers_{0,1}.0, attentions_{0,1}.0, drawn in that order).  Underneath,

  reference                                                      here
  t.spmm over the plain adjacency (:55)                          ops.propagate_sum on the cached plan
  vgae_generate: two [nnz, d] gathers, a [nnz, d] GEMM, a        ops.edge_mlp_logits (csrc/edgemlp.hip): nothing of size nnz x d; the
  boolean index and a NEW sparse tensor per step (:224-237)      kept entries re-valued, the dropped ones 0, as a RevaluedView of the
                                                                 cached plan (ops.edge_keep_view): no new plan, no host round trip
  get_attention: two [nnz, d] gathers, two [nnz, d] GEMMs, a     two [N, d] GEMMs and two [N] dots (the Linear of a gathered row is
  [nnz, 2 d] concat and its GEMM (:274-292)                      the gathered row of the transformed table; the last Linear splits
                                                                 into its two halves): log_alpha[e] = p[row] + q[col] + bias
  hard_concrete_sample, two sparse tensors, sparse.sum, pow,     ops.edge_gate (csrc/gate.hip) on [nnz] and [N] vectors, forward and
  clamp, two gathers, l0_norm (:294-347, :382-394)               backward, no float atomics
  torch_sparse.spmm with learned values (:396)                   ops.spmm_valued: gradients to the values and to x
  t.spmm over the generated sparse tensors (:69)                 ops.spmm over the RevaluedView

`loss_graphcl` (:76-103) stays the torch expression: its denominator excludes the positive, which is not the fused InfoNCE's form,
and its [2 B, 2 B] matrix is small beside what the rows above remove.  The batch-sized decoder of cal_loss_vgae (:199-200) and the
[N, d] encoder MLPs stay in torch and carry their gradients.

Kept as the reference has it: DenoiseNet.features is the snapshot of the embeddings taken in set_adagcl and never refreshed (:271,
:366); set_adagcl registers the model's two embedding tables as parameters of DenoiseNet (:263-264) and the model as a sub-module of
VGAE (:173), set_denoiseNet the DenoiseNet as a sub-module of the model (:34) -- so reg_params(model) covers DenoiseNet's weights and
each of the trainer's three optimizers reaches further than its name says.  DenoiseNet has layers 0 and 1 only (:253-260).

Random draws (parity mode, the default): VGAE's t.randn(shape) comes from torch's CPU generator and is moved to the device (:189);
the gate's u comes from the reference's own np.random.uniform(1e-7, 1 - 1e-7, [nnz, 1]) call (:301), the logistic log u - log(1 - u)
is formed in float64 and rounded once.  With model.device_rng the normal numbers are drawn by the device's generator and u by
rng.philox_uniforms.  A view that keeps no entries is an error (the reference divides by 0); the count lives on the device, so it is
raised where the trainer reads its losses, once per epoch -- or at once by `check_kept`."""
import numpy as np
import torch as t
import torch.nn.functional as F
from torch import nn

from ... import ops
from ...config.configurator import configs
from ...graph import RevaluedView, graph_of
from ..loss_utils import reg_params
from ._graph_cf import GraphCF


class AdaGCL(GraphCF):
    def __init__(self, data_handler):
        super().__init__(data_handler)               # user_embeds, item_embeds: the reference's two draws (:27-28)
        model_cfg = configs['model']
        self.cl_weight = model_cfg['cl_weight']
        self.ib_weight = model_cfg['ib_weight']
        self.temperature = model_cfg['temperature']

    def set_denoiseNet(self, denoiseNet):
        self.denoiseNet = denoiseNet

    def _pick_embeds(self, user_embeds, item_embeds, batch_data):
        ancs, poss, negs = batch_data
        return user_embeds[ancs], item_embeds[poss], item_embeds[negs]

    def _forward_stacked(self, adj):
        if not self.is_training and self.final_embeds is not None:
            return self.final_embeds
        embeds = self._stacked_tables(alias_ok=True)
        if isinstance(adj, RevaluedView):            # a generated view: the values differ per step, one product per layer (:55)
            embeds_list = [embeds]
            for i in range(self.layer_num):
                embeds_list.append(ops.spmm(adj, embeds_list[-1]))
            embeds = sum(embeds_list)
        else:
            embeds = self._propagate_sum(adj, embeds)
        self.final_embeds = embeds
        return embeds

    def forward(self, adj):
        return self._split(self._forward_stacked(adj))

    def forward_(self):
        embedsLst = [self._stacked_tables(alias_ok=True)]
        for i in range(self.layer_num):
            with t.no_grad():
                adj = self.denoiseNet.denoise_generate(x=embedsLst[-1], layer=i)
            embedsLst.append(ops.spmm(adj, embedsLst[-1]))                                              # :69
        return sum(embedsLst)

    def loss_graphcl(self, x1, x2, users, items):
        """:76-103: -log(pos / (row sum - pos)) per row of the [2 B, 2 B] matrix of exp(cosine / T)"""
        T = self.temperature
        x1, x2 = F.normalize(x1, dim=1), F.normalize(x2, dim=1)                                         # (row-wise: the split is immaterial)
        nodes = t.concat([users, items + self.user_num])
        all_embs1, all_embs2 = x1[nodes], x2[nodes]
        all_embs1_abs, all_embs2_abs = all_embs1.norm(dim=1), all_embs2.norm(dim=1)
        sim_matrix = (all_embs1 @ all_embs2.T) / (all_embs1_abs[:, None] * all_embs2_abs[None, :])
        sim_matrix = t.exp(sim_matrix / T)
        pos_sim = t.diagonal(sim_matrix)
        return -t.log(pos_sim / (sim_matrix.sum(dim=1) - pos_sim))

    def cal_loss_cl(self, batch_data, generated_adj):
        self.is_training = True
        ancs, poss, negs = batch_data
        out1 = self._forward_stacked(generated_adj)
        out2 = self.forward_()
        loss = self.loss_graphcl(out1, out2, ancs, poss).mean() * self.cl_weight
        return loss, {'cl_loss': loss}, out1, out2

    def cal_loss_ib(self, batch_data, generated_adj, out1_old, out2_old):
        self.is_training = True
        ancs, poss, negs = batch_data
        out1 = self._forward_stacked(generated_adj)
        out2 = self.forward_()
        loss_ib = self.loss_graphcl(out1, out1_old.detach(), ancs, poss) + self.loss_graphcl(out2, out2_old.detach(), ancs, poss)
        loss = loss_ib.mean() * self.ib_weight
        return loss, {'ib_loss': loss}

    def cal_loss(self, batch_data):
        self.is_training = True
        embeds = self._forward_stacked(self.adj)
        ancs, poss, negs = batch_data
        bpr_loss = ops.bpr_loss_stacked(embeds, self.user_num, ancs, poss, negs, divisor=ancs.shape[0])
        reg_loss = reg_params(self, self.reg_weight)
        loss = bpr_loss + reg_loss
        return loss, {'bpr_loss': bpr_loss, 'reg_loss': reg_loss}

    def _embeddings_for_eval(self):
        self._stacked_e0 = None          # (evaluation never reuses a training step's concatenated tables)
        if self.is_training:
            self.final_embeds = None
            self.is_training = False
        with t.no_grad():
            return self.forward(self.adj)                                                               # :147-148

    def full_predict(self, batch_data):
        users, items = self._embeddings_for_eval()
        return self._score_all_items(users, items, batch_data)

    def train(self, mode=True):
        if mode:                         # back to training: the evaluation cache is stale
            self.is_training = True
        return super().train(mode)


class VGAE(nn.Module):
    def __init__(self):
        super().__init__()
        hidden = configs['model']['embedding_size']
        self.encoder_mean = nn.Sequential(nn.Linear(hidden, hidden), nn.ReLU(inplace=True), nn.Linear(hidden, hidden))
        self.encoder_std = nn.Sequential(nn.Linear(hidden, hidden), nn.ReLU(inplace=True), nn.Linear(hidden, hidden), nn.Softplus())
        self.decoder = nn.Sequential(nn.ReLU(inplace=True), nn.Linear(hidden, hidden), nn.ReLU(inplace=True), nn.Linear(hidden, 1))
        self.sigmoid = nn.Sigmoid()
        self.bceloss = nn.BCELoss(reduction='none')
        self.last = None

    def set_adagcl(self, adagcl):
        self.reg_weight = configs['model']['reg_weight']
        self.adagcl = adagcl

    def forward_encoder(self, adj):
        self.is_training = True
        with t.no_grad():                                        # (:183-185 detach the tables: no graph is needed behind them)
            x = self.adagcl._forward_stacked(adj)
        x_mean = self.encoder_mean(x)
        x_std = self.encoder_std(x)
        if self.adagcl.device_rng is not None:
            gaussian_noise = t.randn(x_mean.shape, device=x_mean.device)
        else:
            gaussian_noise = t.randn(x_mean.shape).to(x_mean.device)                                    # :189
        self.last_noise = gaussian_noise
        x = gaussian_noise * x_std + x_mean
        return x, x_mean, x_std

    def cal_loss_vgae(self, data, batch_data):
        users, items, neg_items = batch_data
        x, x_mean, x_std = self.forward_encoder(data)
        user_num = configs['data']['user_num']
        x_user, x_item = x[:user_num], x[user_num:]
        edge_pos_pred = self.sigmoid(self.decoder(x_user[users] * x_item[items]))
        edge_neg_pred = self.sigmoid(self.decoder(x_user[users] * x_item[neg_items]))
        loss_edge_pos = self.bceloss(edge_pos_pred, t.ones_like(edge_pos_pred))
        loss_edge_neg = self.bceloss(edge_neg_pred, t.zeros_like(edge_neg_pred))
        loss_rec = loss_edge_pos + loss_edge_neg
        kl_divergence = - 0.5 * (1 + 2 * t.log(x_std) - x_mean**2 - x_std**2).sum(dim=1)
        bprLoss = ops.bpr_loss_stacked(x, user_num, users, items, neg_items, divisor=users.shape[0])
        beta = 0.1
        loss = (loss_rec + beta * kl_divergence.mean() + bprLoss).mean()
        return loss, {'generate_loss': loss}

    def vgae_generate(self, data, edge_index=None, adj=None):
        """the generated view (:221-237) as a RevaluedView of the cached plan of `data`; `edge_index` and `adj` are the reference's
        arguments (the entry list and a copy of `data`) and are not needed: the plan holds both.  self.last keeps the logits, the
        keep flags and the kept count (device tensors) of the call."""
        x, _, _ = self.forward_encoder(data)
        graph = graph_of(data)
        dec1, dec2 = self.decoder[1], self.decoder[3]
        logits = ops.edge_mlp_logits(graph, x, dec1.weight, dec1.bias, dec2.weight, dec2.bias)
        view, keep, kept = ops.edge_keep_view(graph, logits)
        self.last = {'logits': logits, 'keep': keep, 'kept': kept}
        return view


def check_kept(kept):
    """raise for a generated view that kept no entries (one host synchronisation)"""
    if int(kept.min().item()) <= 0:
        raise RuntimeError('AdaGCL: a generated view kept no entries of the adjacency (the reference divides by 0 here); the VGAE '
                           'decoder rejects every edge')


class DenoiseNet(nn.Module):
    def __init__(self):
        super().__init__()
        hidden = configs['model']['embedding_size']
        self.edge_weights = []
        self.nblayers_0 = nn.Sequential(nn.Linear(hidden, hidden), nn.ReLU(inplace=True))
        self.nblayers_1 = nn.Sequential(nn.Linear(hidden, hidden), nn.ReLU(inplace=True))
        self.selflayers_0 = nn.Sequential(nn.Linear(hidden, hidden), nn.ReLU(inplace=True))
        self.selflayers_1 = nn.Sequential(nn.Linear(hidden, hidden), nn.ReLU(inplace=True))
        self.attentions_0 = nn.Sequential(nn.Linear(2 * hidden, 1))
        self.attentions_1 = nn.Sequential(nn.Linear(2 * hidden, 1))
        self.last_noise = []

    def set_adagcl(self, adagcl):
        self.user_embeds = adagcl.user_embeds                    # (registers both tables as parameters of this module, as :263-264 do)
        self.item_embeds = adagcl.item_embeds
        self.user_num = adagcl.user_num
        self.item_num = adagcl.item_num
        self.layer_num = configs['model']['layer_num']
        self.reg_weight = configs['model']['reg_weight']
        if self.layer_num > 2:
            raise NotImplementedError('DenoiseNet has the reference\'s two layers (nblayers_0 / nblayers_1): model.layer_num <= 2')
        self.device_rng = adagcl.device_rng
        self.features = t.concat([self.user_embeds, self.item_embeds]).detach()      # the snapshot, never refreshed (:271, :366)
        self.set_fea_adj(self.user_num + self.item_num, adagcl.adj)

    def set_fea_adj(self, nodes, adj):
        self.node_size = nodes
        self.adj_mat = adj

    def _graph(self):
        return graph_of(self.adj_mat)

    def get_attention(self, input1, input2, layer=0):
        """(p, q, bias) with log_alpha[e] = p[row(e)] + q[col(e)] + bias, from the NODE tables input1 (the row end) and input2 (the column
        end): the reference's per-entry weight (:274-292) is exactly that sum"""
        nb_layer, selflayer = getattr(self, 'nblayers_%d' % layer), getattr(self, 'selflayers_%d' % layer)
        att = getattr(self, 'attentions_%d' % layer)[0]
        hidden = input1.shape[1]
        p = nb_layer(input1) @ att.weight[0, :hidden]
        q = selflayer(input2) @ att.weight[0, hidden:]
        return p, q, att.bias

    def hard_concrete_sample(self, nnz, device):
        """the logistic noise log u - log(1 - u) of :299-303 as fp32 [nnz]"""
        if self.device_rng is not None:
            from ...rng import philox_uniforms
            u = philox_uniforms(self.device_rng, self.device_rng.next_stream(), nnz).double().clamp(1e-7, 1.0 - 1e-7)
            return (t.log(u) - t.log(1.0 - u)).float()
        debug_var = 1e-7
        np_random = np.random.uniform(low=debug_var, high=1.0 - debug_var, size=[nnz, 1])
        random_noise = t.tensor(np_random)
        return (t.log(random_noise) - t.log(1.0 - random_noise)).view(-1).float().to(device)

    def denoise_generate(self, x, layer=0):
        p, q, bias = self.get_attention(x, x, layer)
        m = configs['model']
        vals, _ = ops.edge_gate(self._graph(), p, q, bias, m['gamma'], m['zeta'], eps=0.0)             # :319, :328-334
        return RevaluedView(self._graph(), vals)

    def call(self, inputs, training=None):
        temperature = inputs if training else 1.0
        m = configs['model']
        graph = self._graph()
        x = self.features.detach()
        embedsLst = [x]
        self.last_noise = []
        for i in range(self.layer_num):
            p, q, bias = self.get_attention(x, x, layer=i)
            noise = self.hard_concrete_sample(graph.nnz, x.device) if training else None
            self.last_noise.append(noise)
            vals, l0 = ops.edge_gate(graph, p, q, bias, m['gamma'], m['zeta'], beta=temperature, noise=noise, eps=1e-6)
            self.edge_weights.append(l0)                         # (the reference keeps log_alpha for lossl0; its mean term comes out of the kernel)
            x = ops.spmm_valued(graph, vals, x)                                                         # :396
            embedsLst.append(x)
        return sum(embedsLst)

    def lossl0(self, temperature):
        l0_loss = sum(self.edge_weights) if self.edge_weights else t.zeros([], device=self.features.device)
        self.edge_weights = []
        return l0_loss

    def cal_loss_denoise(self, batch_data, temperature):
        x = self.call(temperature, True)
        users, items, neg_items = batch_data
        bprLoss = ops.bpr_loss_stacked(x, self.user_num, users, items, neg_items, divisor=users.shape[0])
        lossl0 = self.lossl0(temperature) * configs['model']['lambda0']
        loss = bprLoss + lossl0
        return loss, {'denoise_loss': loss}
