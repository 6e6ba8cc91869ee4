"""MHCN on the HIP path; interface of the reference's models/social/mhcn.py (:12-171): MHCN(data_handler), forward() ->
(user_embeds, item_embeds), cal_loss(batch) -> (loss, {'bpr_loss', 'reg_loss', 'ss_loss'}), full_predict(batch), the parameters
user_embeds, item_embeds, gating1..4.{weight,bias}, sgating1..3.{weight,bias}, attn, attn_mat with the reference's names and shapes,
drawn in the reference's order (:20-31), so one seed gives its initial parameters and its `state_dict` loads.  Underneath,

  reference                                                        here
  4 + 3 x (Linear, sigmoid, product) (:34-52)                       ops.self_gate: once for the four gates, once for the three sgates
  per layer and at the end: 3 x (matmul, product, row sum),         one ops.channel_mix per layer, which also adds the four normalised
  stack, softmax, 3 scaled sums, 4 F.normalize, 4 list sums         tables to their layer sums, and one after the layers (csrc/mhcn.hip);
  (:54-64, :80-113)                                                 v = attn_mat @ attn.T is formed once per forward
  F.normalize + list sum of the item table (:95-97)                 ops.normalize_add
  5 x t.spmm per layer, 3 in the loss                               as many ops.spmm launches on the plans the handler built
  3 x (3 shuffled [U, d] copies, 5 row scores, 3 log sigmoid)       ops.hier_ssl_loss: no shuffled copy, the loss in double (csrc/mhcn.hip)
  (:120-143)
  3 gathers + softplus sum, reg_params (:152-153)                   the fused gathered BPR on the two final tables, reg_params

The raw SpMM outputs propagate; the normalised ones are summed, as upstream.  log sigmoid is computed in its stable form: it equals the
reference's sigmoid().log() wherever that is finite and stays finite where the reference returns -inf.

Random draws: 15 permutations per step, per channel randperm(U), randperm(d), randperm(U), randperm(d), randperm(U) in the reference's
order (:135, :136, :141) from torch's CPU generator, so one seed gives the reference's permutations and leaves the generator where the
reference leaves it; with model.device_rng they are drawn on the device.  train.hip_graph is refused: the permutations are drawn on the
host (or, on the device, by calls that cannot be captured) in every step."""
import torch as t
from torch import nn

from ... import ops
from ...config.configurator import configs
from ...graph import graph_of
from ..base_model import BaseModel
from ..loss_utils import cal_bpr_loss_gathered, reg_params

init = nn.init.xavier_uniform_


class MHCN(BaseModel):
    def __init__(self, data_handler):
        if configs['train'].get('hip_graph'):
            raise NotImplementedError('train.hip_graph is not supported by MHCN: every step draws its 15 permutations with torch.randperm, '
                                      'which a captured step cannot do')
        super().__init__(data_handler)
        self.data_handler = data_handler
        model_cfg = configs['model']
        self.layer_num = model_cfg['layer_num']
        self.reg_weight = model_cfg['reg_weight']
        self.ss_rate = model_cfg['ss_rate']
        self.device_rng = bool(model_cfg.get('device_rng'))
        d = self.embedding_size

        self.user_embeds = nn.Parameter(init(t.empty(self.user_num, d)))
        self.item_embeds = nn.Parameter(init(t.empty(self.item_num, d)))
        self.gating1 = nn.Linear(d, d)
        self.gating2 = nn.Linear(d, d)
        self.gating3 = nn.Linear(d, d)
        self.gating4 = nn.Linear(d, d)
        self.sgating1 = nn.Linear(d, d)
        self.sgating2 = nn.Linear(d, d)
        self.sgating3 = nn.Linear(d, d)
        self.attn = nn.Parameter(init(t.empty(1, d)))
        self.attn_mat = nn.Parameter(init(t.empty(d, d)))
        self.is_training = True
        self.final_user_embeds = self.final_item_embeds = None
        self.last_perms = None

    # -- the matrices ------------------------------------------------------------------------------------------------------------------
    def _adjs(self):
        """(H_s, H_j, H_p, R, R^T) as the SpMM takes them: the handler's plans on the device, the tensors themselves elsewhere"""
        h = self.data_handler
        if not hasattr(self, '_adj_cache'):
            if h.R.is_cuda:
                r = graph_of(h.R)
                r_t = getattr(h, 'R_t', None) or r.transposed()
                self._adj_cache = (graph_of(h.H_s), graph_of(h.H_j), graph_of(h.H_p), r, r_t)
            else:
                self._adj_cache = (h.H_s, h.H_j, h.H_p, h.R, h.R.t())
        return self._adj_cache

    @staticmethod
    def _spmm(adj, x):
        if x.is_cuda:
            return ops.spmm(adj, x)
        return t.sparse.mm(adj.to(x.dtype), x)         # (host tensors: the reference's statement; the tests' float64 runs use it)

    def _gates(self, names):
        mods = [getattr(self, n) for n in names]
        return [m.weight for m in mods], [m.bias for m in mods]

    # -- forward -----------------------------------------------------------------------------------------------------------------------
    def forward(self):
        if not self.is_training and self.final_user_embeds is not None:
            return self.final_user_embeds, self.final_item_embeds
        H_s, H_j, H_p, R, R_t = self._adjs()
        v = (self.attn_mat @ self.attn.t()).reshape(-1)                      # <e, v> = (attn * (e @ attn_mat)).sum(1)
        c1, c2, c3, simp = ops.self_gate(self.user_embeds, *self._gates(('gating1', 'gating2', 'gating3', 'gating4')))
        sums = (c1, c2, c3, simp)
        item_embeds = self.item_embeds
        item_sum = item_embeds
        mixed = ops.channel_mix(c1, c2, c3, simp, v) if self.layer_num > 0 else None      # layer 0's mixed table (:81)
        for _ in range(self.layer_num):
            c1 = self._spmm(H_s, c1)
            c2 = self._spmm(H_j, c2)
            c3 = self._spmm(H_p, c3)
            new_item_embeds = self._spmm(R_t, mixed)
            simp = self._spmm(R, item_embeds)
            item_sum = ops.normalize_add(item_sum, new_item_embeds)
            item_embeds = new_item_embeds
            # one launch reads the layer's four raw tables once: they join their normalised sums AND give the next layer's mixed table
            mixed, sums = ops.channel_mix(c1, c2, c3, simp, v, sums=sums)
        user_embeds = ops.channel_mix(*sums, v)
        self.final_user_embeds, self.final_item_embeds = user_embeds, item_sum
        return user_embeds, item_sum

    # -- the loss ----------------------------------------------------------------------------------------------------------------------
    def _draw_perms(self, device):
        """the step's 15 permutations, per channel (row_u, col_1, row_1, col_2, row_2), in the reference's order of draws"""
        U, d = self.user_num, self.embedding_size
        gen_dev = device if self.device_rng else 'cpu'
        perms = []
        for _ in range(3):
            perms.append(tuple(t.randperm(n, device=gen_dev) for n in (U, d, U, d, U)))
        return perms

    def _hierarchical_self_supervision(self, em, adj, perms):
        edge = self._spmm(adj, em)
        return ops.hier_ssl_loss(em, edge, [p.to(em.device) for p in perms])

    def cal_loss(self, batch_data):
        self.is_training = True
        self.final_user_embeds = self.final_item_embeds = None          # (the previous step's autograd graph)
        user_embeds, item_embeds = self.forward()
        ancs, poss, negs = batch_data
        if user_embeds.is_cuda:
            bpr_loss = cal_bpr_loss_gathered(user_embeds, item_embeds, ancs, poss, negs)
            reg_loss = reg_params(self, self.reg_weight)
        else:
            a, p, n = user_embeds[ancs], item_embeds[poss], item_embeds[negs]
            bpr_loss = t.nn.functional.softplus((a * n).sum(-1) - (a * p).sum(-1)).sum()
            reg_loss = self.reg_weight * sum(W.square().sum() for W in self.parameters())
        H_s, H_j, H_p = self._adjs()[:3]
        perms = self.last_perms = self._draw_perms(user_embeds.device)
        g1, g2, g3 = ops.self_gate(user_embeds, *self._gates(('sgating1', 'sgating2', 'sgating3')))
        ss_loss = self._hierarchical_self_supervision(g1, H_s, perms[0])
        ss_loss = ss_loss + self._hierarchical_self_supervision(g2, H_j, perms[1])
        ss_loss = ss_loss + self._hierarchical_self_supervision(g3, H_p, perms[2])
        ss_loss = ss_loss * self.ss_rate
        loss = bpr_loss + reg_loss + ss_loss
        losses = {'bpr_loss': bpr_loss, 'reg_loss': reg_loss, 'ss_loss': ss_loss}
        return loss, losses

    # -- evaluation --------------------------------------------------------------------------------------------------------------------
    def _embeddings_for_eval(self):
        """the propagated tables for scoring: the first evaluation after a training step propagates anew, the later ones reuse"""
        if self.is_training or self.final_user_embeds is None:
            self.is_training = True
            self.final_user_embeds = self.final_item_embeds = None
            with t.no_grad():
                self.forward()
            self.is_training = False
        return self.final_user_embeds, self.final_item_embeds

    def train(self, mode=True):
        if mode:                         # back to training: the evaluation cache is stale
            self.is_training = True
            self.final_user_embeds = self.final_item_embeds = None
        return super().train(mode)

    def full_predict(self, batch_data):
        user_embeds, item_embeds = self._embeddings_for_eval()
        pck_users, train_mask = batch_data
        if user_embeds.is_cuda and type(self)._mask_predict is BaseModel._mask_predict and user_embeds.shape[1] <= ops.INFONCE_DIMS[-1]:
            return ops.full_predict(user_embeds, item_embeds, pck_users.long(), train_mask)
        return self._mask_predict(user_embeds[pck_users.long()] @ item_embeds.T, train_mask)

    def predict_topk(self, users, k, trn_csr_device):
        """top-k unseen items without the dense train mask (GraphCF.predict_topk)"""
        user_embeds, item_embeds = self._embeddings_for_eval()
        if int(k) > ops.EVAL_KMAX:
            raise ValueError('predict_topk: k = %d exceeds the kernel\'s %d' % (int(k), ops.EVAL_KMAX))
        return ops.eval_topk(user_embeds, item_embeds, users.long(), k, trn_csr_device)
