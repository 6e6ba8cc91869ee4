"""HCCF on the HIP path; interface of the reference's models/general_cf/hccf.py (:13-108): constructor argument, forward(adj,
keep_rate) and its 3-tuple, cal_loss(batch), full_predict(batch) and the loss dictionary keys.  Underneath,

  reference                                                here
  EdgeDrop rebuilds the COO + t.spmm (:35-36, :47)         ops.spmm over the DroppedView of the cached plan
  2 x (GEMM, F.dropout, HGNNLayer) + concat (:43-51)       ops.hyper_propagate_stacked: no [N, K] tensor, the mask computed in
                                                           the kernels (csrc/hyper.hip)
  cal_infonce_loss_spec_nodes x 2 per layer (:77-81)       the fused gathered InfoNCE on the normalized tables

The hypergraph dropout ALWAYS draws from a Philox state: model.device_rng if set, else a state of the model's own (seeded with the
CPU generator's seed, torch.initial_seed(), which consumes no draw).  The reference draws that mask with the training device's generator, so there is no CPU stream
to reproduce -- the model's one departure from bit-parity.  EdgeDrop follows the usual parity / device_rng switch.  With
keep_rate = 1.0 the model draws nothing."""
import torch as t
from torch import nn

from ... import ops
from ...config.configurator import configs
from ..aug_utils import EdgeDrop
from ..loss_utils import cal_bpr_loss_stacked, cal_infonce_loss_spec_nodes, reg_params
from ._graph_cf import GraphCF

init = nn.init.xavier_uniform_


class HCCF(GraphCF):
    def __init__(self, data_handler):
        super().__init__(data_handler)               # user_embeds, item_embeds: the reference's first two draws (:27-28)
        model_cfg = configs['model']
        self.cl_weight = model_cfg['cl_weight']
        self.hyper_num = model_cfg['hyper_num']
        self.mult = model_cfg['mult']
        self.keep_rate = model_cfg['keep_rate']
        self.temperature = model_cfg['temperature']
        self.leaky = model_cfg['leaky']
        self.user_hyper_embeds = nn.Parameter(init(t.empty(self.embedding_size, self.hyper_num)))      # :30-31
        self.item_hyper_embeds = nn.Parameter(init(t.empty(self.embedding_size, self.hyper_num)))
        self.edge_drop = EdgeDrop(resize_val=True, device_rng=self.device_rng)
        # the seed of the model's own dropout state: the CPU generator's seed, read and not drawn, so the generator stands where the
        # reference's stands after the four parameters (EdgeDrop's parity masks and everything after them see the reference's numbers)
        self._hyper_seed = None if self.device_rng is not None else t.initial_seed() % 2 ** 62
        self._hyper_rng = None

    def _hyper_state(self):
        if self.device_rng is not None:
            return self.device_rng
        if self._hyper_rng is None or self._hyper_rng.state.device != self.user_embeds.device:
            from ...rng import PhiloxState
            self._hyper_rng = PhiloxState(self.user_embeds.device, self._hyper_seed)
        return self._hyper_rng

    def _begin_step(self):
        super()._begin_step()                        # (advances device_rng)
        if self.device_rng is None and self.keep_rate < 1.0:
            self._hyper_state().advance()

    def forward(self, adj, keep_rate):
        if not self.is_training and self.final_embeds is not None:
            return self.final_embeds, None, None
        e0 = self._stacked_tables(alias_ok=True)
        cur = total = e0
        gcn_embeds_list, hyper_embeds_list = [], []
        for i in range(self.layer_num):
            gcn_embeds = ops.spmm(self.edge_drop(adj, keep_rate), cur)                                    # :47, a fresh mask per layer
            rng = None
            if keep_rate < 1.0:                      # one stream per layer, shared by both row ranges
                state = self._hyper_state()
                rng = (state, state.next_stream())
            hyper_embeds = ops.hyper_propagate_stacked(cur, e0, self.user_num, self.user_hyper_embeds, self.item_hyper_embeds, self.mult,
                                                       self.leaky, keep_rate, rng)                       # :43-44, :48-49, :51
            gcn_embeds_list.append(gcn_embeds)
            hyper_embeds_list.append(hyper_embeds)
            cur = gcn_embeds + hyper_embeds                                                               # :52
            total = total + cur
        self.final_embeds = total
        return total, gcn_embeds_list, hyper_embeds_list

    def cal_loss(self, batch_data):
        self.is_training = True
        self._begin_step()
        ancs, poss, negs = batch_data
        embeds, gcn_embeds_list, hyper_embeds_list = self.forward(self.adj, self.keep_rate)
        bpr_loss = cal_bpr_loss_stacked(embeds, self.user_num, ancs, poss, negs, divisor=ancs.shape[0])
        users, items = t.unique(ancs), t.unique(poss)
        cl_loss = 0
        for i in range(self.layer_num):
            embeds1 = gcn_embeds_list[i].detach()                                                         # :78
            embeds2 = hyper_embeds_list[i]
            cl_loss = cl_loss + cal_infonce_loss_spec_nodes(embeds1[:self.user_num], embeds2[:self.user_num], users, self.temperature,
                                                            self.infonce_precision) \
                + cal_infonce_loss_spec_nodes(embeds1[self.user_num:], embeds2[self.user_num:], items, self.temperature, self.infonce_precision)
        reg_loss = reg_params(self) * self.reg_weight
        cl_loss = cl_loss * self.cl_weight
        loss = bpr_loss + reg_loss + cl_loss
        losses = {'bpr_loss': bpr_loss, 'reg_loss': reg_loss, 'cl_loss': cl_loss}
        return loss, losses

    def _embeddings_for_eval(self):
        self._stacked_e0 = None          # (evaluation never reuses a training step's concatenated tables)
        with t.no_grad():
            embeds = self.forward(self.adj, 1.0)[0]
        self.is_training = False
        return embeds[:self.user_num], embeds[self.user_num:]

    def full_predict(self, batch_data):
        users, items = self._embeddings_for_eval()
        return self._score_all_items(users, items, batch_data)
