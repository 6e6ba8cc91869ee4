"""DirectAU on the HIP path; interface of the reference's models/general_cf/directau.py (:10-59): constructor argument, parameter
names and draw order, forward(adj), cal_loss(batch) and its loss dictionary, full_predict(batch).  Underneath,

  reference                                                here
  t.concat + L x t.spmm + sum / len (:30-35)               ops.propagate_sum: one fused SpMM launch per layer that accumulates the
                                                           layer SUM; the division by L + 1 rides on the loss's gather as `scale`
  2 gathers, alignment, 2 x uniformity (:43-47): an        ops.align_uniform_loss_stacked: one autograd node, no [B, B] or
  8.4 M-element pdist vector per call at B = 4096,         [B (B - 1) / 2] tensor forward or backward, the index_put backward of both
  again in the backward, 2 index_put scatters              gathers in the same call, fixed summation order (csrc/au.hip)

The mean table itself is formed for evaluation only (full_predict's scores are the reference's values, not just its ranking).  The
model draws no random number after its two parameters, in any mode; the negatives of a batch are ignored as in the reference."""
import torch as t

from ...config.configurator import configs
from ..loss_utils import cal_align_uniform_loss_stacked
from ._graph_cf import GraphCF


class DirectAU(GraphCF):
    def __init__(self, data_handler):
        super().__init__(data_handler)               # user_embeds, item_embeds: the reference's two draws (:19-20); layer_num
        self.gamma = configs['model']['gamma']

    def forward(self, adj):
        cached = self._cached()
        if cached is not None:
            return cached
        total = self._propagate_sum(adj, self._stacked_tables(alias_ok=True))
        self.final_embeds = total / (self.layer_num + 1)                                                  # :35
        return self._split(self.final_embeds)

    def cal_loss(self, batch_data):
        self.is_training = True
        self._begin_step()
        ancs, poss, _ = batch_data
        total = self._propagate_sum(self.adj, self._stacked_tables(alias_ok=True))
        loss, align_loss, uniform_loss = cal_align_uniform_loss_stacked(total, self.user_num, ancs, poss, self.gamma,
                                                                        scale=1.0 / (self.layer_num + 1))    # :43-47
        return loss, {'align_loss': align_loss, 'uniform_loss': uniform_loss}

    def _embeddings_for_eval(self):
        self._stacked_e0 = None          # (evaluation never reuses a training step's concatenated tables)
        with t.no_grad():
            tables = self.forward(self.adj)
        self.is_training = False
        return tables

    def full_predict(self, batch_data):
        users, items = self._embeddings_for_eval()
        return self._score_all_items(users, items, batch_data)
