"""NCL on the HIP path; interface of the reference's models/general_cf/ncl.py (:11-97): NCL(data_handler), _cluster(), forward(adj) ->
(embeds, embeds_list), _pick_embeds, _cal_struct_loss, _cal_proto_loss, cal_loss(batch) with the 4-tuple batch (ancs, poss, negs,
kmeans_flags), full_predict(batch), the loss dictionary keys bpr_loss / reg_loss / struct_loss / proto_loss, the parameters
user_embeds / item_embeds and the evaluation-time reuse of `final_embeds_list`.  Underneath,

  reference                                                      here
  KMeansClustering: 1000 x ([N, K, d] distances, 2 index_add_)    ops.kmeans (csrc/kmeans.hip): nothing of size N x K, deterministic sums,
  (aug_utils.py:147-157)                                          stops once an iteration changes no row (bitwise the same result)
  max(L, 2 h) x t.spmm (:36-39)                                   as many single ops.spmm launches -- layers 0 and 2 h each carry a loss
                                                                 of their own, so the fused layer-SUM path (ops.propagate_sum, whose
                                                                 layers are not differentiable one by one) does not apply
  4 gathers + 2 cal_infonce_loss on sliced tables (:51-58)        cal_infonce_loss_two_sided on the stacked tables, one autograd node
  gathers + 2 cal_infonce_loss against the centroids (:60-68)     the fused dense cal_infonce_loss with K candidate rows
  3 gathers + cal_bpr_loss, reg_params (:78-83)                   cal_bpr_loss_stacked(..., add=reg_loss), like LightGCN

Random draws: the two t.rand([K, d]) of `_cluster` (users first), from torch's CPU generator in parity mode (replayed on the device
under the default Trainer), from the device's generator with model.device_rng.  train.hip_graph is refused: the clustering reads a
counter on the host."""
import torch as t

from ...config.configurator import configs
from ..aug_utils import KMeansClustering
from ..loss_utils import cal_bpr_loss_stacked, cal_infonce_loss, cal_infonce_loss_two_sided
from .lightgcn import LightGCN


class NCL(LightGCN):
    def __init__(self, data_handler):
        if configs['train'].get('hip_graph'):
            raise NotImplementedError('train.hip_graph is not supported by NCL: every model.epoch_period epochs the step clusters both '
                                      'tables, and the clustering reads its changed-row counter on the host')
        super().__init__(data_handler)
        model_cfg = configs['model']
        self.proto_weight = model_cfg['proto_weight']
        self.struct_weight = model_cfg['struct_weight']
        self.temperature = model_cfg['temperature']
        self.layer_num = model_cfg['layer_num']
        self.high_order = model_cfg['high_order']
        self.kmeans = KMeansClustering(cluster_num=model_cfg['cluster_num'], embedding_size=model_cfg['embedding_size'],
                                       device_rng=self.device_rng is not None)
        self.final_embeds_list = None

    def _cluster(self):
        self.user_centroids, self.user2cluster, _ = self.kmeans(self.user_embeds.detach())
        self.item_centroids, self.item2cluster, _ = self.kmeans(self.item_embeds.detach())

    def forward(self, adj):
        if not self.is_training and self.final_embeds_list is not None:
            embeds_list = self.final_embeds_list
            if self.final_embeds is not None:
                return self.final_embeds, embeds_list
        else:
            embeds_list = [self._stacked_tables(alias_ok=True)]
            for _ in range(max(self.layer_num, self.high_order * 2)):
                embeds_list.append(self._propagate(adj, embeds_list[-1]))
        self.final_embeds_list = embeds_list
        self.final_embeds = sum(embeds_list[:self.layer_num + 1])
        return self.final_embeds, embeds_list

    def _pick_embeds(self, embeds, ancs, poss, negs):
        user_embeds, item_embeds = embeds[:self.user_num], embeds[self.user_num:]
        return user_embeds[ancs], item_embeds[poss], item_embeds[negs]

    def _cal_struct_loss(self, context_embeds, ego_embeds, ancs, poss):
        """(InfoNCE(context_u[ancs], ego_u[ancs], ego_u) + InfoNCE(context_i[poss], ego_i[poss], ego_i)) / B (:51-58) on the stacked tables"""
        return cal_infonce_loss_two_sided(context_embeds, ego_embeds, self.user_num, ancs, poss, self.temperature, self.infonce_precision) / ancs.shape[0]

    def _cal_proto_loss(self, ego_embeds, ancs, poss):
        user_embeds, item_embeds = ego_embeds[:self.user_num], ego_embeds[self.user_num:]
        user_clusters = self.user2cluster[ancs]
        item_clusters = self.item2cluster[poss]
        loss = cal_infonce_loss(user_embeds[ancs], self.user_centroids[user_clusters], self.user_centroids, self.temperature, self.infonce_precision) + \
            cal_infonce_loss(item_embeds[poss], self.item_centroids[item_clusters], self.item_centroids, self.temperature, self.infonce_precision)
        return loss / ancs.shape[0]

    def cal_loss(self, batch_data):
        self.is_training = True
        self._begin_step()
        self.final_embeds_list = None                # (with final_embeds: the previous step's autograd graph, see GraphCF._begin_step)
        ancs, poss, negs, kmeans_flags = batch_data
        if t.sum(kmeans_flags) != 0 or not hasattr(self, 'user2cluster'):
            self._cluster()
        embeds, embeds_list = self.forward(self.adj)
        ego_embeds = embeds_list[0]
        context_embeds = embeds_list[self.high_order * 2]

        struct_loss = self._cal_struct_loss(context_embeds, ego_embeds, ancs, poss) * self.struct_weight
        proto_loss = self._cal_proto_loss(ego_embeds, ancs, poss) * self.proto_weight
        reg_loss = self._table_regularizer()
        base, bpr_loss = cal_bpr_loss_stacked(embeds, self.user_num, ancs, poss, negs, divisor=ancs.shape[0], add=reg_loss)      # bpr + reg
        loss = base + struct_loss + proto_loss
        losses = {'bpr_loss': bpr_loss, 'reg_loss': reg_loss, 'struct_loss': struct_loss, 'proto_loss': proto_loss}
        return loss, losses

    def _embeddings_for_eval(self):
        self._stacked_e0 = None          # (evaluation never reuses a training step's concatenated tables)
        if self.is_training:             # the first evaluation after a training step propagates anew (:31-39), the later ones reuse
            self.final_embeds = self.final_embeds_list = None
        with t.no_grad():
            embeds, _ = self.forward(self.adj)
        self.is_training = False
        return self._split(embeds)

    def full_predict(self, batch_data):
        users, items = self._embeddings_for_eval()
        return self._score_all_items(users, items, batch_data)
