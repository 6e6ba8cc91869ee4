"""AutoCF on the HIP path; interface of the reference's models/general_cf/autocf.py (:11-233): AutoCF(data_handler), forward(encoder_adj,
decoder_adj=None), cal_loss(batch, encoder_adj, decoder_adj), full_predict(batch), sample_subgraphs(), mask_subgraphs(seeds),
get_ego_embeds(), the module classes GCNLayer, GTLayer, LocalGraph and RandomMaskSubgraphs, the loss dictionary keys and the parameter
names (user_embeds, item_embeds, gtLayers.{i}.qTrans|kTrans|vTrans, drawn in that order).  Underneath,

  reference                                                      here
  t.spmm over a rebuilt sparse tensor (:96, :216)                 ops.spmm over a RevaluedView of the cached plan: the masked entries
                                                                 get the value 0, the kept ones the re-normalized value -- computed
                                                                 on the device, no host round trip, no new plan
  GTLayer: 2 gathers, 3 [E, d] GEMMs, index_add_ x 2 (:109-129)   3 [N, d] GEMMs + ops.edge_attention (csrc/gt.hip): nothing of size
                                                                 E x d, no atomics; its pattern is built on the device and cached
  LocalGraph: 3 t.spmm with the all-ones adjacency (:145-149)     ops.spmm over an all-ones RevaluedView of the cached plan
  RandomMaskSubgraphs: a Python loop over seeds, one pass over    set operations per depth: a node flag, one pass over the entries,
  all entries per seed (:180-198)                                 unique endpoints of the removed entries -- the same result

`contrast` (:60-68) stays the torch expression, as log-sum-exp: its rows are NOT normalized and carry no temperature, so the scores
are not the cosines / temp that the fused InfoNCE's default arithmetic is characterised for, and it is three [B, N] products
per step beside an operator that was E x d.

Random draws (parity mode, the default): t.rand(N) in LocalGraph.makeNoise, t.randint(N, [sampNum]) and the two
t.randint(temNum, [nnz]) in the masker come from torch's CPU generator with the reference's calls, shapes and order, so one seed gives
the reference's seeds, masks and decoder graph.  With model.device_rng they are drawn by the device's generator instead.  The model
has no per-step augmentation draw.  The decoder's rows are recovered with an integer division; the reference's float division
(:229) is exact only while N^2 < 2^24."""
import torch as t
import torch.nn.functional as F
from torch import nn

from ... import ops
from ...config.configurator import configs
from ...graph import EdgePattern, RevaluedView, graph_of, pattern_of
from ..loss_utils import reg_params
from ._graph_cf import GraphCF

init = nn.init.xavier_uniform_


def _draw(fn, *args, device, on_device, **kw):
    """a draw with the reference's call on the CPU generator, moved to the device -- or made there (model.device_rng)"""
    if on_device:
        return fn(*args, device=device, **kw)
    return fn(*args, **kw).to(device)


class AutoCF(GraphCF):
    def __init__(self, data_handler):
        super().__init__(data_handler)               # user_embeds, item_embeds: the reference's first two draws (:15-16)
        model_cfg = configs['model']
        self.gcn_layer = model_cfg['gcn_layer']
        self.gt_layer = model_cfg['gt_layer']
        self.ssl_reg = model_cfg['ssl_reg']
        self.gcnLayers = nn.Sequential(*[GCNLayer() for i in range(self.gcn_layer)])
        self.gtLayers = nn.Sequential(*[GTLayer() for i in range(self.gt_layer)])
        self.masker = RandomMaskSubgraphs(on_device=self.device_rng is not None)
        self.sampler = LocalGraph(on_device=self.device_rng is not None)
        self._all_one = None

    def _graph(self):
        return graph_of(self.adj)

    def make_all_one_adj(self):
        """the adjacency's pattern with every value 1 (:32-36), as a view of the cached plan"""
        if self._all_one is None or self._all_one.graph is not self._graph():
            g = self._graph()
            self._all_one = RevaluedView(g, t.ones(g.nnz, dtype=t.float32, device=g.device))
        return self._all_one

    @property
    def all_one_adj(self):
        return self.make_all_one_adj()

    def get_ego_embeds(self):
        return self._stacked_tables(alias_ok=True)

    def sample_subgraphs(self):
        return self.sampler(self.all_one_adj, self.get_ego_embeds())

    def mask_subgraphs(self, seeds):
        return self.masker(self.adj, seeds)

    def forward(self, encoder_adj, decoder_adj=None):
        if not self.is_training and self.final_embeds is not None:
            return self._split(self.final_embeds)
        embeds = self.get_ego_embeds()
        embedsLst = [embeds]
        for gcn in self.gcnLayers:
            embedsLst.append(gcn(encoder_adj, embedsLst[-1]))
        if decoder_adj is not None:
            for gt in self.gtLayers:
                embedsLst.append(gt(decoder_adj, embedsLst[-1]))
        embeds = sum(embedsLst)
        self.final_embeds = embeds
        return self._split(embeds)

    def contrast(self, nodes, allEmbeds, allEmbeds2=None):
        """log(sum_j exp(<p, all_j>)).mean() over the picked rows (:60-68)"""
        if allEmbeds2 is not None:
            return t.logsumexp(allEmbeds[nodes] @ allEmbeds2.T, dim=-1).mean()
        return t.logsumexp(allEmbeds[t.unique(nodes)] @ allEmbeds.T, dim=-1).mean()

    def cal_loss(self, batch_data, encoder_adj, decoder_adj):
        self.is_training = True
        self._begin_step()
        user_embeds, item_embeds = self.forward(encoder_adj, decoder_adj)
        ancs, poss, _ = batch_data
        anc_embeds = user_embeds[ancs]
        pos_embeds = item_embeds[poss]
        rec_loss = (-t.sum(anc_embeds * pos_embeds, dim=-1)).mean()
        reg_loss = reg_params(self) * self.reg_weight
        cl_loss = (self.contrast(ancs, user_embeds) + self.contrast(poss, item_embeds)) * self.ssl_reg + self.contrast(ancs, user_embeds, item_embeds)
        loss = rec_loss + reg_loss + cl_loss
        losses = {'rec_loss': rec_loss, 'reg_loss': reg_loss, 'cl_loss': cl_loss}
        return loss, losses

    def _embeddings_for_eval(self):
        self._stacked_e0 = None          # (evaluation never reuses a training step's concatenated tables)
        if self.is_training:
            self.final_embeds = None
            self.is_training = False
        with t.no_grad():
            return self.forward(self.adj, self.adj)                                                     # :83

    def full_predict(self, batch_data):
        users, items = self._embeddings_for_eval()
        return self._score_all_items(users, items, batch_data)

    def train(self, mode=True):
        if mode:                         # back to training: the evaluation cache is stale
            self.is_training = True
        return super().train(mode)


class GCNLayer(nn.Module):
    def forward(self, adj, embeds):
        return ops.spmm(adj, embeds)                                                                    # :96


class GTLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.head_num = configs['model']['head_num']
        self.embedding_size = configs['model']['embedding_size']
        self.qTrans = nn.Parameter(init(t.empty(self.embedding_size, self.embedding_size)))
        self.kTrans = nn.Parameter(init(t.empty(self.embedding_size, self.embedding_size)))
        self.vTrans = nn.Parameter(init(t.empty(self.embedding_size, self.embedding_size)))

    def forward(self, adj, embeds):
        """adj: an EdgePattern (the masker's decoder graph) or a torch sparse adjacency, whose pattern is cached on it"""
        pattern = adj if isinstance(adj, EdgePattern) else pattern_of(adj)
        return ops.edge_attention(pattern, embeds @ self.qTrans, embeds @ self.kTrans, embeds @ self.vTrans, self.head_num)


class LocalGraph(nn.Module):
    def __init__(self, on_device=False):
        super().__init__()
        self.seed_num = configs['model']['seed_num']
        self.on_device = on_device

    def makeNoise(self, scores):
        noise = _draw(t.rand, scores.shape, device=scores.device, on_device=self.on_device)             # :137
        noise[noise == 0] = 1e-8
        noise = -t.log(-t.log(noise))
        return t.log(scores) + noise

    def forward(self, allOneAdj, embeds):
        """allOneAdj: the all-ones view of the adjacency (no self loops); embeds: the zero-order embeddings (:142-156)"""
        view = allOneAdj if isinstance(allOneAdj, RevaluedView) else graph_of(allOneAdj)
        counts = getattr(view, '_autocf_counts', None)
        if counts is None:                                       # neighbour counts do not depend on the embeddings: once per view
            with t.no_grad():
                one = t.ones(view.shape[0], 1, dtype=t.float32, device=embeds.device)
                order = ops.spmm(view, one)
                fstNum = order
                scdNum = (ops.spmm(view, fstNum) - fstNum) - order
            counts = view._autocf_counts = (order, fstNum + scdNum + 1e-8)
        order, denom = counts
        fstEmbeds = ops.spmm(view, embeds) - embeds
        scdEmbeds = (ops.spmm(view, fstEmbeds) - fstEmbeds) - order * embeds
        subgraphEmbeds = (fstEmbeds + scdEmbeds) / denom
        subgraphEmbeds = F.normalize(subgraphEmbeds, p=2)
        embeds = F.normalize(embeds, p=2)
        scores = t.sigmoid(t.sum(subgraphEmbeds * embeds, dim=-1))
        scores = self.makeNoise(scores)
        _, seeds = t.topk(scores, self.seed_num)
        return scores, seeds


class RandomMaskSubgraphs(nn.Module):
    def __init__(self, on_device=False):
        super().__init__()
        self.mask_depth = configs['model']['mask_depth']
        self.keep_rate = configs['model']['keep_rate']
        self.user_num = configs['data']['user_num']
        self.item_num = configs['data']['item_num']
        self.on_device = on_device

    @staticmethod
    def masked_entries(rows, cols, seeds, n, mask_depth):
        """the reference's per-seed loop (:180-198) as set operations per depth: (keep [nnz] bool, list of mask-node tensors).
        Removing every entry that touches one of the current seeds, seed after seed, removes exactly the entries with an end in
        the seed SET; the next seeds are the unique ends of the removed entries (not collected at the last depth)."""
        keep = t.ones(rows.shape[0], dtype=t.bool, device=rows.device)
        maskNodes = [seeds]
        cur = seeds
        for i in range(mask_depth):
            flag = t.zeros(n, dtype=t.bool, device=rows.device)
            flag[cur] = True
            hit = keep & (flag[rows] | flag[cols])
            keep = keep & ~hit
            if i != mask_depth - 1:
                cur = t.unique(t.concat([rows[hit], cols[hit]]))
                maskNodes.append(cur)
        return keep, maskNodes

    @staticmethod
    def normalized_values(rows, cols, keep, n):
        """values of the kept entries after normalizeAdj (:167-172), 0 for the removed ones, in entry order"""
        degree = t.pow(t.bincount(rows[keep], minlength=n).float() + 1e-12, -0.5)
        return keep.float() * degree[rows] * degree[cols]

    def mask(self, rows, cols, seeds):
        """the masker on an entry list (int64 rows / cols on any device, the caller's order): (keep [nnz] bool, mask nodes (sorted,
        unique), decoder rows, decoder cols) -- the decoder's entries in the order of their keys row * N + col (:199-229)"""
        dev = rows.device
        n, nnz = self.user_num + self.item_num, rows.shape[0]
        keep, maskNodes = self.masked_entries(rows, cols, seeds.to(dev), n, self.mask_depth)
        sampNum = int(n * self.keep_rate)
        sampedNodes = _draw(t.randint, n, size=[sampNum], device=dev, on_device=self.on_device)         # :200
        maskNodes.append(sampedNodes)
        maskNodes = t.unique(t.concat(maskNodes))
        temNum = maskNodes.shape[0]
        temRows = maskNodes[_draw(t.randint, temNum, size=[nnz], device=dev, on_device=self.on_device)]     # :219-220
        temCols = maskNodes[_draw(t.randint, temNum, size=[nnz], device=dev, on_device=self.on_device)]
        every = t.arange(n, device=dev)
        newRows = t.concat([temRows, temCols, every, rows[keep]])
        newCols = t.concat([temCols, temRows, every, cols[keep]])
        hashVal = t.unique(newRows * n + newCols)                # filter duplicated: sorted keys, the pattern's fast path
        newCols = hashVal % n
        newRows = (hashVal - newCols) // n
        return keep, maskNodes, newRows, newCols

    def forward(self, adj, seeds):
        """(encoder_adj, decoder_adj): the adjacency without the masked subgraphs, re-normalized (:216), as a RevaluedView of its
        cached plan; the decoder graph (:232) as an EdgePattern."""
        graph = graph_of(adj)
        dev = graph.device
        idx = getattr(graph, '_autocf_coo', None)
        if idx is None:                                          # the entry list in the caller's order, once per graph
            idx = graph._autocf_coo = adj._indices().to(dev).long()
        rows, cols = idx[0], idx[1]
        n = self.user_num + self.item_num
        keep, maskNodes, newRows, newCols = self.mask(rows, cols, seeds)
        encoder_adj = RevaluedView(graph, self.normalized_values(rows, cols, keep, n))
        self.last = {'keep': keep, 'mask_nodes': maskNodes}      # (for inspection: what the last call removed)
        return encoder_adj, EdgePattern(newRows, newCols, n)
