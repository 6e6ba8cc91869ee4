"""GFormer on the HIP path; interface of the reference's models/general_cf/gformer.py (:16-503): GFormer(data_handler),
forward(handler, is_test, sub, cmp, encoderAdj, decoderAdj=None), cal_loss(batch, encoder_adj, decoder_adj, sub, cmp), full_predict(batch),
getEgoEmbeds(), preSelect_anchor_set(), get_random_anchorset(), the module classes GCNLayer, PNNLayer, GTLayer, LocalGraph and
RandomMaskSubgraphs, the loss dictionary keys and the parameter names, drawn in the constructor's order (:37-44): uEmbeds, iEmbeds,
gtLayers.{q,k,v}Trans, pnnLayers.{i}.linear_out, pnnLayers.{i}.linear_hidden, localGraph.pnn.*.  The unused linear_out exists, is drawn
and is regularised, as upstream; gtLayers is shared with localGraph.gt_layer and counted once.  Underneath,

  reference                                                        here
  get_random_anchorset: a networkx graph, one Python BFS per        ops.anchor_hops (csrc/bfs.hip): one bit-parallel multi-source BFS on
  anchor, a Python double loop over [A, N] (:152-176)               the device, int16 hops [N, A]; `dists_array()` rebuilds the float64
                                                                   array on request
  PNNLayer: [N, A, d] and [N, A, 2d] tensors, a Linear over         ops.anchor_position_features (csrc/pnn.hip): the Linear commuted past
  N * A rows, the [A, N] array uploaded per call (:202-218)         the mean, two [N, d] halves, then one F.linear over N rows
  GTLayer: gathers, [E, d] GEMMs, index_add_ (:235-255)             AutoCF's ops.edge_attention (csrc/gt.hip) on an EdgePattern
  LocalGraph: atten [E, H] of the layer, summed (:351-352)          ops.edge_attention_scores (csrc/gt.hip): fp32 [E], nothing E x H
  masker: three Python `while` loops over all entries, scipy        one boolean mask each; the three matrices are re-valuations of
  matrices rebuilt and re-normalised three times (:378-503)         add_adj's pattern: ONE native plan per resampling + 3 RevaluedViews

The self feature of the PNN layer is a cyclic window, not the row itself: element [n, a] of `embeds.repeat(A, 1).reshape(-1, A, d)` is
row (n A + a) mod N.  A kept diagonal entry has the value 2 before the normalisation: add_adj already holds the whole
diagonal and the encoder / sub / cmp matrices prepend arange(N) again (:411-416, :442-461).  The GT layer attends over the PATTERNS of sub /
cmp / decoderAdj: dropped entries are absent there, not zero-valued.

Random draws: every draw of the model is numpy's global generator, with the reference's calls, sizes and order -- np.random.choice for
the anchors (:154), the two addRate draws of LocalGraph (:336-337), and in the masker the weighted draw without replacement (:436), the
two ext draws (:474-475), the two reRate draws (:483-484) and one weighted draw per create_sub_adj (:388).  The probability vectors
are the reference's numpy float32 expressions on the CPU copy of the scores, including its in-place clamp at 3, which the later
create_sub_adj calls see (:385, :432).  The decoder's rows are recovered with an integer division; the reference's float division
(:495) is exact only while N^2 < 2^24.  model.device_rng is not supported by this model."""
import numpy as np
import torch as t
import torch.nn.functional as F
from torch import nn

from ... import ops
from ...config.configurator import configs
from ...graph import EdgePattern, PropGraph, RevaluedView, graph_of, pattern_of
from ..base_model import BaseModel
from ..loss_utils import reg_params

init = nn.init.xavier_uniform_


class MaskedAdj:
    """one matrix of a resampling: `view` = its values on add_adj's native plan (entries it lacks are 0) for ops.spmm, `pattern` = the
    EdgePattern of the entries it HAS for the GT layer, `entries` = (rows, cols, vals) on the host in coalesced order"""

    def __init__(self, view, pattern, entries):
        self.view, self.pattern, self.entries = view, pattern, entries
        self.shape = pattern.shape if pattern is not None else view.shape


class AddedAdj:
    """LocalGraph's add_adj: the coalesced pattern on the host (int64 rows / cols, sorted by row, then column) and as an EdgePattern"""

    def __init__(self, rows, cols, n, pattern):
        self.rows, self.cols, self.n, self.pattern = rows, cols, n, pattern
        self.shape = (n, n)
        self.nnz = rows.shape[0]


class GFormer(BaseModel):
    def __init__(self, data_handler):
        super().__init__(data_handler)
        self.adj = data_handler.torch_adj
        self.handler = data_handler
        model_cfg = configs['model']
        if model_cfg.get('device_rng'):
            raise NotImplementedError('model.device_rng is not supported by GFormer: its draws are numpy\'s, in the reference\'s order')
        self.layer_num = model_cfg['layer_num']
        self.pnn_layer = model_cfg['pnn_layer']
        self.reg_weight = model_cfg['reg_weight']
        self.keep_rate = model_cfg['keep_rate']
        self.gtw = model_cfg['gtw']
        self.anchor_set_num = model_cfg['anchor_set_num']
        self.ctra = model_cfg['ctra']
        self.ssl_reg = model_cfg['ssl_reg']
        self.reg = model_cfg['reg_weight']
        self.b2 = model_cfg['b2']
        self.batch_train = configs['train']['batch_size']

        self.uEmbeds = nn.Parameter(init(t.empty(self.user_num, self.embedding_size)))
        self.iEmbeds = nn.Parameter(init(t.empty(self.item_num, self.embedding_size)))
        self.gcnLayers = nn.Sequential(*[GCNLayer() for i in range(self.layer_num)])
        self.gcnLayer = GCNLayer()
        self.gtLayers = GTLayer(data_handler)
        self.pnnLayers = nn.Sequential(*[PNNLayer(data_handler) for i in range(self.pnn_layer)])
        self.localGraph = LocalGraph(data_handler, self.gtLayers)
        self.masker = RandomMaskSubgraphs(data_handler)
        self.is_training = True
        self.final_embeds = None

    def getEgoEmbeds(self):
        return t.cat([self.uEmbeds, self.iEmbeds], axis=0)

    def forward(self, handler, is_test, sub, cmp, encoderAdj, decoderAdj=None):
        embeds = t.cat([self.uEmbeds, self.iEmbeds], axis=0)
        embedsLst = [embeds]
        cList = subList = None
        if not is_test:                  # prediction discards cList / subList (:78): the two GT passes over adj are skipped there
            emb, _ = self.gtLayers(cmp, embeds)
            cList = [embeds, self.gtw * emb]
            emb, _ = self.gtLayers(sub, embeds)
            subList = [embeds, self.gtw * emb]
        for gcn in self.gcnLayers:
            embeds = gcn(encoderAdj, embedsLst[-1])
            if not is_test:
                subList.append(gcn(sub, embedsLst[-1]))
                cList.append(gcn(cmp, embedsLst[-1]))
            embedsLst.append(embeds)
        if is_test is False:
            for pnn in self.pnnLayers:
                embedsLst.append(pnn(handler, embedsLst[-1]))
        if decoderAdj is not None:
            embeds, _ = self.gtLayers(decoderAdj, embedsLst[-1])
            embedsLst.append(embeds)
        embeds = sum(embedsLst)
        if not is_test:
            cList, subList = sum(cList), sum(subList)
        return embeds[:self.user_num], embeds[self.user_num:], cList, subList

    def _embeddings_for_eval(self):
        if self.is_training or self.final_embeds is None:
            self.is_training = False
            with t.no_grad():
                user_embeds, item_embeds, _, _ = self.forward(self.handler, True, self.adj, self.adj, self.adj)       # :78
            self.final_embeds = (user_embeds, item_embeds)
        return self.final_embeds

    def full_predict(self, batch_data):
        user_embeds, item_embeds = self._embeddings_for_eval()
        pck_users, train_mask = batch_data
        if user_embeds.is_cuda and type(self)._mask_predict is BaseModel._mask_predict:
            return ops.full_predict(user_embeds, item_embeds, pck_users.long(), train_mask)
        return self._mask_predict(user_embeds[pck_users.long()] @ item_embeds.T, train_mask)

    def predict_topk(self, users, k, trn_csr_device):
        """top-k unseen items without the dense train mask (GraphCF.predict_topk)"""
        user_embeds, item_embeds = self._embeddings_for_eval()
        if int(k) > ops.EVAL_KMAX:
            raise ValueError('predict_topk: k = %d exceeds the kernel\'s %d' % (int(k), ops.EVAL_KMAX))
        return ops.eval_topk(user_embeds, item_embeds, users.long(), k, trn_csr_device)

    def train(self, mode=True):
        if mode:                         # back to training: the evaluation cache is stale
            self.is_training = True
            self.final_embeds = None
        return super().train(mode)

    def cal_loss(self, batch_data, encoder_adj, decoder_adj, sub, cmp):
        self.is_training = True
        self.final_embeds = None
        user_embeds, item_embeds, cList, subLst = self.forward(self.handler, False, sub, cmp, encoder_adj, decoder_adj)
        ancs, poss, negs = batch_data
        ancs, poss, negs = ancs.long(), poss.long(), negs.long()
        ancEmbeds = user_embeds[ancs]
        posEmbeds = item_embeds[poss]
        usrEmbeds2 = subLst[:self.user_num]
        itmEmbeds2 = subLst[self.user_num:]
        ancEmbeds2 = usrEmbeds2[ancs]
        posEmbeds2 = itmEmbeds2[poss]
        negEmbeds = item_embeds[negs]

        bprLoss = (-t.sum(ancEmbeds * posEmbeds, dim=-1)).mean()
        scoreDiff = self.pairPredict(ancEmbeds2, posEmbeds2, negEmbeds)
        bprLoss2 = -(scoreDiff).sigmoid().log().sum() / self.batch_train         # (the configured batch size, not len(ancs): :107)
        regLoss = self.calcRegLoss(self) * self.reg
        contrastLoss = (self.contrast(ancs, user_embeds) + self.contrast(poss, item_embeds)) * self.ssl_reg + self.contrast(
            ancs, user_embeds, item_embeds) + self.ctra * self.contrastNCE(ancs, subLst, cList)
        loss = bprLoss + regLoss + contrastLoss + self.b2 * bprLoss2
        loss_dict = {'bpr_loss': bprLoss, 'reg_loss': regLoss, 'cl_loss': contrastLoss}
        return loss, loss_dict

    def pairPredict(self, ancEmbeds, posEmbeds, negEmbeds):
        return self.innerProduct(ancEmbeds, posEmbeds) - self.innerProduct(ancEmbeds, negEmbeds)

    def innerProduct(self, usrEmbeds, itmEmbeds):
        return t.sum(usrEmbeds * itmEmbeds, dim=-1)

    def calcRegLoss(self, model):
        return reg_params(model)

    def contrast(self, nodes, allEmbeds, allEmbeds2=None):
        """log(sum_j exp(<p, all_j>)).mean() over the picked rows (:129-137): AutoCF's expression, as log-sum-exp in torch"""
        if allEmbeds2 is not None:
            return t.logsumexp(allEmbeds[nodes] @ allEmbeds2.T, dim=-1).mean()
        return t.logsumexp(allEmbeds[t.unique(nodes)] @ allEmbeds.T, dim=-1).mean()

    def contrastNCE(self, nodes, allEmbeds, allEmbeds2=None):
        """element-wise (:139-144): log(exp(p * p2).sum(-1)).mean()"""
        return t.logsumexp(allEmbeds[nodes] * allEmbeds2[nodes], dim=-1).mean()

    def get_random_anchorset(self):
        """:152-176.  Leaves handler.anchorset_id (the reference's name, a numpy array), handler.anchor_hops (device, int16 [N, A]) and
        handler.anchor_ids_device (int32); `dists_array()` gives the reference's float64 array on request"""
        n = self.num_nodes
        annchorset_id = np.random.choice(n, size=configs['model']['anchor_set_num'], replace=False)
        self.handler.anchorset_id = annchorset_id
        self.handler.anchor_hops = ops.anchor_hops(self.adj, annchorset_id)
        self.handler.anchor_ids_device = t.from_numpy(annchorset_id.astype(np.int32)).to(self.handler.anchor_hops.device)

    def preSelect_anchor_set(self):
        self.num_nodes = configs['data']['user_num'] + configs['data']['item_num']
        self.get_random_anchorset()

    def dists_array(self):
        """the reference's handler.dists_array (:166-175): float64 [A, N], 1 / (dist + 1), 0 for an unreached node"""
        hops = self.handler.anchor_hops.cpu().numpy().astype(np.int64).T
        return np.where(hops < 0, 0.0, 1.0 / (np.maximum(hops, 0) + 1.0))


def _spmm_operand(adj):
    return adj.view if isinstance(adj, MaskedAdj) else adj


def _pattern_operand(adj):
    if isinstance(adj, MaskedAdj):
        return adj.pattern
    if isinstance(adj, AddedAdj):
        return adj.pattern
    return adj if isinstance(adj, EdgePattern) else pattern_of(adj)


class GCNLayer(nn.Module):
    def forward(self, adj, embeds):
        return ops.spmm(_spmm_operand(adj), embeds)                                                      # :188


class PNNLayer(BaseModel):
    def __init__(self, handler):
        super().__init__(handler)
        self.gtw = configs['model']['gtw']
        self.anchor_set_num = configs['model']['anchor_set_num']
        self.linear_out = nn.Linear(self.embedding_size, self.embedding_size)
        self.linear_hidden = nn.Linear(2 * self.embedding_size, self.embedding_size)
        self.act = nn.ReLU()

    @staticmethod
    def position_features(embeds, anchor_ids, hops):
        """[s, u] [N, 2d] as a pure torch function of any dtype and device (ops._anchor_position_composed): what the kernels compute"""
        return ops._anchor_position_composed(embeds, t.as_tensor(anchor_ids), hops)

    def forward(self, handler, embeds):
        ids = getattr(handler, 'anchor_ids_device', None)
        z = ops.anchor_position_features(embeds, ids if ids is not None else handler.anchorset_id, handler.anchor_hops)
        return F.linear(z, self.linear_hidden.weight, self.linear_hidden.bias)                          # :214-216, commuted


class GTLayer(BaseModel):
    def __init__(self, handler):
        super().__init__(handler)
        self.qTrans = nn.Parameter(init(t.empty(self.embedding_size, self.embedding_size)))
        self.kTrans = nn.Parameter(init(t.empty(self.embedding_size, self.embedding_size)))
        self.vTrans = nn.Parameter(init(t.empty(self.embedding_size, self.embedding_size)))
        self.head = configs['model']['head']

    def forward(self, adj, embeds, flag=False):
        """(resEmbeds, None): the per-entry attention is never stored; LocalGraph asks `scores` for its sum over the heads"""
        pattern = _pattern_operand(adj)
        return ops.edge_attention(pattern, embeds @ self.qTrans, embeds @ self.kTrans, embeds @ self.vTrans, self.head), None

    def scores(self, adj, embeds):
        """t.sum(att, dim=-1) of :235-250 per entry of the pattern, in coalesced order"""
        return ops.edge_attention_scores(_pattern_operand(adj), embeds @ self.qTrans, embeds @ self.kTrans, self.head)


def _coalesced(rows, cols, n):
    """sorted unique keys row * n + col of an entry list, split again (int64, integer division)"""
    key = np.unique(rows.astype(np.int64) * n + cols.astype(np.int64))
    return key // n, key % n


class LocalGraph(BaseModel):
    def __init__(self, handelr, gtLayer):
        super().__init__(handelr)
        self.gt_layer = gtLayer
        self.num_users = self.user_num
        self.num_items = self.item_num
        self.pnn = PNNLayer(handelr)
        self.addRate = configs['model']['addRate']
        self._coo_cache = None                                   # (adjacency, its entry list on the host)

    def add_adj_entries(self, rows, cols):
        """host part of :333-349 on the adjacency's entry list (numpy, the caller's order): the two addRate draws, then the coalesced
        pattern of [added pairs both ways, the diagonal, the adjacency] as (rows, cols) int64"""
        n = self.num_users + self.num_items
        tmp_rows = np.random.choice(rows, size=[int(len(rows) * self.addRate)])
        tmp_cols = np.random.choice(cols, size=[int(len(cols) * self.addRate)])
        every = np.arange(n, dtype=np.int64)
        newRows = np.concatenate([tmp_rows, tmp_cols, every, rows])
        newCols = np.concatenate([tmp_cols, tmp_rows, every, cols])
        return _coalesced(newRows, newCols, n)

    def _host_entries(self, adj):
        """the adjacency's entry list on the host (int64 numpy rows / cols, the caller's order), copied once per adjacency object"""
        cached = self._coo_cache
        if cached is None or cached[0] is not adj:
            cached = self._coo_cache = (adj, adj._indices().detach().cpu().numpy().astype(np.int64))
        return cached[1][0], cached[1][1]

    def forward(self, adj, embeds, handler):
        """(att_edge fp32 [E] in add_adj's coalesced order, add_adj).  The PNN and the attention run without autograd: the reference
        detaches the result (:382, :386)"""
        rows, cols = self._host_entries(adj)
        with t.no_grad():
            embeds = self.pnn(handler, embeds.detach())
            new_rows, new_cols = self.add_adj_entries(rows, cols)
            n = self.num_users + self.num_items
            dev = embeds.device
            pattern = EdgePattern(t.from_numpy(new_rows).to(dev), t.from_numpy(new_cols).to(dev), n)
            add_adj = AddedAdj(new_rows, new_cols, n, pattern)
            att_edge = self.gt_layer.scores(add_adj, embeds)
        return att_edge, add_adj


class RandomMaskSubgraphs(BaseModel):
    def __init__(self, data_handler):
        super().__init__(data_handler)
        self.flag = False
        self.ext = configs['model']['ext']
        self.reRate = configs['model']['reRate']

    @staticmethod
    def normalized_entries(users_up, items_up, keep, n):
        """the matrix csr_matrix(ones, [arange(n) + kept rows, arange(n) + kept cols]) after D^-1/2 . D^-1/2 (:411-423, :442-468) as
        float32 values on the entries of (users_up, items_up): a kept diagonal entry counts twice, an entry that is neither kept nor on
        the diagonal is absent (value 0, has = False).  scipy's arithmetic: float64 (d_inv[r] * count) * d_inv[c], then float32"""
        diag = users_up == items_up
        count = keep.astype(np.float64) + diag.astype(np.float64)
        rowsum = np.bincount(users_up, weights=count, minlength=n)
        with np.errstate(divide='ignore'):
            d_inv = np.power(rowsum, -0.5)
        d_inv[np.isinf(d_inv)] = 0.
        vals = ((d_inv[users_up] * count) * d_inv[items_up]).astype(np.float32)
        return vals, count > 0

    def create_sub_adj_entries(self, users_up, items_up, att_edge, flag, n):
        """:378-425 on the host: (vals float32 [E], has bool [E]); att_edge is the CPU tensor of the scores, clamped IN PLACE when
        flag is False, as upstream"""
        if flag:
            att = (att_edge.detach().cpu() + 0.001).numpy()
        else:
            att_f = att_edge
            att_f[att_f > 3] = 3
            att = 1.0 / (np.exp((att_f.detach().cpu() + 1E-8).numpy()))
        att_f = att / att.sum()
        keep_index = np.random.choice(np.arange(len(users_up)), int(len(users_up) * configs['model']['sub']), replace=False, p=att_f)
        keep = np.zeros(len(users_up), dtype=bool)
        keep[keep_index] = True
        return self.normalized_entries(users_up, items_up, keep, n)

    def mask_entries(self, users_up, items_up, att_edge):
        """the host part of :427-503 on add_adj's entries (numpy int64, coalesced order) and the CPU tensor of the scores (clamped in
        place): {'enc': (vals, has), 'sub': ..., 'cmp': ..., 'dec': (rows, cols), 'keep': bool [E]} with the reference's draws in
        the reference's order"""
        n = self.user_num + self.item_num
        E = len(users_up)
        att_f = att_edge
        att_f[att_f > 3] = 3
        att_f = 1.0 / (np.exp((att_f.detach().cpu() + 1E-8).numpy()))
        att_f1 = att_f / att_f.sum()
        keep_index = np.random.choice(np.arange(E), int(E * configs['model']['keep_rate']), replace=False, p=att_f1)
        keep = np.zeros(E, dtype=bool)                           # the `while` loop of :444-457 as a mask: drop = ~keep
        keep[keep_index] = True
        every = np.arange(n, dtype=np.int64)
        rows = np.concatenate([every, users_up[keep]])           # (users_up[sorted keep_index])
        cols = np.concatenate([every, items_up[keep]])
        enc = self.normalized_entries(users_up, items_up, keep, n)
        drop_row_ids, drop_col_ids = users_up[~keep], items_up[~keep]
        ext_rows = np.random.choice(rows, size=[int(len(drop_row_ids) * self.ext)])
        ext_cols = np.random.choice(cols, size=[int(len(drop_col_ids) * self.ext)])
        tmp_rows = np.concatenate([ext_rows, drop_row_ids])
        tmp_cols = np.concatenate([ext_cols, drop_col_ids])
        new_rows = np.random.choice(tmp_rows, size=[int(E * self.reRate)])
        new_cols = np.random.choice(tmp_cols, size=[int(E * self.reRate)])
        newRows = np.concatenate([new_rows, new_cols, every, rows])
        newCols = np.concatenate([new_cols, new_rows, every, cols])
        dec = _coalesced(newRows, newCols, n)                    # t.unique(hashVal), rows by integer division
        sub = self.create_sub_adj_entries(users_up, items_up, att_edge, True, n)
        cmp = self.create_sub_adj_entries(users_up, items_up, att_edge, False, n)
        return {'enc': enc, 'sub': sub, 'cmp': cmp, 'dec': dec, 'keep': keep}

    def forward(self, adj, att_edge):
        """(encoderAdj, decoderAdj, sub, cmp) from LocalGraph's (add_adj, att_edge): three MaskedAdj on ONE native plan of add_adj's
        pattern and the decoder as a MaskedAdj with a pattern only.  att_edge is clamped at 3 in place, as upstream"""
        dev = att_edge.device
        att_cpu = att_edge.detach().cpu()
        out = self.mask_entries(adj.rows, adj.cols, att_cpu)
        att_edge.clamp_(max=3)                                   # the caller's tensor sees the clamp too (:431-432)
        n = adj.n
        graph = PropGraph(adj.rows, adj.cols, np.ones(adj.nnz, dtype=np.float32), (n, n), dev)
        rows_d, cols_d = adj.pattern.coo()

        def masked(key, with_pattern):
            vals, has = out[key]
            view = RevaluedView(graph, t.from_numpy(vals).to(dev))
            pattern = None
            if with_pattern:
                has_d = t.from_numpy(has).to(dev)
                pattern = EdgePattern(rows_d[has_d], cols_d[has_d], n)
            return MaskedAdj(view, pattern, (adj.rows[has], adj.cols[has], vals[has]))
        encoderAdj = masked('enc', False)
        sub, cmp = masked('sub', True), masked('cmp', True)
        d_rows, d_cols = out['dec']
        decoderAdj = MaskedAdj(None, EdgePattern(t.from_numpy(d_rows).to(dev), t.from_numpy(d_cols).to(dev), n), (d_rows, d_cols, None))
        return encoderAdj, decoderAdj, sub, cmp
