"""DataHandlerKG: the knowledge-graph scenario's data handler for KGIN -- the contract of the non-diffusion branch of the reference's
data_utils/data_handler_kg.py (:231, :258-268; :33-43 the interaction files, :84-93 the dictionaries, :95-119 the triplets, :121-138 and
:171-177 the graphs): attributes kg_edges (h, t, r), ui_edges, kg_dict, ui_mat, train_user_dict, test_user_dict, train_dataloader,
test_dataloader; sets configs['data']['user_num' / 'item_num' / 'entity_num' / 'node_num' / 'relation_num' / 'triplet_num'].

Triplets are made unique, their inverses are added with the relation offset by max + 1, and both sets are shifted by one for the interact
relation, exactly as upstream.  `kg_edges` is an int64 [E, 3] array and `ui_edges` an int64 [n, 2] array (upstream: lists of lists with
the same rows).  Built ONCE here for the model: `rel_graph`, the graph.RelGraph of the typed edges with relation r - 1 (the three edge
orders of csrc/kgin.hip), and `interact_mat`, the [user_num, entity_num] matrix D^-1 A of kgin.py:238-259 as a torch sparse tensor on
configs['device'] that already carries its SpMM plan.

Real data: ./datasets/kg/{mind,alibaba-fashion,last-fm}_kg/{train.txt,test.txt,kg_final.txt}.  `configs['data']['synthetic']` = one
of synth.KG_SHAPES generates seeded data in memory.  The diffusion branch (model.diff_model) and the TransR branch (model.train_trans)
of the reference handler are refused by name.

Training batches: datasets_general_cf.PairwiseTrnData over the train pairs in file order and the loader choice of the general-CF
handler.  The reference's KGTrainDataset.sample_negs draws np.random.randint(item_num) per pair until the item is unseen -- the same
stream, so ExactPairwiseLoader gives the reference's negatives.  Evaluation: AllRankTstData(tst_mat, trn_mat), so Metric is untouched
and the device top-k path works.  The reference instead ships bare user ids (KGTestDataset), masks from user_history_lists and goes
through test.eval_at_one_forward; both push the train items to -1e8 under the same scores.  The yml key is kept and is not read."""
from collections import defaultdict
from os import path

import numpy as np
import scipy.sparse as sp
import torch as t
import torch.utils.data as data

from ..config.configurator import configs
from ..graph import RelGraph, graph_of
from .datasets_general_cf import AllRankTstData, ExactPairwiseLoader, FastPairwiseLoader, PairwiseTrnData
from . import synth

DATASETS = ('mind', 'alibaba-fashion', 'last-fm')


def si_norm_interact(ui_edges, n_users, n_entities):
    """D^-1 A of the user -> item edges as a [n_users, n_entities] COO matrix (kgin.py:238-253: the reference builds it on the
    [n_nodes, n_nodes] graph and cuts the user rows / entity columns out; the entries, their row-major order and their float64 values
    1 / degree are the same).  A repeated pair is summed, a user without edges keeps an empty row."""
    ui_edges = np.asarray(ui_edges, dtype=np.int64)
    adj = sp.coo_matrix((np.ones(len(ui_edges)), (ui_edges[:, 0], ui_edges[:, 1])), shape=(n_users, n_entities)).tocsr()
    deg = np.asarray(adj.sum(axis=1), dtype=np.float64).reshape(-1)
    inv = np.zeros_like(deg)
    np.divide(1.0, deg, out=inv, where=deg != 0)
    return sp.diags(inv).dot(adj).tocoo()


class DataHandlerKG:
    def __init__(self):
        model_cfg = configs['model']
        if model_cfg.get('diff_model') == 1:
            raise NotImplementedError("the kg data handler's diffusion branch (model.diff_model, DiffKG) is not implemented")
        if model_cfg.get('train_trans'):
            raise NotImplementedError("the kg data handler's triplet loader (model.train_trans, the TransR step of KGCL) is not implemented")
        name = configs['data']['name']
        self.synthetic = configs['data'].get('synthetic')
        if self.synthetic is not None and self.synthetic not in synth.KG_SHAPES:
            raise ValueError("unknown synthetic kg shape '%s' (one of %s)" % (self.synthetic, ', '.join(sorted(synth.KG_SHAPES))))
        if self.synthetic is None and name not in DATASETS:
            raise ValueError("unknown kg dataset '%s' (%s, or set data.synthetic)" % (name, '|'.join(DATASETS)))
        predir = './datasets/kg/%s_kg/' % (name if self.synthetic is None else 'synthetic')
        configs['data']['dir'] = predir
        self.trn_file = path.join(predir, 'train.txt')
        self.val_file = path.join(predir, 'test.txt')
        self.tst_file = path.join(predir, 'test.txt')
        self.kg_file = path.join(predir, 'kg_final.txt')
        self.train_user_dict = defaultdict(list)
        self.test_user_dict = defaultdict(list)

    def _read_cf(self, file_name):
        """[n, 2] (user, item) pairs of a file with one line `user item item ...` per user: the lines in file order, a line's items made
        unique through a set and listed in that set's order (:33-43)"""
        pairs = []
        with open(file_name, 'r') as fs:
            for line in fs:
                ids = [int(x) for x in line.strip().split(' ')]
                pairs.extend([ids[0], i_id] for i_id in list(set(ids[1:])))
        return np.array(pairs)

    def _collect_ui_dict(self, train_data, test_data):
        """user_num / item_num = largest id + 1 over both files; user -> items of either file in pair order (:84-93)"""
        configs['data']['user_num'] = int(max(train_data[:, 0].max(), test_data[:, 0].max())) + 1
        configs['data']['item_num'] = int(max(train_data[:, 1].max(), test_data[:, 1].max())) + 1
        for pairs, store in ((train_data, self.train_user_dict), (test_data, self.test_user_dict)):
            for u_id, i_id in pairs.tolist():
                store[u_id].append(i_id)

    def _read_triplets(self, file_name):
        return self._full_triplets(np.unique(np.loadtxt(file_name, dtype=np.int32, ndmin=2), axis=0))

    def _full_triplets(self, canonical):
        """:99-119 from the unique canonical triplets (h, r, t): every triplet again in the inverse direction under relation
        r + max(r) + 1, then + 1 on every relation, which frees relation 0 for `interact`; canonical triplets first, inverse ones after.
        Sets entity_num, node_num, relation_num, triplet_num."""
        canonical = np.array(canonical, dtype=np.int32)
        n_canonical_rel = int(canonical[:, 1].max()) + 1
        inverse = np.stack([canonical[:, 2], canonical[:, 1] + n_canonical_rel, canonical[:, 0]], axis=1)
        triplets = np.concatenate((canonical, inverse), axis=0)
        triplets[:, 1] += 1
        n_entities = int(max(triplets[:, 0].max(), triplets[:, 2].max())) + 1
        configs['data']['entity_num'] = n_entities
        configs['data']['node_num'] = n_entities + configs['data']['user_num']
        configs['data']['relation_num'] = int(triplets[:, 1].max()) + 1
        configs['data']['triplet_num'] = len(triplets)
        return triplets

    def _build_graphs(self, train_data, triplets):
        """kg_edges [E, 3] as (h, t, r), ui_edges [n, 2], kg_dict: head -> [(r, t), ...] (:121-138)"""
        triplets = np.asarray(triplets, dtype=np.int64)
        kg_edges = np.stack([triplets[:, 0], triplets[:, 2], triplets[:, 1]], axis=1)
        ui_edges = np.asarray(train_data, dtype=np.int64).copy()
        kg_dict = defaultdict(list)
        for h_id, r_id, t_id in triplets.tolist():
            kg_dict[h_id].append((r_id, t_id))
        return kg_edges, ui_edges, kg_dict

    def _build_ui_mat(self, ui_edges):
        """[user_num, item_num] COO matrix of ones, entries in pair order (:171-177)"""
        ui_edges = np.asarray(ui_edges)
        return sp.coo_matrix((np.ones(len(ui_edges)), (ui_edges[:, 0], ui_edges[:, 1])), shape=(configs['data']['user_num'], configs['data']['item_num']))

    def load_data(self):
        if self.synthetic is not None:
            seed = configs['data'].get('synthetic_seed', 2023)
            train_cf, test_cf, can_triplets = synth.make_kg_dataset(self.synthetic, seed, configs['data'].get('synthetic_test_frac'))
            self._collect_ui_dict(train_cf, test_cf)
            kg_triplets = self._full_triplets(can_triplets)
        else:
            train_cf = self._read_cf(self.trn_file)
            test_cf = self._read_cf(self.tst_file)
            self._collect_ui_dict(train_cf, test_cf)
            kg_triplets = self._read_triplets(self.kg_file)
        data_cfg = configs['data']
        if data_cfg['entity_num'] < data_cfg['item_num']:
            raise ValueError('the knowledge graph names %d entities, fewer than the %d items' % (data_cfg['entity_num'], data_cfg['item_num']))
        self.kg_edges, self.ui_edges, self.kg_dict = self._build_graphs(train_cf, kg_triplets)
        self.ui_mat = self._build_ui_mat(self.ui_edges)

        if configs['train']['loss'] != 'pairwise':
            raise NotImplementedError("train.loss '%s'" % configs['train']['loss'])
        n_users, n_items = data_cfg['user_num'], data_cfg['item_num']
        self.trn_mat = self.ui_mat                              # entries in file order: the order of the training pairs
        test_cf = np.asarray(test_cf)
        self.tst_mat = sp.coo_matrix((np.ones(len(test_cf)), (test_cf[:, 0], test_cf[:, 1])), shape=(n_users, n_items))
        trn_data = PairwiseTrnData(self.trn_mat)
        tst_data = AllRankTstData(self.tst_mat, self.trn_mat)
        self.test_dataloader = data.DataLoader(tst_data, batch_size=configs['test']['batch_size'], shuffle=False, num_workers=0)
        dev = configs['device'] if str(configs['device']).startswith('cuda') else None
        if configs['train'].get('fast_loader'):
            self.train_dataloader = FastPairwiseLoader(trn_data, configs['train']['batch_size'], device=dev)
        elif not configs['train'].get('torch_dataloader'):
            self.train_dataloader = ExactPairwiseLoader(trn_data, configs['train']['batch_size'], device=dev)
        else:
            self.train_dataloader = data.DataLoader(trn_data, batch_size=configs['train']['batch_size'], shuffle=True, num_workers=0)

        # what the model needs, built once: the typed graph in its three orders and the plan of the [U, N] interaction matrix
        self.rel_graph = RelGraph(self.kg_edges[:, 0], self.kg_edges[:, 1], self.kg_edges[:, 2] - 1, data_cfg['entity_num'],
                                  data_cfg['relation_num'] - 1, device=configs['device'] if dev is not None else 'cpu')
        coo = si_norm_interact(self.ui_edges, n_users, data_cfg['entity_num'])
        idxs = t.from_numpy(np.vstack([coo.row, coo.col]).astype(np.int64))
        self.interact_mat = t.sparse_coo_tensor(idxs, t.from_numpy(coo.data).float(), coo.shape, check_invariants=False).to(configs['device'])
        if self.interact_mat.is_cuda:
            graph_of(self.interact_mat)
