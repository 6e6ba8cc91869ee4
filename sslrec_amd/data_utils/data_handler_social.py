"""DataHandlerSocial: the social scenario's data handler for MHCN -- the contract of the reference's
data_utils/data_handler_social.py for model.name == 'mhcn' (:16-30 the files, :363-380 loading and the loaders, :98-137 and :530-538 the
matrices): attributes trn_mat, trust_mat, H_s, H_j, H_p, R, train_dataloader, test_dataloader (no validation set: Trainer.evaluate
falls back to the test loader); sets configs['data']['user_num'/'item_num'].

The three motif-induced adjacencies and the joint adjacency R are built ONCE on the host with scipy (`motif_matrices`,
`motif_adjacencies`, `joint_adjacency`) and handed to the HIP SpMM as torch sparse tensors on configs['device'] that already carry
their propagation plans (graph.graph_of); `R_t` is the PropGraph.transposed view of R's plan for R^T.  `trn_mat` is used with the values
it holds (ratings if it holds ratings), as upstream: R and Y Y^T see them.  Rows of an H without entries stay empty: the reference
multiplies them by 1 / 0 = inf, which touches no stored entry; here the reciprocal of an empty row's sum is never formed.

Real data: ./datasets/social/{ciao,epinions,yelp,lastfm}/{trn_mat,tst_mat,trust_mat}.pkl (category.pkl is not read: MHCN does not use
it).  `configs['data']['synthetic']` = one of synth.SOCIAL_SHAPES generates seeded matrices in memory.  The other social models of the
reference (dsl, dcrec, kcgn, smin) need inputs this handler does not build and are refused by name.

Training batches: datasets_general_cf.PairwiseTrnData / AllRankTstData and the loader choice of the general-CF handler -- the
reference's social dataset classes (datasets_social.py:6-50) are the same statements, so the batch stream is the reference's."""
import pickle

import numpy as np
import scipy.sparse as sp
import torch as t
import torch.utils.data as data

from ..config.configurator import configs
from ..graph import graph_of
from .datasets_general_cf import AllRankTstData, ExactPairwiseLoader, FastPairwiseLoader, PairwiseTrnData
from . import synth

DATASETS = ('ciao', 'epinions', 'yelp', 'lastfm')
UNSUPPORTED_MODELS = ('dsl', 'dcrec', 'kcgn', 'smin')


def _csr(m):
    m = sp.csr_matrix(m, dtype=np.float64)
    m.sum_duplicates()
    m.eliminate_zeros()
    return m


def motif_matrices(trust_mat, trn_mat):
    """[A1, ..., A10] of :99-117 as float64 CSR matrices without explicit zeros: the seven triangle motifs of the trust graph S (B = its
    reciprocated part, U = the one-way part), and the three user-user motifs through a shared item (Y Y^T on reciprocated pairs, on
    one-way pairs in either direction, and on pairs without a trust edge, the diagonal included)"""
    S, Y = _csr(trust_mat), _csr(trn_mat)
    B = _csr(S.multiply(S.T))
    U = _csr(S - B)
    Ut, UU, BB = U.T.tocsr(), U.dot(U), B.dot(B)
    BU, UB = B.dot(U), U.dot(B)
    C1 = UU.multiply(Ut)
    A1 = C1 + C1.T
    C2 = BU.multiply(Ut) + UB.multiply(Ut) + UU.multiply(B)
    A2 = C2 + C2.T
    C3 = BB.multiply(U) + BU.multiply(B) + UB.multiply(B)
    A3 = C3 + C3.T
    A4 = BB.multiply(B)
    UUt, UtU = U.dot(Ut), Ut.dot(U)
    C5 = UU.multiply(U) + UUt.multiply(U) + UtU.multiply(U)
    A5 = C5 + C5.T
    A6 = UB.multiply(U) + B.dot(Ut).multiply(Ut) + UtU.multiply(B)
    A7 = Ut.dot(B).multiply(Ut) + BU.multiply(U) + UUt.multiply(B)
    YY = Y.dot(Y.T)
    A8 = YY.multiply(B)
    A9 = YY.multiply(U)
    A9 = A9 + A9.T
    A10 = YY - A8 - A9
    return [_csr(a) for a in (A1, A2, A3, A4, A5, A6, A7, A8, A9, A10)]


def _row_normalized(H):
    """H with every row multiplied by the reciprocal of its sum (:120); a row whose sum is 0 stays as it is (empty)"""
    H = _csr(H)
    sums = np.asarray(H.sum(axis=1)).reshape(-1)
    inv = np.zeros_like(sums)
    np.divide(1.0, sums, out=inv, where=sums != 0)
    H.data = H.data * np.repeat(inv, np.diff(H.indptr))
    if not np.all(np.isfinite(H.data)):
        raise ValueError('a motif adjacency holds a non-finite value')
    return H


def motif_adjacencies(trust_mat, trn_mat, motifs=None):
    """[H_s, H_j, H_p] of :119-126 as float64 CSR matrices: the sums A1..A7 and A8 + A9, and A10 with only its entries > 1 kept, each
    row-normalised"""
    A = motif_matrices(trust_mat, trn_mat) if motifs is None else motifs
    H_s = A[0] + A[1] + A[2] + A[3] + A[4] + A[5] + A[6]
    H_j = A[7] + A[8]
    H_p = A[9].multiply(A[9] > 1)
    return [_row_normalized(H) for H in (H_s, H_j, H_p)]


def joint_adjacency(trn_mat):
    """(rows, cols, float32 values) of R (:128-137): e / sqrt(sum of the user's values) / sqrt(sum of the item's values) for every stored
    entry e of trn_mat, in its entry order (float64 arithmetic, rounded once)"""
    trn_mat = sp.coo_matrix(trn_mat)
    udegree = np.asarray(trn_mat.sum(axis=1), dtype=np.float64).reshape(-1)
    idegree = np.asarray(trn_mat.sum(axis=0), dtype=np.float64).reshape(-1)
    vals = trn_mat.data.astype(np.float64) / np.sqrt(udegree[trn_mat.row]) / np.sqrt(idegree[trn_mat.col])
    if not np.all(np.isfinite(vals)):
        raise ValueError('the joint adjacency holds a non-finite value (a user or an item whose values sum to 0)')
    return trn_mat.row.astype(np.int64), trn_mat.col.astype(np.int64), vals.astype(np.float32)


class DataHandlerSocial:
    def __init__(self):
        model = configs['model']['name']
        if model in UNSUPPORTED_MODELS:
            raise NotImplementedError("the social data handler builds MHCN's matrices only: model '%s' is not supported" % model)
        if model != 'mhcn':
            raise NotImplementedError("social model '%s' is not implemented" % model)
        name = configs['data']['name']
        self.synthetic = configs['data'].get('synthetic')
        if self.synthetic is not None and self.synthetic not in synth.SOCIAL_SHAPES:
            raise ValueError("unknown synthetic social shape '%s' (one of %s)" % (self.synthetic, ', '.join(sorted(synth.SOCIAL_SHAPES))))
        if self.synthetic is None and name not in DATASETS:
            raise ValueError("unknown social dataset '%s' (%s, or set data.synthetic)" % (name, '|'.join(DATASETS)))
        predir = './datasets/social/%s/' % (name if self.synthetic is None else 'synthetic')
        self.trn_file = predir + 'trn_mat.pkl'
        self.tst_file = predir + 'tst_mat.pkl'
        self.trust_file = predir + 'trust_mat.pkl'
        self.category_file = predir + 'category.pkl'

    def _load(self, path):
        if self.synthetic is not None:
            return self._synthetic_mats()[path]
        with open(path, 'rb') as fs:
            return pickle.load(fs)

    def _synthetic_mats(self):
        if not hasattr(self, '_synth_cache'):
            seed = configs['data'].get('synthetic_seed', 2023)
            trn, trust = synth.make_social_dataset(self.synthetic, seed)
            tst = synth.split_holdout(trn, configs['data'].get('synthetic_test_frac', 0.05 if self.synthetic == 'social-tiny' else 0.002), seed + 2)
            self._synth_cache = {self.trn_file: trn, self.tst_file: tst, self.trust_file: trust}
        return self._synth_cache

    def _sparse_mx_to_torch_sparse_tensor(self, sparse_mx):
        """scipy matrix -> float32 torch sparse COO tensor on configs['device'] (:65-73), with its propagation plan attached"""
        coo = sp.coo_matrix(sparse_mx)
        idxs = t.from_numpy(np.vstack((coo.row, coo.col)).astype(np.int64))
        vals = t.from_numpy(coo.data.astype(np.float32))
        return self._with_plan(t.sparse_coo_tensor(idxs, vals, coo.shape, check_invariants=False).to(configs['device']))

    @staticmethod
    def _with_plan(adj):
        if adj.is_cuda:
            graph_of(adj)          # built once here and cached on the tensor: no step pays for it
        return adj

    def _build_motif_induced_adjacency_matrix(self, trust_mat, trn_mat):
        return motif_adjacencies(trust_mat, trn_mat)

    def _build_joint_adjacency(self, trn_mat):
        rows, cols, vals = joint_adjacency(trn_mat)
        idxs = t.from_numpy(np.vstack((rows, cols)))
        return t.sparse_coo_tensor(idxs, t.from_numpy(vals), trn_mat.shape, check_invariants=False)

    def load_data(self):
        trn_mat = self._load(self.trn_file)
        tst_mat = self._load(self.tst_file)
        trust_mat = self._load(self.trust_file)
        if type(trn_mat) != sp.coo_matrix:
            trn_mat = sp.coo_matrix(trn_mat)
        if type(tst_mat) != sp.coo_matrix:
            tst_mat = sp.coo_matrix(tst_mat)
        self.trn_mat = trn_mat
        self.trust_mat = trust_mat
        configs['data']['user_num'], configs['data']['item_num'] = trn_mat.shape

        if configs['train']['loss'] != 'pairwise':
            raise NotImplementedError("train.loss '%s'" % configs['train']['loss'])
        trn_data = PairwiseTrnData(trn_mat)
        tst_data = AllRankTstData(tst_mat, trn_mat)
        self.test_dataloader = data.DataLoader(tst_data, batch_size=configs['test']['batch_size'], shuffle=False, num_workers=0)
        dev = configs['device'] if str(configs['device']).startswith('cuda') else None
        if configs['train'].get('fast_loader'):
            self.train_dataloader = FastPairwiseLoader(trn_data, configs['train']['batch_size'], device=dev)
        elif not configs['train'].get('torch_dataloader'):
            self.train_dataloader = ExactPairwiseLoader(trn_data, configs['train']['batch_size'], device=dev)
        else:
            self.train_dataloader = data.DataLoader(trn_data, batch_size=configs['train']['batch_size'], shuffle=True, num_workers=0)

        H_s, H_j, H_p = self._build_motif_induced_adjacency_matrix(trust_mat, trn_mat)
        self.H_s = self._sparse_mx_to_torch_sparse_tensor(H_s)
        self.H_j = self._sparse_mx_to_torch_sparse_tensor(H_j)
        self.H_p = self._sparse_mx_to_torch_sparse_tensor(H_p)
        self.R = self._with_plan(self._build_joint_adjacency(trn_mat).to(configs['device']))
        self.R_t = graph_of(self.R).transposed() if self.R.is_cuda else None
        self.nnz = {'H_s': int(H_s.nnz), 'H_j': int(H_j.nnz), 'H_p': int(H_p.nnz), 'R': int(trn_mat.nnz)}
