"""Typed-edge graphs for the walks of csrc/kgin.hip and csrc/rgat.hip over a graph.RelEdgeList, built so that a stated geometry holds in
each of the three orders (by head, by tail, by relation): degrees at the 512-slot chunk boundary, keep masks defined per chunk, more long
destinations than one finishing workgroup holds, more work items than the workgroup cap covers in one pass, relation tables on both
sides of the LDS fit, and attention logits in a prescribed slot order.  Shared by test_kg_walk_cases_host.py (which checks the builders'
own claims on the CPU) and test_kg_walk_edges.py (the kernels); test infrastructure, no tests of its own.  numpy and torch on the CPU
only, deterministic.

How a case is laid out.  Entity and relation ids are split into ENGINEERED and PLAIN ranges.  An engineered destination (a head, a tail
or a relation with a prescribed number of slots) takes its partners from the plain ranges only, so it occurs in no other group and its
slots are exactly its group's edges; plain relations are dealt round robin, plain entities drawn at random.  Every group is written in
its intended slot order, then the edges of all groups are shuffled together such that the edges of one group keep their relative order:
RelEdgeList sorts stably, so slot k of an engineered destination is the k-th edge of its group in the caller's order and lies in chunk
k // CHUNK.  `Case.degree` records the claimed degrees; every destination without a claim must stay at or below CHUNK slots."""
import functools

import numpy as np
import torch

import kgcl_reference as CR
import kgin_reference as KR
from kgin_reference import both_precisions, leaf, randn

CHUNK = 512                 # graph.REL_CHUNK (asserted by the host test)
MAX_BLOCKS = 2048           # KG_MAX_BLOCKS / RG_MAX_BLOCKS: workgroups of a walk
MAX_ROW_BLOCKS = 512        # KG_MAX_ROW_BLOCKS: workgroups of the factor modulation
LDS_BYTES = 48 * 1024       # KG_LDS_BYTES / RG_LDS_BYTES
THREADS = 256
DIMS = (32, 64, 128)

# which outputs carry one row per destination of an order
AGG_OUT = {'head': ('y',), 'tail': ('dx',), 'rel': ('dw',)}
ATT_OUT = {'head': ('y', 'dp'), 'tail': ('dx', 'dq'), 'rel': ('dr',)}
AGG_ALL, ATT_ALL = ('y', 'dx', 'dw'), ('y', 'dx', 'dp', 'dq', 'dr')


def rpb(d):
    """lane groups (work items at a time, rows of a pass) per workgroup"""
    return THREADS // (d // 4)


def lds_fits(n_rel, d):
    return n_rel * d * 4 <= LDS_BYTES


class Case:
    """head, tail, rel: int64 [E] in the caller's order; rows: name -> (order, ids), the destinations of one class in 'head', 'tail' or
    'rel' order; keep: bool [E] or None; degree: order -> {id: claimed slots}; slots: (order, id) -> the edge ids of its slots in slot
    order; twins: (order, original, twin); logit: head id -> the float64 logits of its slots (logit_order only)"""

    def __init__(self, name, head, tail, rel, N, R, rows, keep=None, degree=None, slots=None, twins=(), logit=None, dims=DIMS, info=None):
        self.name, self.N, self.R, self.rows, self.dims = name, int(N), int(R), rows, tuple(dims)
        self.head, self.tail, self.rel = (np.ascontiguousarray(a, dtype=np.int64) for a in (head, tail, rel))
        self.keep = None if keep is None else torch.from_numpy(np.asarray(keep, dtype=bool))
        self.degree = degree or {'head': {}, 'tail': {}, 'rel': {}}
        self.slots, self.twins, self.logit, self.info = slots or {}, tuple(twins), logit, info or {}
        self.edges = tuple(torch.from_numpy(a) for a in (self.head, self.tail, self.rel))
        self.E = int(self.head.size)

    def quintuple(self):
        return self.head, self.tail, self.rel, self.N, self.R

    def dest(self, order):
        return {'head': self.head, 'tail': self.tail, 'rel': self.rel}[order]

    def n_dest(self, order):
        return self.R if order == 'rel' else self.N

    def claimed_geometry(self, order):
        """(n_long, n_chunks, work items) that follow from the claimed degrees when nothing else is long"""
        long_ = [n for n in self.degree[order].values() if n > CHUNK]
        n_chunks = sum((n + CHUNK - 1) // CHUNK for n in long_)
        return len(long_), n_chunks, self.n_dest(order) + n_chunks


class _Pool:
    """the plain partners: entities drawn at random from [e0, e1), relations dealt round robin from [r0, r1)"""

    def __init__(self, rng, e0, e1, r0, r1):
        self.rng, self.e0, self.e1, self.r0, self.r1, self.dealt = rng, e0, e1, r0, r1, 0

    def ents(self, n):
        return self.rng.randint(self.e0, self.e1, n).astype(np.int64)

    def rels(self, n):
        out = self.r0 + (self.dealt + np.arange(n, dtype=np.int64)) % (self.r1 - self.r0)
        self.dealt += n
        return out

    def rel_degrees(self):
        """what the round robin has dealt to each plain relation"""
        n = self.r1 - self.r0
        return {self.r0 + j: self.dealt // n + (1 if j < self.dealt % n else 0) for j in range(n)}


def _lay_out(groups, rng):
    """groups: (head, tail, rel) arrays, each in its slot order -> head, tail, rel [E] with the groups' edges shuffled together, every
    group's edges in their relative order, and per group the edge ids of its slots"""
    sizes = [len(g[0]) for g in groups]
    gid = rng.permutation(np.repeat(np.arange(len(groups)), sizes))
    where = np.argsort(gid, kind='stable')                 # the positions of group 0 ascending, then of group 1, ...
    cols = []
    for c in range(3):
        out = np.empty(gid.size, dtype=np.int64)
        out[where] = np.concatenate([np.asarray(g[c], dtype=np.int64) for g in groups])
        cols.append(out)
    ids = np.split(where, np.cumsum(sizes)[:-1])
    return cols[0], cols[1], cols[2], ids


def _assert_plain_short(case, e0):
    """no entity of the plain range [e0, N) is long as head or as tail"""
    for order in ('head', 'tail'):
        deg = np.bincount(case.dest(order), minlength=case.N)
        assert deg[e0:].max() <= CHUNK, (case.name, order, int(deg[e0:].max()))


def _engineered(groups, keys, pool, order, ids, degrees):
    """one group per (id, degree): `order` says which column the id fills"""
    for i, n in zip(ids, degrees):
        own = np.full(n, i, dtype=np.int64)
        if order == 'head':
            groups.append((own, pool.ents(n), pool.rels(n)))
        elif order == 'tail':
            groups.append((pool.ents(n), own, pool.rels(n)))
        else:
            groups.append((pool.ents(n), pool.ents(n), own))
        keys.append((order, int(i)))


# ---- boundary -------------------------------------------------------------------------------------------------------
DEGREES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 511, 512, 513, 1023, 1024, 1025, 1537)
REL_DEGREES = (0, 1, 511, 512, 513, 1024, 1025)


@functools.lru_cache(maxsize=None)
def boundary():
    """N = 1500, R = 40.  Heads 0 .. 15 have the out-degrees DEGREES, tails 16 .. 31 the same in-degrees, relations 0 .. 6 REL_DEGREES
    edges; entities 32 .. 1499 and relations 7 .. 39 are plain (3,000 plain edges; every plain relation is used and stays short).  The
    keep mask is a random half, except: the single edges of head 1 and tail 17 are kept, heads 3 / tails 19 (degree 3) and relation 1
    (one edge) are wholly masked."""
    rng = np.random.RandomState(101)
    N, R, nd, nr = 1500, 40, len(DEGREES), len(REL_DEGREES)
    pool = _Pool(rng, 2 * nd, N, nr, R)
    groups, keys = [], []
    _engineered(groups, keys, pool, 'head', range(nd), DEGREES)
    _engineered(groups, keys, pool, 'tail', range(nd, 2 * nd), DEGREES)
    _engineered(groups, keys, pool, 'rel', range(nr), REL_DEGREES)
    groups.append((pool.ents(3000), pool.ents(3000), pool.rels(3000)))
    head, tail, rel, ids = _lay_out(groups, rng)
    slots = dict(zip(keys, ids))
    keep = rng.rand(head.size) < 0.5
    for key, flag in ((('head', 1), True), (('tail', nd + 1), True), (('head', 3), False), (('tail', nd + 3), False), (('rel', 1), False)):
        keep[slots[key]] = flag
    degree = {'head': dict(zip(range(nd), DEGREES)), 'tail': dict(zip(range(nd, 2 * nd), DEGREES)), 'rel': dict(zip(range(nr), REL_DEGREES))}
    degree['rel'].update(pool.rel_degrees())

    def cls(order, base, degs, lo, hi):
        return (order, np.array([base + i for i, n in enumerate(degs) if lo <= n <= hi]))
    rows = {}
    for order, base in (('head', 0), ('tail', nd)):
        rows['%ss of 1 to 9 slots' % order] = cls(order, base, DEGREES, 1, 9)
        rows['%ss of 511 to 513 slots' % order] = cls(order, base, DEGREES, 511, 513)
        rows['%ss of 1023 to 1537 slots' % order] = cls(order, base, DEGREES, 1023, 1537)
        rows['plain %ss' % order] = (order, np.arange(2 * nd, N))
    rows['relations of 511 to 513 slots'] = cls('rel', 0, REL_DEGREES, 511, 513)
    rows['relations of 1024 and 1025 slots'] = cls('rel', 0, REL_DEGREES, 1024, 1025)
    rows['plain relations'] = ('rel', np.arange(nr, R))
    info = {'empty': {'head': [0], 'tail': [nd], 'rel': [0]}, 'masked_out': {'head': [3], 'tail': [nd + 3], 'rel': [1]},
            'single': {'head': 1, 'tail': nd + 1}}
    case = Case('boundary', head, tail, rel, N, R, rows, keep, degree, slots, info=info)
    _assert_plain_short(case, 2 * nd)
    return case


# ---- masks ----------------------------------------------------------------------------------------------------------
VARIANTS = ('all kept', 'chunk 1 masked', 'chunk 0 masked', 'last slot only', 'all masked', 'chunk 0 only', 'twin')
LONG = 3 * CHUNK + 1        # 1537: chunks of 512, 512, 512 and 1


def variant_mask(variant):
    """the keep flags of the slots of a LONG-slot destination (of the CHUNK-slot twin: all kept)"""
    k = np.arange(LONG) // CHUNK
    return {'all kept': k >= 0, 'chunk 1 masked': k != 1, 'chunk 0 masked': k != 0, 'last slot only': k == 3, 'all masked': k < 0,
            'chunk 0 only': k == 0, 'twin': np.ones(CHUNK, dtype=bool)}[variant]


@functools.lru_cache(maxsize=None)
def masks():
    """N = 1400, R = 67.  Heads 0 .. 6, tails 7 .. 13 and relations 0 .. 6 carry the VARIANTS in this order: six destinations of 1537
    slots with the variant's mask, and a twin of exactly 512 slots that repeats the first 512 partners of 'chunk 0 only' (its table rows
    are copied by tables()).  2,000 plain edges carry a random half mask."""
    rng = np.random.RandomState(202)
    N, R, nv = 1400, 67, len(VARIANTS)
    pool = _Pool(rng, 2 * nv, N, nv, R)
    groups, keys = [], []
    for order, base in (('head', 0), ('tail', nv), ('rel', 0)):
        _engineered(groups, keys, pool, order, range(base, base + nv - 1), [LONG] * (nv - 1))
        src = groups[-1]                                   # 'chunk 0 only'
        twin = np.full(CHUNK, base + nv - 1, dtype=np.int64)
        part = [a[:CHUNK].copy() for a in src]
        part[{'head': 0, 'tail': 1, 'rel': 2}[order]] = twin
        groups.append(tuple(part))
        keys.append((order, base + nv - 1))
    groups.append((pool.ents(2000), pool.ents(2000), pool.rels(2000)))
    head, tail, rel, ids = _lay_out(groups, rng)
    slots = dict(zip(keys, ids))
    keep = rng.rand(head.size) < 0.5
    degree, variant_of = {'head': {}, 'tail': {}, 'rel': {}}, {}
    for order, base in (('head', 0), ('tail', nv), ('rel', 0)):
        for v, name in enumerate(VARIANTS):
            keep[slots[(order, base + v)]] = variant_mask(name)
            degree[order][base + v] = CHUNK if name == 'twin' else LONG
            variant_of[(order, name)] = base + v
    assert np.bincount(rel, minlength=R)[nv:].max() <= CHUNK      # the plain relations (the twins repeat some) stay short
    rows = {}
    for order, base in (('head', 0), ('tail', nv), ('rel', 0)):
        plural = 'relations' if order == 'rel' else order + 's'
        rows['%s with 1025 or more kept slots' % plural] = (order, base + np.array([0, 1, 2]))
        rows['%s with 512 kept slots' % plural] = (order, base + np.array([5, 6]))
        rows['plain %s' % plural] = (order, np.arange(nv, R) if order == 'rel' else np.arange(2 * nv, N))
    twins = [(order, variant_of[(order, 'chunk 0 only')], variant_of[(order, 'twin')]) for order in ('head', 'tail', 'rel')]
    case = Case('masks', head, tail, rel, N, R, rows, keep, degree, slots, twins, info={'variant': variant_of})
    _assert_plain_short(case, 2 * nv)
    return case


# ---- many_long ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def many_long():
    """N = 600, R = 40: heads 0 .. 39 and tails 40 .. 79 of 513 .. 520 slots each (513 + id % 8); their 41,320 edges are dealt round
    robin to the 40 relations, so every relation is long as well.  More than 32 long destinations in every order: the finishing launch
    has several workgroups at every d.  Random half mask."""
    rng = np.random.RandomState(303)
    N, R, n = 600, 40, 40
    pool = _Pool(rng, 2 * n, N, 0, R)
    degs = [CHUNK + 1 + i % 8 for i in range(n)]
    groups, keys = [], []
    _engineered(groups, keys, pool, 'head', range(n), degs)
    _engineered(groups, keys, pool, 'tail', range(n, 2 * n), degs)
    head, tail, rel, ids = _lay_out(groups, rng)
    degree = {'head': dict(zip(range(n), degs)), 'tail': dict(zip(range(n, 2 * n), degs)), 'rel': pool.rel_degrees()}
    rows = {'long heads': ('head', np.arange(n)), 'long tails': ('tail', np.arange(n, 2 * n)), 'plain heads': ('head', np.arange(2 * n, N)),
            'plain tails': ('tail', np.arange(2 * n, N)), 'long relations': ('rel', np.arange(R))}
    case = Case('many_long', head, tail, rel, N, R, rows, rng.rand(head.size) < 0.5, degree, dict(zip(keys, ids)))
    _assert_plain_short(case, 2 * n)
    assert all(case.claimed_geometry(o)[0] > 32 for o in ('head', 'tail', 'rel'))
    return case


# ---- stride ---------------------------------------------------------------------------------------------------------
STRIDE_SHAPES = ((16700, 128), (66000, 32))
HUB = 600


@functools.lru_cache(maxsize=None)
def stride(N, d):
    """more work items by head and by tail than MAX_BLOCKS workgroups take in one pass at this d: 2 N random edges over the plain
    entities 6 .. N - 1, three hub heads 0 .. 2 and three hub tails 3 .. 5 of 600 slots each, whose chunk items come last and therefore
    fall in the second pass.  R = 40, dealt round robin (every relation is long).  Random half mask."""
    rng = np.random.RandomState(N + d)
    R = 40
    pool = _Pool(rng, 6, N, 0, R)
    groups, keys = [], []
    _engineered(groups, keys, pool, 'head', range(3), [HUB] * 3)
    _engineered(groups, keys, pool, 'tail', range(3, 6), [HUB] * 3)
    groups.append((pool.ents(2 * N), pool.ents(2 * N), pool.rels(2 * N)))
    head, tail, rel, ids = _lay_out(groups, rng)
    degree = {'head': {i: HUB for i in range(3)}, 'tail': {i: HUB for i in range(3, 6)}, 'rel': pool.rel_degrees()}
    first = MAX_BLOCKS * rpb(d)                            # destinations of the first pass
    rows = {}
    for order, hubs in (('head', np.arange(3)), ('tail', np.arange(3, 6))):
        rows['hub %ss' % order] = (order, hubs)
        rows['%ss of the first pass' % order] = (order, np.arange(6, first))
        rows['%ss of the second pass' % order] = (order, np.arange(first, N))
    rows['relations'] = ('rel', np.arange(R))
    case = Case('stride %d x %d' % (N, d), head, tail, rel, N, R, rows, rng.rand(head.size) < 0.5, degree, dict(zip(keys, ids)), dims=(d,),
                info={'first_pass': first})
    _assert_plain_short(case, 6)
    for order in ('head', 'tail'):
        assert case.claimed_geometry(order)[2] > first
    return case


# ---- lds_fit --------------------------------------------------------------------------------------------------------
LDS_SHAPES = ((384, 32), (385, 32), (192, 64), (193, 64), (96, 128), (97, 128))


@functools.lru_cache(maxsize=None)
def lds_fit(R, d):
    """R on either side of the last relation table that fits the LDS at this d; N = 300, 4,000 random edges, every relation used (dealt
    round robin), nothing long.  The table is staged in more than one pass of the 256 threads; the rows of later passes form a class."""
    rng = np.random.RandomState(R + d)
    N, E = 300, 4000
    pool = _Pool(rng, 0, N, 0, R)
    head, tail, rel, _ = _lay_out([(pool.ents(E), pool.ents(E), pool.rels(E))], rng)
    rel = rel[rng.permutation(E)]
    first = THREADS // (d // 4)                            # relation rows the first staging pass copies
    rows = {'relations staged by the first pass': ('rel', np.arange(first)), 'relations staged by later passes': ('rel', np.arange(first, R))}
    case = Case('lds_fit R = %d d = %d' % (R, d), head, tail, rel, N, R, rows, rng.rand(E) < 0.5, dims=(d,), info={'staged_first': first})
    assert np.bincount(rel, minlength=R).min() >= 1 and R * (d // 4) > THREADS
    return case


# ---- short ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def short():
    """N = 400, R = 64, 6,000 random edges: no long list in any order (for mask against sub-graph).  Random half mask."""
    rng = np.random.RandomState(404)
    N, R, E = 400, 64, 6000
    pool = _Pool(rng, 0, N, 0, R)
    head, tail, rel, _ = _lay_out([(pool.ents(E), pool.ents(E), pool.rels(E))], rng)
    rows = {'heads': ('head', np.arange(N)), 'tails': ('tail', np.arange(N)), 'relations': ('rel', np.arange(R))}
    return Case('short', head, tail, rel, N, R, rows, rng.rand(E) < 0.5)


# ---- logit_order ----------------------------------------------------------------------------------------------------
SEQUENCES = ('ascending', 'descending', 'maximum at slot 0', 'maximum at slot 512', 'all equal +300', 'all equal -300', 'half zero')
N_SLOTS = 1100


def logit_sequence(name):
    """the float64 logits g_k of the 1,100 slots of one head, in slot order"""
    rng = np.random.RandomState(505 + SEQUENCES.index(name))
    if name == 'ascending':
        return np.linspace(-300.0, 300.0, N_SLOTS)
    if name == 'descending':
        return np.linspace(300.0, -300.0, N_SLOTS)
    if name.startswith('maximum'):
        at = int(name.split()[-1])
        g = rng.uniform(-300.0, 299.5, N_SLOTS)             # (about two slots per unit: the softmax is peaked, not saturated)
        g[at], g[N_SLOTS - 1 if at == 0 else 0] = 300.0, -300.0
        return g
    if name.startswith('all equal'):
        return np.full(N_SLOTS, float(name.split()[-1]))
    g = rng.uniform(-3.0, 3.0, N_SLOTS)
    g[::2] = 0.0
    return g


@functools.lru_cache(maxsize=None)
def logit_order():
    """rel_attention only.  Heads 0 .. 6 carry the SEQUENCES: each has 1,100 distinct tails of its own (7 + 1,100 i ..), all under
    relation 0.  tables() sets P[h] = 0, R[0] = v / |v|^2 and Q[t_k] = g_k v, so that l_k = g_k in exact arithmetic; a slot with g_k = 0
    has a logit of exactly 0 in every precision, and equal g give equal logits in every precision.  N = 7,707, R = 3.  Random half mask.

    With one relation per head dP[h] = R[0] sum_e dl_e, and sum_e dl_e = sum_e slope'_e ds_e is 0 in exact arithmetic wherever every
    slot of noticeable weight has a logit of one sign (every head here but 'half zero', and that one too at slope 1), because the ds_e
    of a softmax add up to 0.  Such a row is rounding and nothing else, and max|ref| is no scale for it; test_kg_walk_edges.py measures
    dP[h] against logit_dp_scale, the magnitude of what is added and subtracted on the way (the terms dl_e R[0] themselves are compared
    as the rows dQ[t_e] of the head's 1,100 distinct tails, in the usual way)."""
    rng = np.random.RandomState(606)
    nh = len(SEQUENCES)
    N, R = nh + nh * N_SLOTS, 3
    groups, keys, logit = [], [], {}
    for h, name in enumerate(SEQUENCES):
        groups.append((np.full(N_SLOTS, h), nh + h * N_SLOTS + np.arange(N_SLOTS), np.zeros(N_SLOTS, dtype=np.int64)))
        keys.append(('head', h))
        logit[h] = logit_sequence(name)
    head, tail, rel, ids = _lay_out(groups, rng)
    degree = {'head': {h: N_SLOTS for h in range(nh)}, 'tail': {}, 'rel': {0: nh * N_SLOTS}}
    rows = {'heads with a peaked softmax': ('head', np.arange(4)), 'heads of equal logits': ('head', np.array([4, 5])),
            'head with half the logits 0': ('head', np.array([6])), 'relation 0': ('rel', np.array([0]))}
    for h, name in enumerate(SEQUENCES):
        rows['tails of the head: %s' % name] = ('tail', nh + h * N_SLOTS + np.arange(N_SLOTS))
    return Case('logit_order', head, tail, rel, N, R, rows, rng.rand(head.size) < 0.5, degree, dict(zip(keys, ids)), logit=logit,
                info={'head_of': {name: h for h, name in enumerate(SEQUENCES)}})


def logit_dp_scale(case, d, h, masked, slope=CR.SLOPE):
    """max|R[0]| (sum_e a_e <|G[h]|, |X[t_e]|> + <|G[h]|, |Y[h]|>) in float64 over the kept slots of head h of logit_order.
    dP[h] = R[0] sum_e slope'_e a_e (<G[h], X[t_e]> - delta_h) with delta_h = <G[h], Y[h]> and Y[h] = sum_e a_e X[t_e]: three levels
    cancel (the products of a dot product, <G, X[t_e]> against delta_h for a slot that dominates, and the ds_e among themselves), so
    the scale is the magnitude of the elementary products before any of it, which is what the rounding of a float32 evaluation is
    proportional to (a kernel that takes delta_h from the stored Y[h] carries the sqrt(n) half-ulps of Y's accumulation into it)"""
    t = tables(case, d)
    ids = case.slots[('head', h)]
    g = case.logit[h]
    if masked:
        sel = case.keep.numpy()[ids]
        ids, g = ids[sel], g[sel]
    s = torch.from_numpy(np.where(g > 0, g, slope * g))
    a = torch.softmax(s, 0)
    x, g_abs = t['x'][torch.from_numpy(case.tail[ids])], t['go'][h].abs()
    return float(((a * (x.abs() @ g_abs)).sum() + (a @ x).abs() @ g_abs) * t['r'][0].abs().max())


def all_cases():
    out = [boundary(), masks(), many_long(), short(), logit_order()]
    out += [stride(N, d) for N, d in STRIDE_SHAPES] + [lds_fit(R, d) for R, d in LDS_SHAPES]
    return out


# ---- tables and restatements ----------------------------------------------------------------------------------------
_TABLES, _REFS = {}, {}


def tables(case, d):
    """float64 x, p, q, go [N, d] and r, w [R, d], the same for every test that asks; p, q and r are scaled by 0.5 (a logit has the
    standard deviation sqrt(2 d) / 4).  A twin's rows are copies of its original's; logit_order's P, Q and R rows are set as described"""
    key = (case.name, d)
    if key not in _TABLES:
        N, R = case.N, case.R
        t = {'x': randn((N, d), 1), 'p': randn((N, d), 4, 0.5), 'q': randn((N, d), 5, 0.5), 'go': randn((N, d), 3),
             'r': randn((R, d), 2, 0.5), 'w': randn((R, d), 6)}
        for order, src, dst in case.twins:
            for name in (('r', 'w') if order == 'rel' else ('x', 'p', 'q', 'go')):
                t[name][dst] = t[name][src]
        if case.logit is not None:
            v = randn((d,), 7)
            t['r'][0] = v / (v * v).sum()
            for h, g in case.logit.items():
                t['p'][h] = 0
                t['q'][torch.from_numpy(case.tail[case.slots[('head', h)]])] = torch.from_numpy(g).unsqueeze(1) * v
        _TABLES[key] = t
    return _TABLES[key]


def reference(case, d, op, masked, slope=CR.SLOPE):
    """(float64, float32) outputs of the restatement of `op` ('agg': kgin_reference.kg_aggregate, y / dx / dw; 'att':
    kgcl_reference.rel_attention, y / dx / dp / dq / dr) on the case's tables, upstream gradient `go`; computed once and left unchanged"""
    key = (case.name, d, op, bool(masked), float(slope))
    if key not in _REFS:
        t = tables(case, d)
        keep = case.keep if masked else None

        def agg(dt):
            x, w = leaf(t['x'], dt), leaf(t['w'], dt)
            y = KR.kg_aggregate(x, w, *case.edges, keep)
            (y * t['go'].to(dt)).sum().backward()
            return {'y': y.detach(), 'dx': x.grad, 'dw': w.grad}

        def att(dt):
            leaves = [leaf(t[n], dt) for n in ('x', 'p', 'q', 'r')]
            y = CR.rel_attention(*leaves, case.edges, keep, slope)
            (y * t['go'].to(dt)).sum().backward()
            return dict(zip(ATT_ALL, [y.detach(), leaves[0].grad, leaves[1].grad, leaves[2].grad, leaves[3].grad]))
        _REFS[key] = both_precisions(agg if op == 'agg' else att)
    return _REFS[key]


def row_groups(case, op):
    """(label, output name, row ids as a torch tensor) for every class of rows of the case and every output that has one row per
    destination of the class's order"""
    outs = AGG_OUT if op == 'agg' else ATT_OUT
    return [(label, k, torch.from_numpy(np.asarray(ids, dtype=np.int64))) for label, (order, ids) in case.rows.items() if len(ids)
            for k in outs[order]]


# ---- factor modulation ----------------------------------------------------------------------------------------------
FM_SHAPES = ((4097, 128, 1), (8195, 128, 3), (8195, 64, 8), (16387, 32, 3))


FM_OUT = ('out', 'd_agg', 'd_u', 'd_latent', 'd_dmat')


def fm_tables(U, d, F):
    """([agg, u [U, d], latent, dmat [F, d]], upstream gradient) in float64, drawn as tests/test_kgin.py's fm_case draws them"""
    seed = 40 + U
    return [randn((U, d), seed), randn((U, d), seed + 1), randn((F, d), seed + 2), randn((F, d), seed + 3, 0.3)], randn((U, d), seed + 4)


def fm_outputs(fn, tens, go, to):
    leaves = [to(x).requires_grad_(True) for x in tens]
    out = fn(*leaves)
    (out * to(go)).sum().backward()
    return dict(zip(FM_OUT, [out.detach()] + [a.grad for a in leaves]))


def fm_reference(U, d, F):
    """(float64, float32) outputs of kgin_reference.factor_modulate, computed once"""
    key = ('fm', U, d, F)
    if key not in _REFS:
        tens, go = fm_tables(U, d, F)
        _REFS[key] = both_precisions(lambda dt: fm_outputs(KR.factor_modulate, tens, go, lambda x: x.detach().to(dt).clone()))
    return _REFS[key]


def fm_geometry(U, d):
    """kg_geom of csrc/kgin.hip: (workgroups, rows per workgroup, passes of the row loop per workgroup)"""
    r = rpb(d)
    passes = (U + r - 1) // r
    g0 = min(passes, MAX_ROW_BLOCKS)
    ppb = (passes + g0 - 1) // g0
    return (passes + ppb - 1) // ppb, ppb * r, ppb
