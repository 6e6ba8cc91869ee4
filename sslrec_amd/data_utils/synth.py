"""Seeded synthetic user-item interaction graphs shaped like the datasets the
BASELINE configs name.  The reference ships only the yelp
train pickle (`.MISSING_LARGE_BLOBS`), and the GPU box has no datasets at all,
so benchmarks and large parity tests synthesize their graphs here.

The generator is plain numpy: user degrees follow a clipped power law, items
are drawn by popularity (another power law), duplicate pairs are removed and
the set is trimmed to exactly `n_edges` interactions.  Output is a scipy COO
matrix of float64 ones, i.e. the same object `pickle.load` yields for the
reference's `train_mat.pkl` (docs/GuideDataCF.md:1-33 of the reference).
"""
import numpy as np
import scipy.sparse as sp

# (users, items, train interactions) per BASELINE.json config
SHAPES = {
    'gowalla': (25557, 19747, 295000),        # cfg 1 (train pickle missing upstream)
    'amazon-book': (52643, 91599, 2380730),   # cfg 2/3 (LightGCN-paper Amazon-Book)
    'yelp': (42712, 26822, 182357),           # cfg 4 (same shape as the real pickle)
    'tiny': (300, 220, 3000),                 # unit tests / golden fixtures
}


# social scenario: (users, items, train interactions, trust edges) -- the two bench shapes have the user / item counts of the
# reference's yelp and epinions test pickles (its train and trust pickles are not shipped); the interaction and trust counts are chosen
# so that the host builds the motif matrices of data_handler_social.py in well under a minute (their nnz: profiles/mhcn/)
SOCIAL_SHAPES = {
    'social-yelp': (43043, 66576, 400000, 400000),
    'social-epinions': (18081, 251722, 300000, 250000),
    'social-tiny': (150, 120, 900, 700),          # unit tests: all ten motifs occur, H_s and H_j have empty rows
}


# kg scenario: (users, items, entities incl. items, canonical relations, train interactions, canonical triplets) -- the two bench
# shapes have the counts of the reference's last-fm and alibaba-fashion knowledge graphs (KGIN paper, table 1); the handler doubles the
# triplets with their inverses and adds the interact relation
KG_SHAPES = {
    'kg-last-fm': (23566, 48123, 106389, 9, 3034796, 464567),
    'kg-alibaba': (114737, 30040, 89196, 51, 1781093, 279155),
    'kg-tiny': (60, 50, 90, 4, 400, 300),          # unit tests: an entity without edges, a pair under two relations, a relation that occurs once
}


def powerlaw_bipartite(n_user, n_item, n_edges, seed=2023, user_exp=2.0, item_exp=0.5,
                       max_user_frac=0.05):
    rng = np.random.default_rng(seed)
    # user degrees: Pareto tail, >=1, clipped, rescaled so the sum overshoots n_edges a bit
    raw = rng.pareto(user_exp - 1.0, size=n_user) + 1.0
    cap = max(1.0, max_user_frac * n_item)
    raw = np.minimum(raw, cap)
    target = n_edges * 1.15
    deg = np.maximum(1, np.floor(raw * (target / raw.sum()))).astype(np.int64)
    deg = np.minimum(deg, int(cap))
    # item popularity: Zipf-like weights over a random permutation of item ids
    w = 1.0 / np.power(np.arange(1, n_item + 1, dtype=np.float64), item_exp)
    cdf = np.cumsum(w / w.sum())
    item_of_rank = rng.permutation(n_item)

    keys = np.empty(0, dtype=np.int64)
    rounds = 0
    while keys.size < n_edges and rounds < 64:
        users = np.repeat(np.arange(n_user, dtype=np.int64), deg)
        ranks = np.searchsorted(cdf, rng.random(users.size), side='right')
        ranks = np.minimum(ranks, n_item - 1)
        items = item_of_rank[ranks]
        keys = np.unique(np.concatenate([keys, users * n_item + items]))
        rounds += 1
    if keys.size < n_edges:
        raise RuntimeError('could not reach the requested number of interactions')
    if keys.size > n_edges:
        keys = rng.choice(keys, size=n_edges, replace=False)
    # upstream pickles hold rows in no particular order: shuffle
    keys = rng.permutation(keys)
    rows = (keys // n_item).astype(np.int32)
    cols = (keys % n_item).astype(np.int32)
    return sp.coo_matrix((np.ones(n_edges, dtype=np.float64), (rows, cols)), shape=(n_user, n_item))


def community_bipartite(n_user, n_item, n_edges, n_comm=64, p_in=0.8, seed=2023, user_exp=2.0, item_exp=0.5, max_user_frac=0.05):
    """powerlaw_bipartite with PLANTED COMMUNITIES: users and items are dealt to `n_comm` communities (ids scattered over the id
    range, like real catalogues), a user draws an item from its own community with probability p_in (by popularity inside the
    community) and from the whole catalogue otherwise.  Same degree laws as powerlaw_bipartite -- the graph the locality-aware
    plan (csrc/plan.cpp: cocluster_rows) is measured on beside the structure-free headline graph."""
    rng = np.random.default_rng(seed)
    raw = rng.pareto(user_exp - 1.0, size=n_user) + 1.0
    cap = max(1.0, max_user_frac * n_item)
    raw = np.minimum(raw, cap)
    deg = np.maximum(1, np.floor(raw * (n_edges * 1.15 / raw.sum()))).astype(np.int64)
    deg = np.minimum(deg, int(cap))
    comm_u = rng.integers(0, n_comm, n_user)
    comm_i = rng.integers(0, n_comm, n_item)
    order = np.argsort(comm_i, kind='stable')                       # items grouped by community
    start = np.searchsorted(comm_i[order], np.arange(n_comm + 1))
    w = 1.0 / np.power(np.arange(1, n_item + 1, dtype=np.float64), item_exp)
    cdf = np.cumsum(w / w.sum())
    item_of_rank = rng.permutation(n_item)
    keys = np.empty(0, dtype=np.int64)
    rounds = 0
    while keys.size < n_edges and rounds < 64:
        users = np.repeat(np.arange(n_user, dtype=np.int64), deg)
        inside = rng.random(users.size) < p_in
        glob = item_of_rank[np.minimum(np.searchsorted(cdf, rng.random(users.size), side='right'), n_item - 1)]
        cu = comm_u[users]
        size = (start[cu + 1] - start[cu]).astype(np.float64)
        # inside a community: rank ~ u^(1/(1-item_exp)) reproduces the same popularity law over the community's items
        pick = np.minimum((np.power(rng.random(users.size), 1.0 / max(1e-6, 1.0 - item_exp)) * size).astype(np.int64), np.maximum(size.astype(np.int64) - 1, 0))
        loc = order[np.minimum(start[cu] + pick, n_item - 1)]
        items = np.where(inside & (size > 0), loc, glob)
        keys = np.unique(np.concatenate([keys, users * n_item + items]))
        rounds += 1
    if keys.size < n_edges:
        raise RuntimeError('could not reach the requested number of interactions')
    if keys.size > n_edges:
        keys = rng.choice(keys, size=n_edges, replace=False)
    keys = rng.permutation(keys)
    return sp.coo_matrix((np.ones(n_edges, dtype=np.float64), ((keys // n_item).astype(np.int32), (keys % n_item).astype(np.int32))),
                         shape=(n_user, n_item))


def make_dataset(name, seed=2023):
    n_user, n_item, n_edges = SHAPES[name]
    return powerlaw_bipartite(n_user, n_item, n_edges, seed)


def uniform_bipartite(n_user, n_item, n_edges, seed=2023):
    """`n_edges` distinct (user, item) pairs drawn uniformly: float64 ones in a COO matrix, entries in no particular order"""
    rng = np.random.default_rng(seed)
    keys = rng.choice(n_user * n_item, size=n_edges, replace=False).astype(np.int64)
    return sp.coo_matrix((np.ones(n_edges, dtype=np.float64), ((keys // n_item).astype(np.int32), (keys % n_item).astype(np.int32))),
                         shape=(n_user, n_item))


def trust_graph(n_user, n_edges, reciprocal=0.3, n_isolated=None, seed=2023, comm_size=None, p_in=0.8):
    """Seeded DIRECTED trust graph [n_user, n_user] as a COO matrix of float64 ones: no self loops, no duplicate entries, about
    `reciprocal` of the entries have their reverse entry too, and `n_isolated` users (default: 1 in 30, at least 1) have no trust edge
    in either direction.  Sources and targets are uniform over the other users; with `comm_size` the users with edges are dealt to
    communities of that many and a pair lies inside one community with probability `p_in` (trust graphs are clustered: a uniform graph
    of the bench sizes has next to no triangle, and MHCN's H_s is made of triangles).  `n_edges` is met to within rounding."""
    rng = np.random.default_rng(seed)
    if n_isolated is None:
        n_isolated = max(1, n_user // 30)
    active = np.sort(rng.permutation(n_user)[:n_user - n_isolated]).astype(np.int64)
    m = active.size
    if m < 2:
        raise ValueError('trust_graph: fewer than two users with trust edges')
    n_pairs = int(round(n_edges * reciprocal / 2.0))            # unordered pairs that get both directions
    n_single = max(0, n_edges - 2 * n_pairs)
    want = n_pairs + n_single
    if want > m * (m - 1) // 2:
        raise ValueError('trust_graph: %d edges do not fit %d users' % (n_edges, m))
    keys = np.empty(0, dtype=np.int64)                          # distinct unordered pairs lo < hi as lo * m + hi
    rounds = 0
    while keys.size < want and rounds < 64:
        a = rng.integers(0, m, size=2 * (want - keys.size) + 16)
        b = rng.integers(0, m, size=a.size)
        if comm_size is not None:
            start = (a // comm_size) * comm_size
            inside = start + rng.integers(0, comm_size, size=a.size)
            b = np.where((rng.random(a.size) < p_in) & (inside < m), inside, b)
        ok = a != b
        lo, hi = np.minimum(a, b)[ok], np.maximum(a, b)[ok]
        keys = np.unique(np.concatenate([keys, lo * m + hi]))
        rounds += 1
    if keys.size < want:
        raise RuntimeError('could not reach the requested number of trust edges')
    keys = rng.permutation(keys)[:want]
    lo, hi = active[keys // m], active[keys % m]
    flip = rng.random(want) < 0.5                               # direction of the one-way edges
    src = np.where(flip, hi, lo)
    dst = np.where(flip, lo, hi)
    rows = np.concatenate([src, dst[:n_pairs]])                 # the first n_pairs pairs are reciprocated
    cols = np.concatenate([dst, src[:n_pairs]])
    order = rng.permutation(rows.size)
    return sp.coo_matrix((np.ones(rows.size, dtype=np.float64), (rows[order].astype(np.int32), cols[order].astype(np.int32))),
                         shape=(n_user, n_user))


def make_social_dataset(name, seed=2023):
    """(trn_mat, trust_mat) of SOCIAL_SHAPES[name]: power-law interactions for the bench shapes, uniform ones for social-tiny (whose
    motif counts the tests pin), and a trust graph with 30 % reciprocated entries"""
    n_user, n_item, n_edges, n_trust = SOCIAL_SHAPES[name]
    if name == 'social-tiny':
        trn = uniform_bipartite(n_user, n_item, n_edges, seed)
        # (seed + 19: at the default seed 2023 the graph then holds all ten motifs, the fully reciprocated triangle among them -- about
        # one graph in three of this size does; tests/test_mhcn_host.py asserts it)
        trust = trust_graph(n_user, n_trust, 0.3, 5, seed + 19)
    else:
        trn = powerlaw_bipartite(n_user, n_item, n_edges, seed)
        trust = trust_graph(n_user, n_trust, 0.3, None, seed + 17, comm_size=40)
    return trn, trust


def kg_triplets(n_item, n_entity, n_rel, n_triplets, seed=2023, tail_exp=1.0, p_item_head=0.85):
    """`n_triplets` distinct canonical triplets (head, relation, tail) as an int32 [T, 3] array in np.unique's row order -- what
    np.unique(np.loadtxt('kg_final.txt'), axis=0) yields.  Entities [0, n_item) are the items, the others attributes.  Heads are items
    (`p_item_head`) or attributes, tails are attributes drawn by a Zipf law of exponent `tail_exp`, so a few attribute entities are hubs with
    a large share of all edges.  By construction: the attribute n_item + (n_entity - n_item) // 2 occurs in no triplet, one (head, tail)
    pair occurs under two relations, relation n_rel - 1 occurs exactly once (with tail n_entity - 1, so both maxima are present)."""
    if n_rel < 3 or n_entity - n_item < 4 or n_triplets < 3:
        raise ValueError('kg_triplets: at least 3 relations, 4 attribute entities and 3 triplets')
    rng = np.random.default_rng(seed)
    n_attr = n_entity - n_item
    isolated = n_item + n_attr // 2
    w = 1.0 / np.power(np.arange(1, n_attr + 1, dtype=np.float64), tail_exp)
    cdf = np.cumsum(w / w.sum())
    attr_of_rank = n_item + rng.permutation(n_attr)
    rel_w = 1.0 / np.arange(1, n_rel, dtype=np.float64)             # relations 0 .. n_rel - 2, skewed
    rel_cdf = np.cumsum(rel_w / rel_w.sum())
    need = n_triplets - 2
    keys = np.empty(0, dtype=np.int64)                              # (h * n_rel + r) * n_entity + t
    rounds = 0
    while keys.size < need and rounds < 64:
        m = 2 * (need - keys.size) + 64
        h = np.where(rng.random(m) < p_item_head, rng.integers(0, n_item, m), n_item + rng.integers(0, n_attr, m)).astype(np.int64)
        t = attr_of_rank[np.minimum(np.searchsorted(cdf, rng.random(m), side='right'), n_attr - 1)].astype(np.int64)
        r = np.minimum(np.searchsorted(rel_cdf, rng.random(m), side='right'), n_rel - 2).astype(np.int64)
        ok = (h != t) & (h != isolated) & (t != isolated)
        keys = np.unique(np.concatenate([keys, ((h * n_rel + r) * n_entity + t)[ok]]))
        rounds += 1
    if keys.size < need:
        raise RuntimeError('could not reach the requested number of triplets')
    if keys.size > need:
        keys = rng.choice(keys, size=need, replace=False)
    have = set(keys.tolist())
    h0, r0, t0 = int(keys[0] // n_entity // n_rel), int(keys[0] // n_entity % n_rel), int(keys[0] % n_entity)
    twin = next(k for k in (((h0 * n_rel + (r0 + s) % (n_rel - 1)) * n_entity + t0) for s in range(1, n_rel - 1)) if k not in have)
    rare = ((n_item - 1) * n_rel + (n_rel - 1)) * n_entity + (n_entity - 1)
    keys = np.concatenate([keys, np.array([twin, rare], dtype=np.int64)])
    trip = np.stack([keys // n_entity // n_rel, keys // n_entity % n_rel, keys % n_entity], axis=1).astype(np.int32)
    return np.unique(trip, axis=0)


def make_kg_dataset(name, seed=2023, test_frac=None):
    """(train_cf [n, 2], test_cf [m, 2], canonical triplets [T, 3]) of KG_SHAPES[name]: the (user, item) pairs in the order the
    reference's `_read_cf` yields them from train.txt / test.txt (by user; the items of a user in ascending order) and what
    np.unique(np.loadtxt(kg_final.txt), axis=0) yields.  Power-law interactions for the bench shapes, uniform ones for kg-tiny."""
    n_user, n_item, n_entity, n_rel, n_inter, n_trip = KG_SHAPES[name]
    tiny = name == 'kg-tiny'
    trn = uniform_bipartite(n_user, n_item, n_inter, seed) if tiny else powerlaw_bipartite(n_user, n_item, n_inter, seed)
    tst = split_holdout(trn, test_frac if test_frac is not None else (0.05 if tiny else 0.002), seed + 2)

    def pairs(m):
        order = np.lexsort((m.col, m.row))
        return np.stack([m.row[order], m.col[order]], axis=1).astype(np.int64)
    return pairs(trn), pairs(tst), kg_triplets(n_item, n_entity, n_rel, n_trip, seed + 23)


def split_holdout(trn_mat, frac, seed):
    """Tiny helper for fixtures: a disjoint random hold-out with the same shape
    (stands in for valid_mat / test_mat)."""
    rng = np.random.default_rng(seed)
    n_user, n_item = trn_mat.shape
    n = max(1, int(frac * trn_mat.nnz))
    existing = set((trn_mat.row.astype(np.int64) * n_item + trn_mat.col).tolist())
    picked = []
    while len(picked) < n:
        k = int(rng.integers(0, n_user * n_item))
        if k not in existing:
            existing.add(k)
            picked.append(k)
    keys = np.array(picked, dtype=np.int64)
    return sp.coo_matrix((np.ones(n), ((keys // n_item).astype(np.int32), (keys % n_item).astype(np.int32))),
                         shape=(n_user, n_item))


def cell_bipartite(n_user, n_item, n_edges, world, ru, ri, seed=2023):
    """Shard-local generation for row-sharded training (BASELINE cfg 5: a 10 M x 10 M graph nobody can build on one
    host): the global graph is DEFINED as the union of world^2 cells, cell (ru, ri) holding the interactions between
    users = ru mod world and items = ri mod world, generated from its own seed.  Rank p builds cells (p, *) for its rows
    of A and cells (*, p) for its rows of A^T -- 2/world of the graph, no communication; degrees are exchanged
    afterwards (`sharded_lightgcl_values`).  Returns (users, items) int64 global ids of the cell."""
    uc = (n_user - ru + world - 1) // world
    ic = (n_item - ri + world - 1) // world
    ec = n_edges // (world * world) + (1 if (ru * world + ri) < n_edges % (world * world) else 0)
    if uc <= 0 or ic <= 0 or ec <= 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    m = powerlaw_bipartite(uc, ic, min(ec, uc * ic // 2), seed + 7919 * (ru * world + ri))
    return m.row.astype(np.int64) * world + ru, m.col.astype(np.int64) * world + ri


def sharded_cells(n_user, n_item, n_edges, world, rank, seed=2023):
    """(users_f, items_f), (users_b, items_b): the interactions of this rank's user rows and of its item rows"""
    fu, fi, bu, bi = [], [], [], []
    for k in range(world):
        u, i = cell_bipartite(n_user, n_item, n_edges, world, rank, k, seed)
        fu.append(u); fi.append(i)
        u, i = cell_bipartite(n_user, n_item, n_edges, world, k, rank, seed)
        bu.append(u); bi.append(i)
    return (np.concatenate(fu), np.concatenate(fi)), (np.concatenate(bu), np.concatenate(bi))
