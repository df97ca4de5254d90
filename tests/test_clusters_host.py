"""CPU (no GPU): the host side of face clustering.

* ``dbscan_ref`` and ``sums_ref``: plain restatements (breadth-first search, no union-find) of the
  rules in include/prpe.h that the GPU tests (tests/test_gpu_clusters.py) use as their yardstick,
  pinned here by hand-worked cases and by a second restatement written the other way (union-find
  over a sorted edge list) on 200 seeded random graphs;
* the input builders of the GPU file (``half_rows``, ``chain_rows``, ``planted_rows``) and, for
  every seeded random input the GPU file compares against fp64, the margin conditions that keep
  that comparison from hiding a flip (``margins``): no fp64 score within tol of the threshold, and
  every border row's two best core neighbours more than 2 tol apart (or exactly equal), with
  tol = 4 e_ref measured on the input as in tests/test_gpu_gallery.py. No row is left out on these
  grounds: the seeds and thresholds below were picked so that both hold, and it is asserted here;
* the exact inputs of the multi-tile walk (tests/test_gpu_pairs_walk.py) with their conditions: the
  ring of many tiles cut into arcs, ~200 clusters scattered over the tile rows, and the compaction
  scan past one chunk with its per-group reference, pinned to ``dbscan_ref`` at a small chunk;
* the ABI entries, every refusal of the header (the pointers below are never read), and the
  ``FaceClusters`` / ``FaceClustering`` bookkeeping with the ops calls stubbed.
"""
import collections
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from prpe import _lib

Ref = collections.namedtuple("Ref", "root kind degree cluster sizes n_clusters")
LEFT_OUT, NOISE, BORDER, CORE = 0, 1, 2, 3


# ---------------------------------------------------------------------------------- restatements
def neighbours_ref(scores, valid, threshold):
    """bool [N, N]: i != j, both rows take part, the score is finite and >= threshold (compared
    in the scores' own precision)."""
    s = np.asarray(scores)
    n = s.shape[0]
    on = np.ones(n, dtype=bool) if valid is None else np.asarray(valid) != 0
    with np.errstate(invalid="ignore"):
        nb = np.isfinite(s) & (s >= s.dtype.type(threshold))
    return nb & on[:, None] & on[None, :] & ~np.eye(n, dtype=bool), on


def dbscan_ref(scores, valid, threshold, min_samples, max_clusters=None):
    """The stated DBSCAN on a symmetric score matrix [N, N]. Core rows are visited in ascending
    order; a breadth-first search over core neighbours from an unvisited one collects its cluster,
    whose root is therefore its lowest core row and whose id counts up with the root. A border row
    takes the cluster of its best core neighbour (highest score, then lowest row). ``sizes`` holds
    min(C, max_clusters) entries; ``cluster`` keeps the ids past them."""
    s = np.asarray(scores)
    n = s.shape[0]
    nb, on = neighbours_ref(s, valid, threshold)
    degree = nb.sum(axis=1).astype(np.int64)
    core = on & (degree + 1 >= min_samples)
    root = np.full(n, -1, dtype=np.int64)
    cluster = np.full(n, -1, dtype=np.int64)
    kind = np.where(on, NOISE, LEFT_OUT).astype(np.int64)
    kind[core] = CORE
    C = 0
    for i in range(n):
        if not core[i] or root[i] >= 0:
            continue
        root[i], cluster[i] = i, C
        queue = collections.deque([i])
        while queue:
            u = queue.popleft()
            for v in np.flatnonzero(nb[u] & core):
                if root[v] < 0:
                    root[v], cluster[v] = i, C
                    queue.append(v)
        C += 1
    for i in range(n):
        if on[i] and not core[i]:
            cand = np.flatnonzero(nb[i] & core)
            if cand.size:
                best = cand[0]
                for c in cand[1:]:                                             # ascending: a tie keeps the lower row
                    if s[i, c] > s[i, best]:
                        best = c
                root[i], cluster[i], kind[i] = root[best], cluster[best], BORDER
    lim = C if max_clusters is None else min(C, max_clusters)
    sizes = np.bincount(cluster[(cluster >= 0) & (cluster < lim)], minlength=lim).astype(np.int64)
    return Ref(root, kind, degree, cluster, sizes, C)


def _dbscan_union_find(scores, valid, threshold, min_samples):
    """The other way round: the sorted list of accepted pairs i < j, degrees counted off it, a
    union-find over the core-core pairs, the border rule as a sort."""
    s = np.asarray(scores)
    n = s.shape[0]
    on = [True] * n if valid is None else [bool(v) for v in valid]
    thr = s.dtype.type(threshold)
    edges = sorted((i, j) for i in range(n) for j in range(i + 1, n)
                   if on[i] and on[j] and np.isfinite(s[i, j]) and s[i, j] >= thr)
    degree = [0] * n
    for i, j in edges:
        degree[i] += 1
        degree[j] += 1
    core = [on[i] and degree[i] + 1 >= min_samples for i in range(n)]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for i, j in edges:
        if core[i] and core[j]:
            a, b = find(i), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)
    root, kind = [-1] * n, [LEFT_OUT] * n
    for i in range(n):
        if core[i]:
            root[i], kind[i] = find(i), CORE
        elif on[i]:
            cand = sorted((-float(s[min(e), max(e)]), e[0] + e[1] - i) for e in edges if i in e and core[e[0] + e[1] - i])
            kind[i] = BORDER if cand else NOISE
            if cand:
                root[i] = find(cand[0][1])
    ids = {r: c for c, r in enumerate(sorted({root[i] for i in range(n) if kind[i] == CORE}))}
    cluster = [ids[r] if r >= 0 else -1 for r in root]
    sizes = [cluster.count(c) for c in range(len(ids))]
    return Ref(np.array(root), np.array(kind), np.array(degree), np.array(cluster), np.array(sizes, dtype=np.int64),
               len(ids))


def same_ref(a, b):
    return (a.n_clusters == b.n_clusters and all(np.array_equal(np.asarray(x), np.asarray(y))
                                                 for x, y in zip(a[:5], b[:5])))


def sums_ref(rows_fp32, cluster, n):
    """int64 [n, D]: per cluster id < n and column, the sum over its members of
    rint(a[i][d] * 2^32). The product is exact in fp32 and in fp64 alike and rint rounds to
    nearest even as llrintf does. (The sums of a cluster with a NaN or infinite element are
    unspecified; such rows are noise in the tests, and their conversion here is not used.)"""
    x = np.asarray(rows_fp32, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        q = np.rint(x.astype(np.float64) * 4294967296.0).astype(np.int64)
    out = np.zeros((n, x.shape[1]), dtype=np.int64)
    for i, c in enumerate(np.asarray(cluster)):
        if 0 <= c < n:
            out[c] += q[i]
    return out


def centroids_ref(sums):
    return (np.asarray(sums, dtype=np.int64).astype(np.float64) * 2.0 ** -32).astype(np.float32)


# ---------------------------------------------------------------------------------- input builders
def half_rows(n, D, seed, pool=12):
    """Rows with four entries of +-0.5 among ``pool`` seeded columns: the norm is exactly 1 and
    every dot product a multiple of 0.25, equal in any arithmetic."""
    g = np.random.default_rng(seed)
    cols = np.sort(g.permutation(D)[:pool])
    x = np.zeros((n, D), dtype=np.float32)
    for i in range(n):
        x[i, g.choice(cols, 4, replace=False)] = g.choice([-0.5, 0.5], 4)
    return x


def chain_rows(n, D):
    """Row i holds 0.5 on the columns 2 i .. 2 i + 3 (mod D): rows i and i + 1 share two columns
    and score 0.5, rows further apart score 0. The pattern wraps after D / 2 rows: at D = 512 row
    256 repeats row 0 (score 1) and row 255 shares two columns with both, so 257 rows are a ring
    0 - 1 - .. - 255 - 0 with row 256 lying on row 0."""
    x = np.zeros((n, D), dtype=np.float32)
    for i in range(n):
        x[i, (2 * i + np.arange(4)) % D] = 0.5
    return x


def planted_rows(n, D, seed, identities=40, spread=0.7, bridges=4, outliers=6):
    """Raw rows: random centres, members = centre + spread * noise in a seeded order, then
    ``bridges`` rows between two centres and ``outliers`` rows of noise alone, at seeded places."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(identities, D, generator=g)
    ids = torch.arange(n) % identities
    x = centres[ids] + spread * torch.randn(n, D, generator=g)
    place = torch.randperm(n, generator=g)
    for k in range(bridges):
        x[place[k]] = centres[2 * k] + centres[2 * k + 1] + 0.3 * torch.randn(D, generator=g)
    for k in range(bridges, bridges + outliers):
        x[place[k]] = torch.randn(D, generator=g)
    return x[torch.randperm(n, generator=g)].contiguous()


def random_rows(n, D, seed):
    return torch.randn(n, D, generator=torch.Generator().manual_seed(seed))


def margins(x_raw, threshold, min_samples, valid=None):
    """(fp64 scores, tol, dbscan_ref on them, worst margins) of raw rows ``x_raw`` (a float32
    tensor): asserts the two margin conditions of this file's docstring for every row."""
    s64 = (F.normalize(x_raw.double(), dim=1) @ F.normalize(x_raw.double(), dim=1).t()).numpy()
    s32 = (F.normalize(x_raw, dim=1) @ F.normalize(x_raw, dim=1).t()).numpy()
    e_ref = float(np.abs(s32.astype(np.float64) - s64).max())
    tol = 4 * e_ref
    n = s64.shape[0]
    on = np.ones(n, dtype=bool) if valid is None else np.asarray(valid) != 0
    pair = on[:, None] & on[None, :] & ~np.eye(n, dtype=bool)
    edge_margin = float(np.abs(s64 - threshold)[pair].min()) if pair.any() else np.inf
    assert edge_margin > tol, (edge_margin, tol)
    ref = dbscan_ref(s64, valid, threshold, min_samples)
    nb, _ = neighbours_ref(s64, valid, threshold)
    tie_margin = np.inf
    for i in np.flatnonzero(ref.kind == BORDER):
        top = np.sort(s64[i, nb[i] & (ref.kind == CORE)])[::-1]
        if top.size > 1 and top[0] != top[1]:
            tie_margin = min(tie_margin, float(top[0] - top[1]))
    assert tie_margin > 2 * tol, (tie_margin, tol)
    return s64, tol, ref, dict(e_ref=e_ref, edge_margin=edge_margin, tie_margin=tie_margin)


# the seeded random inputs the GPU file compares against fp64: (n, D, seed, threshold, min_samples)
PLANTED = [(257, 512, 501, 0.66, 4), (257, 512, 502, 0.67, 3), (257, 512, 503, 0.58, 2), (129, 96, 504, 0.62, 4)]
LEFT_OUT_CASE = (257, 96, 505, 0.66, 4)


def left_out_valid(n):
    """Valid bytes with zeros at both tile borders and at the last row, which padding re-reads."""
    valid = np.ones(n, dtype=np.uint8)
    valid[[0, 5, 127, 128, n // 2 + 3, n - 1]] = 0
    return valid


@functools.lru_cache(maxsize=None)
def planted_case(n, D, seed, threshold, min_samples, with_valid=False):
    x = planted_rows(n, D, seed, identities=max(4, n * 40 // 257))
    valid = left_out_valid(n) if with_valid else None
    s64, tol, ref, report = margins(x, threshold, min_samples, valid)
    return x, valid, ref, report


# ---------------------------------------------------------------------------------- hand-worked cases
def _sym(n, pairs, fill=0.0, dtype=np.float32):
    s = np.full((n, n), fill, dtype=dtype)
    np.fill_diagonal(s, 1.0)
    for (i, j), v in pairs.items():
        s[i, j] = s[j, i] = v
    return s


TWO_TRIANGLES = _sym(6, {(0, 1): 0.9, (0, 2): 0.9, (1, 2): 0.9, (3, 4): 0.9, (3, 5): 0.9, (4, 5): 0.9, (2, 3): 0.8})


def test_two_triangles_joined_by_one_edge():
    """Rows 0 1 2 and 3 4 5 are triangles, 2 - 3 the joining edge; threshold 0.5. Degrees
    2 2 3 3 2 2. min_samples 1, 2, 3: every row is core, one cluster rooted at 0. min_samples 4:
    only rows 2 and 3 are core (3 + 1 >= 4) and linked; rows 0 1 are border of 2, rows 4 5 of 3:
    still one cluster, rooted at 2."""
    for ms in (1, 2, 3):
        r = dbscan_ref(TWO_TRIANGLES, None, 0.5, ms)
        assert r.degree.tolist() == [2, 2, 3, 3, 2, 2] and r.kind.tolist() == [CORE] * 6
        assert r.root.tolist() == [0] * 6 and r.cluster.tolist() == [0] * 6
        assert r.n_clusters == 1 and r.sizes.tolist() == [6]
    r = dbscan_ref(TWO_TRIANGLES, None, 0.5, 4)
    assert r.kind.tolist() == [BORDER, BORDER, CORE, CORE, BORDER, BORDER]
    assert r.root.tolist() == [2] * 6 and r.cluster.tolist() == [0] * 6 and r.sizes.tolist() == [6]
    # at 0.85 the joining edge is gone: two clusters, ids ascending with the root
    r = dbscan_ref(TWO_TRIANGLES, None, 0.85, 3)
    assert r.root.tolist() == [0, 0, 0, 3, 3, 3] and r.cluster.tolist() == [0, 0, 0, 1, 1, 1]
    assert r.n_clusters == 2 and r.sizes.tolist() == [3, 3]
    # min_samples 5: nobody is core, everything is noise
    r = dbscan_ref(TWO_TRIANGLES, None, 0.5, 5)
    assert r.kind.tolist() == [NOISE] * 6 and r.root.tolist() == [-1] * 6 and r.n_clusters == 0 and r.sizes.size == 0


def _two_clusters_and_a_border(s_first, s_second):
    """Rows 0..3 and rows 4..7 are complete graphs (0.9) that are not joined; row 8 scores
    ``s_first`` against row 1, ``s_second`` against row 6 and 0 against the rest. At min_samples 4
    the eight rows are core (3 + 1) and row 8, with two neighbours, is not."""
    pairs = {(i, j): 0.9 for i in range(4) for j in range(i + 1, 4)}
    pairs.update({(i, j): 0.9 for i in range(4, 8) for j in range(i + 1, 8)})
    pairs.update({(1, 8): s_first, (6, 8): s_second})
    return _sym(9, pairs)


def test_border_row_between_two_clusters_takes_the_higher_score():
    """K4s on rows 0..3 and 4..7, min_samples 4, threshold 0.5; row 8 scores 0.6 against row 1 and
    0.7 against row 6: degree 2, not core, border of the second cluster (root 4)."""
    r = dbscan_ref(_two_clusters_and_a_border(0.6, 0.7), None, 0.5, 4)
    assert r.degree.tolist() == [3, 4, 3, 3, 3, 3, 4, 3, 2]
    assert r.kind.tolist() == [CORE] * 8 + [BORDER] and r.root.tolist() == [0] * 4 + [4] * 4 + [4]
    assert r.cluster.tolist() == [0] * 4 + [1] * 5 and r.sizes.tolist() == [4, 5] and r.n_clusters == 2
    r = dbscan_ref(_two_clusters_and_a_border(0.7, 0.6), None, 0.5, 4)
    assert r.root[8] == 0 and r.cluster[8] == 0 and r.sizes.tolist() == [5, 4]


def test_border_row_with_equal_scores_takes_the_lower_core_row():
    """The same with 0.625 on both sides: the lower core row (1, in the first cluster) wins."""
    r = dbscan_ref(_two_clusters_and_a_border(0.625, 0.625), None, 0.5, 4)
    assert r.kind[8] == BORDER and r.root[8] == 0 and r.cluster[8] == 0 and r.sizes.tolist() == [5, 4]


def test_border_row_whose_only_neighbour_is_a_border_row_stays_noise():
    """K4 on rows 0..3, min_samples 4, threshold 0.5; row 4 scores 0.8 against row 0 (border), row
    5 scores 0.8 against row 4 alone: its only neighbour is not core, so it is noise."""
    pairs = {(i, j): 0.9 for i in range(4) for j in range(i + 1, 4)}
    pairs.update({(0, 4): 0.8, (4, 5): 0.8})
    r = dbscan_ref(_sym(6, pairs), None, 0.5, 4)
    assert r.degree.tolist() == [4, 3, 3, 3, 2, 1]
    assert r.kind.tolist() == [CORE] * 4 + [BORDER, NOISE] and r.root.tolist() == [0] * 5 + [-1]
    assert r.cluster.tolist() == [0] * 5 + [-1] and r.sizes.tolist() == [5]


def test_a_score_equal_to_the_threshold_is_accepted_and_one_ulp_below_is_not():
    """Three rows, fp32 threshold t = 0.3 (not exact in binary): score(0, 1) == t is accepted,
    score(1, 2) == nextafter(t, -inf) is not; min_samples 2."""
    t = np.float32(0.3)
    below = np.nextafter(t, np.float32(-np.inf))
    r = dbscan_ref(_sym(3, {(0, 1): t, (1, 2): below}), None, t, 2)
    assert r.degree.tolist() == [1, 1, 0] and r.kind.tolist() == [CORE, CORE, NOISE] and r.root.tolist() == [0, 0, -1]
    r = dbscan_ref(_sym(3, {(0, 1): t, (1, 2): below}), None, below, 2)
    assert r.degree.tolist() == [1, 2, 1] and r.root.tolist() == [0, 0, 0]
    # a negative threshold orders the same way
    r = dbscan_ref(_sym(3, {(0, 1): -t, (1, 2): np.nextafter(-t, np.float32(-np.inf))}, fill=-1.0), None, -t, 2)
    assert r.degree.tolist() == [1, 1, 0]


def test_a_nan_or_infinite_score_is_no_neighbour():
    """Rows 0 1 2 a triangle at 0.9 but score(0, 2) is NaN and score(1, 3) is +inf: neither
    counts; threshold 0.5, min_samples 2: degrees 1 2 1 0, one cluster 0 1 2, row 3 noise."""
    r = dbscan_ref(_sym(4, {(0, 1): 0.9, (1, 2): 0.9, (0, 2): np.nan, (1, 3): np.inf}), None, 0.5, 2)
    assert r.degree.tolist() == [1, 2, 1, 0] and r.kind.tolist() == [CORE, CORE, CORE, NOISE]
    assert r.root.tolist() == [0, 0, 0, -1] and r.sizes.tolist() == [3]


def test_a_row_with_valid_byte_zero_takes_part_in_nothing():
    """The two triangles with row 2 left out: the joining edge goes with it; min_samples 2:
    clusters {0, 1} and {3, 4, 5}; row 2 has kind 0, degree 0, root and cluster -1."""
    r = dbscan_ref(TWO_TRIANGLES, [1, 1, 0, 1, 1, 1], 0.5, 2)
    assert r.degree.tolist() == [1, 1, 0, 2, 2, 2] and r.kind.tolist() == [CORE, CORE, LEFT_OUT, CORE, CORE, CORE]
    assert r.root.tolist() == [0, 0, -1, 3, 3, 3] and r.cluster.tolist() == [0, 0, -1, 1, 1, 1]
    assert r.sizes.tolist() == [2, 3]


def test_a_single_row():
    """N = 1: no pair. min_samples 1: the row is core and a cluster of its own; 2: noise; left out: nothing."""
    one = np.ones((1, 1), dtype=np.float32)
    r = dbscan_ref(one, None, 0.5, 1)
    assert (r.degree.tolist(), r.kind.tolist(), r.root.tolist(), r.cluster.tolist(), r.sizes.tolist(),
            r.n_clusters) == ([0], [CORE], [0], [0], [1], 1)
    r = dbscan_ref(one, None, 0.5, 2)
    assert (r.kind.tolist(), r.root.tolist(), r.cluster.tolist(), r.n_clusters) == ([NOISE], [-1], [-1], 0)
    r = dbscan_ref(one, [0], 0.5, 1)
    assert (r.kind.tolist(), r.root.tolist(), r.n_clusters) == ([LEFT_OUT], [-1], 0)


def test_no_core_row_at_all():
    """A path 0 - 1 - 2 at min_samples 4: degrees 1 2 1, nobody is core, no border without a core
    neighbour: all noise, C = 0."""
    r = dbscan_ref(_sym(3, {(0, 1): 0.9, (1, 2): 0.9}), None, 0.5, 4)
    assert r.degree.tolist() == [1, 2, 1] and r.kind.tolist() == [NOISE] * 3 and r.n_clusters == 0
    assert r.root.tolist() == [-1] * 3 and r.cluster.tolist() == [-1] * 3 and r.sizes.size == 0


def test_max_clusters_smaller_than_the_number_of_clusters():
    """Three pairs (0 1) (2 3) (4 5), min_samples 2: C = 3. max_clusters 2: cluster keeps the id
    2 for rows 4 5, n_clusters is 3, sizes has two entries; sums_ref gives two rows."""
    s = _sym(6, {(0, 1): 0.9, (2, 3): 0.9, (4, 5): 0.9})
    r = dbscan_ref(s, None, 0.5, 2, max_clusters=2)
    assert r.cluster.tolist() == [0, 0, 1, 1, 2, 2] and r.n_clusters == 3 and r.sizes.tolist() == [2, 2]
    x = np.arange(12, dtype=np.float32).reshape(6, 2) / 16
    sums = sums_ref(x, r.cluster, 2)
    assert sums.tolist() == [[(0 + 2) * 2 ** 28, (1 + 3) * 2 ** 28], [(4 + 6) * 2 ** 28, (5 + 7) * 2 ** 28]]
    assert centroids_ref(sums).tolist() == [[0.125, 0.25], [0.625, 0.75]]


def test_sums_round_to_nearest_even_and_are_exact():
    """2^-33 * 2^32 = 0.5 rounds to 0, 3 * 2^-33 to 2 (ties to even), -2^-33 to -0; 2^24 rows of
    +-1 would reach 2^56, inside int64."""
    x = np.array([[2.0 ** -33, 3 * 2.0 ** -33, -2.0 ** -33, 1.0, -1.0]], dtype=np.float32)
    assert sums_ref(x, [0], 1).tolist() == [[0, 2, 0, 2 ** 32, -2 ** 32]]
    assert 2 ** 24 * 2 ** 32 < 2 ** 63


# ---------------------------------------------------------------------------------- the two restatements agree
def test_the_two_restatements_agree_on_200_random_graphs():
    g = np.random.default_rng(2026)
    seen = collections.Counter()
    for case in range(200):
        n = int(g.integers(1, 25))
        s = g.integers(-8, 9, (n, n)).astype(np.float32) / 8                   # few distinct scores: many ties
        s = np.triu(s, 1) + np.triu(s, 1).T + np.eye(n, dtype=np.float32)
        if case % 3 == 0 and n > 1:
            i, j = g.choice(n, 2, replace=False)
            s[i, j] = s[j, i] = [np.nan, np.inf, -np.inf][case % 9 // 3]
        valid = (g.random(n) > 0.15).astype(np.uint8) if case % 2 else None
        thr, ms = float(g.integers(-2, 8)) / 8, int(g.integers(1, 6))
        a, b = dbscan_ref(s, valid, thr, ms), _dbscan_union_find(s, valid, thr, ms)
        assert same_ref(a, b), (case, n, thr, ms)
        for k in range(4):
            seen[k] += int((a.kind == k).sum())
        seen["clusters"] += a.n_clusters
    assert all(seen[k] > 50 for k in (LEFT_OUT, NOISE, BORDER, CORE)) and seen["clusters"] > 100, seen


# ---------------------------------------------------------------------------------- margins of the GPU inputs
@pytest.mark.parametrize("case", PLANTED)
def test_planted_inputs_meet_the_margin_conditions(case):
    x, valid, ref, report = planted_case(*case)
    counts = np.bincount(ref.kind, minlength=4)
    print(f"planted {case}: {report} kinds={counts.tolist()} clusters={ref.n_clusters}")
    assert ref.n_clusters >= 10 and counts[CORE] > 0 and counts[NOISE] > 0
    if case[4] > 2:
        assert counts[BORDER] > 0


def test_left_out_input_meets_the_margin_conditions():
    x, valid, ref, report = planted_case(*LEFT_OUT_CASE, with_valid=True)
    counts = np.bincount(ref.kind, minlength=4)
    print(f"left out {LEFT_OUT_CASE}: {report} kinds={counts.tolist()} clusters={ref.n_clusters}")
    assert counts[LEFT_OUT] == 6 and ref.n_clusters >= 10 and counts[BORDER] > 0


def test_chain_rows_are_a_ring_with_a_repeated_row():
    x = chain_rows(257, 512).astype(np.float64)
    s = x @ x.T
    assert (x * x).sum(axis=1).tolist() == [1.0] * 257 and np.array_equal(x[256], x[0])
    want = np.zeros((257, 257))
    for i in range(256):
        want[i, (i + 1) % 256] = want[(i + 1) % 256, i] = 0.5
    want[256], want[:, 256] = want[0], want[:, 0]
    want[0, 256] = want[256, 0] = 1.0
    np.fill_diagonal(want, 1.0)
    assert np.array_equal(s, want)
    for ms in (1, 3):
        r = dbscan_ref(s, None, 0.5, ms)
        assert r.n_clusters == 1 and r.sizes.tolist() == [257] and (r.kind == CORE).all()
    cut = np.ones(257, dtype=np.uint8)
    cut[[40, 130, 200]] = 0
    assert dbscan_ref(s, cut, 0.5, 1).n_clusters == 3


# ---------------------------------------------------------------------------------- the tile walk
# Inputs of tests/test_gpu_pairs_walk.py, at the sizes where every workgroup of the two pair passes
# walks at least three 128 x 128 tiles (``walk_sizes``, tests/test_faceverif_host.py) and where
# fc_compact_kernel scans more than one chunk of SCAN_CHUNK rows. Every input is exact: rows of
# four +-0.5, whose fp32 scores x @ x.T are the fp64 ones, so every comparison is an equality.
TILE = 128
SCAN_CHUNK = 8192
RING_CUTS = (40, 130, 200)
RING_MIN_SAMPLES = (1, 40)


def scores32(x):
    """The fp32 score matrix of exact rows (multiples of 0.25, at most four terms a sum)."""
    return x @ x.T


def left_out_walk(n):
    """Valid bytes with zeros on both sides of the first, a middle and the last tile border, at
    rows 0 and 5 and at the last row (the padded tile row's only row when n = k T + 1)."""
    valid = np.ones(n, dtype=np.uint8)
    mid, last = (n // TILE // 2) * TILE, (n - 1) // TILE * TILE
    valid[[0, 5, TILE - 1, TILE, mid - 1, mid, last - 1, last, n - 1]] = 0
    return valid


def ring_valid(n, cuts=RING_CUTS):
    """``chain_rows(n, 512)`` repeats with period 256: row i scores 0.5 with the rows of residue
    i +- 1 (mod 256) and 1.0 with those of its own. Leaving out every row of three residues cuts
    the ring of residues into three arcs, each with rows in tiles all over the triangle."""
    return (~np.isin(np.arange(n) % 256, cuts)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def ring_case(n):
    """(rows, valid, fp32 scores) of the cut ring of n rows; the arrays are shared: do not write them."""
    x = chain_rows(n, 512)
    return x, ring_valid(n), scores32(x)


def same_partition(cluster_a, cluster_b):
    """Two cluster id vectors over the same rows name the same partition (and the same rows -1)."""
    pairs = {(int(a), int(b)) for a, b in zip(cluster_a, cluster_b)}
    return (len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})
            and bool(((np.asarray(cluster_a) < 0) == (np.asarray(cluster_b) < 0)).all()))


SCATTERED = dict(D=96, seed=4200, threshold=0.75, min_samples=6, satellites=160, loners=25)


def scattered_rows(n, D, seed, satellites, loners):
    """Many small clusters whose members lie all over the rows. The last 18 columns are a pool of
    "extra" columns, the others 3-column triples; a group is a triple with one of 8 sign patterns
    (two groups' triples score at most 0.25 with each other). A member holds its group's triple
    and one seeded extra entry: two members of a group score 0.75, +-0.25 when they share the
    extra column; members of different groups at most 0.5. A satellite holds two columns of a
    group's triple and two extra entries: 0.75 with the few members that share one of those (also
    of the sibling group that differs in the third sign only), below that with all others. A loner
    holds four extra entries. A seeded permutation scatters all of them. Returns the rows and, per
    row, the group (-1: satellite, -2: loner)."""
    g = np.random.default_rng(seed)
    base, pool = D - 18, 18
    groups = base // 3 * 8
    x = np.zeros((n, D), dtype=np.float32)
    group = np.empty(n, dtype=np.int64)
    members = n - satellites - loners
    for k in range(n):
        if k < members:
            group[k] = k % groups
            t, sg = divmod(k % groups, 8)
            for e in range(3):
                x[k, 3 * t + e] = -0.5 if sg >> e & 1 else 0.5
            x[k, base + g.integers(pool)] = g.choice([-0.5, 0.5])
        elif k < members + satellites:
            group[k] = -1
            t, sg = divmod(int(g.integers(groups)), 8)
            for e in (0, 1):
                x[k, 3 * t + e] = -0.5 if sg >> e & 1 else 0.5
            x[k, base + g.choice(pool, 2, replace=False)] = g.choice([-0.5, 0.5], 2)
        else:
            group[k] = -2
            x[k, base + g.choice(pool, 4, replace=False)] = g.choice([-0.5, 0.5], 4)
    perm = g.permutation(n)
    return x[perm], group[perm]


@functools.lru_cache(maxsize=None)
def scattered_case(n):
    """(rows, group, valid, fp32 scores, dbscan_ref) of the scattered clusters at n rows; shared."""
    x, group = scattered_rows(n, SCATTERED["D"], SCATTERED["seed"], SCATTERED["satellites"], SCATTERED["loners"])
    valid = left_out_walk(n)
    s = scores32(x)
    return x, group, valid, s, dbscan_ref(s, valid, SCATTERED["threshold"], SCATTERED["min_samples"])


def _patterns(count, seed):
    """``count`` distinct rows of four +-0.5 in 32 columns: any two score at most 0.75."""
    import itertools
    combos = np.array(list(itertools.combinations(range(32), 4)))
    assert count <= 16 * len(combos)
    order = np.random.default_rng(seed).permutation(16 * len(combos))[:count]
    x = np.zeros((count, 32), dtype=np.float32)
    for k, o in enumerate(order):
        for e in range(4):
            x[k, combos[o // 16, e]] = -0.5 if o % 16 >> e & 1 else 0.5
    return x


@functools.lru_cache(maxsize=None)
def scan_case(n, chunk=SCAN_CHUNK, seed=4300):
    """Input and expected result of the compaction scan past one chunk, at threshold 1.0 and
    min_samples 2 on D = 32 rows: two rows are neighbours exactly when they are the same pattern,
    so the score matrix is block-sparse by construction and the reference is written per group
    (no n x n matrix): a pattern's rows that take part are one cluster rooted at the lowest when
    there are two or more, noise when there is one. Walking the rows upwards, a free row becomes a
    cluster root with 1 to 3 further members at seeded free rows up to chunk / 8 above, a noise
    row with a pattern of its own, or a left-out row (valid 0) that repeats an earlier row's
    pattern. Rows chunk - 1, chunk, 2 chunk - 1 and 2 chunk are roots. Returns (rows, valid, Ref)."""
    assert n > 2 * chunk + 2
    g = np.random.default_rng(seed)
    pat = np.full(n, -1, dtype=np.int64)
    valid = np.ones(n, dtype=np.uint8)
    reserved = np.zeros(n, dtype=bool)
    forced = [chunk - 1, chunk, 2 * chunk - 1, 2 * chunk]
    reserved[forced] = True
    npat = 0
    for i in range(n):
        if pat[i] >= 0:
            continue
        u = g.random()
        free = i + 1 + np.flatnonzero((pat[i + 1:i + 1 + chunk // 8] < 0) & ~reserved[i + 1:i + 1 + chunk // 8])
        if (reserved[i] or u < 0.45) and free.size:
            pat[i] = npat
            pat[g.choice(free, min(int(g.integers(1, 4)), free.size), replace=False)] = npat
            npat += 1
        elif u < 0.8 or i == 0:
            pat[i] = npat
            npat += 1
        else:
            pat[i] = pat[g.integers(i)]
            valid[i] = 0
    x = _patterns(npat, seed + 1)[pat]
    root = np.full(n, -1, dtype=np.int64)
    kind = np.where(valid != 0, NOISE, LEFT_OUT).astype(np.int64)
    degree = np.zeros(n, dtype=np.int64)
    rows_of = collections.defaultdict(list)
    for i in np.flatnonzero(valid):
        rows_of[int(pat[i])].append(int(i))
    for rows in rows_of.values():
        degree[rows] = len(rows) - 1
        if len(rows) >= 2:
            root[rows], kind[rows] = rows[0], CORE
    roots = np.unique(root[root >= 0])
    cluster = np.where(root >= 0, np.searchsorted(roots, root), -1)
    assert all(root[r] == r for r in forced)
    return x, valid, Ref(root, kind, degree, cluster, np.bincount(cluster[cluster >= 0]).astype(np.int64), len(roots))


def test_ring_of_many_tiles_meets_its_conditions():
    """At the 4865 rows of a 256-CU device: three clusters, each with rows in at least 19 of the
    39 tile rows (an arc inside one half of the residues lies in every second tile row), each
    rooted at its lowest (core) row. At min_samples 40 the rows next to a cut are border rows
    (degree 37: 18 of their own residue, 19 on one side) whose core neighbours all score 0.5, so
    the lowest row decides; everything else that takes part is core (degree >= 56)."""
    tn, n = 39, 4865
    x, valid, s = ring_case(n)
    assert np.array_equal(s[:300], (x[:300].astype(np.float64) @ x.astype(np.float64).T).astype(np.float32))
    res = np.arange(n) % 256
    for ms in RING_MIN_SAMPLES:
        ref = dbscan_ref(s, valid, 0.5, ms)
        assert ref.n_clusters == 3 and (ref.kind[valid == 0] == LEFT_OUT).all() and (ref.kind != NOISE).all()
        for c in range(3):
            rows = np.flatnonzero(ref.cluster == c)
            assert np.unique(rows // TILE).size >= (tn - 1) // 2
            assert (ref.root[rows] == rows[ref.kind[rows] == CORE].min()).all()
        next_to_cut = np.isin(res, [r + d for r in RING_CUTS for d in (-1, 1)])
        if ms == 1:
            assert (ref.kind[valid != 0] == CORE).all()
            continue
        assert (ref.kind[next_to_cut] == BORDER).all() and (ref.kind[(valid != 0) & ~next_to_cut] == CORE).all()
        assert ref.degree[next_to_cut].max() == 37 and ref.degree[(valid != 0) & ~next_to_cut].min() == 56
        for i in np.flatnonzero(next_to_cut)[::7]:
            cand = s[i, (ref.kind == CORE) & (s[i] >= 0.5) & (valid != 0)]
            assert cand.size >= 19 and (cand == 0.5).all()


def test_scattered_clusters_meet_their_conditions():
    tn, n = 39, 4865
    x, group, valid, s, ref = scattered_case(n)
    thr = np.float32(SCATTERED["threshold"])
    assert np.array_equal(s[:300], (x[:300].astype(np.float64) @ x.astype(np.float64).T).astype(np.float32))
    assert ((x * x).sum(axis=1) == 1).all()
    counts = np.bincount(ref.kind, minlength=4)
    assert ref.n_clusters >= 50 and counts[NOISE] > 0 and counts[BORDER] > 0 and counts[CORE] > 0
    assert counts[LEFT_OUT] == 8 and np.array_equal(np.flatnonzero(valid == 0),
                                                    [0, 5, 127, 128, 19 * 128 - 1, 19 * 128, n - 2, n - 1])
    spread = [np.unique(np.flatnonzero(ref.cluster == c) // TILE).size for c in range(ref.n_clusters)]
    assert np.median(spread) >= 3 and min(spread) >= 3
    on = valid != 0
    pair = on[:, None] & on[None, :] & ~np.eye(n, dtype=bool)
    assert (s[pair] == thr).any() and (s[pair] > thr).any() and (s[pair] < thr).any()
    # a border row between two clusters whose best core neighbours tie: the lowest row decides
    decided = 0
    for i in np.flatnonzero(ref.kind == BORDER):
        cand = np.flatnonzero(pair[i] & (s[i] >= thr) & (ref.kind == CORE))
        best = cand[s[i, cand] == s[i, cand].max()]
        decided += np.unique(ref.cluster[best]).size > 1
    print(f"scattered n={n}: clusters={ref.n_clusters} kinds={counts.tolist()} median tile rows={np.median(spread)} "
          f"border rows tied between clusters={decided}")
    assert decided >= 1


def test_scan_case_is_dbscan_ref_at_a_small_chunk_and_meets_its_conditions():
    """The per-group reference of ``scan_case`` against ``dbscan_ref`` with the chunk scaled down
    to 64 rows; at the real chunk: core roots, noise and left-out rows in every scan pass, roots
    on both sides of both chunk borders, ids ascending with the root."""
    for seed in (1, 2, 3):
        x, valid, ref = scan_case(2 * 64 + 50, chunk=64, seed=seed)
        assert same_ref(ref, dbscan_ref(scores32(x), valid, 1.0, 2))
        assert all(ref.root[r] == r for r in (63, 64, 127, 128))
    n = 2 * SCAN_CHUNK + 3 * TILE + 1
    x, valid, ref = scan_case(n)
    assert n == 131 * TILE + 1 and ((x * x).sum(axis=1) == 1).all()
    is_root = ref.root == np.arange(n)
    assert is_root[[SCAN_CHUNK - 1, SCAN_CHUNK, 2 * SCAN_CHUNK - 1, 2 * SCAN_CHUNK]].all()
    for p in range(3):
        rows = slice(p * SCAN_CHUNK, min((p + 1) * SCAN_CHUNK, n))
        assert is_root[rows].sum() >= 20 and {LEFT_OUT, NOISE, CORE} == set(ref.kind[rows].tolist())
    assert np.array_equal(ref.cluster[is_root], np.arange(ref.n_clusters)) and ref.n_clusters > 1000
    assert (ref.kind[valid == 0] == LEFT_OUT).all() and ref.sizes.sum() == (ref.kind == CORE).sum()
    # a cluster has members in a later pass than its root, and a left-out row repeats a live pattern
    assert (ref.root[2 * SCAN_CHUNK:] < 2 * SCAN_CHUNK)[ref.root[2 * SCAN_CHUNK:] >= 0].any()
    some = np.flatnonzero(valid == 0)[:200]
    assert any((x[valid != 0] == x[i]).all(axis=1).any() for i in some)


# ---------------------------------------------------------------------------------- ABI and refusals
NAMES = (("int64_t", "prpe_face_cluster_workspace_bytes", 1), ("int", "prpe_pair_degree", 8),
         ("int", "prpe_pair_link", 11), ("int", "prpe_cluster_finish", 13), ("int", "prpe_cluster_centroids", 10))


def test_abi_table_has_the_clustering_entry_points():
    header = open(os.path.join(ROOT, "include", "prpe.h")).read()
    assert int(re.search(r"#define PRPE_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 12
    L = _lib.lib()
    for res, name, nargs in NAMES:
        decl = re.search(r"\b%s %s\s*\(([^;]*)\);" % (res, name), header)
        assert decl and len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(L, name)


def workspace_bytes_ref(n):
    return (12 * n + 255) // 256 * 256


def test_workspace_bytes():
    L = _lib.lib()
    for n in (1, 21, 22, 257, 2 ** 24):
        assert L.prpe_face_cluster_workspace_bytes(n) == workspace_bytes_ref(n)
    for n in (0, -1, 2 ** 24 + 1):
        assert L.prpe_face_cluster_workspace_bytes(n) == -22


ROWS_REFUSALS = [dict(a=None), dict(N=0), dict(N=-1), dict(N=2 ** 24 + 1), dict(D=0), dict(D=48), dict(D=16),
                 dict(D=544), dict(lda=508), dict(lda=514), dict(a=0x1008)]
NAN, INF = float("nan"), float("inf")


def cluster_refusals():
    """Every -EINVAL case of the header: (entry point, keyword overrides of ``call_cluster``)."""
    out = [("degree", kw) for kw in ROWS_REFUSALS + [dict(thr=NAN), dict(thr=INF), dict(thr=-INF), dict(degree=None)]]
    out += [("link", kw) for kw in ROWS_REFUSALS + [dict(thr=NAN), dict(thr=INF), dict(degree=None), dict(ms=0),
                                                    dict(ms=-3), dict(ws=None), dict(ws_off=128), dict(ws_off=8),
                                                    dict(ws_short=1), dict(ws_bytes=0)]]
    out += [("finish", kw) for kw in [dict(N=0), dict(N=2 ** 24 + 1), dict(ms=0), dict(degree=None), dict(ws=None),
                                      dict(ws_off=64), dict(ws_short=1), dict(root=None), dict(kind=None),
                                      dict(cluster=None), dict(n_clusters=None), dict(sizes=None), dict(max_clusters=0),
                                      dict(max_clusters=-1)]]
    out += [("centroids", kw) for kw in ROWS_REFUSALS + [dict(cluster=None), dict(n_clusters=None), dict(sums=None),
                                                         dict(centroids=None), dict(max_clusters=0)]]
    return out


def call_cluster(L, which, a=0x1000, lda=512, N=100, valid=None, D=512, thr=0.5, ms=2, degree=0x100000, ws=0x200000,
                 ws_off=0, ws_short=0, ws_bytes=None, root=0x300000, kind=0x400000, cluster=0x500000,
                 n_clusters=0x600000, max_clusters=100, sizes=0x700000, sums=0x800000, centroids=0x900000):
    if ws_bytes is None:
        ws_bytes = workspace_bytes_ref(max(N, 1)) - ws_short
    ws = None if ws is None else ws + ws_off
    if which == "degree":
        return L.prpe_pair_degree(a, lda, N, valid, D, thr, degree, None)
    if which == "link":
        return L.prpe_pair_link(a, lda, N, valid, D, thr, ms, degree, ws, ws_bytes, None)
    if which == "finish":
        return L.prpe_cluster_finish(N, valid, ms, degree, ws, ws_bytes, root, kind, cluster, n_clusters, max_clusters,
                                     sizes, None)
    return L.prpe_cluster_centroids(a, lda, N, D, cluster, n_clusters, max_clusters, sums, centroids, None)


def test_library_rejects_bad_clustering_arguments_before_launch():
    L = _lib.lib()
    for which, kw in cluster_refusals():
        assert call_cluster(L, which, **kw) == -22, (which, kw)


# ---------------------------------------------------------------------------------- FaceClusters
def test_face_clusters_bookkeeping_with_the_kernels_stubbed(monkeypatch):
    import prpe
    from prpe import clusters as cmod
    from prpe import gallery as gmod
    assert "FaceClusters" in prpe.__all__ and "FaceClustering" in prpe.__all__
    calls = []

    def pair_degree(a, threshold, *, degree, valid=None):
        calls.append(("degree", tuple(a.shape), threshold, valid is not None))

    def pair_link(a, threshold, min_samples, *, degree, workspace, valid=None):
        calls.append(("link", threshold, min_samples, workspace.numel()))

    def cluster_finish(N, min_samples, *, degree, workspace, root, kind, cluster, n_clusters, sizes, valid=None):
        calls.append(("finish", N, min_samples, sizes.numel()))
        n_clusters[0] = 3
        sizes[:3] = torch.tensor([2, 1, 2], dtype=torch.int32)

    def cluster_centroids(a, *, cluster, n_clusters, sums, centroids):
        calls.append(("centroids", tuple(sums.shape)))
        centroids[:3] = torch.arange(3, dtype=torch.float32)[:, None] + 1

    def gallery_enrol(x, gallery, norms, row0=0):
        gallery[row0:row0 + x.shape[0]] = x

    monkeypatch.setattr(cmod.ops, "pair_degree", pair_degree)
    monkeypatch.setattr(cmod.ops, "pair_link", pair_link)
    monkeypatch.setattr(cmod.ops, "cluster_finish", cluster_finish)
    monkeypatch.setattr(cmod.ops, "cluster_centroids", cluster_centroids)
    monkeypatch.setattr(cmod.ops, "face_cluster_workspace_bytes", workspace_bytes_ref)
    monkeypatch.setattr(gmod.ops, "gallery_enrol", gallery_enrol)
    monkeypatch.setattr(prpe.FaceGallery, "_embeddings", lambda self, what, e: e.float().contiguous())
    c = prpe.FaceClusters(dim=64, capacity=8, device="cpu")
    with pytest.raises(ValueError, match="no rows"):
        c.cluster(0.5)
    assert c.add(torch.ones(5, 64)) == (0, 5) and len(c) == 5
    assert c.store.labels[:5].tolist() == [0] * 5
    with pytest.raises(ValueError, match="capacity"):
        c.add(torch.ones(4, 64))
    with pytest.raises(ValueError, match="max_clusters"):
        c.cluster(0.5, max_clusters=0)
    res = c.cluster(0.25, min_samples=3)
    assert calls == [("degree", (5, 64), 0.25, True), ("link", 0.25, 3, workspace_bytes_ref(5)), ("finish", 5, 3, 5),
                     ("centroids", (5, 64))]
    assert res.max_clusters == 5 and (res.threshold, res.min_samples) == (0.25, 3)
    gal = prpe.FaceGallery(dim=64, capacity=3, device="cpu")
    gal.add(torch.ones(1, 64), [7])
    assert res.enrol_into(gal, 100, min_size=2) == ((1, 3), [100, 102]) and len(gal) == 3
    assert gal.labels.tolist() == [7, 100, 102] and gal.rows[1:, 0].tolist() == [1.0, 3.0]
    with pytest.raises(ValueError, match="capacity"):
        res.enrol_into(gal, 200)
    assert len(gal) == 3 and gal.labels.tolist() == [7, 100, 102]
    assert res.enrol_into(gal, 200, min_size=3) == ((3, 3), [])
    res.n_clusters[0] = 6                                                      # more clusters than max_clusters
    with pytest.raises(ValueError, match="max_clusters"):
        res.enrol_into(prpe.FaceGallery(dim=64, capacity=9, device="cpu"), 0)
    with pytest.raises(ValueError, match="dim"):
        res.enrol_into(prpe.FaceGallery(dim=32, capacity=9, device="cpu"), 0)
    view = prpe.FaceClusters.of_gallery(gal)
    assert view.store is gal and len(view) == 3
    with pytest.raises(ValueError):
        prpe.FaceClusters.of_gallery(c)
