"""GPU: the all-pairs kernels where a workgroup walks several tiles -- pair_hist_kernel
(csrc/pairhist.hip) and pair_cluster_kernel<1|2> with the stages behind them
(csrc/facecluster.hip, §5j). Their grid is min(tiles, CUs) workgroups, each running
``for (id = blockIdx.x; id < ntiles; id += gridDim.x)`` over 128 x 128 score tiles; up to the 257
rows of tests/test_gpu_faceverif.py and tests/test_gpu_clusters.py that loop runs once. Here the
sizes come from the device (``walk_sizes``, tests/test_faceverif_host.py): the smallest triangle
with three tiles per workgroup, one row past a tile multiple, so that every workgroup has a first,
a middle and a last tile and the padded tile row comes late in the walk (256 CUs: 39 tile rows,
4865 rows, 780 tiles; cross mode 2049 x 5761 rows, 17 x 46 tiles). Every test asserts
tiles >= 3 CUs for each launch it makes. What the second and later iterations alone execute: the
accumulators zeroed in the epilogue, the labels / flags / local parents / best neighbours re-read
behind the loop-top barrier, the LDS counters kept across tiles, the first chunk re-staged after
the last one's barrier, the tile-id mapping (the square root with its two corrections; id / tn in
cross mode) past a handful of ids, global unions and 64-bit maxima on the same rows from hundreds
of workgroups, the pointer chase over trees built by many flushes, and (from 8193 rows on)
fc_compact_kernel's running base across scan chunks.

The harness is the one of the two files above (``Guarded`` buffers with sentinels, ``Out`` /
``pair_hist`` / ``launch``, ``Outs`` / ``run`` / ``same``); the inputs, their conditions and the
references are built and asserted on the CPU in tests/test_faceverif_host.py and
tests/test_clusters_host.py. All inputs compared with a reference are exact (rows of four +-0.5:
every score a multiple of 0.25 in any arithmetic), so every comparison is an equality; the random
rows are only compared with other launches on the same rows.

Measured on an MI355X: see DESIGN.md §5i and §5j.
"""
import functools

import numpy as np
import pytest
import torch

from prpe import ops
from test_clusters_host import (BORDER, CORE, LEFT_OUT, NOISE, RING_MIN_SAMPLES, SCAN_CHUNK, SCATTERED, dbscan_ref,
                                ring_case, same_partition, scan_case, scattered_case)
from test_faceverif_host import (TILE, four_halves, pair_hist_ref_blocks, tiles_of, walk_labels, walk_sizes,
                                 walk_sizes_cross)
from test_gpu_clusters import run, same
from test_gpu_faceverif import Out, enrol, launch, pair_hist

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def cus():
    """The CU count the kernels size their grid by (hipDeviceAttributeMultiprocessorCount)."""
    n = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"pairs walk: {n} CUs, self {walk_sizes(n)} (tile rows, rows), cross {walk_sizes_cross(n)} (tm, tn, M, N)")
    return n


def walk_n():
    assert TILE == ops.PAIR_HIST_TILE
    tn, n = walk_sizes(cus())
    assert tiles_of(n) == tn * (tn + 1) // 2 >= 3 * cus()
    return n


def dev(x):
    return torch.from_numpy(x).to(DEV)


# ---------------------------------------------------------------------------------- pair_hist: exact counts
NBINS = (256, 4096)


@functools.lru_cache(maxsize=None)
def exact_self():
    n = walk_n()
    x = four_halves(n, 32, 4100)
    labels, valid = walk_labels(n, 4101)
    return (x, labels, valid) + pair_hist_ref_blocks(x, None, labels, None, valid, None, NBINS)


@functools.lru_cache(maxsize=None)
def exact_cross():
    tm, tn, M, N = walk_sizes_cross(cus())
    assert tiles_of(M, N) == tiles_of(N, M) == tm * tn >= 3 * cus() and M != N
    x = four_halves(M + N, 32, 4110)
    (la, va), (lb, vb) = walk_labels(M, 4111), walk_labels(N, 4112)
    return (x[:M], x[M:], la, va, lb, vb) + pair_hist_ref_blocks(x[:M], x[M:], la, lb, va, vb, NBINS)


@pytest.mark.parametrize("nbins", NBINS)
def test_exact_inputs_give_the_integer_counts_self_many_tiles(nbins):
    """Labels change within and across tiles, a few are -1, valid bytes are 0 on tile borders and
    at the last row (the whole padded tile row counts nothing). ``hist.sum() + skipped`` is the
    number of participating pairs: no tile is walked twice or left out."""
    x, labels, valid, hists, want_skipped = exact_self()
    n = len(x)
    assert tiles_of(n) >= 3 * cus()
    hist, skipped = pair_hist(nbins, dev(x), labels, va=valid)
    n_on = int(((labels >= 0) & (valid != 0)).sum())
    assert n - 30 < n_on < n and hist.sum() + skipped == n_on * (n_on - 1) // 2
    assert skipped == want_skipped == 0 and np.array_equal(hist, hists[nbins])
    assert (hist[0] > 0).sum() == (hist[1] > 0).sum() == 9                     # the scores -1, -0.75 .. 1 of both classes


@pytest.mark.parametrize("nbins", NBINS)
def test_exact_inputs_give_the_integer_counts_cross_many_tiles(nbins):
    a, b, la, va, lb, vb, hists, want_skipped = exact_cross()
    assert tiles_of(len(a), len(b)) >= 3 * cus()
    hist, skipped = pair_hist(nbins, dev(a), la, dev(b), lb, va, vb)
    on_a, on_b = int(((la >= 0) & (va != 0)).sum()), int(((lb >= 0) & (vb != 0)).sum())
    assert hist.sum() + skipped == on_a * on_b
    assert skipped == want_skipped == 0 and np.array_equal(hist, hists[nbins])
    # the other way round: another tn in id / tn, the transposed scores, the same histogram
    hist_t, skipped_t = pair_hist(nbins, dev(b), lb, dev(a), la, vb, va)
    assert skipped_t == 0 and np.array_equal(hist_t, hists[nbins])


# ---------------------------------------------------------------------------------- pair_hist: decomposition
@functools.lru_cache(maxsize=None)
def random_set():
    """2 n + 7 normalised random rows of D = 32 around 7 centres, labels (a few -1) and valid bytes."""
    n = walk_n()
    total = 2 * n + 7
    g = torch.Generator().manual_seed(4120)
    ids = torch.randint(0, 7, (total,), generator=g)
    x = torch.randn(7, 32, generator=g)[ids] + 0.7 * torch.randn(total, 32, generator=g)
    labels, valid = walk_labels(total, 4121)
    labels = np.where(labels < 0, -1, ids.numpy())
    return enrol(x), labels, valid


def test_self_is_the_two_parts_and_their_cross_many_tiles():
    """hist_self(A u B) == hist_self(A) + hist_self(B) + hist_cross(A, B), bin for bin, on random
    normalised rows split one row past a tile multiple: a pair's score bits do not depend on the
    tile, the workgroup or the place in the walk it lands in. All four launches walk >= 3 tiles
    per workgroup."""
    rows, labels, valid = random_set()
    m, total, nbins = walk_n(), len(labels), 4096
    assert m % TILE == 1 and min(tiles_of(total), tiles_of(m), tiles_of(total - m), tiles_of(m, total - m)) >= 3 * cus()
    whole, skipped = pair_hist(nbins, rows, labels, va=valid)
    live = int(((labels >= 0) & (valid != 0)).sum())
    assert skipped == 0 and whole.sum() == live * (live - 1) // 2 and (whole > 0).sum() > nbins // 2
    out = Out(nbins)
    launch(out, nbins, rows[:m], labels[:m], va=valid[:m])
    launch(out, nbins, rows[m:], labels[m:], va=valid[m:])
    launch(out, nbins, rows[:m], labels[:m], rows[m:], labels[m:], va=valid[:m], vb=valid[m:])
    parts, skipped = out.host()
    assert skipped == 0 and np.array_equal(parts, whole)


def test_pairs_that_are_not_finite_are_skipped_once_many_tiles():
    """A NaN in the first tile row, in a middle one and in the last row, which the padded tile row
    re-reads 127 times: ``myskip`` is carried in registers over the whole walk and must be neither
    lost nor counted twice."""
    n, nbins = walk_n(), 512
    x = four_halves(n, 32, 4130).copy()
    bad = [5, (n // TILE // 2) * TILE + 77, n - 1]
    x[bad, [3, 0, 7]] = np.nan
    labels = np.random.default_rng(4131).integers(0, 4, n)
    hists, want_skipped = pair_hist_ref_blocks(x, None, labels, None, None, None, (nbins,))
    assert want_skipped == 3 * (n - 3) + 3 and tiles_of(n) >= 3 * cus()
    hist, skipped = pair_hist(nbins, dev(x), labels)
    assert skipped == want_skipped and hist.sum() + skipped == n * (n - 1) // 2
    assert np.array_equal(hist, hists[nbins])


def test_pair_hist_two_runs_give_identical_bytes_many_tiles():
    rows, labels, valid = random_set()
    n = walk_n()
    assert tiles_of(n) >= 3 * cus()
    a = pair_hist(4096, rows[:n], labels[:n], va=valid[:n])
    b = pair_hist(4096, rows[:n], labels[:n], va=valid[:n])
    assert a[1] == b[1] == 0 and a[0].tobytes() == b[0].tobytes() and a[0].sum() > 0


# ---------------------------------------------------------------------------------- clustering: the ring
@pytest.mark.parametrize("ms", RING_MIN_SAMPLES)
def test_a_ring_through_every_tile_cut_into_three_arcs(ms):
    """``chain_rows`` at D = 512 repeats with period 256, so the rows are one ring of residues whose
    links (0.5 to the residues next to it, 1.0 within one) lie in tiles all over the triangle;
    leaving out three residues cuts it into three components, each put together from unions that
    many workgroups flush at the same time. min_samples 1: every row is core. min_samples 40: the
    rows next to a cut are border rows whose core neighbours tie at 0.5
    (tests/test_clusters_host.py asserts it). Two seeded permutations, under which a component's
    links arrive from other tiles in another order, give the same partition."""
    n = walk_n()
    assert tiles_of(n) >= 3 * cus()
    x, valid, s = ring_case(n)
    ref = dbscan_ref(s, valid, 0.5, ms)
    assert ref.n_clusters == 3 and set(ref.kind.tolist()) == ({LEFT_OUT, CORE} if ms == 1 else {LEFT_OUT, BORDER, CORE})
    same(run(dev(x), 0.5, ms, valid, max_clusters=8), ref, x, 8)
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(n)
        xp, vp = x[perm], valid[perm]
        got = run(dev(xp), 0.5, ms, vp, max_clusters=8)
        same(got, dbscan_ref(s[np.ix_(perm, perm)], vp, 0.5, ms), xp, 8)
        there = np.empty(n, dtype=np.int64)
        there[perm] = got["cluster"]
        assert same_partition(ref.cluster, there)


# ---------------------------------------------------------------------------------- clustering: scattered clusters
def test_many_small_clusters_scattered_over_the_tiles():
    """About 200 clusters whose members a seeded permutation scatters over the tile rows, border
    rows between two clusters whose best core neighbours tie, noise, left-out rows on tile borders
    and at the last row, pairs exactly on the threshold (asserted in tests/test_clusters_host.py
    for 256 CUs); ``max_clusters`` above and below the number of clusters."""
    n = walk_n()
    assert tiles_of(n) >= 3 * cus()
    x, group, valid, s, ref = scattered_case(n)
    assert ref.n_clusters >= 50 and set(ref.kind.tolist()) == {LEFT_OUT, NOISE, BORDER, CORE}
    for max_clusters in (ref.n_clusters + 5, ref.n_clusters // 3):
        got = run(dev(x), SCATTERED["threshold"], SCATTERED["min_samples"], valid, max_clusters=max_clusters)
        same(got, ref, x, max_clusters)


def test_clustering_two_runs_give_identical_bytes_many_tiles():
    n = walk_n()
    assert tiles_of(n) >= 3 * cus()
    x, group, valid, s, ref = scattered_case(n)
    a = run(dev(x), SCATTERED["threshold"], SCATTERED["min_samples"], valid, max_clusters=ref.n_clusters)
    b = run(dev(x), SCATTERED["threshold"], SCATTERED["min_samples"], valid, max_clusters=ref.n_clusters)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ---------------------------------------------------------------------------------- degree against pair_hist
def test_degree_sum_is_what_pair_hist_puts_in_the_bins_above_many_tiles():
    rows, labels, valid = random_set()
    n, nbins = walk_n(), 2048
    assert tiles_of(n) >= 3 * cus()
    rows = rows[:n]
    hist, skipped = pair_hist(nbins, rows, np.zeros(n, dtype=np.int64))
    assert skipped == 0 and hist[1].sum() == 0 and hist[0].sum() == n * (n - 1) // 2
    h = nbins // 2
    for b in (h - 30, h, h + 45):
        degree = run(rows, (b - h) / h, 2, upto=1)["degree"]
        pairs = int(hist[0, b:].sum())
        assert 0 < pairs < n * (n - 1) // 2 and int(degree.sum()) == 2 * pairs, b


# ---------------------------------------------------------------------------------- the compaction scan
def test_compaction_scan_carries_its_base_across_chunks():
    """2 x 8192 + 385 rows: fc_compact_kernel scans three chunks, its running ``base`` carried
    from one to the next. Rows 8191, 8192, 16383 and 16384 are cluster roots, every chunk holds
    roots, noise and left-out rows, clusters reach across chunk borders
    (tests/test_clusters_host.py); the reference is written per group there. The two pair passes
    run as well (131 x 132 / 2 = 8646 tiles at D = 32). ``max_clusters`` above and below C."""
    n = 2 * SCAN_CHUNK + 3 * TILE + 1
    assert tiles_of(n) >= 3 * cus()
    x, valid, ref = scan_case(n)
    C = ref.n_clusters
    for max_clusters in (C + 3, C // 2):
        got = run(dev(x), 1.0, 2, valid, max_clusters=max_clusters)
        same(got, ref, x, max_clusters)
        roots = np.flatnonzero(got["root"] == np.arange(n))
        assert int(got["n_clusters"][0]) == C == roots.size and np.array_equal(got["cluster"][roots], np.arange(C))
        assert np.array_equal(got["sizes"][:min(C, max_clusters)], ref.sizes[:max_clusters])
