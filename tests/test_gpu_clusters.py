"""GPU: clustering of unlabelled face embeddings (csrc/facecluster.hip) --
prpe_pair_degree, prpe_pair_link, prpe_cluster_finish, prpe_cluster_centroids and ``FaceClusters``
above them -- against the host restatements of tests/test_clusters_host.py (``dbscan_ref``,
``sums_ref``), which also builds the inputs and asserts their margins on the CPU.

Every output and the workspace live in sentinel-filled buffers with guards on both sides
(``Guarded``, tests/test_gpu_rowops.py); every run is followed by a check that the guards are
untouched. T = ops.PAIR_HIST_TILE: the shapes sit on both sides of one and two tiles, and 2 T + 1
rows give six triangle tiles, so unions have to cross tiles. Six tiles are fewer than the CUs, so
every workgroup here takes one tile: the walk of several tiles per workgroup (4865 rows on 256 CUs)
and the compaction scan past one 8192-row chunk are tested in tests/test_gpu_pairs_walk.py.

* exact inputs (rows of four +-0.5) must give ``dbscan_ref`` / ``sums_ref`` exactly at thresholds
  that sit on attainable scores; chains (a ring of 0.5 links through every tile) and their
  permutations; the score bits and the equality edge against ``FaceGallery.search``; the degree sum
  against prpe_pair_hist's bins; planted clusters against fp64 (margins asserted on the CPU);
  determinism; left-out rows, NaN rows, row strides, max_clusters < C, refusals; the public
  interface end to end.

Measured on an MI355X: see DESIGN.md §5j.
"""
import numpy as np
import pytest
import torch

from prpe import FaceClusters, FaceGallery, _lib, ops
from test_clusters_host import (BORDER, CORE, LEFT_OUT, LEFT_OUT_CASE, NOISE, PLANTED, call_cluster, centroids_ref,
                                chain_rows, cluster_refusals, dbscan_ref, half_rows, left_out_valid, planted_case,
                                planted_rows, random_rows, sums_ref)
from test_gpu_rowops import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = ops.PAIR_HIST_TILE
ISENT, BSENT, FSENT = -7777, 0xEE, -7777.0


# ---------------------------------------------------------------------------------- harness
class Outs:
    """Guarded, sentinel-filled outputs and workspace of one clustering of n rows."""

    def __init__(self, n, D, max_clusters):
        self.n, self.D, self.max_clusters = n, D, max_clusters
        self.degree = Guarded((n,), fill=ISENT, dtype=torch.int32)
        self.root = Guarded((n,), fill=ISENT, dtype=torch.int32)
        self.cluster = Guarded((n,), fill=ISENT, dtype=torch.int32)
        self.kind = Guarded((n,), fill=BSENT, dtype=torch.uint8)
        self.n_clusters = Guarded((1,), fill=ISENT, dtype=torch.int32)
        self.sizes = Guarded((max_clusters,), fill=ISENT, dtype=torch.int32)
        self.sums = Guarded((max_clusters, D), fill=ISENT, dtype=torch.int64)
        self.centroids = Guarded((max_clusters, D), fill=FSENT)
        self.ws = Guarded((ops.face_cluster_workspace_bytes(n),), shift=192, fill=BSENT, dtype=torch.uint8)
        assert self.ws.view.data_ptr() % 256 == 0
        self.all = dict(degree=self.degree, root=self.root, cluster=self.cluster, kind=self.kind,
                        n_clusters=self.n_clusters, sizes=self.sizes, sums=self.sums, centroids=self.centroids)

    def untouched(self):
        return all(g.untouched() for g in self.all.values()) and self.ws.untouched()

    def host(self):
        assert self.untouched()
        return {k: g.cpu().numpy() for k, g in self.all.items()}

    def still_sentinel(self):
        h = self.host()
        return all((v.view(np.int32) == np.float32(FSENT).view(np.int32)).all() if k == "centroids" else
                   (v == (BSENT if k == "kind" else ISENT)).all() for k, v in h.items())


def _dev(t, dtype):
    return None if t is None else torch.as_tensor(np.asarray(t)).to(dtype).to(DEV)


def run(rows, threshold, min_samples, valid=None, max_clusters=None, upto=4):
    """The four stages on device rows [n, D]; the outputs on the host, guards checked."""
    n, D = rows.shape
    out = Outs(n, D, n if max_clusters is None else max_clusters)
    v = _dev(valid, torch.uint8)
    ops.pair_degree(rows, threshold, degree=out.degree.view, valid=v)
    if upto >= 2:
        ops.pair_link(rows, threshold, min_samples, degree=out.degree.view, workspace=out.ws.view, valid=v)
    if upto >= 3:
        ops.cluster_finish(n, min_samples, degree=out.degree.view, workspace=out.ws.view, root=out.root.view,
                           kind=out.kind.view, cluster=out.cluster.view, n_clusters=out.n_clusters.view,
                           sizes=out.sizes.view, valid=v)
    if upto >= 4:
        ops.cluster_centroids(rows, cluster=out.cluster.view, n_clusters=out.n_clusters.view, sums=out.sums.view,
                              centroids=out.centroids.view)
    return out.host()


def same(got, ref, rows_host, max_clusters=None):
    """Every output against a ``dbscan_ref`` result and the ``sums_ref`` of the stored rows; what
    lies past min(C, max_clusters) must still hold the sentinel."""
    n = ref.degree.size
    lim = ref.n_clusters if max_clusters is None else min(ref.n_clusters, max_clusters)
    assert np.array_equal(got["degree"], ref.degree), "degree"
    assert np.array_equal(got["kind"], ref.kind), "kind"
    assert np.array_equal(got["root"], ref.root), "root"
    assert np.array_equal(got["cluster"], ref.cluster), "cluster"
    assert int(got["n_clusters"][0]) == ref.n_clusters, "n_clusters"
    sizes = np.bincount(ref.cluster[(ref.cluster >= 0) & (ref.cluster < lim)], minlength=lim)
    assert np.array_equal(got["sizes"][:lim], sizes), "sizes"
    want = sums_ref(rows_host, ref.cluster, lim)
    assert np.array_equal(got["sums"][:lim], want), "sums"
    assert np.array_equal(got["centroids"][:lim].view(np.int32), centroids_ref(want).view(np.int32)), "centroids"
    assert (got["sizes"][lim:] == ISENT).all() and (got["sums"][lim:] == ISENT).all()
    assert (got["centroids"][lim:] == np.float32(FSENT)).all()
    assert n == got["degree"].size


def enrol(x):
    """Raw host rows -> normalised device rows, as a gallery stores them."""
    n, D = x.shape
    rows, norms = torch.empty(n, D, device=DEV), torch.empty(n, device=DEV)
    ops.gallery_enrol(x.to(DEV).contiguous(), rows, norms, 0)
    return rows


def exact_scores(x):
    return (x.astype(np.float64) @ x.astype(np.float64).T).astype(np.float32)


# ---------------------------------------------------------------------------------- 1. exact inputs
SHAPES = [(n, D) for n in (1, 2, 17, T - 1, T, T + 1, 2 * T + 1) for D in (32, 96, 512)]
THRESHOLDS = (0.25, 0.5, 0.75, 1.0)
MIN_SAMPLES = {32: (1, 3), 96: (2, 5), 512: (1, 2, 3, 5)}


@pytest.mark.parametrize("n,D", SHAPES)
def test_exact_inputs_give_the_reference_exactly(n, D):
    x = half_rows(n, D, 3000 + n + D)
    rows = torch.from_numpy(x).to(DEV)
    s = exact_scores(x)
    seen = set()
    for thr in THRESHOLDS:
        if n >= T - 1 and thr < 1.0:
            assert (s[np.triu_indices(n, 1)] == np.float32(thr)).any()            # equality is exercised
        for ms in MIN_SAMPLES[D]:
            ref = dbscan_ref(s, None, thr, ms)
            same(run(rows, thr, ms), ref, x)
            seen.update(ref.kind.tolist())
    if n >= T - 1:
        assert seen == {NOISE, BORDER, CORE}


# ---------------------------------------------------------------------------------- 2. chains
@pytest.mark.parametrize("ms", [1, 3])
def test_chains_link_across_every_tile_and_under_permutations(ms):
    """2 T + 1 = 257 rows at D = 512: the column pattern of ``chain_rows`` wraps once, so row 256
    repeats row 0 and the rows are a ring of 0.5 links with row 256 lying on row 0. The expected
    result is ``dbscan_ref``'s on the exact scores. Three left-out rows cut the ring into three
    components; three seeded permutations must give the same partition."""
    n, D = 2 * T + 1, 512
    x = chain_rows(n, D)
    cut = np.ones(n, dtype=np.uint8)
    cut[[40, 130, 200]] = 0
    for valid in (None, cut):
        ref = dbscan_ref(exact_scores(x), valid, 0.5, ms)
        same(run(torch.from_numpy(x).to(DEV), 0.5, ms, valid), ref, x)
        assert ref.n_clusters == (1 if valid is None else 3)
        for seed in (1, 2, 3):
            perm = np.random.default_rng(seed).permutation(n)
            xp, vp = x[perm], None if valid is None else valid[perm]
            got = run(torch.from_numpy(xp).to(DEV), 0.5, ms, vp)
            same(got, dbscan_ref(exact_scores(xp), vp, 0.5, ms), xp)
            # the partition of the original rows: rows together here are together there
            there = np.empty(n, dtype=np.int64)
            there[perm] = got["cluster"]
            pairs = {(int(a), int(b)) for a, b in zip(ref.cluster, there)}
            assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})
            assert ((there < 0) == (ref.cluster < 0)).all()


# ---------------------------------------------------------------------------------- 3. score bits, equality edge
@pytest.mark.parametrize("D", [96, 512])
def test_degree_counts_the_scores_search_returns(D):
    n = 8
    x = random_rows(n, D, 60 + D)
    gal = FaceGallery(dim=D, capacity=n, device=DEV)
    gal.add(x.to(DEV), list(range(n)))
    sc, idx, _ = gal.search(x.to(DEV), k=n)
    sc, idx = sc.cpu().numpy(), idx.cpu().numpy()
    assert (np.sort(idx, axis=1) == np.arange(n)).all()
    me = idx == np.arange(n)[:, None]
    others = np.unique(sc[~me])
    for t in (others[0], others[len(others) // 2], others[-1]):
        for thr in (np.float32(t), np.nextafter(np.float32(t), np.float32(np.inf))):
            want = (sc >= thr).sum(axis=1) - (me & (sc >= thr)).sum(axis=1)
            got = run(gal.rows[:n], float(thr), 2, upto=1)["degree"]
            assert np.array_equal(got, want), (float(thr), got, want)
        assert ((sc == t) & ~me).sum() >= 2                                   # the pair, seen from both rows


# ---------------------------------------------------------------------------------- 4. the shipped kernel
def test_degree_sum_is_what_pair_hist_puts_in_the_bins_above():
    n, D, nbins = 2 * T + 1, 512, 2048
    rows = enrol(random_rows(n, D, 71))
    hist = torch.zeros(2, nbins, device=DEV, dtype=torch.int64)
    skipped = torch.zeros(1, device=DEV, dtype=torch.int64)
    ops.pair_hist(rows, torch.zeros(n, device=DEV, dtype=torch.int64), nbins=nbins, hist=hist, skipped=skipped)
    hist = hist.cpu().numpy()
    assert int(skipped[0]) == 0 and hist[1].sum() == 0 and hist[0].sum() == n * (n - 1) // 2
    h = nbins // 2
    for b in (h - 30, h, h + 45):
        degree = run(rows, (b - h) / h, 2, upto=1)["degree"]
        pairs = int(hist[0, b:].sum())
        assert 0 < pairs < n * (n - 1) // 2 and int(degree.sum()) == 2 * pairs, b


# ---------------------------------------------------------------------------------- 5. planted clusters
@pytest.mark.parametrize("case", PLANTED)
def test_planted_clusters_equal_the_fp64_reference(case):
    x, _, ref, report = planted_case(*case)
    rows = enrol(x)
    got = run(rows, case[3], case[4])
    print(f"planted {case}: {report} kinds={np.bincount(ref.kind, minlength=4).tolist()} clusters={ref.n_clusters}")
    same(got, ref, rows.cpu().numpy())


def test_two_runs_give_identical_bytes():
    case = PLANTED[0]
    rows = enrol(planted_case(*case)[0])
    a, b = run(rows, case[3], case[4]), run(rows, case[3], case[4])
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ---------------------------------------------------------------------------------- 6. other cases
def test_left_out_rows_take_part_in_nothing():
    x, valid, ref, _ = planted_case(*LEFT_OUT_CASE, with_valid=True)
    assert valid[-1] == 0 and np.array_equal(valid, left_out_valid(len(valid)))
    rows = enrol(x)
    got = run(rows, LEFT_OUT_CASE[3], LEFT_OUT_CASE[4], valid)
    same(got, ref, rows.cpu().numpy())
    assert (got["kind"][valid == 0] == LEFT_OUT).all() and (got["degree"][valid == 0] == 0).all()
    # nothing takes part at all
    got = run(rows, LEFT_OUT_CASE[3], 1, np.zeros(len(valid), dtype=np.uint8))
    assert int(got["n_clusters"][0]) == 0 and (got["kind"] == 0).all() and (got["root"] == -1).all()
    assert (got["cluster"] == -1).all() and (got["degree"] == 0).all() and (got["sizes"] == ISENT).all()


def test_a_nan_row_is_nobodys_neighbour():
    """NaN in row 5 and in the last row (which the padding of the last tile re-reads), +inf in row
    T: every score of these rows is NaN, so they are noise at min_samples >= 2."""
    n, D = T + 2, 96
    x = half_rows(n, D, 90)
    x[5, 3], x[n - 1, 0], x[T, 7] = np.nan, np.nan, np.inf
    with np.errstate(invalid="ignore"):
        s = (x.astype(np.float64) @ x.astype(np.float64).T).astype(np.float32)
    assert not np.isfinite(s[[5, n - 1, T]]).any()
    for thr, ms in ((0.25, 2), (0.75, 2), (-0.5, 2)):
        ref = dbscan_ref(s, None, thr, ms)
        assert (ref.kind[[5, n - 1, T]] == NOISE).all() and ref.n_clusters > 0
        same(run(torch.from_numpy(x).to(DEV), thr, ms), ref, x)


def test_a_wider_row_stride_changes_nothing():
    n, D = T + 1, 96
    x = half_rows(n, D, 91)
    wide = Guarded((n, D), stride=(D + 8, 1), fill=float("nan"))               # NaN between the rows and around them
    wide.view.copy_(torch.from_numpy(x))
    assert wide.view.stride(0) == D + 8 and wide.view.data_ptr() % 16 == 0
    ref = dbscan_ref(exact_scores(x), None, 0.75, 2)
    assert ref.n_clusters > 3 and set(ref.kind.tolist()) == {NOISE, CORE}
    same(run(wide.view, 0.75, 2), ref, x)
    # the rows are an input: nothing may have written them or the NaN around them. (NaN != NaN, so
    # ``Guarded.untouched`` cannot check a NaN fill: compare with isnan instead.)
    host = wide.buf.cpu()
    inside = torch.zeros(host.numel(), dtype=torch.bool)
    torch.as_strided(inside, wide.size, wide.stride, wide.start).fill_(True)
    assert torch.isnan(host[~inside]).all() and torch.equal(wide.cpu(), torch.from_numpy(x))


def test_max_clusters_below_the_number_of_clusters():
    case = PLANTED[0]
    x, _, ref, _ = planted_case(*case)
    rows = enrol(x)
    for max_clusters in (1, 7):
        assert ref.n_clusters > max_clusters
        got = run(rows, case[3], case[4], max_clusters=max_clusters)
        same(got, ref, rows.cpu().numpy(), max_clusters)
        assert got["cluster"].max() == ref.n_clusters - 1 and got["sizes"].shape == (max_clusters,)
    # more room than clusters: the rows past C keep the sentinel (``same`` compares them)
    same(run(rows, case[3], case[4], max_clusters=ref.n_clusters + 3), ref, rows.cpu().numpy(), ref.n_clusters + 3)


def test_refusals_launch_nothing_and_write_nothing():
    L = _lib.lib()
    n, D = 100, 512
    a = torch.zeros(n, D, device=DEV)
    out = Outs(n, D, n)
    real = dict(a=a.data_ptr(), degree=out.degree.view.data_ptr(), ws=out.ws.view.data_ptr(),
                root=out.root.view.data_ptr(), kind=out.kind.view.data_ptr(), cluster=out.cluster.view.data_ptr(),
                n_clusters=out.n_clusters.view.data_ptr(), sizes=out.sizes.view.data_ptr(),
                sums=out.sums.view.data_ptr(), centroids=out.centroids.view.data_ptr())
    for which, kw in cluster_refusals():
        args = dict(real)
        args.update({k: (v if k != "a" or v is None else a.data_ptr() + (v & 0xF)) for k, v in kw.items()})
        assert call_cluster(L, which, **args) == -22, (which, kw)
    torch.cuda.synchronize()
    assert out.still_sentinel() and (out.ws.cpu() == BSENT).all()
    deg, ws = out.degree.view, out.ws.view
    for bad in (lambda: ops.pair_degree(a.cpu(), 0.5, degree=deg), lambda: ops.pair_degree(a, float("nan"), degree=deg),
                lambda: ops.pair_degree(a, 0.5, degree=deg[:50]), lambda: ops.pair_degree(a[:, :500], 0.5, degree=deg),
                lambda: ops.pair_degree(a, 0.5, degree=deg, valid=torch.ones(n, device=DEV)),
                lambda: ops.pair_link(a, 0.5, 0, degree=deg, workspace=ws),
                lambda: ops.pair_link(a, 0.5, 2, degree=deg, workspace=ws[:-1]),
                lambda: ops.pair_link(a, 0.5, 2, degree=deg, workspace=out.ws.buf[8:8 + ws.numel()]),
                lambda: ops.cluster_finish(n, 2, degree=deg, workspace=ws, root=out.root.view, kind=out.kind.view,
                                           cluster=out.cluster.view.long(), n_clusters=out.n_clusters.view,
                                           sizes=out.sizes.view),
                lambda: ops.cluster_centroids(a, cluster=out.cluster.view, n_clusters=out.n_clusters.view,
                                              sums=out.sums.view[:, :64], centroids=out.centroids.view)):
        with pytest.raises(ValueError):
            bad()
    torch.cuda.synchronize()
    assert out.still_sentinel() and (out.ws.cpu() == BSENT).all()


# ---------------------------------------------------------------------------------- 7. public interface
def test_face_clusters_end_to_end_at_64_rows():
    n, D, thr, first = 64, 512, 0.6, 1000
    x = planted_rows(n, D, 95, identities=8, spread=0.5, bridges=0, outliers=2)
    fc = FaceClusters(dim=D, capacity=n, device=DEV)
    assert fc.add(x.to(DEV)) == (0, n) and len(fc) == n
    res = fc.cluster(thr, min_samples=3)
    rows = fc.store.rows[:n].cpu().numpy()
    C = int(res.n_clusters[0])
    cluster, sizes = res.cluster.cpu().numpy(), res.sizes.cpu().numpy()
    assert C == 8 and sizes[:C].sum() == (cluster >= 0).sum() == n - 2 and res.max_clusters == n
    want = sums_ref(rows, cluster, C)
    assert np.array_equal(res.sums.cpu().numpy()[:C], want)
    assert np.array_equal(res.centroids_raw.cpu().numpy()[:C].view(np.int32), centroids_ref(want).view(np.int32))
    assert torch.equal(res.centroids[:C], enrol(res.centroids_raw[:C].cpu()))
    gal = FaceGallery(dim=D, capacity=n, device=DEV)
    (r0, r1), labels = res.enrol_into(gal, first, min_size=1)
    assert (r0, r1) == (0, C) and labels == [first + c for c in range(C)] and len(gal) == C
    assert torch.equal(gal.rows[:C], res.centroids[:C]) and gal.labels[:C].tolist() == labels
    # what identify must answer, from the centroids on the host: the best centroid's label when its
    # score passes. The margins keep fp32 against fp64 from deciding anything
    s = rows.astype(np.float64) @ res.centroids[:C].cpu().numpy().astype(np.float64).T
    top = np.sort(s, axis=1)
    assert (np.abs(top[:, -1] - thr) > 1e-4).all() and (top[:, -1] - top[:, -2] > 1e-4).all()
    want_ident = np.where(top[:, -1] >= thr, first + s.argmax(axis=1), -1)
    ident, score = gal.identify(torch.from_numpy(rows).to(DEV), thr)
    assert np.array_equal(ident.cpu().numpy(), want_ident)
    member = cluster >= 0
    own = s[np.arange(n), np.maximum(cluster, 0)]
    passes = member & (own >= thr)
    assert passes.sum() >= n - 4 and (want_ident[passes] == first + cluster[passes]).all()
    with pytest.raises(ValueError, match="capacity"):
        res.enrol_into(FaceGallery(dim=D, capacity=C - 1, device=DEV), first)
    small = fc.cluster(thr, min_samples=3, max_clusters=3)
    with pytest.raises(ValueError, match="max_clusters"):
        small.enrol_into(gal, first + 100)
    assert len(gal) == C and int(small.n_clusters[0]) == C
    # a view of an enrolled gallery sees later removals
    ids = list(range(n))
    store = FaceGallery(dim=D, capacity=n, device=DEV)
    store.add(x.to(DEV), ids)
    view = FaceClusters.of_gallery(store)
    before = view.cluster(thr, min_samples=3)
    assert torch.equal(before.cluster, res.cluster) and torch.equal(before.sums, res.sums)
    gone = np.flatnonzero(cluster == 3)
    store.remove([ids[i] for i in gone])
    after = view.cluster(thr, min_samples=3)
    assert int(after.n_clusters[0]) == C - 1 and (after.kind.cpu().numpy()[gone] == LEFT_OUT).all()
    assert (after.cluster.cpu().numpy()[gone] == -1).all()
