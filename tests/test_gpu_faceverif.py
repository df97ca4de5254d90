"""GPU: 1:1 face verification (csrc/pairhist.hip) -- prpe_pair_hist, the all-pairs
score histogram, and ``FaceVerification`` / ``FaceIdentifier.calibrate`` above it -- against the
host restatements of tests/test_faceverif_host.py (``pair_hist_ref``, ``curve_ref``).

``hist`` and ``skipped`` live in sentinel-filled buffers with guards on both sides (``Guarded``,
tests/test_gpu_rowops.py); every launch is followed by a check that the guards are untouched.
T = ops.PAIR_HIST_TILE: the shapes sit on both sides of one and two tiles. At most nine tiles are
fewer than the CUs, so every workgroup here takes one tile: the walk of several tiles per workgroup
(4865 rows, cross 2049 x 5761, on 256 CUs) is tested in tests/test_gpu_pairs_walk.py.

* exact inputs (rows of four +-0.5: unit norm, every dot product a multiple of 0.25, exact in any
  order) must give the integer counts of fp64, in self and cross mode, at every nbins;
* random rows must give the histogram of the scores ``FaceGallery.search`` returns, bit for bit;
* against fp64 on random data every edge of both classes is bracketed with tol = 4 e_ref (e_ref as
  in tests/test_gpu_gallery.py: the fp32 CPU evaluation's largest distance from fp64);
* self(a) == self(a[:m]) + self(a[m:]) + cross(a[:m], a[m:]), accumulation, row strides, left-out
  rows, skipped pairs, refusals, and the public interface end to end at 64 x 64.

Measured on an MI355X: see DESIGN.md §5i.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from prpe import CombinedModel, FaceGallery, FaceIdentifier, FaceVerification, _lib, ops
from test_faceverif_host import (NBINS, call_pair_hist, curve_ref, pair_hist_ref, pair_hist_refusals, same_curve,
                                 thresholds_ref)
from test_gpu_rowops import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = ops.PAIR_HIST_TILE
ISENT = -7777


# ---------------------------------------------------------------------------------- harness
class Out:
    """Guarded, zeroed hist [2, nbins] and skipped [1]."""

    def __init__(self, nbins):
        self.hist = Guarded((2, nbins), fill=ISENT, dtype=torch.int64)
        self.skipped = Guarded((1,), fill=ISENT, dtype=torch.int64)
        self.hist.view.zero_()
        self.skipped.view.zero_()

    def host(self):
        assert self.hist.untouched() and self.skipped.untouched()
        return self.hist.cpu().numpy(), int(self.skipped.cpu()[0])


def _dev(t, dtype):
    return None if t is None else torch.as_tensor(np.asarray(t)).to(dtype).to(DEV)


def launch(out, nbins, a, la, b=None, lb=None, va=None, vb=None):
    ops.pair_hist(a, _dev(la, torch.int64), b, _dev(lb, torch.int64), nbins=nbins, hist=out.hist.view,
                  skipped=out.skipped.view, a_valid=_dev(va, torch.uint8), b_valid=_dev(vb, torch.uint8))


def pair_hist(nbins, a, la, b=None, lb=None, va=None, vb=None):
    out = Out(nbins)
    launch(out, nbins, a, la, b, lb, va, vb)
    return out.host()


def enrol(x):
    """Raw host rows -> normalised device rows, as a gallery stores them."""
    n, D = x.shape
    rows, norms = torch.empty(n, D, device=DEV), torch.empty(n, device=DEV)
    ops.gallery_enrol(x.to(DEV).contiguous(), rows, norms, 0)
    return rows


def half_rows(n, D, seed, zero_row=None):
    """Rows with four entries of +-0.5 among 24 seeded columns: the norm is exactly 1 and every dot
    product a multiple of 0.25."""
    g = np.random.default_rng(seed)
    pool = np.sort(g.permutation(D)[:24])
    x = np.zeros((n, D), dtype=np.float32)
    for i in range(n):
        x[i, g.choice(pool, 4, replace=False)] = g.choice([-0.5, 0.5], 4)
    if zero_row is not None and zero_row < n:
        x[zero_row] = 0
    return x


def exact_case(n, D, seed, zero_row=None):
    x = half_rows(n, D, seed, zero_row)
    rows = enrol(torch.from_numpy(x))
    assert torch.equal(rows.cpu(), torch.from_numpy(x))                        # enrol leaves unit rows unchanged
    labels = np.random.default_rng(seed + 1).integers(0, 5, n)
    return x, rows, labels


# ---------------------------------------------------------------------------------- 1. exact counts
SELF_N = [1, 2, 17, T - 1, T, T + 1, 2 * T + 1]
SELF_CASES = [(n, D, NBINS[(i + 2 * j) % 5]) for i, n in enumerate(SELF_N) for j, D in enumerate((32, 96, 512))]


@pytest.mark.parametrize("n,D,nbins", SELF_CASES)
def test_exact_inputs_give_the_integer_counts_self(n, D, nbins):
    x, rows, labels = exact_case(n, D, 1000 + n + D, zero_row=n // 2)
    s = (x.astype(np.float64) @ x.astype(np.float64).T).astype(np.float32)
    want, _ = pair_hist_ref(s, labels, labels, None, None, nbins, True)
    hist, skipped = pair_hist(nbins, rows, labels)
    assert skipped == 0 and hist.sum() == n * (n - 1) // 2
    assert np.array_equal(hist, want)
    if n > 2:
        assert hist[:, nbins // 2].sum() > 0                                   # the zero row scores 0: bin h


@pytest.mark.parametrize("m,n,D,nbins", [(1, 1, 32, 256), (17, 2 * T + 1, 512, 4096), (2 * T + 1, 17, 96, 512),
                                         (T + 1, T + 1, 512, 1024), (T + 1, T + 1, 32, 2048)])
def test_exact_inputs_give_the_integer_counts_cross(m, n, D, nbins):
    x, rows, labels = exact_case(m + n, D, 2000 + m + n + D, zero_row=m + n // 2)
    s = (x[:m].astype(np.float64) @ x[m:].astype(np.float64).T).astype(np.float32)
    want, _ = pair_hist_ref(s, labels[:m], labels[m:], None, None, nbins, False)
    hist, skipped = pair_hist(nbins, rows[:m], labels[:m], rows[m:], labels[m:])
    assert skipped == 0 and hist.sum() == m * n
    assert np.array_equal(hist, want)
    # the other way round: the transposed scores, the same histogram
    hist_t, _ = pair_hist(nbins, rows[m:], labels[m:], rows[:m], labels[:m])
    assert np.array_equal(hist_t, want)


# ---------------------------------------------------------------------------------- 2. the gallery's bits
def search_scores(q_raw, g_raw):
    """Every (query, row) fp32 score as ``FaceGallery.search`` returns it, from galleries of 8 rows
    searched with k = 8 and reassembled by row index."""
    Q, D = q_raw.shape
    n = g_raw.shape[0]
    s = torch.full((Q, n), float("nan"))
    for r0 in range(0, n, 8):
        gal = FaceGallery(dim=D, capacity=8, device=DEV)
        gal.add(g_raw[r0:r0 + 8].to(DEV), list(range(r0, min(r0 + 8, n))))
        sc, rows, _ = gal.search(q_raw.to(DEV), k=8)
        sc, rows = sc.cpu(), rows.cpu().long()
        k = min(8, n - r0)
        assert (rows[:, :k] >= 0).all() and (rows[:, k:] == -1).all()
        s[torch.arange(Q)[:, None].expand(Q, k), r0 + rows[:, :k]] = sc[:, :k]
    assert torch.isfinite(s).all()
    return s.numpy()


@pytest.mark.parametrize("D", [96, 512])
def test_score_bits_are_the_gallerys(D):
    g = torch.Generator().manual_seed(40 + D)
    n, m = 70, 37
    ids = torch.randint(0, 6, (n,), generator=g)
    centres = torch.randn(6, D, generator=g)
    x = centres[ids] + 0.8 * torch.randn(n, D, generator=g)
    y = centres[:m % 6 + 1].repeat(m, 1)[:m] + 0.8 * torch.randn(m, D, generator=g)
    ly = (torch.arange(m) % (m % 6 + 1)).numpy()
    rows, yrows = enrol(x), enrol(y)
    nbins = 4096                                                               # the finest bins: the most edges to cross
    want, _ = pair_hist_ref(search_scores(x, x), ids.numpy(), ids.numpy(), None, None, nbins, True)
    hist, skipped = pair_hist(nbins, rows, ids.numpy())
    assert skipped == 0 and np.array_equal(hist, want)
    want, _ = pair_hist_ref(search_scores(y, x), ly, ids.numpy(), None, None, nbins, False)
    hist, skipped = pair_hist(nbins, yrows, ly, rows, ids.numpy())
    assert skipped == 0 and np.array_equal(hist, want)


# ---------------------------------------------------------------------------------- 3. fp64, every edge
@functools.lru_cache(maxsize=None)
def random_case(n, D, seed, identities=40):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, identities, (n,), generator=g)
    x = torch.randn(identities, D, generator=g)[ids] + 0.7 * torch.randn(n, D, generator=g)
    return x, ids.numpy(), enrol(x)


def test_every_edge_is_bracketed_by_fp64_within_four_e_ref():
    n, D, nbins = 2 * T + 1, 512, 2048
    x, ids, rows = random_case(n, D, 77)
    s64 = (F.normalize(x.double(), dim=1) @ F.normalize(x.double(), dim=1).t()).numpy()
    s32 = (F.normalize(x, dim=1) @ F.normalize(x, dim=1).t()).numpy()
    e_ref = float(np.abs(s32.astype(np.float64) - s64).max())
    tol = 4 * e_ref
    hist, skipped = pair_hist(nbins, rows, ids)
    assert skipped == 0 and hist.sum() == n * (n - 1) // 2
    iu = np.triu_indices(n, 1)
    same = (ids[:, None] == ids[None, :])[iu]
    edges = thresholds_ref(nbins)[1:nbins]                                     # every finite edge, b = 1 .. nbins - 1
    worst = {}
    for cls, name in ((0, "genuine"), (1, "impostor")):
        v = np.sort(s64[iu][same if cls == 0 else ~same])
        assert hist[cls].sum() == v.size
        got = np.cumsum(hist[cls][::-1])[::-1][1:]                             # pairs in the bins >= b
        lo = v.size - np.searchsorted(v, edges + tol, side="left")             # fp64 scores >= edge + tol
        hi = v.size - np.searchsorted(v, edges - tol, side="left")             # fp64 scores >= edge - tol
        exact = v.size - np.searchsorted(v, edges, side="left")
        worst[name] = dict(pairs=int(v.size), margin=int(np.minimum(got - lo, hi - got).min()),
                           width=int((hi - lo).max()), off_fp64=int(np.abs(got - exact).max()),
                           edges_off=int((got != exact).sum()))
        assert (lo <= got).all() and (got <= hi).all(), name
    print(f"pair_hist fp64 bracket N={n} D={D} nbins={nbins}: e_ref={e_ref:.3e} tol={tol:.3e} {worst}")


# ---------------------------------------------------------------------------------- 4. decomposition
@pytest.mark.parametrize("m", [1, T, T + 1, 2 * T])
def test_self_is_the_two_parts_and_their_cross(m):
    n, D, nbins = 2 * T + 1, 96, 1024
    x, ids, rows = random_case(n, D, 78, identities=7)
    ids = ids.copy()
    ids[[0, T - 1, T, 2 * T]] = -1
    va = np.ones(n, dtype=np.uint8)
    va[[5, T + 1, 2 * T - 1]] = 0
    whole, _ = pair_hist(nbins, rows, ids, va=va)
    live = int(((ids >= 0) & (va != 0)).sum())
    assert whole.sum() == live * (live - 1) // 2
    out = Out(nbins)                                                           # the three parts added into one hist
    if m > 0:
        launch(out, nbins, rows[:m], ids[:m], va=va[:m])
    launch(out, nbins, rows[m:], ids[m:], va=va[m:])
    launch(out, nbins, rows[:m], ids[:m], rows[m:], ids[m:], va=va[:m], vb=va[m:])
    parts, skipped = out.host()
    assert skipped == 0 and np.array_equal(parts, whole)


# ---------------------------------------------------------------------------------- 5. accumulation, strides
def test_two_launches_add_and_a_wider_row_stride_changes_nothing():
    n, D, nbins = T + 1, 96, 512
    x, ids, rows = random_case(n, D, 79, identities=7)
    once, _ = pair_hist(nbins, rows, ids)
    out = Out(nbins)
    launch(out, nbins, rows, ids)
    launch(out, nbins, rows, ids)
    twice, skipped = out.host()
    assert skipped == 0 and np.array_equal(twice, 2 * once)
    wide = Guarded((n, D), stride=(D + 8, 1), fill=float("nan"))               # NaN between the rows and around them
    wide.view.copy_(rows)
    assert wide.view.stride(0) == D + 8 and wide.view.data_ptr() % 16 == 0
    got, skipped = pair_hist(nbins, wide.view, ids)
    assert skipped == 0 and np.array_equal(got, once)
    got, skipped = pair_hist(nbins, wide.view[:40], ids[:40], rows[40:], ids[40:])
    want, _ = pair_hist(nbins, rows[:40], ids[:40], wide.view[40:], ids[40:])
    assert skipped == 0 and np.array_equal(got, want)


# ---------------------------------------------------------------------------------- 6. left-out rows, skipped pairs
def test_left_out_rows_and_pairs_that_are_not_finite():
    m, n, D, nbins = T + 3, 2 * T + 1, 96, 256
    x = half_rows(m + n, D, 80)
    x[3, 5], x[T, 0] = np.nan, np.inf                                          # in a
    x[m + T - 1, 7], x[m + 2 * T, 1] = -np.inf, np.nan                         # in b
    rows = torch.from_numpy(x).to(DEV)
    la = np.random.default_rng(81).integers(0, 4, m)
    lb = np.random.default_rng(82).integers(0, 4, n)
    la[[0, T - 1, T + 2]] = -1
    lb[[T, 2 * T - 1]] = -5
    va, vb = np.ones(m, dtype=np.uint8), np.ones(n, dtype=np.uint8)
    va[[1, T + 1]] = 0
    vb[[0, T - 1, T + 1]] = 0                                                  # the -inf row of b is left out
    with np.errstate(invalid="ignore"):
        s = x[:m] @ x[m:].T
        s_self = x[m:] @ x[m:].T
    finite_rows = np.isfinite(x).all(axis=1)
    assert (np.isfinite(s) == (finite_rows[:m, None] & finite_rows[None, m:])).all()
    want, want_skipped = pair_hist_ref(s, la, lb, va, vb, nbins, False)
    hist, skipped = pair_hist(nbins, rows[:m], la, rows[m:], lb, va, vb)
    live_a, live_b = int(((la >= 0) & (va != 0)).sum()), int(((lb >= 0) & (vb != 0)).sum())
    assert want_skipped > 0 and skipped == want_skipped and np.array_equal(hist, want)
    assert hist.sum() + skipped == live_a * live_b
    want, want_skipped = pair_hist_ref(s_self, lb, lb, vb, vb, nbins, True)
    hist, skipped = pair_hist(nbins, rows[m:], lb, va=vb)
    assert want_skipped > 0 and skipped == want_skipped and np.array_equal(hist, want)
    assert hist.sum() + skipped == live_b * (live_b - 1) // 2
    # nothing takes part at all
    hist, skipped = pair_hist(nbins, rows[m:], np.full(n, -1))
    assert hist.sum() == 0 and skipped == 0


# ---------------------------------------------------------------------------------- 7. refusals
def test_refusals_launch_nothing_and_write_nothing():
    L = _lib.lib()
    a, la = torch.zeros(100, 512, device=DEV), torch.zeros(100, dtype=torch.int64, device=DEV)
    out = Out(2048)
    for kw in pair_hist_refusals():
        args = dict(a=a.data_ptr(), la=la.data_ptr(), hist=out.hist.view.data_ptr(), skipped=out.skipped.view.data_ptr())
        args.update(kw)
        assert call_pair_hist(L, **args) == -22, kw
    torch.cuda.synchronize()
    hist, skipped = out.host()
    assert hist.sum() == 0 and skipped == 0 and (hist == 0).all()
    h, s = torch.zeros(2, 2048, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    for bad in (dict(a=a.cpu()), dict(la=la.cpu()), dict(hist=h.cpu()), dict(skipped=s.cpu()), dict(nbins=100),
                dict(a=a[:, :500]), dict(la=la[:50]), dict(la=la.int()), dict(hist=h[:, :1024]),
                dict(b=a), dict(lb=la), dict(b=a.cpu(), lb=la), dict(vb=torch.ones(100, dtype=torch.uint8, device=DEV))):
        kw = dict(a=a, la=la, b=None, lb=None, vb=None, nbins=2048, hist=h, skipped=s)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.pair_hist(kw["a"], kw["la"], kw["b"], kw["lb"], nbins=kw["nbins"], hist=kw["hist"],
                          skipped=kw["skipped"], b_valid=kw["vb"])
    torch.cuda.synchronize()
    assert int(h.sum()) == 0 and int(s.sum()) == 0
    # M = 1 in self mode is legal and counts nothing
    hist, skipped = pair_hist(256, a[:1], [3])
    assert hist.sum() == 0 and skipped == 0


# ---------------------------------------------------------------------------------- 8. end to end
def test_face_verification_end_to_end_at_64x64(state_dict):
    model = CombinedModel(state_dict, device=DEV)
    model.set_task("pose_estimation")
    g = torch.Generator().manual_seed(31)
    x = torch.rand(8, 3, 64, 64, generator=g).to(DEV)
    labels = [2 ** 35, 2 ** 35, 2 ** 35, 7, 7, 7, 9, 9]
    fid = FaceIdentifier(model, FaceGallery(dim=512, capacity=8, device=DEV))
    ver = FaceVerification(dim=512, capacity=8, device=DEV)
    assert ver.add_frames(fid, x, labels) == (0, 8) and len(ver) == 8
    far = (0.5, 0.1, 0.01)
    out = ver.compute(far=far)
    assert (out["genuine"], out["impostor"], out["skipped"]) == (3 + 3 + 1, 28 - 7, 0)
    same_curve(out, curve_ref(out["hist"], far))
    hist_dev, _ = ver.histogram()
    assert np.array_equal(hist_dev.cpu().numpy(), out["hist"])
    # a gallery enrolled with the same frames: the same histogram through the view, also after a removal
    fid.enrol(x, labels)
    view = FaceVerification.of_gallery(fid.gallery)
    assert np.array_equal(view.compute(far=far)["hist"], out["hist"])
    # calibrate: the threshold's false accepts are the impostor pairs search scores at or above it
    assert fid.threshold == 0.3
    row = fid.calibrate(view, 0.1)
    assert fid.threshold == row["threshold"] and row == view.compute(far=(0.1,))["at_far"][0]
    sc, rows, lab = fid.gallery.search(fid.embed(x), k=8)
    sc, rows, lab = sc.cpu(), rows.cpu(), lab.cpu()
    mine = torch.tensor(labels)[:, None].expand(8, 8)
    upper = torch.arange(8)[:, None] < rows                                    # each pair once: i < j
    assert int(upper.sum()) == 28
    impostor = upper & (lab != mine)
    assert int((impostor & (sc >= row["threshold"])).sum()) == row["false_accepts"]
    assert int((upper & (lab == mine) & (sc >= row["threshold"])).sum()) == row["true_accepts"]
    fid.gallery.remove([7])
    after = view.compute(far=far)
    assert (after["genuine"], after["impostor"]) == (3 + 1, 6) and not np.array_equal(after["hist"], out["hist"])
    # cross mode against the gallery: every pair of a row here and a valid row there
    cross = ver.compute(against=fid.gallery)
    assert cross["genuine"] + cross["impostor"] == 8 * 5 and cross["genuine"] == 9 + 4
    # no genuine pairs: NaN rates, nothing raises
    lone = FaceVerification(dim=512, capacity=4, device=DEV)
    lone.add_frames(fid, x[:3], [1, 2, 3])
    res = lone.compute()
    assert res["genuine"] == 0 and res["impostor"] == 3 and np.isnan(res["eer"]) and np.isnan(res["roc"]["tar"]).all()
    assert all(np.isnan(r["tar"]) for r in res["at_far"])
    assert model.current_task == "pose_estimation"
