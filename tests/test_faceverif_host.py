"""CPU (no GPU): the host side of 1:1 face verification.

* ``pair_hist_ref`` and ``curve_ref``: numpy restatements of the rules in include/prpe.h and
  prpe/verification.py that the GPU tests (tests/test_gpu_faceverif.py) use as their yardstick,
  each pinned here to a second, plain statement in Python loops;
* the bin rule at its edges, which pairs count, hand-worked curves, and the equivalence the design
  rests on: FA[b] == #(score >= fp32 edge_b);
* the sizes, inputs and blocked reference of the multi-tile walk (tests/test_gpu_pairs_walk.py):
  three tiles per workgroup from the CU count, exact rows, labels of both classes in every tile;
* the ABI entry, every refusal of the header (the pointers below are never read), and
  ``FaceVerification`` / ``FaceIdentifier.calibrate`` bookkeeping with the ops call stubbed.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from prpe import _lib

NBINS = (256, 512, 1024, 2048, 4096)


# ---------------------------------------------------------------------------------- restatements
def bin_ref(s, nbins):
    """bin(s) = clamp((int)floorf(s * h) + h, 0, nbins - 1) on an fp32 array of finite scores."""
    h = nbins // 2
    with np.errstate(over="ignore"):                                          # a huge score clamps to an outer bin
        t = np.floor(np.asarray(s, dtype=np.float32) * np.float32(h))        # exact: h is a power of two
    return (np.clip(t, -h, h - 1).astype(np.int64) + h)


def pair_hist_ref(scores_fp32, la, lb, va, vb, nbins, self_mode):
    """(hist int64 [2, nbins], skipped): ``scores_fp32`` [M, N] binned by the stated rule. A row
    with label < 0 or valid byte 0 takes part in no pair; self mode takes i < j only; equal labels
    are genuine (row 0), others impostor (row 1); a score that is not finite is skipped."""
    s = np.asarray(scores_fp32, dtype=np.float32)
    la, lb = np.asarray(la, dtype=np.int64), np.asarray(lb, dtype=np.int64)
    ra = la >= 0 if va is None else (la >= 0) & (np.asarray(va) != 0)
    rb = lb >= 0 if vb is None else (lb >= 0) & (np.asarray(vb) != 0)
    on = ra[:, None] & rb[None, :]
    if self_mode:
        on &= np.arange(s.shape[0])[:, None] < np.arange(s.shape[1])[None, :]
    fin = np.isfinite(s)
    skipped = int((on & ~fin).sum())
    on &= fin
    same = la[:, None] == lb[None, :]
    b = bin_ref(np.where(fin, s, np.float32(0)), nbins)
    hist = np.zeros((2, nbins), dtype=np.int64)
    hist[0] = np.bincount(b[on & same], minlength=nbins)
    hist[1] = np.bincount(b[on & ~same], minlength=nbins)
    return hist, skipped


def thresholds_ref(nbins):
    h = nbins // 2
    return np.array([-np.inf] + [(b - h) / h for b in range(1, nbins)] + [np.inf])


def curve_ref(hist, far):
    """The curve rule of prpe/verification.py restated: suffix sums TA / FA over b = 0..nbins, the
    lowest b with FA[b] <= f * impostor per requested FAR, the EER at the smallest |FAR - FRR| and
    the best accuracy, lowest b on ties; NaN where a rate would divide by zero."""
    hist = np.asarray(hist, dtype=np.int64)
    nbins = hist.shape[1]
    TA = np.array([int(hist[0, b:].sum()) for b in range(nbins + 1)], dtype=np.int64)
    FA = np.array([int(hist[1, b:].sum()) for b in range(nbins + 1)], dtype=np.int64)
    G, I = int(TA[0]), int(FA[0])
    thr = thresholds_ref(nbins)
    tar = TA / G if G else np.full(nbins + 1, np.nan)
    fr = FA / I if I else np.full(nbins + 1, np.nan)
    out = {"genuine": G, "impostor": I, "thresholds": thr, "tar": tar, "far": fr, "at_far": []}
    for f in far:
        b = int(np.nonzero(FA <= float(f) * float(I))[0][0])
        out["at_far"].append({"far": float(f), "bin": b, "threshold": float(thr[b]), "tar": float(tar[b]),
                              "false_accepts": int(FA[b]), "true_accepts": int(TA[b])})
    out["eer"] = out["eer_threshold"] = out["best_accuracy"] = out["best_threshold"] = float("nan")
    if G and I:
        gap = np.abs(fr - (1 - tar))
        b = int(np.nonzero(gap == gap.min())[0][0])
        out["eer"], out["eer_threshold"] = float((fr[b] + 1 - tar[b]) / 2), float(thr[b])
    if G + I:
        ok = TA + I - FA
        b = int(np.nonzero(ok == ok.max())[0][0])
        out["best_accuracy"], out["best_threshold"] = float(ok[b] / (G + I)), float(thr[b])
    return out


def same_curve(got, want):
    """A ``verification_curve`` / ``compute`` dict against ``curve_ref``'s, exactly (NaN == NaN)."""
    assert got["genuine"] == want["genuine"] and got["impostor"] == want["impostor"]
    np.testing.assert_array_equal(got["roc"]["thresholds"], want["thresholds"])
    np.testing.assert_array_equal(got["roc"]["tar"], want["tar"])
    np.testing.assert_array_equal(got["roc"]["far"], want["far"])
    assert len(got["at_far"]) == len(want["at_far"])
    for g, w in zip(got["at_far"], want["at_far"]):
        for k in ("far", "bin", "threshold", "false_accepts", "true_accepts", "tar"):
            np.testing.assert_array_equal(g[k], w[k], err_msg=k)
    for k in ("eer", "eer_threshold", "best_accuracy", "best_threshold"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


# ---------------------------------------------------------------------------------- plain statements
def _bin_loop(s, nbins):
    h = nbins // 2
    return min(max(math.floor(float(s) * h) + h, 0), nbins - 1)              # float(s) * h is exact in fp64 too


def _pair_hist_loops(s, la, lb, va, vb, nbins, self_mode):
    hist = [[0] * nbins, [0] * nbins]
    skipped = 0
    for i in range(len(la)):
        if la[i] < 0 or (va is not None and not va[i]):
            continue
        for j in range(len(lb)):
            if lb[j] < 0 or (vb is not None and not vb[j]) or (self_mode and not i < j):
                continue
            v = float(s[i][j])
            if math.isnan(v) or math.isinf(v):
                skipped += 1
            else:
                hist[0 if la[i] == lb[j] else 1][_bin_loop(v, nbins)] += 1
    return np.array(hist, dtype=np.int64), skipped


def _curve_loops(hist, far):
    nbins = len(hist[0])
    h = nbins // 2
    TA, FA = [0] * (nbins + 1), [0] * (nbins + 1)
    for b in range(nbins - 1, -1, -1):
        TA[b], FA[b] = TA[b + 1] + int(hist[0][b]), FA[b + 1] + int(hist[1][b])
    G, I = TA[0], FA[0]
    nan = float("nan")

    def thr(b):
        return -math.inf if b == 0 else (math.inf if b == nbins else (b - h) / h)

    rows = []
    for f in far:
        b = 0
        while not FA[b] <= f * I:
            b += 1
        rows.append((b, thr(b), TA[b] / G if G else nan, FA[b], TA[b]))
    eer = eer_t = acc = acc_t = nan
    if G and I:
        best = None
        for b in range(nbins + 1):
            gap = abs(FA[b] / I - (1 - TA[b] / G))
            if best is None or gap < best:
                best, eer, eer_t = gap, (FA[b] / I + 1 - TA[b] / G) / 2, thr(b)
    if G + I:
        best = None
        for b in range(nbins + 1):
            ok = TA[b] + I - FA[b]
            if best is None or ok > best:
                best, acc, acc_t = ok, ok / (G + I), thr(b)
    return rows, eer, eer_t, acc, acc_t


def _check_curve_against_loops(hist, far):
    ref = curve_ref(hist, far)
    rows, eer, eer_t, acc, acc_t = _curve_loops(hist, far)
    for r, (b, t, tar, fa, ta) in zip(ref["at_far"], rows):
        np.testing.assert_array_equal([r["bin"], r["threshold"], r["tar"], r["false_accepts"], r["true_accepts"]],
                                      [b, t, tar, fa, ta])
    np.testing.assert_array_equal([ref["eer"], ref["eer_threshold"], ref["best_accuracy"], ref["best_threshold"]],
                                  [eer, eer_t, acc, acc_t])
    from prpe.verification import verification_curve
    same_curve(verification_curve(hist, far), ref)
    return ref


# ---------------------------------------------------------------------------------- the bin rule
@pytest.mark.parametrize("nbins", NBINS)
def test_bin_rule_at_its_edges(nbins):
    h = nbins // 2
    f32 = np.float32
    below = lambda v: np.nextafter(f32(v), f32(-2))
    edges = [b for b in (1, 2, h - 1, h, h + 1, nbins - 2, nbins - 1)]
    for b in edges:
        e = f32((b - h) / h)
        assert float(e) == (b - h) / h                                        # the edge is exact in fp32
        assert bin_ref([e], nbins)[0] == b and bin_ref([below(e)], nbins)[0] == b - 1
    cases = {-0.0: h, 0.0: h, -1e-30: h - 1, 1e-30: h, 1.0000001: nbins - 1, 1.0: nbins - 1, -1.0: 0,
             -1.0000001: 0, float(below(1.0)): nbins - 1, float(below(0.0)): h - 1, 3.0e38: nbins - 1,
             -3.0e38: 0}
    for s, want in cases.items():
        assert bin_ref([f32(s)], nbins)[0] == want, s
        assert _bin_loop(f32(s), nbins) == want, s
    g = np.random.default_rng(nbins)
    s = np.concatenate([g.uniform(-1.01, 1.01, 4000), g.normal(0, 1e-3, 1000)]).astype(f32)
    assert bin_ref(s, nbins).tolist() == [_bin_loop(v, nbins) for v in s]


def test_nan_and_infinities_are_skipped_and_land_in_no_bin():
    s = np.array([[0.5, np.nan, np.inf], [-np.inf, 0.25, -0.25]], dtype=np.float32)
    la, lb = [1, 2], [1, 2, 1]
    for nbins in NBINS:
        hist, skipped = pair_hist_ref(s, la, lb, None, None, nbins, False)
        loops = _pair_hist_loops(s, la, lb, None, None, nbins, False)
        assert skipped == 3 == loops[1] and hist.sum() == 3 and np.array_equal(hist, loops[0])
        h = nbins // 2
        assert hist[0, h + h // 2] == 1 and hist[0, h + h // 4] == 1 and hist[1, h - h // 4] == 1


# ---------------------------------------------------------------------------------- which pairs count
def test_negative_labels_valid_bytes_and_the_upper_triangle():
    g = np.random.default_rng(5)
    n = 23
    s = g.uniform(-1, 1, (n, n)).astype(np.float32)
    s = np.triu(s) + np.triu(s, 1).T                                          # symmetric, as the kernel's scores are
    la = g.integers(0, 4, n)
    la[[0, 7, 22]] = -1
    la[3] = -(2 ** 40)
    va = np.ones(n, dtype=np.uint8)
    va[[1, 7, 21]] = 0
    hist, skipped = pair_hist_ref(s, la, la, va, va, 256, True)
    loops = _pair_hist_loops(s, la, la, va, va, 256, True)
    live = n - 6                                                              # row 7 is left out twice
    assert skipped == 0 and np.array_equal(hist, loops[0]) and hist.sum() == live * (live - 1) // 2
    # cross mode over the same rows takes every ordered pair, the diagonal included
    hist2, _ = pair_hist_ref(s, la, la, va, va, 256, False)
    assert np.array_equal(hist2, _pair_hist_loops(s, la, la, va, va, 256, False)[0]) and hist2.sum() == live * live
    diag = np.zeros((2, 256), dtype=np.int64)
    for i in range(n):
        if la[i] >= 0 and va[i]:
            diag[0, bin_ref([s[i, i]], 256)[0]] += 1
    assert np.array_equal(hist2, 2 * hist + diag)
    # without valid bytes only the labels decide; a rectangular cross case
    m = 9
    lb = g.integers(-1, 3, m)
    hist3, _ = pair_hist_ref(s[:, :m], la, lb, None, va[:m], 512, False)
    assert np.array_equal(hist3, _pair_hist_loops(s[:, :m], la, lb, None, va[:m], 512, False)[0])
    assert hist3.sum() == (la >= 0).sum() * ((lb >= 0) & (va[:m] != 0)).sum()


# ---------------------------------------------------------------------------------- the curve
def _hist(nbins, genuine, impostor):
    h = np.zeros((2, nbins), dtype=np.int64)
    for b, c in genuine.items():
        h[0, b] = c
    for b, c in impostor.items():
        h[1, b] = c
    return h


def test_curve_hand_worked():
    # 256 bins, h = 128. Genuine: 6 pairs in bin 200, 4 in bin 140. Impostor: 90 in bin 120, 9 in
    # bin 140, 1 in bin 255 (the top bin)
    hist = _hist(256, {200: 6, 140: 4}, {120: 90, 140: 9, 255: 1})
    ref = _check_curve_against_loops(hist, (1.0, 0.1, 0.05, 0.01, 0.001))
    assert (ref["genuine"], ref["impostor"]) == (10, 100)
    r = ref["at_far"]
    assert (r[0]["bin"], r[0]["threshold"], r[0]["tar"], r[0]["false_accepts"]) == (0, -np.inf, 1.0, 100)   # met at b = 0
    assert (r[1]["bin"], r[1]["threshold"], r[1]["false_accepts"], r[1]["true_accepts"]) == (121, -7 / 128, 10, 10)
    assert (r[2]["bin"], r[2]["threshold"], r[2]["false_accepts"], r[2]["true_accepts"]) == (141, 13 / 128, 1, 6)
    assert (r[3]["bin"], r[3]["false_accepts"], r[3]["tar"]) == (141, 1, 0.6)
    # 0.001 x 100 = 0.1 < 1: only the edge past the top bin meets it; nothing is accepted there
    assert (r[4]["bin"], r[4]["threshold"], r[4]["false_accepts"], r[4]["true_accepts"], r[4]["tar"]) == \
        (256, np.inf, 0, 0, 0.0)
    # accuracy: b in 121..140 gives 10 + 90 = 100 of 110; b = 141 gives 6 + 99 = 105
    assert ref["best_accuracy"] == 105 / 110 and ref["best_threshold"] == 13 / 128
    # |FAR - FRR|: b = 121..140 -> |0.1 - 0| = 0.1; b = 141..200 -> |0.01 - 0.4| = 0.39: EER 0.05 at b = 121
    assert ref["eer"] == pytest.approx(0.05) and ref["eer_threshold"] == -7 / 128


def test_curve_ties_take_the_lowest_bin():
    # perfectly separated: every b in 101..150 has FAR = FRR = 0 and accuracy 1 -> b = 101
    hist = _hist(256, {150: 5}, {100: 7})
    ref = _check_curve_against_loops(hist, (0.5, 0.0))
    assert ref["eer"] == 0.0 and ref["eer_threshold"] == (101 - 128) / 128
    assert ref["best_accuracy"] == 1.0 and ref["best_threshold"] == (101 - 128) / 128
    assert [r["bin"] for r in ref["at_far"]] == [101, 101]
    # a symmetric overlap: b = 129 and b = 130 both give FAR = FRR = 0.5 -> the lower one; every b
    # classifies 2 of the 4 pairs correctly -> b = 0
    hist = _hist(256, {128: 1, 130: 1}, {128: 1, 130: 1})
    ref = _check_curve_against_loops(hist, (0.5,))
    assert ref["eer"] == 0.5 and ref["eer_threshold"] == 1 / 128 and ref["best_accuracy"] == 0.5
    assert ref["best_threshold"] == -np.inf and ref["at_far"][0]["bin"] == 129


def test_curve_without_genuine_or_without_impostor_pairs_gives_nan_and_does_not_raise():
    no_gen = _check_curve_against_loops(_hist(512, {}, {10: 3, 300: 1}), (0.5, 0.1))
    assert no_gen["genuine"] == 0 and np.isnan(no_gen["tar"]).all() and np.isnan(no_gen["eer"])
    assert np.isnan(no_gen["at_far"][0]["tar"]) and no_gen["at_far"][0]["false_accepts"] == 1
    assert no_gen["at_far"][1]["bin"] == 301 and no_gen["best_accuracy"] == 1.0
    no_imp = _check_curve_against_loops(_hist(512, {10: 3}, {}), (0.5,))
    assert no_imp["impostor"] == 0 and np.isnan(no_imp["far"]).all() and np.isnan(no_imp["eer"])
    assert no_imp["at_far"][0]["bin"] == 0 and no_imp["at_far"][0]["tar"] == 1.0 and no_imp["best_accuracy"] == 1.0
    empty = _check_curve_against_loops(_hist(256, {}, {}), (0.1,))
    assert np.isnan(empty["best_accuracy"]) and np.isnan(empty["at_far"][0]["tar"])


@pytest.mark.parametrize("nbins", NBINS)
def test_false_accepts_at_an_edge_are_the_scores_at_or_above_it(nbins):
    """FA[b] == #(score >= fp32 edge_b): what lets a histogram stand for identify's threshold."""
    g = np.random.default_rng(100 + nbins)
    s = np.concatenate([g.normal(0, 0.05, 30000), g.uniform(-1.001, 1.001, 8000), [1.0, -1.0, 0.0, -0.0, 1.0000001],
                        (np.arange(-6, 7) / (nbins // 2))]).astype(np.float32)[None, :]
    hist, skipped = pair_hist_ref(s, [0], np.ones(s.shape[1], dtype=np.int64), None, None, nbins, False)
    assert skipped == 0 and hist[0].sum() == 0 and hist[1].sum() == s.shape[1]
    thr = thresholds_ref(nbins)
    FA = np.concatenate([np.cumsum(hist[1][::-1])[::-1], [0]])
    for b in range(nbins + 1):
        assert FA[b] == int((s >= np.float32(thr[b])).sum()), b
    _check_curve_against_loops(hist, (1e-1, 1e-2, 1e-3, 1e-4))


# ---------------------------------------------------------------------------------- the tile walk
# Sizes and inputs of tests/test_gpu_pairs_walk.py: prpe_pair_hist's grid is min(tiles, CUs) workgroups,
# each walking the 128 x 128 score tiles id, id + grid, ..; these are the sizes at which every
# workgroup walks at least three.
TILE = 128


def walk_sizes(cus):
    """(tile rows tn, rows n) of the self-mode walk on a device of ``cus`` compute units: the
    smallest tn whose triangle tn (tn + 1) / 2 holds 3 tiles per workgroup, and n = (tn - 1) T + 1,
    so that the last tile row holds one row and is padded."""
    tn = 1
    while tn * (tn + 1) // 2 < 3 * cus:
        tn += 1
    return tn, (tn - 1) * TILE + 1


def walk_sizes_cross(cus):
    """(tm, tn, M, N) of the cross-mode walk: tm about sqrt(3 cus / 2.75) (17 at 256 CUs), tn the
    smallest with tm tn >= 3 cus and tn != tm; M and N one row past a tile multiple."""
    tm = max(2, math.ceil(math.sqrt(3 * cus / 2.75)))
    tn = -(-3 * cus // tm)
    if tn == tm:
        tn += 1
    return tm, tn, (tm - 1) * TILE + 1, (tn - 1) * TILE + 1


def tiles_of(m, n=None):
    """Score tiles prpe_pair_hist walks: the upper triangle of m rows, or the m x n rectangle."""
    tm = -(-m // TILE)
    return tm * (tm + 1) // 2 if n is None else tm * -(-n // TILE)


def four_halves(n, D, seed, pool=24):
    """Rows with four entries of +-0.5 among ``pool`` seeded columns: the norm is exactly 1 and
    every dot product a multiple of 0.25, equal in any arithmetic (float32 included)."""
    g = np.random.default_rng(seed)
    cols = np.sort(g.permutation(D)[:pool])
    x = np.zeros((n, D), dtype=np.float32)
    for i in range(n):
        x[i, g.choice(cols, 4, replace=False)] = g.choice([-0.5, 0.5], 4)
    return x


def walk_labels(n, seed, classes=4):
    """(labels, valid) for n rows: a seeded label of ``classes`` per row, so that genuine and
    impostor pairs meet in every tile; label -1 at a few seeded rows and at one tile border; valid
    bytes 0 on both sides of the first, a middle and the last tile border, at row 5 and at the
    last row (which is the padded tile row's only row when n = k T + 1)."""
    g = np.random.default_rng(seed)
    labels = g.integers(0, classes, n).astype(np.int64)
    labels[g.choice(n, min(7, n), replace=False)] = -1
    valid = np.ones(n, dtype=np.uint8)
    if n > 2 * TILE:
        labels[2 * TILE - 1] = -1
        last = (n - 1) // TILE * TILE
        mid = (n // TILE // 2) * TILE
        valid[[TILE - 1, TILE, mid - 1, mid, last - 1, last]] = 0
    valid[[min(5, n - 1), n - 1]] = 0
    return labels, valid


def pair_hist_ref_blocks(a, b, la, lb, va, vb, nbins, block=1024):
    """``pair_hist_ref`` for several ``nbins`` at once without the whole score matrix: fp32 scores
    a[r0:r1] @ b.T of ``block`` rows at a time (exact for ``four_halves`` rows; a row with a NaN
    makes every score of it NaN, as on the device), b None for self mode (pairs i < j).
    Returns {nbins: hist}, skipped."""
    self_mode = b is None
    if self_mode:
        b, lb, vb = a, la, va
    la, lb = np.asarray(la, dtype=np.int64), np.asarray(lb, dtype=np.int64)
    ra = la >= 0 if va is None else (la >= 0) & (np.asarray(va) != 0)
    rb = lb >= 0 if vb is None else (lb >= 0) & (np.asarray(vb) != 0)
    hists = {nb: np.zeros((2, nb), dtype=np.int64) for nb in nbins}
    skipped = 0
    cols = np.arange(b.shape[0])
    for r0 in range(0, a.shape[0], block):
        r1 = min(r0 + block, a.shape[0])
        with np.errstate(invalid="ignore"):
            s = a[r0:r1] @ b.T
        on = ra[r0:r1, None] & rb[None, :]
        if self_mode:
            on &= np.arange(r0, r1)[:, None] < cols[None, :]
        fin = np.isfinite(s)
        skipped += int((on & ~fin).sum())
        on &= fin
        same = la[r0:r1, None] == lb[None, :]
        gen, imp = s[on & same], s[on & ~same]
        for nb in nbins:
            hists[nb][0] += np.bincount(bin_ref(gen, nb), minlength=nb)
            hists[nb][1] += np.bincount(bin_ref(imp, nb), minlength=nb)
    return hists, skipped


def test_walk_sizes_give_three_tiles_per_workgroup():
    assert walk_sizes(256) == (39, 4865) and tiles_of(4865) == 780
    assert walk_sizes_cross(256) == (17, 46, 2049, 5761) and tiles_of(2049, 5761) == 782
    for cus in (1, 8, 64, 80, 104, 120, 228, 256, 304):
        tn, n = walk_sizes(cus)
        assert tiles_of(n) >= 3 * cus > (tn - 1) * tn // 2 and n % TILE == 1 and -(-n // TILE) == tn
        tm, tc, M, N = walk_sizes_cross(cus)
        assert tiles_of(M, N) == tm * tc >= 3 * cus and M != N and M % TILE == 1 and N % TILE == 1


def test_walk_inputs_are_exact_and_both_classes_meet_in_every_full_tile():
    """The multi-tile inputs: fp32 scores of ``four_halves`` rows equal the fp64 ones; with
    ``walk_labels`` every tile of full tile rows holds genuine and impostor pairs that count, the
    padded tile row holds none (its one row is left out), and both borders of three tiles are
    left out."""
    tn, n = walk_sizes(256)
    x = four_halves(n, 32, 4100)
    s = x[:700] @ x.T
    assert np.array_equal(s, (x[:700].astype(np.float64) @ x.astype(np.float64).T).astype(np.float32))
    assert np.array_equal(np.unique(s * 4), np.arange(-4, 5))
    assert ((x * x).sum(axis=1) == 1).all()
    labels, valid = walk_labels(n, 4101)
    on = (labels >= 0) & (valid != 0)
    assert valid[n - 1] == 0 and not valid[[127, 128, 19 * 128 - 1, 19 * 128, n - 2]].any() and (labels < 0).sum() >= 8
    for t in range(tn - 1):
        tile = labels[t * TILE:(t + 1) * TILE][on[t * TILE:(t + 1) * TILE]]
        assert set(tile.tolist()) == {0, 1, 2, 3} and (np.bincount(tile) >= 2).all()
    assert not on[(tn - 1) * TILE:].any()


def test_blocked_reference_is_pair_hist_ref():
    g = np.random.default_rng(77)
    n, m = 301, 140
    x = four_halves(n + m, 32, 78)
    x[[3, 130, n - 1], 0] = np.nan
    x[n + 7, 5] = np.inf
    la, va = walk_labels(n, 79)
    lb, vb = g.integers(-1, 3, m), (g.random(m) > 0.1).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        s_self, s_cross = x[:n] @ x[:n].T, x[:n] @ x[n:].T
    for valid in (None, va):
        got, skipped = pair_hist_ref_blocks(x[:n], None, la, None, valid, None, (256, 4096), block=64)
        for nbins in (256, 4096):
            want, want_skipped = pair_hist_ref(s_self, la, la, valid, valid, nbins, True)
            assert np.array_equal(got[nbins], want) and skipped == want_skipped > 0
    got, skipped = pair_hist_ref_blocks(x[:n], x[n:], la, lb, va, vb, (512,), block=100)
    want, want_skipped = pair_hist_ref(s_cross, la, lb, va, vb, 512, False)
    assert np.array_equal(got[512], want) and skipped == want_skipped > 0


# ---------------------------------------------------------------------------------- ABI and refusals
def test_abi_table_has_the_pair_hist_entry_point():
    header = open(os.path.join(ROOT, "include", "prpe.h")).read()
    assert int(re.search(r"#define PRPE_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 12
    decl = re.search(r"\bint prpe_pair_hist\s*\(([^;]*)\);", header)
    assert decl and len(decl.group(1).split(",")) == 15 == len(_lib.SIGNATURES["prpe_pair_hist"][1])
    assert hasattr(_lib.lib(), "prpe_pair_hist")


def pair_hist_refusals():
    """Every -EINVAL case of the header as keyword overrides of ``call_pair_hist``."""
    self_mode = [dict(a=None), dict(la=None), dict(hist=None), dict(skipped=None), dict(lb=0x7000), dict(vb=0x8000),
                 dict(M=0), dict(M=-1), dict(M=2 ** 24 + 1), dict(D=0), dict(D=48), dict(D=16), dict(D=544),
                 dict(nbins=0), dict(nbins=128), dict(nbins=300), dict(nbins=8192), dict(nbins=-256), dict(lda=508),
                 dict(lda=514), dict(a=0x1008)]
    cross = [dict(b=0x2000), dict(b=0x2000, lb=0x7000, N=0), dict(b=0x2000, lb=0x7000, N=2 ** 24 + 1),
             dict(b=0x2000, lb=0x7000, ldb=508), dict(b=0x2000, lb=0x7000, ldb=513), dict(b=0x2004, lb=0x7000),
             dict(b=0x2000, vb=0x8000)]
    return self_mode + cross


def call_pair_hist(L, a=0x1000, lda=512, M=100, la=0x5000, va=None, b=None, ldb=512, N=50, lb=None, vb=None, D=512,
                   nbins=2048, hist=0x10000, skipped=0x20000):
    return L.prpe_pair_hist(a, lda, M, la, va, b, ldb, N, lb, vb, D, nbins, hist, skipped, None)


def test_library_rejects_bad_pair_hist_arguments_before_launch():
    L = _lib.lib()
    for kw in pair_hist_refusals():
        assert call_pair_hist(L, **kw) == -22, kw


# ---------------------------------------------------------------------------------- FaceVerification
def test_face_verification_bookkeeping_with_the_kernel_stubbed(monkeypatch):
    import prpe
    from prpe import gallery as gmod
    from prpe import verification as vmod
    assert "FaceVerification" in prpe.__all__
    calls = []

    def pair_hist(a, a_labels, b=None, b_labels=None, *, nbins, hist, skipped, a_valid=None, b_valid=None):
        calls.append((tuple(a.shape), None if b is None else tuple(b.shape), nbins, a_valid is not None,
                      b_valid is not None))
        hist[0, nbins // 2 + 40] += 3
        hist[1, nbins // 2 - 2] += 99
        hist[1, nbins // 2 + 41] += 1
        skipped += 2

    monkeypatch.setattr(vmod.ops, "pair_hist", pair_hist)
    monkeypatch.setattr(gmod.ops, "gallery_enrol", lambda x, gallery, norms, row0=0: None)
    monkeypatch.setattr(prpe.FaceGallery, "_embeddings", lambda self, what, e: e.float().contiguous())
    v = prpe.FaceVerification(dim=64, capacity=8, device="cpu")
    with pytest.raises(ValueError, match="no rows"):
        v.histogram()
    assert v.add(torch.ones(5, 64), [1, 1, 2, 2, 3]) == (0, 5) and len(v) == 5
    with pytest.raises(ValueError, match="capacity"):
        v.add(torch.ones(4, 64), [1, 2, 3, 4])
    gal = prpe.FaceGallery(dim=64, capacity=4, device="cpu")
    gal.add(torch.ones(3, 64), [1, 2, 3])
    view = prpe.FaceVerification.of_gallery(gal)
    assert view.store is gal and len(view) == 3
    out = v.compute(nbins=256, far=(0.5, 0.005), against=view)
    assert calls == [((5, 64), (3, 64), 256, True, True)]
    assert (out["genuine"], out["impostor"], out["skipped"]) == (3, 100, 2)
    same_curve(out, curve_ref(out["hist"], (0.5, 0.005)))
    with pytest.raises(ValueError, match="dim"):
        v.histogram(against=prpe.FaceGallery(dim=32, capacity=2, device="cpu"))
    # calibrate: the threshold of the row, the default left alone until then
    fid = prpe.FaceIdentifier(model=None, gallery=prpe.FaceGallery(dim=512, capacity=1, device="cpu"))
    assert fid.threshold == 0.3
    row = fid.calibrate(v, 0.01)
    assert calls[-1] == ((5, 64), None, 2048, True, False)
    assert row["false_accepts"] == 1 and row["threshold"] == fid.threshold == -1 / 1024
    assert row["true_accepts"] == 3 and row["tar"] == 1.0
