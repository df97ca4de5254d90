"""CPU (no GPU): the host side of the open-set 1:N identification evaluation.

* ``ident_eval_ref``: a plain restatement of include/prpe.h in Python loops over probes and rows
  on float32 scalars, with the 64-bit key order; ``ident_eval_sorted``: a second statement, written
  apart, through an fp64 score matrix and a sort per probe (no keys, no floor: bins by counting
  edges). The two must agree on every case the GPU tests (tests/test_gpu_identeval.py) use;
  ``ident_eval_blocks`` is the vectorised form for the sizes at which a workgroup walks several
  tiles, pinned here to the loops;
* the key packing at its edges, ``identification_curve`` on hand-worked histograms, the inputs of
  the GPU tests with the conditions that let them assert equalities (ties, margins), the ABI
  entries, every refusal of the header (the pointers below are never read), and
  ``IdentificationEval`` / ``FaceIdentifier.calibrate_fpir`` bookkeeping with the ops stubbed.
"""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from prpe import _lib
from prpe.identification import identification_curve
from test_faceverif_host import bin_ref, four_halves, thresholds_ref, walk_labels, walk_sizes, walk_sizes_cross

R = 64
FIELDS = ("mate_key", "non_key", "mate_score", "mate_row", "non_score", "non_row", "rank_minus_1", "rank", "hist",
          "rank_hist", "counts", "skipped")


# ---------------------------------------------------------------------------------- the key
def image_ref(s):
    """The order-preserving uint32 image of a finite float32: -0 becomes +0, then the sign flip."""
    s = np.float32(s)
    if s == 0:
        s = np.float32(0.0)
    u = int(s.view(np.uint32))
    return u ^ (0xFFFFFFFF if u >> 31 else 0x80000000)


def key_ref(s, row):
    return image_ref(s) << 32 | (0xFFFFFFFF - int(row))


def unkey(k):
    """(score float32, row) of a key; (-inf, -1) for 0."""
    if not k:
        return np.float32(-np.inf), -1
    img = int(k) >> 32
    u = img ^ (0x80000000 if img >> 31 else 0xFFFFFFFF)
    return np.array([u], dtype=np.uint32).view(np.float32)[0], 0xFFFFFFFF - (int(k) & 0xFFFFFFFF)


def _bin(s, nbins):
    return int(bin_ref([s], nbins)[0])


def _finish_ref(probe, mk, nk, rm1, nbins):
    """prpe_ident_finish restated over host lists."""
    M = len(probe)
    out = {"mate_key": np.array(mk, dtype=np.uint64), "non_key": np.array(nk, dtype=np.uint64),
           "mate_score": np.empty(M, np.float32), "non_score": np.empty(M, np.float32),
           "mate_row": np.empty(M, np.int32), "non_row": np.empty(M, np.int32),
           "rank_minus_1": np.array(rm1, dtype=np.int32), "rank": np.zeros(M, np.int32),
           "hist": np.zeros((3, nbins), np.int64), "rank_hist": np.zeros(R + 1, np.int64), "counts": np.zeros(4, np.int64)}
    for i in range(M):
        (ms, mr), (ns, nr) = unkey(mk[i]), unkey(nk[i])
        out["mate_score"][i], out["mate_row"][i], out["non_score"][i], out["non_row"][i] = ms, mr, ns, nr
        if not probe[i]:
            out["counts"][2] += 1
        elif mk[i]:
            rank = rm1[i] + 1
            out["rank"][i] = rank
            out["counts"][0] += 1
            if mk[i] > nk[i]:
                out["hist"][0, _bin(ms, nbins)] += 1
            else:
                out["hist"][1, _bin(ns, nbins)] += 1
            out["rank_hist"][min(rank, R + 1) - 1] += 1
        else:
            out["counts"][1] += 1
            if nk[i]:
                out["hist"][2, _bin(ns, nbins)] += 1
            else:
                out["counts"][3] += 1
    return out


def ident_eval_ref(s, la, lb, va, vb, nbins, self_mode=False, b_row0=0):
    """include/prpe.h in loops: ``s`` [M, N] float32 scores (self mode: of the set against itself,
    the diagonal is left out here). Returns every output of the three stages as host arrays."""
    s = np.asarray(s, dtype=np.float32)
    M, N = s.shape
    if self_mode:
        lb, vb = la, va
    mk, nk, rm1, probe, skipped = [0] * M, [0] * M, [0] * M, [False] * M, 0
    for i in range(M):
        probe[i] = bool(la[i] >= 0 and (va is None or va[i]))
        if not probe[i]:
            continue
        others = []
        for j in range(N):
            if (self_mode and i == j) or (vb is not None and not vb[j]):
                continue
            v = s[i, j]
            if not math.isfinite(v):
                skipped += 1
                continue
            k = key_ref(v, b_row0 + j)
            if lb[j] == la[i]:
                mk[i] = max(mk[i], k)
            else:
                nk[i] = max(nk[i], k)
                others.append(k)
        if mk[i]:
            rm1[i] = sum(k > mk[i] for k in others)
    out = _finish_ref(probe, mk, nk, rm1, nbins)
    out["skipped"] = skipped
    return out


def ident_eval_sorted(s64, la, lb, va, vb, nbins, self_mode=False):
    """The second statement: fp64 scores, the candidates of a probe sorted by (score descending,
    row ascending), the first mate's position as the rank, and a bin as the number of finite edges
    at or below the score. Returns mate_row, non_row, mate_score, non_score (fp64), rank, hist,
    rank_hist, counts, skipped."""
    s64 = np.asarray(s64, dtype=np.float64)
    la = np.asarray(la, dtype=np.int64)
    M, N = s64.shape
    if self_mode:
        lb, vb = la, va
    lb = np.asarray(lb, dtype=np.int64)
    edges = thresholds_ref(nbins)[1:nbins]
    live_b = np.ones(N, dtype=bool) if vb is None else np.asarray(vb) != 0
    out = {"mate_row": np.full(M, -1), "non_row": np.full(M, -1), "mate_score": np.full(M, -np.inf),
           "non_score": np.full(M, -np.inf), "rank": np.zeros(M, np.int64), "hist": np.zeros((3, nbins), np.int64),
           "rank_hist": np.zeros(R + 1, np.int64), "counts": np.zeros(4, np.int64), "skipped": 0}
    which = lambda v: int(np.searchsorted(edges, v, side="right"))
    for i in range(M):
        if la[i] < 0 or (va is not None and not va[i]):
            out["counts"][2] += 1
            continue
        take = live_b.copy()
        if self_mode:
            take[i] = False
        fin = np.isfinite(s64[i])
        out["skipped"] += int((take & ~fin).sum())
        cols = np.flatnonzero(take & fin)
        order = cols[np.lexsort((cols, -s64[i, cols]))]
        mate = lb[order] == la[i]
        first_mate, first_non = np.flatnonzero(mate)[:1], np.flatnonzero(~mate)[:1]
        if first_non.size:
            out["non_row"][i], out["non_score"][i] = order[first_non[0]], s64[i, order[first_non[0]]]
        if first_mate.size:
            p = int(first_mate[0])
            out["mate_row"][i], out["mate_score"][i], out["rank"][i] = order[p], s64[i, order[p]], p + 1
            out["counts"][0] += 1
            out["rank_hist"][min(p, R)] += 1
            if p == 0:
                out["hist"][0, which(out["mate_score"][i])] += 1
            else:
                out["hist"][1, which(out["non_score"][i])] += 1
        else:
            out["counts"][1] += 1
            if first_non.size:
                out["hist"][2, which(out["non_score"][i])] += 1
            else:
                out["counts"][3] += 1
    return out


def agree(ref, srt):
    """``ident_eval_ref``'s dict against ``ident_eval_sorted``'s on scores that are exact in fp32."""
    for k in ("mate_row", "non_row", "rank", "hist", "rank_hist", "counts"):
        np.testing.assert_array_equal(ref[k], srt[k], err_msg=k)
    for k in ("mate_score", "non_score"):
        np.testing.assert_array_equal(ref[k].astype(np.float64), srt[k], err_msg=k)
    assert ref["skipped"] == srt["skipped"]


def images(s):
    """``image_ref`` on a float32 array of finite scores, as uint64."""
    u = (np.asarray(s, dtype=np.float32) + np.float32(0)).view(np.uint32).astype(np.uint64)   # -0 + 0 = +0
    return np.where(u >> np.uint64(31), u ^ np.uint64(0xFFFFFFFF), u ^ np.uint64(0x80000000))


def ident_eval_blocks(a, b, la, lb, va, vb, nbins, block=512):
    """``ident_eval_ref`` without the whole score matrix and without Python loops over pairs: fp32
    scores a[r0:r1] @ b.T of ``block`` probes at a time (exact for ``four_halves`` rows), keys as
    uint64 arrays. b None: self mode."""
    self_mode = b is None
    if self_mode:
        b, lb, vb = a, la, va
    la, lb = np.asarray(la, dtype=np.int64), np.asarray(lb, dtype=np.int64)
    M, N = a.shape[0], b.shape[0]
    probe = la >= 0 if va is None else (la >= 0) & (np.asarray(va) != 0)
    cand = np.ones(N, dtype=bool) if vb is None else np.asarray(vb) != 0
    low = np.uint64(0xFFFFFFFF) - np.arange(N, dtype=np.uint64)
    mk, nk, rm1 = np.zeros(M, np.uint64), np.zeros(M, np.uint64), np.zeros(M, np.int64)
    skipped = 0
    for r0 in range(0, M, block):
        r1 = min(r0 + block, M)
        with np.errstate(invalid="ignore"):
            s = a[r0:r1] @ b.T
        on = probe[r0:r1, None] & cand[None, :]
        if self_mode:
            on &= np.arange(r0, r1)[:, None] != np.arange(N)[None, :]
        fin = np.isfinite(s)
        skipped += int((on & ~fin).sum())
        on &= fin
        key = np.where(on, images(np.where(fin, s, np.float32(0))) << np.uint64(32) | low[None, :], np.uint64(0))
        same = la[r0:r1, None] == lb[None, :]
        mk[r0:r1] = np.where(same, key, np.uint64(0)).max(axis=1)
        non = np.where(same, np.uint64(0), key)
        nk[r0:r1] = non.max(axis=1)
        rm1[r0:r1] = np.where(mk[r0:r1] != 0, (non > mk[r0:r1, None]).sum(axis=1), 0)
    out = _finish_ref(probe.tolist(), mk.tolist(), nk.tolist(), rm1.tolist(), nbins)
    out["skipped"] = skipped
    return out


def same_outputs(got, want, fields=FIELDS):
    for k in fields:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, k
        assert g.tobytes() == w.astype(g.dtype).tobytes(), (k, g.reshape(-1)[:8], w.reshape(-1)[:8])


# ---------------------------------------------------------------------------------- inputs of the GPU tests
def exact_scores(a, b):
    """fp32 scores of ``four_halves`` rows: multiples of 0.25, the same in any arithmetic; a row
    with a NaN or an infinity makes every score of it not finite, as on the device."""
    with np.errstate(invalid="ignore"):
        s = a @ b.T
        s64 = a.astype(np.float64) @ b.astype(np.float64).T
    fin = np.isfinite(s64)
    assert np.array_equal(fin, np.isfinite(s)) and np.array_equal(s[fin].astype(np.float64), s64[fin])
    return s


def exact_case(M, N, D, seed, identities=9, spoil=False):
    """Probes [M, D] and gallery [N, D] of ``four_halves`` rows. Labels: ``identities`` in the
    gallery, two more among the probes (strangers), a few -1 / negative and a few valid bytes 0 on
    both sides and around the tile borders. ``spoil``: NaN / inf elements in two probes and two
    gallery rows. N = 0: one set for self mode (lb, vb None)."""
    g = np.random.default_rng(seed)
    x = four_halves(M + N, D, seed + 1)
    la = g.integers(0, identities + 2, M).astype(np.int64)
    va = np.ones(M, dtype=np.uint8)
    la[g.choice(M, min(3, M), replace=False)] = -1
    va[g.choice(M, min(3, M), replace=False)] = 0
    if M > 129:
        va[[127, 129]], la[128] = 0, -(2 ** 40)
    if N == 0:
        la[la == identities] = identities + 100 + np.arange((la == identities).sum())   # single rows: strangers to the rest
        if spoil:
            x[[1, M // 2], [0, 3]] = [np.nan, np.inf]
        return x, None, la, None, va, None
    lb = g.integers(0, identities, N).astype(np.int64)
    lb[g.choice(N, 3, replace=False)] = [-1, -7, -1]                          # compared only: they equal no probe's
    vb = np.ones(N, dtype=np.uint8)
    vb[g.choice(N, min(5, N), replace=False)] = 0
    for r in (127, 128, 255, 256):
        if r < N:
            vb[r] = 0
    if spoil:
        x[[1, M // 2], [0, 3]] = [np.nan, np.inf]
        x[[M + 2, M + N - 1], [5, 1]] = [-np.inf, np.nan]
        vb[[2, N - 1]] = 1
    return x[:M], x[M:], la, lb, va, vb


def tie_case(D=32):
    """Hand-made ties. Gallery rows: e0 e0 e0 e1 e1 e2(invalid) e2 with labels 5 6 5 7 8 9 9;
    e_k the unit row of column k. Probes (score 1 with the rows of their column, 0 with the rest):
      e0 label 5: mate rows 0, 2 and non-mate row 1 tie at 1: mate_row 0, rank 1, non_row 1;
      e0 label 6: mate row 1, non-mate rows 0, 2 tie with it: row 0 is ahead: rank 2, non_row 0;
      e1 label 8: mate row 4, non-mate row 3 ahead at the same score: rank 2;
      e1 label 7: mate row 3, non-mate row 4 behind it: rank 1;
      e2 label 9: row 5 is invalid: mate row 6, every other row scores 0: rank 1, non_row 0;
      e3 label 5: every row scores 0: mate row 0, rank 1 (row 0 leads all ties), non_row 1;
      e3 label 8: mate row 4 at 0, rows 0..3 ahead of it: rank 5, non_row 0;
      e0 label 77: a stranger: non_row 0 at score 1."""
    e = np.eye(D, dtype=np.float32)
    b = e[[0, 0, 0, 1, 1, 2, 2]]
    lb = np.array([5, 6, 5, 7, 8, 9, 9], dtype=np.int64)
    vb = np.array([1, 1, 1, 1, 1, 0, 1], dtype=np.uint8)
    a = e[[0, 0, 1, 1, 2, 3, 3, 0]]
    la = np.array([5, 6, 8, 7, 9, 5, 8, 77], dtype=np.int64)
    want = {"mate_row": [0, 1, 4, 3, 6, 0, 4, -1], "non_row": [1, 0, 3, 4, 0, 1, 0, 0], "rank": [1, 2, 2, 1, 1, 1, 5, 0],
            "mate_score": [1, 1, 1, 1, 1, 0, 0, -np.inf], "non_score": [1, 1, 1, 1, 0, 0, 0, 1]}
    return a, b, la, lb, None, vb, want


def planted_case(D=128, identities=40, per=6, strangers=60, seed=11):
    """40 identities x 6 rows and 60 strangers (labels of their own), raw rows: a centre per
    identity plus noise wide enough that some probes rank above 1. Returns (x raw float32 torch,
    labels, gallery mask): 4 rows of an identity are enrolled, 2 are probes, as the strangers are."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.arange(identities).repeat_interleave(per)
    x = torch.randn(identities, D, generator=g)[ids] + 2.2 * torch.randn(identities * per, D, generator=g)
    xs = torch.randn(strangers, D, generator=g)
    labels = torch.cat([ids, 1000 + torch.arange(strangers)]).numpy().astype(np.int64)
    in_gallery = np.concatenate([np.tile([1, 1, 1, 1, 0, 0], identities), np.zeros(strangers, int)]).astype(bool)
    return torch.cat([x, xs]), labels, in_gallery


PLANTED_TOL = 1e-6          # the GPU test asserts 4 e_ref below it; every margin here is above twice it


def planted_margins(s64, srt, la, lb, nbins, self_mode=False):
    """The smallest distance that decides an output of ``ident_eval_sorted``: between the best mate
    and every other candidate, between the best non-mate and the next non-mate, and from
    mate_score and non_score to the nearest bin edge."""
    edges = thresholds_ref(nbins)[1:nbins]
    worst = np.inf
    for i in range(s64.shape[0]):
        sc = s64[i].copy()
        if self_mode:
            sc[i] = np.nan
        for row, others in ((srt["mate_row"][i], np.ones(len(lb), bool)), (srt["non_row"][i], lb != la[i])):
            if row < 0:
                continue
            others = others.copy()
            others[row] = False
            d = np.abs(sc[others] - sc[row])
            worst = min(worst, np.nanmin(d) if d.size else np.inf, np.abs(edges - sc[row]).min())
    return worst


@functools.lru_cache(maxsize=None)
def planted_reference(nbins=256):
    """fp64 scores of the planted case (cross: probes x gallery; self: all rows), the sorted
    statement of both and e_ref, the fp32 CPU evaluation's largest distance from fp64 (off the
    diagonal: no row is compared with itself)."""
    x, labels, in_gallery = planted_case()
    n64, n32 = F.normalize(x.double(), dim=1).numpy(), F.normalize(x, dim=1).numpy()
    out = {"x": x, "labels": labels, "in_gallery": in_gallery, "nbins": nbins}
    p, q = ~in_gallery, in_gallery
    err = np.abs((n32 @ n32.T).astype(np.float64) - n64 @ n64.T)
    np.fill_diagonal(err, 0)
    out["e_ref"] = float(err.max())
    out["cross_s64"], out["self_s64"] = n64[p] @ n64[q].T, n64 @ n64.T
    out["cross"] = ident_eval_sorted(out["cross_s64"], labels[p], labels[q], None, None, nbins)
    out["self"] = ident_eval_sorted(out["self_s64"], labels, None, None, None, nbins, self_mode=True)
    return out


# ---------------------------------------------------------------------------------- tests: the key
def test_key_packing_at_its_edges():
    f32 = np.float32
    tiny, big = f32(1e-45), f32(3.4028235e38)                                  # the smallest denormal, FLT_MAX
    assert image_ref(f32(-0.0)) == image_ref(f32(0.0)) == 0x80000000
    order = [-big, f32(-1), f32(-1e-38), -tiny, f32(0), tiny, f32(1e-38), f32(0.25), f32(1), big]
    imgs = [image_ref(v) for v in order]
    assert imgs == sorted(imgs) and len(set(imgs)) == len(imgs) and min(imgs) > 0
    assert np.array_equal(images(np.array(order + [f32(-0.0)])), np.array(imgs + [0x80000000], dtype=np.uint64))
    # equal scores on two rows: the lower row has the larger key; a larger score beats any row
    assert key_ref(0.5, 3) > key_ref(0.5, 4) > key_ref(f32(0.5) - f32(2 ** -25), 0)
    top = 2 ** 24 - 1
    assert key_ref(-big, top) > 0 and key_ref(-big, 2 ** 31 - 2) > 0
    for s, row in ((f32(-0.0), top), (tiny, 0), (-tiny, 7), (f32(0.75), top), (-big, 2 ** 31 - 2)):
        back = unkey(key_ref(s, row))
        assert back[1] == row and back[0] == s and (s != 0 or not np.signbit(back[0]))
    assert unkey(0) == (-np.inf, -1)


# ---------------------------------------------------------------------------------- tests: the two statements
def _both(a, b, la, lb, va, vb, nbins):
    self_mode = b is None
    s = exact_scores(a, a if self_mode else b)
    ref = ident_eval_ref(s, la, lb, va, vb, nbins, self_mode)
    agree(ref, ident_eval_sorted(s.astype(np.float64), la, lb, va, vb, nbins, self_mode))
    same_outputs(ident_eval_blocks(a, b, la, lb, va, vb, nbins, block=50), ref)
    return ref


@pytest.mark.parametrize("D", [32, 96, 512])
def test_the_two_statements_agree_on_the_exact_cases(D):
    ref = _both(*exact_case(130, 257, D, 300 + D, spoil=D == 96), 256)
    assert ref["counts"][:3].sum() == 130 and ref["counts"][:3].min() > 0 and (ref["rank"] > 1).any()
    assert ref["hist"].sum(axis=1).min() > 0 and (ref["skipped"] > 0) == (D == 96)
    ref = _both(*exact_case(257, 0, D, 400 + D, spoil=D == 96), 512)
    assert ref["counts"][:3].sum() == 257 and ref["counts"][:3].min() > 0 and (ref["rank"] > 1).any()


def test_the_tie_case_is_what_its_docstring_says():
    a, b, la, lb, va, vb, want = tie_case()
    ref = _both(a, b, la, lb, va, vb, 256)
    for k, v in want.items():
        np.testing.assert_array_equal(ref[k], np.asarray(v, dtype=ref[k].dtype), err_msg=k)
    assert ref["counts"].tolist() == [7, 1, 0, 0] and ref["rank_hist"][[0, 1, 4]].tolist() == [4, 2, 1]
    # rows 0 (right), 1 (wrong name), 2 (stranger): the scores 1 land in the top bin, 0 in bin h
    assert ref["hist"][0, 255] == 3 and ref["hist"][0, 128] == 1 and ref["hist"][1, 255] == 2
    assert ref["hist"][1, 128] == 1 and ref["hist"][2, 255] == 1 and ref["hist"].sum() == 8


def test_self_mode_is_cross_mode_against_itself_without_the_diagonal():
    x, _, la, _, va, _ = exact_case(70, 0, 32, 55, identities=5, spoil=True)
    s = exact_scores(x, x)
    self_ref = ident_eval_ref(s, la, None, va, None, 256, self_mode=True)
    singles = [i for i in range(70) if la[i] >= 0 and va[i] and ((la == la[i]) & (va != 0)).sum() == 1]
    assert singles and all(self_ref["rank"][i] == 0 and self_ref["mate_row"][i] == -1 for i in singles)
    assert self_ref["counts"][1] >= len(singles)
    # cross mode counts the diagonal: remove it by hand -- a probe's own row is a mate at score 1
    masked = s.copy()
    masked[np.arange(70), np.arange(70)] = np.nan
    cross = ident_eval_ref(masked, la, la, va, va, 256)
    on = (la >= 0) & (va != 0)
    assert cross["skipped"] == self_ref["skipped"] + on.sum()
    same_outputs(self_ref, cross, [k for k in FIELDS if k != "skipped"])


def test_a_probe_without_any_candidate_and_the_left_out_ones():
    x = four_halves(6, 32, 9)
    la = np.array([1, 1, -1], dtype=np.int64)
    ref = ident_eval_ref(exact_scores(x[:3], x[3:]), la, [1, 2, 3], [1, 0, 1], [0, 0, 0], 256)
    assert ref["counts"].tolist() == [0, 1, 2, 1] and ref["hist"].sum() == 0 and ref["rank"].tolist() == [0, 0, 0]
    assert (ref["mate_row"] == -1).all() and (ref["non_row"] == -1).all() and np.isneginf(ref["non_score"]).all()


def test_planted_identities_hold_their_margins():
    ref = planted_reference()
    assert 4 * ref["e_ref"] < PLANTED_TOL
    labels, q = ref["labels"], ref["in_gallery"]
    cross, self_ = ref["cross"], ref["self"]
    assert cross["counts"].tolist() == [80, 60, 0, 0] and self_["counts"].tolist() == [240, 60, 0, 0]
    assert (cross["rank"] > 1).sum() >= 5 and cross["hist"][1].sum() >= 5 and cross["hist"][0].sum() >= 40
    assert (self_["rank"] > 1).sum() >= 5
    assert planted_margins(ref["cross_s64"], cross, labels[~q], labels[q], ref["nbins"]) > 2 * PLANTED_TOL
    assert planted_margins(ref["self_s64"], self_, labels, labels, ref["nbins"], self_mode=True) > 2 * PLANTED_TOL


def test_walk_inputs_hold_mates_non_mates_and_strangers():
    """The inputs of the walked GPU case at 256 CUs (``walk_sizes``: every workgroup takes three
    tiles): exact rows, labels of four classes, left-out rows on tile borders."""
    tm, tn, M, N = walk_sizes_cross(256)
    assert (M, N) == (2049, 5761) and walk_sizes(256)[1] == 4865
    a, b, la, lb, va, vb = walk_case(300, 700)
    ref = ident_eval_blocks(a, b, la, lb, va, vb, 256)
    same_outputs(ref, ident_eval_ref(exact_scores(a, b), la, lb, va, vb, 256))
    assert ref["counts"][0] > 200 and ref["counts"][2] > 5 and (ref["rank"] > 1).sum() > 20
    ref = ident_eval_blocks(a, None, la, None, va, None, 256)
    same_outputs(ref, ident_eval_ref(exact_scores(a, a), la, None, va, None, 256, self_mode=True))


def walk_case(M, N, seed=4200):
    """Probes [M, 32] and gallery [N, 32] of exact rows with ``walk_labels``; N = 0: one set."""
    x = four_halves(M + N, 32, seed)
    la, va = walk_labels(M, seed + 1)
    if N == 0:
        return x, None, la, None, va, None
    lb, vb = walk_labels(N, seed + 2)
    lb = np.where(lb < 0, -3, lb)
    la[::17] = 9                                                               # strangers to the gallery
    return x[:M], x[M:], la, lb, va, vb


# ---------------------------------------------------------------------------------- tests: the curve
def _hist3(nbins, right, wrong, stranger):
    h = np.zeros((3, nbins), dtype=np.int64)
    for row, d in enumerate((right, wrong, stranger)):
        for b, c in d.items():
            h[row, b] = c
    return h


def test_curve_hand_worked():
    # 256 bins, h = 128. 10 mated probes: 6 right in bin 200, 2 right in bin 140, 2 wrong in bin 150.
    # 100 strangers: 90 in bin 120, 9 in bin 140, 1 in the top bin
    hist = _hist3(256, {200: 6, 140: 2}, {150: 2}, {120: 90, 140: 9, 255: 1})
    rank_hist = np.zeros(R + 1, dtype=np.int64)
    rank_hist[[0, 2, R]] = [8, 1, 1]
    out = identification_curve(hist, rank_hist, [10, 100, 3, 0], fpir=(1.0, 0.1, 0.05, 0.001, 0.0))
    assert (out["mated"], out["non_mated"], out["left_out"], out["no_candidate"]) == (10, 100, 3, 0)
    r = out["at_fpir"]
    assert (r[0]["bin"], r[0]["threshold"], r[0]["dir"], r[0]["false_positives"]) == (0, -np.inf, 0.8, 100)
    assert (r[1]["bin"], r[1]["threshold"], r[1]["false_positives"], r[1]["right_names"], r[1]["wrong_names"]) == \
        (121, -7 / 128, 10, 8, 2)
    assert (r[2]["bin"], r[2]["threshold"], r[2]["false_positives"], r[2]["dir"], r[2]["wrong"]) == (141, 13 / 128, 1, 0.6, 0.2)
    assert r[2]["fnir"] == pytest.approx(0.4)
    # 0.001 x 100 < 1 and FPIR 0: only the edge past the top bin meets them; nothing is named there
    for row in r[3:]:
        assert (row["bin"], row["threshold"], row["false_positives"], row["dir"], row["fnir"]) == (256, np.inf, 0, 0.0, 1.0)
    c = out["curve"]
    assert c["dir"][0] == 0.8 and c["wrong"][0] == 0.2 and c["fpir"][0] == 1.0 and c["fpir"][121] == 0.1
    assert c["thresholds"][0] == -np.inf and c["thresholds"][256] == np.inf and c["dir"][201] == 0.0
    assert out["cmc"].shape == (R,) and out["cmc"][0] == 0.8 and out["cmc"][1] == 0.8 and out["cmc"][2] == 0.9
    assert out["cmc"][R - 1] == 0.9 and out["beyond_cmc"] == 1


def test_curve_ties_on_the_lowest_edge_and_empty_classes():
    # no stranger is named from bin 101 on: every edge 101.. meets FPIR 0 -> the lowest
    out = identification_curve(_hist3(256, {150: 5}, {}, {100: 7}), None, [5, 7, 0, 0], fpir=(0.5, 0.0))
    assert [r["bin"] for r in out["at_fpir"]] == [101, 101] and out["at_fpir"][1]["dir"] == 1.0 and out["cmc"] is None
    # all strangers: DIR, wrong and the CMC are NaN, the FPIR is not; nothing raises
    out = identification_curve(_hist3(256, {}, {}, {10: 3, 200: 1}), np.zeros(R + 1, np.int64), [0, 5, 0, 1],
                               fpir=(0.2, 1.0, -1.0))
    assert np.isnan(out["curve"]["dir"]).all() and np.isnan(out["cmc"]).all() and np.isnan(out["at_fpir"][0]["dir"])
    assert out["curve"]["fpir"][0] == 0.8 and out["at_fpir"][0]["bin"] == 11 and out["at_fpir"][0]["false_positives"] == 1
    assert out["at_fpir"][1]["bin"] == 0 and out["at_fpir"][2]["bin"] == 256       # a request below 0 is met by no edge but the last
    # no strangers: the FPIR is NaN, every request is met at the lowest edge
    out = identification_curve(_hist3(256, {130: 2}, {131: 1}, {}), None, [3, 0, 0, 0], fpir=(0.01,))
    assert np.isnan(out["curve"]["fpir"]).all() and out["at_fpir"][0]["bin"] == 0 and out["at_fpir"][0]["dir"] == 2 / 3
    # nothing at all
    out = identification_curve(np.zeros((3, 512), np.int64), np.zeros(R + 1, np.int64), [0, 0, 4, 0], fpir=(0.1,))
    assert np.isnan(out["at_fpir"][0]["dir"]) and out["at_fpir"][0]["bin"] == 0 and out["left_out"] == 4


@pytest.mark.parametrize("nbins", (256, 4096))
def test_suffix_sums_at_an_edge_are_the_probes_identify_names(nbins):
    """S_r[b] == #(probes of row r whose best score >= fp32 edge_b): what lets the histograms stand
    for identify's threshold."""
    x, labels, q = planted_case(D=32, identities=12, strangers=30, seed=3)
    n = F.normalize(x, dim=1).numpy()
    s = n[~q] @ n[q].T
    ref = ident_eval_ref(s, labels[~q], labels[q], None, None, nbins)
    out = identification_curve(ref["hist"], ref["rank_hist"], ref["counts"])
    best = np.maximum(ref["mate_score"], ref["non_score"])
    right = (ref["rank"] == 1)
    wrong, stranger = (ref["rank"] > 1), (ref["rank"] == 0)
    thr = thresholds_ref(nbins)
    for b in list(range(0, nbins + 1, max(1, nbins // 64))) + [nbins]:
        named = best >= np.float32(thr[b])
        got = [int(round(out["curve"][k][b] * d)) for k, d in (("dir", 24), ("wrong", 24), ("fpir", 30))]
        assert got == [int((named & right).sum()), int((named & wrong).sum()), int((named & stranger).sum())], b


# ---------------------------------------------------------------------------------- ABI and refusals
def test_abi_table_has_the_ident_entry_points():
    header = open(os.path.join(ROOT, "include", "prpe.h")).read()
    assert int(re.search(r"#define PRPE_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 12
    assert int(re.search(r"#define PRPE_IDENT_RANKS (\d+)", header).group(1)) == R
    for name, n in (("prpe_ident_best", 16), ("prpe_ident_rank", 15), ("prpe_ident_finish", 16)):
        decl = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header)
        assert decl and len(decl.group(1).split(",")) == n == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(_lib.lib(), name)


def ident_refusals():
    """Every -EINVAL cause the two passes share, as keyword overrides of ``call_ident``."""
    self_mode = [dict(a=None), dict(la=None), dict(lb=0x7000), dict(vb=0x8000), dict(b_row0=1), dict(M=0), dict(M=-1),
                 dict(M=2 ** 24 + 1), dict(D=0), dict(D=48), dict(D=16), dict(D=544), dict(lda=508), dict(lda=514),
                 dict(a=0x1008)]
    cross = [dict(b=0x2000), dict(b=0x2000, lb=0x7000, N=0), dict(b=0x2000, lb=0x7000, N=2 ** 24 + 1),
             dict(b=0x2000, lb=0x7000, ldb=508), dict(b=0x2000, lb=0x7000, ldb=513), dict(b=0x2004, lb=0x7000),
             dict(b=0x2000, vb=0x8000), dict(b=0x2000, lb=0x7000, b_row0=-1),
             dict(b=0x2000, lb=0x7000, b_row0=2 ** 31 - 50)]
    return self_mode + cross


def call_ident(L, which, a=0x1000, lda=512, M=100, la=0x5000, va=None, b=None, ldb=512, N=50, lb=None, vb=None,
               b_row0=0, D=512, mate=0x10000, non=0x20000, skipped=0x30000, rm1=0x40000):
    head = (a, lda, M, la, va, b, ldb, N, lb, vb, b_row0, D)
    if which == "best":
        return L.prpe_ident_best(*head, mate, non, skipped, None)
    return L.prpe_ident_rank(*head, mate, rm1, None)


def finish_refusals():
    return [dict(M=0), dict(M=2 ** 24 + 1), dict(la=None), dict(mate=None), dict(non=None), dict(mate=0x10004),
            dict(nbins=128), dict(nbins=300), dict(nbins=8192), dict(ms=None), dict(mr=None), dict(ns=None), dict(nr=None),
            dict(rank=None), dict(hist=None), dict(hist=0x90004), dict(counts=None), dict(rank_hist=None),
            dict(rm1=None), dict(rank_hist=0xA0004)]


def call_finish(L, M=100, la=0x5000, va=None, mate=0x10000, non=0x20000, rm1=0x40000, nbins=2048, ms=0x50000, mr=0x60000,
                ns=0x70000, nr=0x80000, rank=0x88000, hist=0x90000, rank_hist=0xA0000, counts=0xB0000):
    return L.prpe_ident_finish(M, la, va, mate, non, rm1, nbins, ms, mr, ns, nr, rank, hist, rank_hist, counts, None)


def test_library_rejects_bad_ident_arguments_before_launch():
    L = _lib.lib()
    for kw in ident_refusals():
        assert call_ident(L, "best", **kw) == -22 and call_ident(L, "rank", **kw) == -22, kw
    for kw in (dict(mate=None), dict(non=None), dict(skipped=None), dict(mate=0x10004), dict(skipped=0x30004)):
        assert call_ident(L, "best", **kw) == -22, kw
    for kw in (dict(mate=None), dict(rm1=None), dict(mate=0x10004)):
        assert call_ident(L, "rank", **kw) == -22, kw
    for kw in finish_refusals():
        assert call_finish(L, **kw) == -22, kw


# ---------------------------------------------------------------------------------- IdentificationEval
def test_identification_eval_bookkeeping_with_the_kernels_stubbed(monkeypatch):
    import prpe
    from prpe import gallery as gmod
    from prpe import identification as imod
    assert "IdentificationEval" in prpe.__all__
    calls = []

    def ident_best(a, a_labels, b=None, b_labels=None, *, mate_key, non_key, skipped, a_valid=None, b_valid=None, b_row0=0):
        calls.append(("best", tuple(a.shape), None if b is None else tuple(b.shape), a_valid is not None, b_valid is not None))
        skipped += 2

    def ident_rank(a, a_labels, b=None, b_labels=None, *, mate_key, rank_minus_1, a_valid=None, b_valid=None, b_row0=0):
        calls.append(("rank", tuple(a.shape), None if b is None else tuple(b.shape)))

    def ident_finish(a_labels, *, mate_key, non_key, nbins, mate_score, mate_row, non_score, non_row, rank, hist, counts,
                     rank_minus_1=None, rank_hist=None, a_valid=None):
        calls.append(("finish", nbins, rank_minus_1 is not None, rank_hist is not None))
        hist[0, nbins // 2 + 40] += 3
        hist[1, nbins // 2 + 10] += 1
        hist[2, nbins // 2 - 2] += 99
        hist[2, nbins // 2 + 41] += 1
        counts += torch.tensor([4, 100, 1, 0])
        if rank_hist is not None:
            rank_hist[0] += 3
            rank_hist[5] += 1

    for name, f in (("ident_best", ident_best), ("ident_rank", ident_rank), ("ident_finish", ident_finish)):
        monkeypatch.setattr(imod.ops, name, f)
    monkeypatch.setattr(gmod.ops, "gallery_enrol", lambda x, gallery, norms, row0=0: None)
    monkeypatch.setattr(prpe.FaceGallery, "_embeddings", lambda self, what, e: e.float().contiguous())
    gal = prpe.FaceGallery(dim=64, capacity=4, device="cpu")
    ev = prpe.IdentificationEval(gal, capacity=8)
    with pytest.raises(ValueError, match="no probes"):
        ev.evaluate()
    assert ev.add(torch.ones(5, 64), [1, 1, 2, 2, 3]) == (0, 5) and len(ev) == 5
    with pytest.raises(ValueError, match="no gallery rows"):
        ev.evaluate()
    gal.add(torch.ones(3, 64), [1, 2, 3])
    out = ev.compute(nbins=256, fpir=(0.5, 0.005))
    assert calls == [("best", (5, 64), (3, 64), True, True), ("rank", (5, 64), (3, 64)), ("finish", 256, True, True)]
    assert (out["mated"], out["non_mated"], out["left_out"], out["skipped"]) == (4, 100, 1, 2)
    assert out["cmc"][0] == 0.75 and out["cmc"][5] == 1.0 and out["beyond_cmc"] == 0
    assert [r["bin"] for r in out["at_fpir"]] == [127, 170] and out["at_fpir"][0]["false_positives"] == 1
    # leave-one-out: the gallery's own rows, no second operand, no probe store of its own
    loo = prpe.IdentificationEval.leave_one_out(gal)
    assert loo.probes is gal and len(loo) == 3
    with pytest.raises(ValueError, match="leave-one-out"):
        loo.add(torch.ones(1, 64), [1])
    del calls[:]
    loo.compute(nbins=512, cmc=False)
    assert calls == [("best", (3, 64), None, True, False), ("finish", 512, False, False)]
    # calibrate_fpir: the threshold of the row, the default left alone until then; no second pass
    fid = prpe.FaceIdentifier(model=None, gallery=prpe.FaceGallery(dim=512, capacity=1, device="cpu"))
    assert fid.threshold == 0.3
    del calls[:]
    row = fid.calibrate_fpir(ev, 0.01)
    assert [c[0] for c in calls] == ["best", "finish"] and calls[-1] == ("finish", 2048, False, False)
    assert row["false_positives"] == 1 and row["threshold"] == fid.threshold == -1 / 1024
    assert row["right_names"] == 3 and row["dir"] == 0.75
